// k_quant.h -- a read set counted against the resident unitig set: how often does the sample spell the k-mer at every position of every
// unitig (cdbg_quantify / cdbg_fetch_quant / cdbg_quant_reset of include/cdbg.h; the `bcalm -quantify` mode).
//
// ONE uint32 COUNTER PER K-MER POSITION, in the numbering the index computes (kmer_off[u] + offset, k_index.h): the counters of a unitig
// are consecutive and in the orientation of its sequence -- the layout of cdbg_fetch_unitig_abundances without a gather.
//   k_quant<W>       the window walker (k_window.h) over tiles of QUANT_TILE positions, QUANT_RUN per lane -- one probe, then up to 31
//                    extensions -- with the counting sink: 1 added to the counter of the position cdbg_query would report, an atomic
//                    whose result nobody reads.  Nothing is stored per base; the staged codes are the kernel's only LDS.
//   k_quant_clamp    cnt = min(cnt, ceiling): the host runs it before 2^31 more windows could be added, so that no counter wraps
//   k_quant_report   the reported value of every counter (exact below the ceiling, 2147483647 from there on), for the read-out
//   k_quant_reduce   KC (sum of the reported values) and covered positions per unitig: the positions are split over the lanes as
//                    k_index_insert splits them, whatever the unitigs' lengths; a lane adds one partial sum per unitig it touches
#pragma once
#include "k_index.h"

namespace cdbg {

constexpr int QUANT_THREADS = 256;
constexpr int QUANT_RUN = 32;                       // consecutive query positions per lane: one probe, then up to 31 extensions
constexpr int QUANT_TILE = QUANT_THREADS * QUANT_RUN;
constexpr int QUANT_REDUCE_RUN = 32;                // consecutive k-mer positions per lane of the reduction
constexpr uint32_t QUANT_SATURATED = 2147483647u;

struct QuantParams : WindowParams {         // out: [0] windows looked at  [1] windows found  [2] of those, answered by extension
    uint32_t* cnt;                          // [P]
};

struct QuantSink {
    static constexpr bool PALINDROME_STRAND0 = false;
    const QuantParams& P;
    uint64_t u_cnt;                                         // the first counter of the latest hit's unitig
    CDBG_DEV void fresh(uint64_t u) { u_cnt = P.kmer_off[u]; }
    CDBG_DEV void window(int, bool found, uint64_t, uint32_t o, uint32_t) { if (found) (void)atomic_add_u32(&P.cnt[u_cnt + o], 1u); }
    CDBG_DEV void finish() {}
};

template <int W>
__global__ void __launch_bounds__(QUANT_THREADS) k_quant(QuantParams P) {
    CDBG_SHARED uint8_t code[QUANT_TILE + QUERY_HALO];
    const uint64_t tile0 = (uint64_t)blockIdx.x * QUANT_TILE;
    window_stage<QUANT_TILE, QUANT_THREADS>(P, tile0, code);
    __syncthreads();
    QuantSink sink{ P, 0 };
    const WindowTally t = window_walk<W, QUANT_RUN, true>(P, tile0, code, sink);
    const uint64_t n_win = wave_sum_u64(t.windows), n_found = wave_sum_u64(t.found), n_ext = wave_sum_u64(t.extended);
    if ((threadIdx.x & 63) == 0 && n_win) { atomic_add_u64(&P.out[0], n_win); if (n_found) atomic_add_u64(&P.out[1], n_found); if (n_ext) atomic_add_u64(&P.out[2], n_ext); }
}

__global__ void k_quant_clamp(uint32_t* cnt, uint64_t n, uint32_t ceiling) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = cnt[i];
        if (v > ceiling) cnt[i] = ceiling;
    }
}

CDBG_DEV uint32_t quant_reported(uint32_t v, uint32_t ceiling) { return v < ceiling ? v : QUANT_SATURATED; }

__global__ void k_quant_report(const uint32_t* cnt, uint32_t* out, uint64_t n, uint32_t ceiling) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = quant_reported(cnt[i], ceiling);
}

struct QuantReduceParams {
    const uint32_t* cnt; const uint64_t* kmer_off;
    uint64_t u0, u1;               // unitigs [u0, u1): positions [kmer_off[u0], kmer_off[u1])
    uint64_t pos0, pos1;
    uint32_t ceiling;
    uint64_t* kc; uint32_t* covered;   // [u1 - u0], zeroed by the host
};

__global__ void k_quant_reduce(QuantReduceParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * QUANT_REDUCE_RUN;
    for (uint64_t first = P.pos0 + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * QUANT_REDUCE_RUN; first < P.pos1; first += stride) {
        const uint64_t end = first + QUANT_REDUCE_RUN < P.pos1 ? first + QUANT_REDUCE_RUN : P.pos1;
        uint64_t u = last_le(P.kmer_off, P.u0, P.u1, first), g = first;   // the unitig of position `first`
        while (g < end) {
            const uint64_t k1 = P.kmer_off[u + 1];
            if (g >= k1) { ++u; continue; }
            const uint64_t stop = end < k1 ? end : k1;
            uint64_t sum = 0; uint32_t cov = 0;
            for (; g < stop; ++g) { const uint32_t v = P.cnt[g]; sum += quant_reported(v, P.ceiling); cov += v ? 1u : 0u; }
            if (cov) { (void)atomic_add_u64(&P.kc[u - P.u0], sum); (void)atomic_add_u32(&P.covered[u - P.u0], cov); }
            ++u;
        }
    }
}

}  // namespace cdbg
