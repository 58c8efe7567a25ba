// k_quant.h -- a read set counted against the resident unitig set: how often does the sample spell the k-mer at every position of every
// unitig (cdbg_quantify / cdbg_fetch_quant / cdbg_quant_reset of include/cdbg.h; the `bcalm -quantify` mode).
//
// ONE uint32 COUNTER PER K-MER POSITION, in the numbering the index computes (kmer_off[u] + offset, k_index.h): the counters of a unitig
// are consecutive and in the orientation of its sequence -- the layout of cdbg_fetch_unitig_abundances without a gather.
//   k_quant<W>       k_query's shape without its output: one workgroup per tile of query text with a k - 1 halo, staged as 2-bit codes in
//                    LDS (the kernel's only LDS); a lane rolls both strands over QUANT_RUN consecutive positions and adds 1 -- an atomic
//                    whose result nobody reads -- to the counter of the position cdbg_query would report.  Nothing is stored per base.
//                    EXTENSION: a lane that has just hit (u, o, strand) answers the next window from ONE arena base: on strand 0 the hit
//                    is (u, o + 1) if the unitig goes on (o + 1 <= LN - k) with the query's new base at u[o + k]; on strand 1 it is
//                    (u, o - 1) if o >= 1 and u[o - 1] is the complement of the new base.  The k - 1 bases the two windows share are
//                    equal by induction, so the unitig spells the window there: no hash, no slot, no unaligned k-mer read.  In a set that
//                    spells every k-mer once (every built graph) that position is the only one and hence the one a probe reports; in a set
//                    with repeated k-mers the neighbour need not be the SMALLEST occurrence, and the host turns extension off
//                    (QuantParams::extend).  The state never leaves a lane's run: each run starts with a probe.
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

struct QuantParams {
    const uint8_t* text; uint64_t n_text;   // one batch of the caller's bases
    uint64_t n_out;                         // windows that START in [0, n_out) are this batch's
    const uint32_t* bnd; uint32_t n_bnd;    // the sequence ends inside the batch, ascending; the last one is n_text
    int k; int extend;
    const uint8_t* packed; const uint64_t* unitig_off; const uint32_t* unitig_len; const uint64_t* kmer_off;
    const uint64_t* slots; uint64_t mask;
    uint32_t* cnt;                          // [P]
    uint64_t* out;                          // [0] windows looked at  [1] windows found  [2] of those, answered by extension
};

template <int W>
__global__ void __launch_bounds__(QUANT_THREADS) k_quant(QuantParams P) {
    CDBG_SHARED uint8_t code[QUANT_TILE + QUERY_HALO];      // 0 .. 3, 0xFF: a byte outside ACGTacgt (or behind the batch)
    const int tid = (int)threadIdx.x, k = P.k;
    const uint64_t tile0 = (uint64_t)blockIdx.x * QUANT_TILE;
    for (int i = tid; i < QUANT_TILE + k - 1; i += QUANT_THREADS) {
        const uint64_t g = tile0 + (uint64_t)i;
        const uint32_t c = g < P.n_text ? P.text[g] : (uint32_t)'\n';
        code[i] = base_valid(c) ? (uint8_t)base_code(c) : (uint8_t)0xFF;
    }
    __syncthreads();
    const int p0 = tid * QUANT_RUN;
    uint64_t n_win = 0, n_found = 0, n_ext = 0;
    if (tile0 + (uint64_t)p0 < P.n_out) {
        uint32_t lo = 0, hi = P.n_bnd - 1;                   // the first sequence end behind p0 (bnd[n_bnd - 1] = n_text is one)
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)P.bnd[mid] > tile0 + (uint64_t)p0) hi = mid; else lo = mid + 1; }
        uint32_t bi = lo; uint64_t seq_end = P.bnd[bi];
        int ok_from = p0;                                   // windows that start before it hold an invalid byte
        Kmer<W> fw = Kmer<W>::zero();
        for (int j = p0; j < p0 + k - 1; ++j) {
            uint32_t c = code[j];
            if (c == 0xFFu) { ok_from = j + 1; c = 0; }
            fw.push_right(k, c);
        }
        Kmer<W> rc = fw.rc(k);
        // the latest hit: arena offset of its unitig, the unitig's first counter, its k-mer positions, the offset in it, the strand
        bool have = false; uint64_t u_base = 0, u_cnt = 0; uint32_t u_npos = 0, o = 0, strand = 0;
        for (int i = 0; i < QUANT_RUN; ++i) {
            const int p = p0 + i, j = p + k - 1;
            const uint64_t g = tile0 + (uint64_t)p;
            uint32_t c = code[j];
            if (c == 0xFFu) { ok_from = j + 1; c = 0; }
            fw.push_right(k, c); rc.push_left(k, 3u - c);
            bool valid = false;
            if (g < P.n_out) {
                while (g >= seq_end) seq_end = P.bnd[++bi];
                valid = p >= ok_from && g + (uint64_t)k <= seq_end;
            }
            bool hit = false;
            if (valid) {
                ++n_win;
                if (have) {                                 // (the window before this one was valid and hit: same sequence, no invalid byte between)
                    if (strand == 0) { if (o + 1u < u_npos && packed_base(P.packed, u_base + o + (uint64_t)k) == c) { ++o; hit = true; } }
                    else if (o >= 1u && packed_base(P.packed, u_base + o - 1u) == 3u - c) { --o; hit = true; }
                    n_ext += hit ? 1u : 0u;
                }
                if (!hit) {
                    uint64_t s = index_hash<W>(rc < fw ? rc : fw) & P.mask, probes = 0, at = INDEX_EMPTY;
                    bool done, rev = false;
#pragma clang loop unroll(disable)
                    do {                                    // single exit; the table holds at least one empty slot
                        const uint64_t v = P.slots[s];
                        bool f = false, r = false;
                        if (v != INDEX_EMPTY) {
                            const Kmer<W> x = packed_kmer<W>(P.packed, P.unitig_off[v >> 32] + (v & 0xFFFFFFFFULL), k);
                            f = x == fw; r = !f && x == rc;
                        }
                        at = (f | r) ? v : at; rev = r;
                        done = (v == INDEX_EMPTY) | f | r;
                        s = (s + 1) & P.mask; ++probes;
                    } while (!done && probes <= P.mask);
                    if (at != INDEX_EMPTY) {
                        const uint64_t u = at >> 32;
                        o = (uint32_t)at; strand = rev ? 1u : 0u; hit = true;
                        u_base = P.unitig_off[u]; u_cnt = P.kmer_off[u]; u_npos = P.unitig_len[u] - (uint32_t)k + 1u;
                    }
                }
                if (hit) { ++n_found; (void)atomic_add_u32(&P.cnt[u_cnt + o], 1u); }
            }
            have = hit && P.extend != 0;
        }
    }
    n_win = wave_sum_u64(n_win); n_found = wave_sum_u64(n_found); n_ext = wave_sum_u64(n_ext);
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
        uint64_t lo = P.u0, hi = P.u1;                          // the unitig of position `first`: the last u with kmer_off[u] <= first
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (P.kmer_off[mid] <= first) lo = mid; else hi = mid; }
        uint64_t u = lo, g = first;
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
