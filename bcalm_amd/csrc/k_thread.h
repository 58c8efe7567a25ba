// k_thread.h -- the walk of a sequence through the resident unitig set: the maximal runs of consecutive k-mers that lie on one unitig, on
// one strand, at consecutive offsets (cdbg_thread / cdbg_fetch_runs of include/cdbg.h; the `bcalm -thread` mode).  The third consumer of
// the index (k_index.h): the hit word of every position stays in HBM, only the runs leave the device.
//
// A RUN IS DEFINED BY THE HIT WORDS cdbg_query reports, and by nothing else: position g CONTINUES g - 1 when neither word is a miss, the
// unitigs and the strands are equal and the offset moved by +1 (strand 0) or -1 (strand 1).  A HEAD is a hit that does not continue its
// predecessor, a TAIL a hit whose successor does not continue it; the i-th head and the i-th tail, in position order, bound the i-th
// run.  Heads and tails are ranked SEPARATELY: a run may be longer than any tile (a unitig threaded by itself is one run).
//   k_thread_hits<W>  the producer: the window walker (k_window.h) over k_query's tiles -- QUERY_TILE positions, QUERY_RUN per lane --
//                     with extension and the hit-word sink.  What it stores is the word a probe would: a window that is its own
//                     reverse complement (even k) reached along strand 1 is reported on strand 0 (the sink's PALINDROME_STRAND0).
//   k_thread_count    per tile of THREAD_TILE positions the number of heads and of tails (hits[g - 1], hits[g], hits[g + 1]; outside
//                     the batch the neighbour is "no hit").  The host scans the two count arrays (exscan_u32).
//   k_thread_emit     recomputes the flags and ranks them inside the workgroup -- wave_incl_sum_u32 across a wave, one LDS word per
//                     wave across the waves; no atomic cursor: the output order is the position order, the same on every run.  A head
//                     stores its position and its hit word at its rank, a tail its position at its rank.
//   k_thread_len      len = tail - head + 1 per run
#pragma once
#include "k_quant.h"

namespace cdbg {

constexpr int THREAD_THREADS = 256;
constexpr int THREAD_ITEMS = 4;                     // consecutive positions per lane of the run kernels
constexpr int THREAD_TILE = THREAD_THREADS * THREAD_ITEMS;

struct ThreadHitParams : WindowParams {     // out: [0] windows looked at  [1] windows found  [2] of those, answered by extension
    uint64_t* hits;                         // [n_out]
};

template <int W>
__global__ void __launch_bounds__(QUERY_THREADS) k_thread_hits(ThreadHitParams P) {
    CDBG_SHARED uint8_t code[QUERY_TILE + QUERY_HALO];
    CDBG_SHARED uint64_t hit[QUERY_TILE];
    const uint64_t tile0 = (uint64_t)blockIdx.x * QUERY_TILE;
    window_stage<QUERY_TILE, QUERY_THREADS>(P, tile0, code);
    __syncthreads();
    HitWordSink<true> sink{ hit };
    const WindowTally t = window_walk<W, QUERY_RUN, true>(P, tile0, code, sink);
    __syncthreads();
    window_store_hits<QUERY_TILE, QUERY_THREADS>(hit, tile0, P.n_out, P.hits);
    const uint64_t n_win = wave_sum_u64(t.windows), n_found = wave_sum_u64(t.found), n_ext = wave_sum_u64(t.extended);
    if ((threadIdx.x & 63) == 0 && n_win) { atomic_add_u64(&P.out[0], n_win); if (n_found) atomic_add_u64(&P.out[1], n_found); if (n_ext) atomic_add_u64(&P.out[2], n_ext); }
}

// does the hit word b, one position behind the hit word a, continue a's run (on the host too: the batch seams, host_thread.h)
CDBG_HD bool thread_continues(uint64_t a, uint64_t b) {
    if (a == INDEX_EMPTY || b == INDEX_EMPTY) return false;
    if (((a ^ b) >> 33) != 0 || ((a ^ b) & 1ULL) != 0) return false;
    const uint32_t oa = (uint32_t)(a >> 1), ob = (uint32_t)(b >> 1);
    return (a & 1ULL) ? (oa != 0u && ob == oa - 1u) : (ob == oa + 1u);
}

struct ThreadRunParams {
    const uint64_t* hits; uint64_t n;       // one batch's hit words
    uint64_t base;                          // the batch's first position in the call's numbering
    uint32_t* n_heads; uint32_t* n_tails;   // [tiles]      k_thread_count
    const uint64_t* head_off; const uint64_t* tail_off;   // [tiles + 1]  their exclusive scans
    uint64_t* start; uint64_t* place; uint64_t* tail;     // [runs]       k_thread_emit
    uint32_t* len; uint64_t n_runs;                       // [runs]       k_thread_len
};

// heads (low half) and tails (high half) among the lane's THREAD_ITEMS positions from g0 on, as a bit per position each, and the hit words
CDBG_DEV uint32_t thread_flags(const ThreadRunParams& P, uint64_t g0, uint64_t (&h)[THREAD_ITEMS]) {
    uint64_t prev = (g0 >= 1 && g0 - 1 < P.n) ? P.hits[g0 - 1] : INDEX_EMPTY;
#pragma unroll
    for (int i = 0; i < THREAD_ITEMS; ++i) h[i] = g0 + (uint64_t)i < P.n ? P.hits[g0 + (uint64_t)i] : INDEX_EMPTY;
    const uint64_t next = g0 + (uint64_t)THREAD_ITEMS < P.n ? P.hits[g0 + (uint64_t)THREAD_ITEMS] : INDEX_EMPTY;
    uint32_t f = 0;
#pragma unroll
    for (int i = 0; i < THREAD_ITEMS; ++i) {
        const uint64_t nx = i + 1 < THREAD_ITEMS ? h[i + 1 < THREAD_ITEMS ? i + 1 : 0] : next;
        if (h[i] != INDEX_EMPTY) {
            if (!thread_continues(prev, h[i])) f |= 1u << i;
            if (!thread_continues(h[i], nx)) f |= 0x10000u << i;
        }
        prev = h[i];
    }
    return f;
}

// heads in the low 16 bits, tails in the high 16: a tile holds at most THREAD_TILE of each
CDBG_DEV uint32_t thread_flag_counts(uint32_t f) { return (uint32_t)__popc(f & 0xFFFFu) | ((uint32_t)__popc(f >> 16) << 16); }
static_assert(THREAD_TILE < 65536 && THREAD_ITEMS <= 16, "two 16-bit counts per tile in one word");

__global__ void __launch_bounds__(THREAD_THREADS) k_thread_count(ThreadRunParams P) {
    CDBG_SHARED uint32_t wsum[THREAD_THREADS / 64];
    const int tid = (int)threadIdx.x;
    uint64_t h[THREAD_ITEMS];
    const uint32_t f = thread_flags(P, (uint64_t)blockIdx.x * THREAD_TILE + (uint64_t)tid * THREAD_ITEMS, h);
    const uint32_t incl = wave_incl_sum_u32(thread_flag_counts(f));
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < THREAD_THREADS / 64; ++w) t += wsum[w];
        P.n_heads[blockIdx.x] = t & 0xFFFFu; P.n_tails[blockIdx.x] = t >> 16;
    }
}

__global__ void __launch_bounds__(THREAD_THREADS) k_thread_emit(ThreadRunParams P) {
    CDBG_SHARED uint32_t wsum[THREAD_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * THREAD_TILE + (uint64_t)tid * THREAD_ITEMS;
    uint64_t h[THREAD_ITEMS];
    const uint32_t f = thread_flags(P, g0, h);
    const uint32_t mine = thread_flag_counts(f);
    const uint32_t incl = wave_incl_sum_u32(mine);
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine;                           // the flags of the lanes before this one: its wave, then the waves before it
#pragma unroll
    for (int w = 0; w < THREAD_THREADS / 64; ++w) before += w < (tid >> 6) ? wsum[w] : 0u;
    uint64_t rh = P.head_off[blockIdx.x] + (before & 0xFFFFu), rt = P.tail_off[blockIdx.x] + (before >> 16);
#pragma unroll
    for (int i = 0; i < THREAD_ITEMS; ++i) {
        if (f & (1u << i)) { if (rh < P.n_runs) { P.start[rh] = P.base + g0 + (uint64_t)i; P.place[rh] = h[i]; } ++rh; }
        if (f & (0x10000u << i)) { if (rt < P.n_runs) P.tail[rt] = P.base + g0 + (uint64_t)i; ++rt; }
    }
}

__global__ void k_thread_len(ThreadRunParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n_runs) P.len[i] = (uint32_t)(P.tail[i] - P.start[i] + 1);
}

}  // namespace cdbg
