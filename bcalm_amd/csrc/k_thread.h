// k_thread.h -- the walk of a sequence through the resident unitig set: the maximal runs of consecutive k-mers that lie on one unitig, on
// one strand, at consecutive offsets (cdbg_thread / cdbg_fetch_runs of include/cdbg.h; the `bcalm -thread` mode).  The third consumer of
// the index (k_index.h): the hit word of every position stays in HBM, only the runs leave the device.
//
// A RUN IS DEFINED BY THE HIT WORDS cdbg_query reports, and by nothing else: position g CONTINUES g - 1 when neither word is a miss, the
// unitigs and the strands are equal and the offset moved by +1 (strand 0) or -1 (strand 1).  A HEAD is a hit that does not continue its
// predecessor, a TAIL a hit whose successor does not continue it; the i-th head and the i-th tail, in position order, bound the i-th
// run.  Heads and tails are ranked SEPARATELY: a run may be longer than any tile (a unitig threaded by itself is one run).
//   k_thread_hits<W>  the producer: k_query's tile -- one workgroup per QUERY_TILE positions, a k - 1 halo, 2-bit codes in LDS, the hit
//                     words through LDS into coalesced stores -- with k_quant's extension: a lane that has just hit (u, o, strand)
//                     answers the next window from ONE arena base.  What it stores is the word a probe would: a window that is its own
//                     reverse complement (even k) reached along strand 1 is reported on strand 0, as k_query's compare order has it.
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

struct ThreadHitParams {
    const uint8_t* text; uint64_t n_text;   // one batch of the caller's bases
    uint64_t n_out;                         // positions of it to answer: hits[0 .. n_out)
    const uint32_t* bnd; uint32_t n_bnd;    // the sequence ends inside the batch, ascending; the last one is n_text
    int k; int extend;
    const uint8_t* packed; const uint64_t* unitig_off; const uint32_t* unitig_len;
    const uint64_t* slots; uint64_t mask;
    uint64_t* hits;                         // [n_out]
    uint64_t* out;                          // [0] windows looked at  [1] windows found  [2] of those, answered by extension
};

template <int W>
__global__ void __launch_bounds__(QUERY_THREADS) k_thread_hits(ThreadHitParams P) {
    CDBG_SHARED uint8_t code[QUERY_TILE + QUERY_HALO];      // 0 .. 3, 0xFF: a byte outside ACGTacgt (or behind the batch)
    CDBG_SHARED uint64_t hit[QUERY_TILE];
    const int tid = (int)threadIdx.x, k = P.k;
    const uint64_t tile0 = (uint64_t)blockIdx.x * QUERY_TILE;
    for (int i = tid; i < QUERY_TILE + k - 1; i += QUERY_THREADS) {
        const uint64_t g = tile0 + (uint64_t)i;
        const uint32_t c = g < P.n_text ? P.text[g] : (uint32_t)'\n';
        code[i] = base_valid(c) ? (uint8_t)base_code(c) : (uint8_t)0xFF;
    }
    __syncthreads();
    const int p0 = tid * QUERY_RUN;
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
        // the latest hit: its unitig, the arena offset of that unitig, its k-mer positions, the offset in it, the strand
        bool have = false; uint64_t u = 0, u_base = 0; uint32_t u_npos = 0, o = 0, strand = 0;
        for (int i = 0; i < QUERY_RUN; ++i) {
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
            bool found = false;
            if (valid) {
                ++n_win;
                if (have) {                                 // (the window before this one was valid and hit: same sequence, no invalid byte between)
                    if (strand == 0) { if (o + 1u < u_npos && packed_base(P.packed, u_base + o + (uint64_t)k) == c) { ++o; found = true; } }
                    else if (o >= 1u && packed_base(P.packed, u_base + o - 1u) == 3u - c) {
                        --o; found = true;
                        if (fw == rc) strand = 0;           // its own reverse complement: the unitig reads there as the window itself, and a probe says so
                    }
                    n_ext += found ? 1u : 0u;
                }
                if (!found) {
                    uint64_t s = index_hash<W>(rc < fw ? rc : fw) & P.mask, probes = 0, at = INDEX_EMPTY;
                    bool done, rev = false;
#pragma clang loop unroll(disable)
                    do {                                    // single exit; the table holds at least one empty slot
                        const uint64_t v = P.slots[s];
                        bool f = false, r = false;
                        if (v != INDEX_EMPTY) {
                            const Kmer<W> x = packed_kmer<W>(P.packed, P.unitig_off[v >> 32] + (v & 0xFFFFFFFFULL), k);
                            f = x == fw; r = !f && x == rc;   // (a k-mer that is its own reverse complement: strand 0)
                        }
                        at = (f | r) ? v : at; rev = r;
                        done = (v == INDEX_EMPTY) | f | r;
                        s = (s + 1) & P.mask; ++probes;
                    } while (!done && probes <= P.mask);
                    if (at != INDEX_EMPTY) {
                        u = at >> 32; o = (uint32_t)at; strand = rev ? 1u : 0u; found = true;
                        u_base = P.unitig_off[u]; u_npos = P.unitig_len[u] - (uint32_t)k + 1u;
                    }
                }
                n_found += found ? 1u : 0u;
            }
            hit[p] = found ? ((u << 33) | ((uint64_t)o << 1) | (uint64_t)strand) : INDEX_EMPTY;
            have = found && P.extend != 0;
        }
    }
    __syncthreads();
    for (int i = tid; i < QUERY_TILE; i += QUERY_THREADS) {
        const uint64_t g = tile0 + (uint64_t)i;
        if (g < P.n_out) P.hits[g] = hit[i];
    }
    n_win = wave_sum_u64(n_win); n_found = wave_sum_u64(n_found); n_ext = wave_sum_u64(n_ext);
    if ((threadIdx.x & 63) == 0 && n_win) { atomic_add_u64(&P.out[0], n_win); if (n_found) atomic_add_u64(&P.out[1], n_found); if (n_ext) atomic_add_u64(&P.out[2], n_ext); }
}

// does the hit word b, one position behind the hit word a, continue a's run
CDBG_DEV bool thread_continues(uint64_t a, uint64_t b) {
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
