// k_color_query.h -- pseudoalignment of a caller's sequences to the coloured unitig set: which of the N samples a read, a contig or a gene
// belongs to (cdbg_color_query / cdbg_fetch_color_query / cdbg_fetch_color_query_counts of include/cdbg.h; the `bcalm -colors -color-query`
// mode).  The join of the two run structures the library already keeps -- the THREAD RUNS of the sequences (k_thread.h: maximal walks
// along one unitig on one strand) and the COLOUR RUNS of the unitigs (k_color.h: maximal intervals of one colour set) -- and the fold of
// the joined pieces per sequence.
//
// A SEGMENT is a thread run cut where the colour set changes: (start, place, len, cls).  A thread run on unitig u over the offsets
// [lo, hi] meets the colour runs of u whose intervals touch [lo, hi]; they are consecutive in cl_offset[cl_run_off[u] .. cl_run_off[u + 1]),
// which ascends, so two binary searches find the first and the last.  On strand 1 the sequence walks the unitig downwards: its first
// segment lies in the LAST of those colour runs.
//   k_cq_span          one lane per thread run: the unitig and offset interval of the run (strand 1: o - len + 1 .. o), the colour runs that
//                      hold its two ends -> the first colour run in query order and the number of segments.  The host scans the numbers
//                      (exscan_u32): no atomic cursor, segment order is position order, the same on every run.
//   k_cq_emit          one lane per SEGMENT -- a unitig threaded by itself through thousands of colour runs is not one lane's work: the
//                      thread run by binary search in the scanned offsets, the colour run at first +- (s - seg_scan[run]), clipped to the
//                      thread run; start / place / len / cls at the segment's own index.  The first n_seqs + 1 lanes also write
//                      seg_off[i] = seg_scan[run_off[i]].
//   k_cq_fold<COUNTS>  one lane per (sequence, word j of 32 colours); neighbouring j are neighbouring lanes, so a class row is read coalesced.
//                      Loops over the sequence's segments, loads cl_bits[cls * NW + j] once per segment and keeps 32 counters in registers
//                      (fully unrolled: cnt[b] += (0 - ((w >> b) & 1)) & len), applies the threshold and stores one word of bits.  The
//                      colours per sequence are added with one atomic per lane that reports any (N <= 32: a plain store), and the lane
//                      whose add found the counter at zero counts the sequence among those with a colour (one atomic per wave).  found[i]
//                      comes from the j = 0 lane.  COUNTS stores the 32 counters instead and nothing else: the counts fetch only.
// The number of launches is fixed, whatever the data, and none of the three depends on the k-mer width W.  24 bytes per segment stay.
#pragma once
#include "k_color.h"

namespace cdbg {

constexpr int CQ_THREADS = 256;                     // (a multiple of 64: k_cq_fold keeps every lane of a wave alive)

struct ColorQueryParams {
    // the thread runs of the call (host_thread.h), uploaded: 20 bytes per run
    const uint64_t* run_start; const uint64_t* run_place; const uint32_t* run_len; uint64_t n_runs;
    const uint64_t* run_off; uint64_t n_seqs;           // [n_seqs + 1]
    // the colour runs and class rows of the latest cdbg_color_classes
    const uint64_t* cl_run_off; const uint32_t* cl_offset; const uint32_t* cl_len; const uint32_t* cl_cls; const uint32_t* cl_bits;
    uint64_t n_unitigs, n_cl_runs, n_classes; uint32_t n_colors, nw;
    uint32_t* span_first; uint32_t* span_n;             // [n_runs]      k_cq_span
    const uint64_t* seg_scan; uint64_t n_segs;          // [n_runs + 1]  the exclusive scan of span_n
    uint64_t* seg_off;                                  // [n_seqs + 1]  k_cq_emit
    uint64_t* seg_start; uint64_t* seg_place; uint32_t* seg_len; uint32_t* seg_cls;   // [n_segs]
    // the fold
    const uint32_t* total;                              // [n_seqs]      max(0, length - k + 1)
    uint32_t num, den; int of_found;
    uint64_t first, n_fold;                             // the sequences [first, first + n_fold) are folded
    uint32_t* found; uint32_t* n_col; uint32_t* bits;   // [n_seqs], [n_seqs] (zeroed by the host when nw > 1), [n_seqs][nw]
    uint32_t* counts;                                   // [n_fold][n_colors]  (COUNTS)
    uint64_t* out;                                      // [0] sequences with at least one colour reported
};

// the unitig, the offset interval and the strand of thread run r; false for a run that cannot be (never an access out of bounds)
CDBG_DEV bool cq_run_interval(const ColorQueryParams& P, uint64_t r, uint64_t& u, uint32_t& lo, uint32_t& hi, uint32_t& strand) {
    const uint64_t place = P.run_place[r]; const uint32_t len = P.run_len[r];
    u = place >> 33; strand = (uint32_t)(place & 1ULL);
    const uint32_t o = (uint32_t)(place >> 1);
    if (u >= P.n_unitigs || len == 0u) return false;
    if (strand) { if (o < len - 1u) return false; lo = o - (len - 1u); hi = o; }
    else { lo = o; hi = o + (len - 1u); if (hi < lo) return false; }
    return true;
}

// the last colour run in [a, b) whose offset is <= o (a when there is none: the first run of a unitig starts at offset 0)
CDBG_DEV uint64_t cq_run_of(const uint32_t* cl_offset, uint64_t a, uint64_t b, uint32_t o) {
    return last_le(cl_offset, a, b, o);
}

__global__ void __launch_bounds__(CQ_THREADS) k_cq_span(ColorQueryParams P) {
    const uint64_t r = (uint64_t)blockIdx.x * CQ_THREADS + threadIdx.x;
    if (r >= P.n_runs) return;
    uint64_t u; uint32_t lo, hi, strand, first = 0, n = 0;
    if (cq_run_interval(P, r, u, lo, hi, strand)) {
        const uint64_t a = P.cl_run_off[u], b = P.cl_run_off[u + 1];
        if (a < b && b <= P.n_cl_runs) {
            const uint64_t ra = cq_run_of(P.cl_offset, a, b, lo), rb = cq_run_of(P.cl_offset, a, b, hi);
            first = (uint32_t)(strand ? rb : ra); n = (uint32_t)(rb - ra + 1);
        }
    }
    P.span_first[r] = first; P.span_n[r] = n;
}

__global__ void __launch_bounds__(CQ_THREADS) k_cq_emit(ColorQueryParams P) {
    const uint64_t s = (uint64_t)blockIdx.x * CQ_THREADS + threadIdx.x;
    if (s <= P.n_seqs) { const uint64_t r = P.run_off[s]; P.seg_off[s] = P.seg_scan[r <= P.n_runs ? r : P.n_runs]; }
    if (s >= P.n_segs) return;
    const uint64_t r = last_le(P.seg_scan, 0, P.n_runs, s), j = s - P.seg_scan[r];   // the thread run of segment s
    uint64_t u; uint32_t lo, hi, strand;
    uint64_t start = 0, place = INDEX_EMPTY; uint32_t len = 0, cls = 0;
    if (cq_run_interval(P, r, u, lo, hi, strand)) {
        const uint64_t first = P.span_first[r], cr = strand ? first - j : first + j;
        if (cr < P.n_cl_runs && (!strand || j <= first)) {
            const uint32_t co = P.cl_offset[cr], cn = P.cl_len[cr];
            const uint32_t a = co > lo ? co : lo, ce = co + (cn - 1u), b = ce < hi ? ce : hi;      // the colour run clipped to the thread run
            if (cn && a <= b) {
                len = b - a + 1u; cls = P.cl_cls[cr];
                start = P.run_start[r] + (uint64_t)(strand ? hi - b : a - lo);
                place = (u << 33) | ((uint64_t)(strand ? b : a) << 1) | (uint64_t)strand;
            }
        }
    }
    P.seg_start[s] = start; P.seg_place[s] = place; P.seg_len[s] = len; P.seg_cls[s] = cls;
}

// one lane per (sequence, word of 32 colours); every lane of the launch stays alive (the wave sum)
template <bool COUNTS>
__global__ void __launch_bounds__(CQ_THREADS) k_cq_fold(ColorQueryParams P) {
    const uint64_t idx = (uint64_t)blockIdx.x * CQ_THREADS + threadIdx.x;
    const bool live = idx < P.n_fold * P.nw;
    uint64_t reported = 0;
    if (live) {
        const uint64_t i = P.first + idx / P.nw; const uint32_t j = (uint32_t)(idx % P.nw);
        uint32_t cnt[32];
#pragma unroll
        for (int b = 0; b < 32; ++b) cnt[b] = 0u;
        uint32_t found = 0;
        const uint64_t s0 = P.seg_off[i], s1 = P.seg_off[i + 1];
        for (uint64_t s = s0; s < s1 && s < P.n_segs; ++s) {
            const uint32_t len = P.seg_len[s], cls = P.seg_cls[s];
            const uint32_t w = cls < P.n_classes ? P.cl_bits[(uint64_t)cls * P.nw + j] : 0u;
            found += len;
#pragma unroll
            for (int b = 0; b < 32; ++b) cnt[b] += (0u - ((w >> b) & 1u)) & len;
        }
        if (COUNTS) {
            uint32_t* row = P.counts + (i - P.first) * (uint64_t)P.n_colors + (uint64_t)j * 32u;
            const uint32_t n = P.n_colors - j * 32u < 32u ? P.n_colors - j * 32u : 32u;
#pragma unroll
            for (int b = 0; b < 32; ++b) if ((uint32_t)b < n) row[b] = cnt[b];
        } else {
            const uint64_t base = P.of_found ? (uint64_t)found : (uint64_t)P.total[i];
            const uint64_t need = (uint64_t)P.num * base;
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 32; ++b) v |= (cnt[b] >= 1u && (uint64_t)cnt[b] * (uint64_t)P.den >= need) ? 1u << b : 0u;
            if (base == 0) v = 0;
            P.bits[idx + P.first * P.nw] = v;
            if (j == 0u) P.found[i] = found;
            const uint32_t pc = popc_u32(v);
            if (P.nw == 1u) { P.n_col[i] = pc; reported = pc ? 1u : 0u; }
            else if (pc) reported = atomic_add_u32(&P.n_col[i], pc) == 0u ? 1u : 0u;   // (adds are positive: exactly one lane of a sequence finds zero)
        }
    }
    if (!COUNTS) {
        reported = wave_sum_u64(reported);
        if ((threadIdx.x & 63) == 0 && reported) atomic_add_u64(&P.out[0], reported);
    }
}

}  // namespace cdbg
