// k_relink.h -- edges between the sequences of a unitig set the CALLER supplies (cdbg_load_unitigs + cdbg_link; the `bcalm -redo-links`
// mode): the junction join of k_links.h WITHOUT a degree bound.
//
// k_links.h keeps at most LINK_PER_FLAG ends per (junction, strand): right for the unitigs of ONE graph, whose k-mers are all distinct
// (four k-mers c + J, one more at even k).  A FASTA from anywhere else -- pieces cut at reference extremities, contigs of another
// assembler, a file that lists a record twice -- puts any number of ends on one oriented junction.  Here every (slot, flag) of the junction
// table gets a RUN of exactly its size (count, exclusive scan, scatter), every run is put in ascending order of end id, and the links of
// end e are a copy of the opposite run (the same run at a palindromic junction): nothing is dropped or clamped, link_to of every end is
// ascending and the same bytes on every execution.  Keys, flags and the end / sign encoding are those of k_links.h (link_end_kmer).
//
// Runs are ordered by RANK: the end ids of a run are distinct, so the place of e in its sorted run is the number of members below e.
// One lane per end counts them; a run longer than a wave is counted by the whole wave for each of its ends (RELINK_WAVE_MIN), as is
// the copy of a long run into link_to -- one end of huge degree costs its wave degree / 64 steps, not degree.
#pragma once
#include "k_links.h"

namespace cdbg {

constexpr int RELINK_THREADS = 256;                 // (a multiple of 64: the order and fill kernels keep every lane of a wave alive)
constexpr uint32_t RELINK_WAVE_MIN = 64;            // runs longer than this are handled by all lanes of the wave together

// ---- cdbg_load_unitigs: the caller's bases checked and folded to upper case where they lie (16 bytes per lane) ----
struct LoadCheckParams { uint8_t* bases; uint64_t n_bases; uint64_t* first_bad; };   // first_bad: smallest 16-byte chunk with a byte outside ACGTacgt (UINT64_MAX: none)
__global__ void k_relink_check(LoadCheckParams P) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c * 16 >= P.n_bases) return;
    uint4* const p = reinterpret_cast<uint4*>(P.bases) + c;       // (the arena is padded to whole chunks)
    const uint4 v = *p;
    uint32_t w[4] = { v.x, v.y, v.z, v.w };
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t x = w[t] & 0xDFDFDFDFu;                    // fold case
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t ch = (x >> (8 * b)) & 0xFFu;
            if (c * 16 + (uint64_t)(4 * t + b) < P.n_bases) ok &= (ch == 'A') | (ch == 'C') | (ch == 'G') | (ch == 'T');
        }
        w[t] = x;
    }
    uint4 o; o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    *p = o;
    if (!ok) {                                                    // 64-bit minimum by compare-and-swap
        uint64_t old = ld_agent_u64(P.first_bad);
        while (c < old) { const uint64_t prev = atomic_cas_u64(P.first_bad, old, c); if (prev == old) break; old = prev; }
    }
}

struct RelinkParams {
    uint64_t n_unitigs; int k;
    const uint64_t* unitig_off; const uint32_t* unitig_len; const uint8_t* bases;
    uint64_t* keys; uint32_t mask;          // junction table (KTable)
    uint32_t* cnt;                          // [2 cap]      ends per (slot, flag); counted up by insert, down to zero by scatter
    const uint64_t* run_off;                // [2 cap + 1]  exclusive scan of cnt: where the run of every (slot, flag) begins
    uint32_t* runs;                         // [2U]         the runs in arrival order
    uint32_t* sorted;                       // [2U]         the runs in ascending order of end id
    uint32_t* end_own;                      // [2U]         2 slot + flag of each end: the run it is a member of
    uint32_t* end_opp;                      // [2U]         the run it links to: the other flag, the same one at a palindromic key
    uint32_t* deg;                          // [2U]
    const uint64_t* link_off; uint32_t* link_to;
};

template <int W>
__global__ void k_relink_insert(RelinkParams P) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * P.n_unitigs) return;
    const uint64_t u = e >> 1; const uint32_t side = (uint32_t)(e & 1);
    const Kmer<W> x = link_end_kmer<W>(P.bases + P.unitig_off[u], P.unitig_len[u], P.k, side);
    const Kmer<W> j = suffix_km1<W>(x, P.k);
    const Kmer<W> r = j.rc(P.k - 1);
    const bool pal = (r == j);
    const uint32_t flag = (!pal && r < j) ? 1u : 0u;
    const Kmer<W> jc = flag ? r : j;
    const KTable<W> T{ P.keys, P.mask };
    bool nw; const uint32_t s = ktable_insert<W, true>(T, jc, nw);
    const uint32_t own = s * 2 + flag;
    atomic_add_u32(&P.cnt[own], 1u);
    P.end_own[e] = own;
    P.end_opp[e] = pal ? own : own ^ 1u;
}
__global__ void k_relink_scatter(RelinkParams P) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * P.n_unitigs) return;
    const uint32_t own = P.end_own[e];
    const uint32_t pos = atomic_sub_u32(&P.cnt[own], 1u) - 1u;    // (any order: k_relink_order sorts)
    P.runs[P.run_off[own] + pos] = (uint32_t)e;
}
// sorted[run begin + rank of e] = e.  A run that no end links to (its opposite run is empty) is never read and stays unordered.
__global__ void k_relink_order(RelinkParams P) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    uint64_t o = 0; uint32_t n = 0;
    if (e < 2 * P.n_unitigs) {                                    // (no early return: the wave loop below needs every lane)
        const uint32_t own = P.end_own[e], opp = P.end_opp[e];
        if (P.run_off[opp + 1] > P.run_off[opp]) { o = P.run_off[own]; n = (uint32_t)(P.run_off[own + 1] - o); }
    }
    uint32_t rank = 0;
    if (n <= RELINK_WAVE_MIN) for (uint32_t i = 0; i < n; ++i) rank += P.runs[o + i] < (uint32_t)e ? 1u : 0u;
    uint64_t m = __ballot(n > RELINK_WAVE_MIN);                   // wave-uniform: one turn per end of a long run
    while (m) {
        const int l = __ffsll((long long)m) - 1; m &= m - 1;
        const uint64_t lo = __shfl(o, l); const uint32_t ln = __shfl(n, l), le = __shfl((uint32_t)e, l);
        uint32_t part = 0;
        for (uint32_t i = (uint32_t)lane; i < ln; i += 64) part += P.runs[lo + i] < le ? 1u : 0u;
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
        if (lane == l) rank = part;
    }
    if (n) P.sorted[o + rank] = (uint32_t)e;
}
__global__ void k_relink_count(RelinkParams P) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * P.n_unitigs) return;
    const uint32_t opp = P.end_opp[e];
    P.deg[e] = (uint32_t)(P.run_off[opp + 1] - P.run_off[opp]);
}
__global__ void k_relink_fill(RelinkParams P) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    uint64_t src = 0, dst = 0; uint32_t n = 0;
    if (e < 2 * P.n_unitigs) { src = P.run_off[P.end_opp[e]]; dst = P.link_off[e]; n = P.deg[e]; }
    if (n <= RELINK_WAVE_MIN) for (uint32_t i = 0; i < n; ++i) P.link_to[dst + i] = P.sorted[src + i];
    uint64_t m = __ballot(n > RELINK_WAVE_MIN);
    while (m) {
        const int l = __ffsll((long long)m) - 1; m &= m - 1;
        const uint64_t ls = __shfl(src, l), ld = __shfl(dst, l); const uint32_t ln = __shfl(n, l);
        for (uint32_t i = (uint32_t)lane; i < ln; i += 64) P.link_to[ld + i] = P.sorted[ls + i];
    }
}

}  // namespace cdbg
