// k_components.h -- connected components of the unitig graph (cdbg_components / cdbg_fetch_components of include/cdbg.h; the
// `bcalm -components` mode): which unitigs hang together, how many pieces there are, how big each one is.  Read-only: the kernels read
// link_off / link_to (k_links.h, k_relink.h), unitig_len and unitig_kc and write arrays of their own.  Nothing here depends on the k-mer
// width W.
//
// Two unitigs share a component exactly when a path of links joins them; sign and direction of a link are ignored, a link of a unitig to
// itself joins nothing.  Four phases, each a fixed number of launches whatever the graph looks like -- a chain of unitigs has a diameter
// equal to its length, so nothing iterates "until stable":
//   k_comp_hook      lock-free union-find in ONE pass over the links.  parent[u] starts as u.  Parallelism is over LINKS, not ends (a
//                    loaded set has no degree bound: one end may carry millions): a lane takes COMP_RUN consecutive link indices, finds
//                    the end that owns the first one by a binary search in link_off and keeps a running end from there on (the pattern
//                    of k_index_insert).  For a link u -- v it finds both roots with path halving and hooks the LARGER root under the
//                    smaller one with a compare-and-swap of parent[hi] from hi to lo; a lost race starts again from the roots it found.
//                    Roots only ever hook to smaller ids: parent[x] <= x always (no cycle can form), and when the pass is over the root of
//                    a tree is the smallest unitig id of its component, whichever lane won which race.
//   k_comp_compress  parent[u] = root of u, one lane per unitig, in a launch of its own (every hook has happened); the finds of this pass
//                    halve the paths that thousands of simultaneous hooks have left long (a chain hooked all at once is ONE path).
//   k_comp_flag / k_comp_number   flag = (parent[u] == u), exclusive scan (exscan_u32), comp[u] = rank[parent[u]]: components are numbered
//                    in the order of their smallest unitig, the same bytes on every run.
//   k_comp_totals / k_comp_summary   per component: unitigs, bases, k-mers, KC as 64-bit INTEGER atomic adds (any order, same sums) and the
//                    root's id; then singletons and the largest component.
//
// EVERY ACCESS TO parent[] IN THE HOOK AND COMPRESS KERNELS IS AN AGENT-SCOPE RELAXED ATOMIC (comp_ld / comp_min / comp_cas).  The card is
// eight XCDs with an L2 each, and a CU's L1 is never refreshed by another CU's stores: a plain load may be served from a stale line for as
// long as the kernel runs, a plain store may sit where no other XCD sees it.  The algorithm tolerates a STALE ancestor pointer -- a stale
// value is an older, still valid ancestor, and the compare-and-swap validates the root it hooks -- but it needs the compare-and-swap and the
// halving updates to be real memory operations at the device's coherence point.  No ordering is needed between them (relaxed): each word is
// its own protocol.
//
// The shape of a real graph is one giant component beside thousands of singletons (20 391 unitigs, 1 939 components, 18 453 unitigs in the
// largest, for 200 000 reads of the config-3 generator at k = 31): per-lane adds would put U adds on four addresses.  k_comp_totals
// therefore aggregates INSIDE THE WAVE first: the lanes that share the component of the first lane still waiting are summed across the wave
// and issue one add per array; that is repeated COMP_AGG_ROUNDS times for what remains, then the rest adds per lane.
#pragma once
#include "k_links.h"

namespace cdbg {

constexpr int COMP_THREADS = 256;                   // (a multiple of 64: the totals and summary kernels keep every lane of a wave alive)
constexpr int COMP_RUN = 8;                         // consecutive link indices per lane of the hook
constexpr int COMP_AGG_ROUNDS = 4;                  // wave-aggregated adds before the per-lane fallback

// agent-scope relaxed accesses to parent[] (the simulator runs one lane at a time: plain accesses there)
CDBG_DEV uint32_t comp_ld(const uint32_t* p) {
#ifdef CDBG_HOSTSIM
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
CDBG_DEV void comp_min(uint32_t* p, uint32_t v) {
#ifdef CDBG_HOSTSIM
    (void)atomicMin(p, v);
#else
    (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// -> the value found: cmp when the swap happened
CDBG_DEV uint32_t comp_cas(uint32_t* p, uint32_t cmp, uint32_t v) {
#ifdef CDBG_HOSTSIM
    return atomicCAS(p, cmp, v);
#else
    (void)__hip_atomic_compare_exchange_strong(p, &cmp, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return cmp;
#endif
}

// root of x, with path halving: every second node on the way is pointed at its grandparent.  A non-root never becomes a root again and
// only ever receives ancestors of itself, so a racing or stale update still leaves a valid tree.  The update is an atomic MINIMUM, not a
// store: ids fall strictly along a path to the root, so the minimum is the ancestor nearest the root, and a lane that read an older
// grandparent can never move a pointer BACK from where another lane has put it -- in k_comp_compress that would undo a finished unitig
// (seen on the device with plain stores: a chain of 200 000 left unitigs pointing at a non-root).
CDBG_DEV uint32_t comp_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = comp_ld(parent + x);
        if (p == x) return x;
        const uint32_t g = comp_ld(parent + p);
        if (g == p) return p;
        comp_min(parent + x, g);
        x = g;
    }
}

struct CompParams {
    uint64_t n_unitigs, n_links; int k;
    const uint64_t* link_off; const uint32_t* link_to;       // [2U + 1], [n_links]: link_to = 2 x target unitig + side
    const uint32_t* unitig_len; const uint64_t* unitig_kc;
    uint32_t* parent;                   // [U]
    uint32_t* comp;                     // [U]      the root flag first (k_comp_flag), the component of every unitig in the end (k_comp_number)
    const uint64_t* rank;               // [U + 1]  exclusive scan of the root flags; rank[U] = components
    uint64_t n_comp;
    uint64_t* c_unitigs; uint64_t* c_bases; uint64_t* c_kmers; uint64_t* c_kc; uint32_t* c_first;   // [n_comp] each; the four sums zeroed by the host
    uint64_t* out;                      // [0] components of one unitig  [1] max of (unitigs << 32) | (0xFFFFFFFF - component)  [2] links to an id >= U (must be 0)
};

__global__ void k_comp_init(CompParams P) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < P.n_unitigs) P.parent[u] = (uint32_t)u;
}

__global__ void k_comp_hook(CompParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * COMP_RUN;
    const uint64_t NE = 2 * P.n_unitigs;
    uint64_t n_bad = 0;
    for (uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * COMP_RUN; first < P.n_links; first += stride) {
        const uint64_t end = first + COMP_RUN < P.n_links ? first + COMP_RUN : P.n_links;
        uint64_t lo = 0, hi = NE;                               // the end of link `first`: the last e with link_off[e] <= first ...
        while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (P.link_off[mid] <= first) lo = mid; else hi = mid; }
        uint64_t e = lo;
        for (uint64_t i = first; i < end; ++i) {
            while (e + 1 < NE && i >= P.link_off[e + 1]) ++e;   // ... and the running end behind it (ends without links are stepped over; link_off[NE] = n_links > i)
            uint32_t u = (uint32_t)(e >> 1), v = P.link_to[i] >> 1;
            if (v >= P.n_unitigs) { ++n_bad; continue; }
            if (u == v) continue;
            for (;;) {
                u = comp_find(P.parent, u); v = comp_find(P.parent, v);
                if (u == v) break;
                const uint32_t big = u > v ? u : v, small = u > v ? v : u;
                if (comp_cas(P.parent + big, big, small) == big) break;
            }
        }
    }
    if (n_bad) atomic_add_u64(&P.out[2], n_bad);
}

__global__ void k_comp_compress(CompParams P) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= P.n_unitigs) return;
    const uint32_t r = comp_find(P.parent, (uint32_t)u);
    if (r != (uint32_t)u) comp_min(P.parent + u, r);         // (the root is the smallest id of the tree: no later halving of another lane changes it)
}

__global__ void k_comp_flag(CompParams P) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < P.n_unitigs) P.comp[u] = P.parent[u] == (uint32_t)u ? 1u : 0u;
}
__global__ void k_comp_number(CompParams P) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < P.n_unitigs) P.comp[u] = (uint32_t)P.rank[P.parent[u]];
}

// one lane per unitig
__global__ void k_comp_totals(CompParams P) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    bool todo = u < P.n_unitigs;                                  // (no early return: the wave rounds below need every lane)
    uint32_t c = 0; uint64_t len = 0, kc = 0;
    if (todo) {
        c = P.comp[u]; len = P.unitig_len[u]; kc = P.unitig_kc[u];
        if (c >= P.n_comp) todo = false;                          // (cannot happen: rank[] is a scan of the flags; never an add out of bounds)
        else if (P.parent[u] == (uint32_t)u) P.c_first[c] = (uint32_t)u;
    }
    const uint64_t km1 = (uint64_t)(P.k - 1);
    for (int round = 0; round < COMP_AGG_ROUNDS; ++round) {
        const uint64_t m = __ballot(todo);
        if (!m) break;                                            // (wave-uniform)
        const int l = __ffsll((long long)m) - 1;
        const uint32_t lc = __shfl(c, l);
        const bool mine = todo && c == lc;
        const uint64_t n = (uint64_t)__popcll(__ballot(mine));
        const uint64_t sb = wave_sum_u64(mine ? len : 0), sk = wave_sum_u64(mine ? kc : 0);
        if (lane == l) {
            atomic_add_u64(&P.c_unitigs[lc], n); atomic_add_u64(&P.c_bases[lc], sb);
            atomic_add_u64(&P.c_kmers[lc], sb - n * km1); atomic_add_u64(&P.c_kc[lc], sk);
        }
        todo = todo && !mine;
    }
    if (todo) {
        atomic_add_u64(&P.c_unitigs[c], 1); atomic_add_u64(&P.c_bases[c], len);
        atomic_add_u64(&P.c_kmers[c], len - km1); atomic_add_u64(&P.c_kc[c], kc);
    }
}

// one lane per component, one atomic per wave and number: the components of exactly one unitig, and the largest one -- by unitigs, a tie
// goes to the smaller id -- as one 64-bit maximum
__global__ void k_comp_summary(CompParams P) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    uint64_t key = 0; bool single = false;
    if (c < P.n_comp) { const uint64_t n = P.c_unitigs[c]; single = n == 1; key = (n << 32) | (0xFFFFFFFFull - c); }
    const uint64_t ns = (uint64_t)__popcll(__ballot(single));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_xor(key, d); key = o > key ? o : key; }
    if (lane == 0) {
        if (ns) atomic_add_u64(&P.out[0], ns);
        if (key) (void)atomicMax((unsigned long long*)&P.out[1], (unsigned long long)key);
    }
}

}  // namespace cdbg
