// k_color.h -- the resident unitig set coloured by sample: which of N samples hold the k-mer at every position of every unitig, where along
// a unitig that answer changes, and how many distinct sample sets there are (cdbg_color_open / cdbg_color / cdbg_color_classes /
// cdbg_fetch_color_runs / cdbg_fetch_color_classes of include/cdbg.h; the `bcalm -colors` mode).
//
// N BIT PLANES OF P BITS, COLOUR-MAJOR: plane[c][g >> 5] bit g & 31, g = kmer_off[u] + offset as the index and cdbg_quantify number the
// positions.  Neighbouring positions of a unitig share a word, and "does the colour set change between g - 1 and g" is a word operation:
// ustart | OR_c (x_c ^ ((x_c << 1) | bit 31 of the word before)).  One more plane, ustart, holds a bit at every kmer_off[u].
//   k_color_mark<W>   the window walker (k_window.h) over k_quant's tiles (QUANT_TILE positions, QUANT_RUN per lane, extension) with the
//                     marking sink: instead of one atomic per hit a lane keeps (word index, mask) in registers, ORs the hit's bit into
//                     the mask and writes the mask with one atomic OR when the word index changes -- hits walk up on strand 0 and down
//                     on strand 1 -- and at the end of its run.  (A miss does not flush: the mask stays valid across it, and a later
//                     hit in the same word joins it.)  Before the atomic it loads the word plainly and skips the atomic when every bit
//                     is there: bits are only ever set while marking, so a stale read can only cause a redundant atomic.  Nothing is
//                     stored per base.
//   k_color_ustart    one lane per unitig: the bit of its first position
//   k_color_heads     one lane per 32-position word: the N plane words and each one's predecessor bit -> the word's head mask (stored: the
//                     emit pass reads 4 bytes per word, not N), heads per wave (a tile is the 64 words of a wave: no LDS), positions with a
//                     colour.  The host scans the per-wave counts (exscan_u32).
//   k_color_emit      ranks the heads inside the wave (wave_incl_sum_u32) behind the wave's scanned offset -- no atomic cursor: run order is
//                     position order, the same on every run -- and stores each run's first position at its rank
//   k_color_runs      one lane per run: len = next start - start (the last run ends at P), its unitig by a binary search in kmer_off, its
//                     offset; a run at offset 0 writes run_off[unitig]; unitigs that are one run are counted
//   k_color_insert    the class table: open addressing, 64-bit slots that hold a RUN INDEX; the key is the colour set read from the planes
//                     at the run's first position (as k_index reads its keys from the arena).  Per run: hash the N-bit vector, CAS empty ->
//                     my run; else if the vector of the slot's run equals mine, atomic minimum with my run; else the next slot.  Every value
//                     a slot ever holds has the same vector, so the comparison is stable while the minimum moves, and a vector has ONE
//                     slot: slots never empty again, so two runs of equal vectors walk the same occupied prefix.  The slot is remembered.
//   k_color_rep       rep[r] = what the remembered slot holds in the end (the smallest run of the class); flag = (rep[r] == r)
//   k_color_number    class = rank of the representative in the scan of the flags (classes in the order of their first run); runs and
//                     positions per class by wave-aggregated 64-bit adds, as k_comp_totals does
//   k_color_gather    one lane per (class, 32 colours): the class's bits from the planes at its first run, padding bits zero; colours
//                     per class
// The number of launches is fixed, whatever the data.  Nothing but k_color_mark depends on the k-mer width W.
#pragma once
#include "k_quant.h"

namespace cdbg {

constexpr int COLOR_THREADS = 256;                  // (a multiple of 64: the run and class kernels keep every lane of a wave alive)
constexpr int COLOR_AGG_ROUNDS = 4;                 // wave-aggregated adds before the per-lane fallback (k_color_number)
constexpr uint64_t COLOR_EMPTY = 0xFFFFFFFFFFFFFFFFULL;

struct ColorMarkParams : WindowParams {     // out: [0] windows looked at  [1] windows found  [2] of those, answered by extension  [3] atomics issued
    uint32_t* plane; uint64_t n_words;      // the colour's plane: ceil(P / 32) words
};

// the lane's pending bits go to the plane: -> atomics issued (0 or 1)
CDBG_DEV uint32_t color_flush(const ColorMarkParams& P, uint64_t w, uint32_t m) {
    if (!m || w >= P.n_words) return 0u;                    // (w < n_words for every position of the set: never an atomic out of bounds)
    if ((P.plane[w] & m) == m) return 0u;
    (void)atomic_or_u32(P.plane + w, m);
    return 1u;
}

struct ColorMarkSink {
    static constexpr bool PALINDROME_STRAND0 = false;
    const ColorMarkParams& P;
    uint64_t u_pos;                                         // the first position of the latest hit's unitig
    uint64_t cur_w; uint32_t cur_m;                         // the bits not yet written: a word of the plane and a mask
    uint64_t n_atom;
    CDBG_DEV void fresh(uint64_t u) { u_pos = P.kmer_off[u]; }
    CDBG_DEV void window(int, bool found, uint64_t, uint32_t o, uint32_t) {
        if (!found) return;
        const uint64_t at = u_pos + o, w = at >> 5;
        if (w != cur_w) { n_atom += color_flush(P, cur_w, cur_m); cur_w = w; cur_m = 0; }
        cur_m |= 1u << (uint32_t)(at & 31u);
    }
    CDBG_DEV void finish() { n_atom += color_flush(P, cur_w, cur_m); }
};

template <int W>
__global__ void __launch_bounds__(QUANT_THREADS) k_color_mark(ColorMarkParams P) {
    CDBG_SHARED uint8_t code[QUANT_TILE + QUERY_HALO];
    const uint64_t tile0 = (uint64_t)blockIdx.x * QUANT_TILE;
    window_stage<QUANT_TILE, QUANT_THREADS>(P, tile0, code);
    __syncthreads();
    ColorMarkSink sink{ P, 0, 0, 0, 0 };
    const WindowTally t = window_walk<W, QUANT_RUN, true>(P, tile0, code, sink);
    const uint64_t n_win = wave_sum_u64(t.windows), n_found = wave_sum_u64(t.found), n_ext = wave_sum_u64(t.extended), n_atom = wave_sum_u64(sink.n_atom);
    if ((threadIdx.x & 63) == 0 && n_win) {
        atomic_add_u64(&P.out[0], n_win);
        if (n_found) atomic_add_u64(&P.out[1], n_found);
        if (n_ext) atomic_add_u64(&P.out[2], n_ext);
        if (n_atom) atomic_add_u64(&P.out[3], n_atom);
    }
}

__global__ void k_color_ustart(const uint64_t* kmer_off, uint64_t n_unitigs, uint32_t* ustart, uint64_t n_words) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_unitigs) return;
    const uint64_t g = kmer_off[u];
    if ((g >> 5) < n_words) (void)atomic_or_u32(ustart + (g >> 5), 1u << (uint32_t)(g & 31u));
}

struct ColorRunParams {
    const uint32_t* planes; const uint32_t* ustart;     // [n_colors][n_words], [n_words]
    uint64_t n_words, n_pos; uint32_t n_colors;
    uint32_t* heads;                    // [n_words]    the head mask of every word (k_color_heads)
    uint32_t* tile_cnt;                 // [tiles]      heads per wave of k_color_heads: a tile is 64 words
    const uint64_t* tile_off;           // [tiles + 1]  their exclusive scan
    uint64_t* start; uint64_t n_runs;   // [n_runs]     the first position of every run (k_color_emit)
    const uint64_t* kmer_off; const uint32_t* unitig_len; uint64_t n_unitigs; int k;
    uint64_t* run_off; uint32_t* offset; uint32_t* len;   // [U + 1], [n_runs], [n_runs]  (k_color_runs)
    uint64_t* out;                      // [0] positions with at least one colour  [1] unitigs that are one run
};

// one lane per word of 32 positions; every lane of the launch stays alive (the wave scan)
__global__ void __launch_bounds__(COLOR_THREADS) k_color_heads(ColorRunParams P) {
    const uint64_t w = (uint64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
    uint32_t head = 0, any = 0;
    if (w < P.n_words) {
        head = P.ustart[w];
        for (uint32_t c = 0; c < P.n_colors; ++c) {
            const uint32_t* pl = P.planes + (uint64_t)c * P.n_words;
            const uint32_t x = pl[w], carry = w ? pl[w - 1] >> 31 : 0u;
            head |= x ^ ((x << 1) | carry);
            any |= x;
        }
        const uint64_t rem = P.n_pos - w * 32u;             // (> 0: n_words = ceil(n_pos / 32))
        if (rem < 32u) head &= (1u << (uint32_t)rem) - 1u;  // (no bit of a plane is ever set behind P; the shifted-in neighbour of the last one is not a head)
        P.heads[w] = head;
    }
    const uint32_t incl = wave_incl_sum_u32(popc_u32(head));
    if ((threadIdx.x & 63) == 63) P.tile_cnt[w >> 6] = incl;
    const uint64_t cov = wave_sum_u64((uint64_t)popc_u32(any));
    if ((threadIdx.x & 63) == 0 && cov) atomic_add_u64(&P.out[0], cov);
}

__global__ void __launch_bounds__(COLOR_THREADS) k_color_emit(ColorRunParams P) {
    const uint64_t w = (uint64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
    uint32_t head = w < P.n_words ? P.heads[w] : 0u;
    const uint32_t mine = popc_u32(head);
    const uint32_t incl = wave_incl_sum_u32(mine);
    uint64_t r = P.tile_off[w >> 6] + (uint64_t)(incl - mine);
    while (head) {
        const uint32_t b = ctz_u32(head);
        head &= head - 1u;
        if (r < P.n_runs) P.start[r] = w * 32u + b;
        ++r;
    }
}

// one lane per run; every lane stays alive (the ballot)
__global__ void __launch_bounds__(COLOR_THREADS) k_color_runs(ColorRunParams P) {
    const uint64_t r = (uint64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
    bool single = false;
    if (r < P.n_runs) {
        const uint64_t g = P.start[r], end = r + 1 < P.n_runs ? P.start[r + 1] : P.n_pos;
        const uint64_t lo = last_le(P.kmer_off, 0, P.n_unitigs, g);   // the unitig of position g
        const uint32_t o = (uint32_t)(g - P.kmer_off[lo]), n = (uint32_t)(end - g);
        P.offset[r] = o; P.len[r] = n;
        if (o == 0u) { P.run_off[lo] = r; single = n == P.unitig_len[lo] - (uint32_t)P.k + 1u; }
        if (r == 0) P.run_off[P.n_unitigs] = P.n_runs;
    }
    const uint64_t ns = (uint64_t)__popcll(__ballot(single));
    if ((threadIdx.x & 63) == 0 && ns) atomic_add_u64(&P.out[1], ns);
}

struct ColorClassParams {
    const uint32_t* planes; uint64_t n_words; uint32_t n_colors, nw;   // nw = ceil(n_colors / 32): words per class row
    const uint64_t* start; const uint32_t* len; uint64_t n_runs;
    uint64_t* slots; uint64_t mask;     // the class table: a run index per slot, COLOR_EMPTY
    uint64_t* where;                    // [n_runs]      the slot of every run's colour set (k_color_insert)
    uint32_t* rep;                      // [n_runs]      the first run of its class (k_color_rep)
    uint32_t* cls;                      // [n_runs]      the representative flag first (k_color_rep), the class in the end (k_color_number)
    const uint64_t* rank;               // [n_runs + 1]  exclusive scan of the flags; rank[n_runs] = classes
    uint64_t n_classes;
    uint32_t* c_rep; uint64_t* c_runs; uint64_t* c_kmers; uint32_t* c_ncol; uint32_t* c_bits;   // [n_classes] each, c_bits [n_classes][nw]; the three sums zeroed by the host
};

// colours [32 j, 32 j + 32) of position g as a word, colour 32 j in bit 0; the bits behind n_colors are zero
CDBG_DEV uint32_t color_word(const ColorClassParams& P, uint64_t g, uint32_t j) {
    const uint32_t* p = P.planes + (uint64_t)j * 32u * P.n_words + (g >> 5);
    const uint32_t sh = (uint32_t)(g & 31u), n = P.n_colors - j * 32u < 32u ? P.n_colors - j * 32u : 32u;
    uint32_t v = 0;
    for (uint32_t c = 0; c < n; ++c) v |= ((p[(uint64_t)c * P.n_words] >> sh) & 1u) << c;
    return v;
}
CDBG_DEV uint64_t color_hash(const ColorClassParams& P, uint64_t g) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    for (uint32_t j = 0; j < P.nw; ++j) { h = (h ^ (uint64_t)color_word(P, g, j)) * 0xFF51AFD7ED558CCDULL; h ^= h >> 32; }
    h *= 0xC4CEB9FE1A85EC53ULL;
    return h ^ (h >> 29);
}
CDBG_DEV bool color_same(const ColorClassParams& P, uint64_t a, uint64_t b) {
    if (a == b) return true;
    bool same = true;
    for (uint32_t j = 0; j < P.nw && same; ++j) same = color_word(P, a, j) == color_word(P, b, j);
    return same;
}

__global__ void __launch_bounds__(COLOR_THREADS) k_color_insert(ColorClassParams P) {
    const uint64_t r = (uint64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
    if (r >= P.n_runs) return;
    const uint64_t g = P.start[r];
    uint64_t s = color_hash(P, g) & P.mask, probes = 0, at = COLOR_EMPTY;
    bool done;
#pragma clang loop unroll(disable)
    do {                                                    // single exit; the table holds more slots than there are runs
        const uint64_t v = atomic_cas_u64(P.slots + s, COLOR_EMPTY, r);
        bool mine = v == COLOR_EMPTY;
        if (!mine && v < P.n_runs && color_same(P, g, P.start[v])) { (void)atomic_min_u64(P.slots + s, r); mine = true; }
        at = mine ? s : at; done = mine;
        s = (s + 1) & P.mask; ++probes;
    } while (!done && probes <= P.mask);
    P.where[r] = at;
}

__global__ void k_color_rep(ColorClassParams P) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.n_runs) return;
    const uint64_t at = P.where[r];
    const uint64_t v = at <= P.mask ? P.slots[at] : r;      // (a run that found no slot cannot happen; it would be a class of its own, never an access out of bounds)
    const uint32_t rep = v < P.n_runs ? (uint32_t)v : (uint32_t)r;
    P.rep[r] = rep; P.cls[r] = rep == (uint32_t)r ? 1u : 0u;
}

// one lane per run; every lane stays alive (the wave rounds)
__global__ void __launch_bounds__(COLOR_THREADS) k_color_number(ColorClassParams P) {
    const uint64_t r = (uint64_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    bool todo = r < P.n_runs;
    uint32_t c = 0; uint64_t n_pos = 0;
    if (todo) {
        const uint32_t rep = P.rep[r];
        c = (uint32_t)P.rank[rep]; n_pos = P.len[r];
        P.cls[r] = c;
        if (c >= P.n_classes) todo = false;                   // (cannot happen: rank[] is a scan of the flags; never an add out of bounds)
        else if (rep == (uint32_t)r) P.c_rep[c] = (uint32_t)r;
    }
    for (int round = 0; round < COLOR_AGG_ROUNDS; ++round) {
        const uint64_t m = __ballot(todo);
        if (!m) break;                                        // (wave-uniform)
        const int l = __ffsll((long long)m) - 1;
        const uint32_t lc = __shfl(c, l);
        const bool mine = todo && c == lc;
        const uint64_t n = (uint64_t)__popcll(__ballot(mine));
        const uint64_t sp = wave_sum_u64(mine ? n_pos : 0);
        if (lane == l) { atomic_add_u64(&P.c_runs[lc], n); atomic_add_u64(&P.c_kmers[lc], sp); }
        todo = todo && !mine;
    }
    if (todo) { atomic_add_u64(&P.c_runs[c], 1); atomic_add_u64(&P.c_kmers[c], n_pos); }
}

// one lane per (class, word of its row)
__global__ void k_color_gather(ColorClassParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_classes * P.nw) return;
    const uint64_t c = i / P.nw; const uint32_t j = (uint32_t)(i % P.nw);
    const uint32_t r = P.c_rep[c];
    const uint32_t v = r < P.n_runs ? color_word(P, P.start[r], j) : 0u;
    P.c_bits[i] = v;
    if (v) (void)atomic_add_u32(&P.c_ncol[c], popc_u32(v));
}

}  // namespace cdbg
