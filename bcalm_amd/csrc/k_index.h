// k_index.h -- node lookup in the resident unitig set: where is this k-mer (which unitig, which offset, which strand), or is it not in the
// graph at all (cdbg_index / cdbg_query of include/cdbg.h; the `bcalm -query` mode).
//
// THE ARENA IS THE KEY STORE.  The index is one open-address table in HBM of 64-bit slots that hold POSITIONS, not keys: a slot value is
// (unitig << 32) | offset, UINT64_MAX is empty (no position: unitig ids are <= 2^31 - 2), and the key of a slot is the k-mer which the
// resident 2-bit arena (unitig_packed) spells there.  8 bytes per slot for every k from 3 to 255, where a KTable<W> costs 8 W + 4.
//   k_index_insert<W>  every k-mer position of every unitig.  The positions are numbered through the set (an exclusive scan of LN - k + 1),
//                      a lane takes INDEX_RUN consecutive ones -- whatever the unitigs' lengths, k or millions -- and rolls the forward
//                      k-mer and its reverse complement along them.  It hashes the canonical one and probes linearly with a
//                      compare-and-swap of EMPTY against its position; an occupant's k-mer is read from the arena and compared with the
//                      lane's two k-mers: the same k-mer -> atomic minimum of the two positions, another -> next slot.  Insert-only
//                      linear probing makes equal k-mers meet in ONE slot, whichever arrives first, and an occupied slot never changes
//                      its k-mer: no pending state, no key to publish.  Which k-mer ends in which slot depends on the arrival order,
//                      what a lookup returns does not: a built graph spells every k-mer once, a loaded set may repeat k-mers and the
//                      slot then holds the SMALLEST (unitig, offset) of the occurrences.
//   index_find<W>      the read-only probe of every consumer: hash the canonical one of a window's two k-mers, then compare every occupant
//                      with the forward k-mer (strand 0) and its reverse complement (strand 1) until a hit or an empty slot.
//   k_query<W>         the window walker (k_window.h) over tiles of QUERY_TILE positions, QUERY_RUN per lane, without extension, with
//                      the hit-word sink: the words go through LDS and leave as coalesced 8-byte stores, one per position.
// The arena is little-endian by base (base j = bits 2 (j & 3) of byte j >> 2), Kmer<W> keeps the first base in its highest bits:
// packed_kmer() is the one place that turns one into the other, at any 2-bit alignment.
#pragma once
#include "k_verify.h"

namespace cdbg {

constexpr int INDEX_THREADS = 256;
constexpr int INDEX_RUN = 32;                       // consecutive k-mer positions per lane of the insert
constexpr int QUERY_THREADS = 256;
constexpr int QUERY_RUN = 16;                       // consecutive query positions per lane
constexpr int QUERY_TILE = QUERY_THREADS * QUERY_RUN;
constexpr int QUERY_HALO = 256;                     // >= k - 1 for every k the library takes
constexpr uint64_t INDEX_EMPTY = ~0ULL;

CDBG_DEV uint32_t packed_base(const uint8_t* arena, uint64_t j) { return ((uint32_t)arena[j >> 2] >> (2u * (uint32_t)(j & 3))) & 3u; }

// the k-mer that starts at base `pos` of a 2-bit arena.  Reads whole 64-bit words from the k-mer's first byte on, and only those that
// hold a base of it: at most 7 bytes beyond its last byte (the arena carries 16 bytes of slack behind its last chunk, pack_unitigs).
template <int W>
CDBG_DEV Kmer<W> packed_kmer(const uint8_t* arena, uint64_t pos, int k) {
    const uint8_t* const p = arena + (pos >> 2);
    const int sh = 2 * (int)(pos & 3), bits = sh + 2 * k;
    uint64_t r[W + 1];
#pragma unroll
    for (int i = 0; i <= W; ++i) r[i] = (64 * i < bits) ? ld_unaligned_u64(p + 8 * i) : 0ULL;
    // base t of the k-mer at bits 2 t (little-endian), then the order of the 2-bit groups reversed over the W words and the
    // 64 W - 2 k bits below the k-mer shifted out: the three shift branches of Kmer<W>::rc, without the complement
    Kmer<W> t;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const uint64_t lo = r[W - 1 - i], hi = r[W - i];
        t.w[i] = rev2(sh ? ((lo >> sh) | (hi << (64 - sh))) : lo);
    }
    const int s = 64 * W - 2 * k;                    // 2 .. 64 under the span rule 32 (W - 1) <= k < 32 W
    Kmer<W> x;
    if (s < 64) {
#pragma unroll
        for (int i = 0; i < W; ++i) x.w[i] = (t.w[i] >> s) | (i + 1 < W ? t.w[i + 1 < W ? i + 1 : 0] << (64 - s) : 0ULL);
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) x.w[i] = i + 1 < W ? t.w[i + 1 < W ? i + 1 : 0] : 0ULL;
    }
    return x;
}

// slot of a canonical k-mer: every word through mix64 (as verify_mix), 64 bits -- the table of a config-3 graph has more than 2^31 slots
template <int W>
CDBG_DEV uint64_t index_hash(const Kmer<W>& c) {
    uint64_t h = 0x13198A2E03707344ULL;
#pragma unroll
    for (int i = 0; i < W; ++i) h = mix64(h ^ c.w[i]);
    return h;
}

// the last i in [lo, hi) with off[i] <= g (lo when there is none): the unitig of a k-mer position in kmer_off[], the run of a segment in a scan
template <class T>
CDBG_DEV uint64_t last_le(const T* off, uint64_t lo, uint64_t hi, T g) {
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

struct IndexParams {
    uint64_t n_unitigs; int k;
    const uint64_t* unitig_off; const uint32_t* unitig_len; const uint8_t* packed;
    uint32_t* kcount;              // [U]      LN - k + 1
    const uint64_t* kmer_off;      // [U + 1]  exclusive scan of kcount: the first k-mer position of every unitig in the set's numbering
    uint64_t n_pos;                // P = kmer_off[U]
    uint64_t* slots; uint64_t mask;
    uint64_t* out;                 // [0] positions inserted  [1] slots claimed (distinct k-mers)  [2] positions that found no slot (must be 0)
};

__global__ void k_index_lens(IndexParams P) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < P.n_unitigs) { const uint32_t n = P.unitig_len[u]; P.kcount[u] = n >= (uint32_t)P.k ? n - (uint32_t)P.k + 1u : 0u; }
}

template <int W>
__global__ void k_index_insert(IndexParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * INDEX_RUN;
    uint64_t n_ins = 0, n_new = 0, n_lost = 0;
    for (uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * INDEX_RUN; first < P.n_pos; first += stride) {
        const uint64_t end = first + INDEX_RUN < P.n_pos ? first + INDEX_RUN : P.n_pos;
        uint64_t u = last_le(P.kmer_off, 0, P.n_unitigs, first), g = first;   // the unitig of position `first`
        while (g < end) {
            const uint64_t k0 = P.kmer_off[u], k1 = P.kmer_off[u + 1];
            if (g >= k1) { ++u; continue; }
            const uint64_t o = g - k0, take = (end - g < k1 - g) ? end - g : k1 - g;
            const uint64_t a = P.unitig_off[u] + o;                // arena position of the run's first k-mer
            Kmer<W> fw = packed_kmer<W>(P.packed, a, P.k);
            Kmer<W> rc = fw.rc(P.k);                               // once per run: the positions behind it roll both strands
            for (uint64_t t = 0; t < take; ++t) {
                if (t) { const uint32_t b = packed_base(P.packed, a + t + (uint64_t)(P.k - 1)); fw.push_right(P.k, b); rc.push_left(P.k, 3u - b); }
                const uint64_t v = (u << 32) | (o + t);
                uint64_t s = index_hash<W>(rc < fw ? rc : fw) & P.mask, probes = 0;
                bool done, mine;
                // single exit (see ktable_insert); an occupant is a position of SOME k-mer and stays one of the same k-mer for good
#pragma clang loop unroll(disable)
                do {
                    const uint64_t old = atomic_cas_u64(&P.slots[s], INDEX_EMPTY, v);
                    mine = old == INDEX_EMPTY;
                    bool same = false;
                    if (!mine) {
                        const Kmer<W> x = packed_kmer<W>(P.packed, P.unitig_off[old >> 32] + (old & 0xFFFFFFFFULL), P.k);
                        same = (x == fw) | (x == rc);
                        if (same) (void)atomic_min_u64(&P.slots[s], v);
                    }
                    done = mine | same;
                    s = done ? s : ((s + 1) & P.mask); ++probes;
                } while (!done && probes <= P.mask);
                ++n_ins; n_new += mine ? 1u : 0u; n_lost += done ? 0u : 1u;
            }
            g += take; ++u;
        }
    }
    n_ins = wave_sum_u64(n_ins); n_new = wave_sum_u64(n_new); n_lost = wave_sum_u64(n_lost);
    if ((threadIdx.x & 63) == 0 && n_ins) { atomic_add_u64(&P.out[0], n_ins); atomic_add_u64(&P.out[1], n_new); if (n_lost) atomic_add_u64(&P.out[2], n_lost); }
}

// where the table holds the window whose strands are fw and rc: the slot value (unitig << 32 | offset) or INDEX_EMPTY, the strand it
// matched on (a k-mer that is its own reverse complement: strand 0), and the slots read.  Read-only; k_index_insert's CAS loop is its own.
template <int W>
CDBG_DEV uint64_t index_find(const Kmer<W>& fw, const Kmer<W>& rc, int k, const uint8_t* packed, const uint64_t* unitig_off,
                             const uint64_t* slots, uint64_t mask, uint32_t& strand, uint64_t& probes) {
    uint64_t s = index_hash<W>(rc < fw ? rc : fw) & mask, n = 0, at = INDEX_EMPTY;
    bool done, rev = false;
#pragma clang loop unroll(disable)
    do {                                                    // single exit; the table holds at least one empty slot
        const uint64_t v = slots[s];
        bool f = false, r = false;
        if (v != INDEX_EMPTY) {
            const Kmer<W> x = packed_kmer<W>(packed, unitig_off[v >> 32] + (v & 0xFFFFFFFFULL), k);
            f = x == fw; r = !f && x == rc;
        }
        at = (f | r) ? v : at; rev = r;
        done = (v == INDEX_EMPTY) | f | r;
        s = (s + 1) & mask; ++n;
    } while (!done && n <= mask);
    strand = rev ? 1u : 0u; probes = n;
    return at;
}

}  // namespace cdbg

#include "k_window.h"                                       // (needs everything above; k_query below needs it)

namespace cdbg {

struct QueryParams : WindowParams {         // out: (CDBG_PROFILE_PHASES builds) [0] k-mers looked up  [1] slots read
    uint64_t* hits;                         // [n_out]
};

template <int W>
__global__ void k_query(QueryParams P) {
    CDBG_SHARED uint8_t code[QUERY_TILE + QUERY_HALO];
    CDBG_SHARED uint64_t hit[QUERY_TILE];
    const uint64_t tile0 = (uint64_t)blockIdx.x * QUERY_TILE;
    window_stage<QUERY_TILE, QUERY_THREADS>(P, tile0, code);
    __syncthreads();
    HitWordSink<false> sink{ hit };
    const WindowTally t = window_walk<W, QUERY_RUN, false>(P, tile0, code, sink);
    __syncthreads();
    window_store_hits<QUERY_TILE, QUERY_THREADS>(hit, tile0, P.n_out, P.hits);
#if defined(CDBG_PROFILE_PHASES) && !defined(CDBG_HOSTSIM)
    const uint64_t n_q = wave_sum_u64(t.windows), n_probe = wave_sum_u64(t.probes);
    if ((threadIdx.x & 63) == 0 && n_q) { atomic_add_u64(&P.out[0], n_q); atomic_add_u64(&P.out[1], n_probe); }
#else
    (void)t;
#endif
}

}  // namespace cdbg
