// k_window.h -- the walk of a lane over consecutive k-mer windows of a caller's text, shared by every consumer of the index: k_query
// (k_index.h), k_quant (k_quant.h), k_thread_hits (k_thread.h) and k_color_mark (k_color.h).  Included by k_index.h behind index_find,
// which it calls; the four kernels differ in their tile, in whether they extend, and in their SINK: what becomes of a window's answer.
//
// THE CONTRACT, in one place.
//   Text and batches.  The host cuts the caller's bases into batches that overlap by k - 1 bases (host_window.h).  A batch is n_text
//     bytes; the windows that START in [0, n_out) are this batch's -- n_out = n_text for the last batch, n_text - (k - 1) before it -- and
//     those that start in the overlap belong to the next batch: answered there, and only there.
//   Boundaries.  bnd[] holds the sequence ends inside the batch in its own coordinates, ascending and distinct, closed by n_text.  A lane
//     finds the first end behind its first position by binary search and advances from there; a window at g is inside one sequence when
//     g + k <= seq_end.
//   ok_from.  The tile and a k - 1 halo are staged as codes 0 .. 3, 0xFF for a byte outside ACGTacgt or behind the batch.  0xFF enters
//     the rolled k-mers as 0 and moves ok_from behind it: a window that starts before ok_from holds such a byte.  A window is VALID when
//     it is this batch's, starts at or behind ok_from, and ends inside its sequence.  Only valid windows are counted or looked up.
//   Extension (EXTEND).  A lane that has just found (u, o, strand) answers the next window from ONE arena base: on strand 0 the answer is
//     (u, o + 1) if the unitig goes on (o + 1 <= LN - k) with the window's new base at u[o + k]; on strand 1 it is (u, o - 1) if o >= 1
//     and u[o - 1] is the complement of the new base.  The window before was valid and found, so both lie in one sequence with no invalid
//     byte between, and the k - 1 bases they share equal the unitig's by induction: the unitig spells the window there -- no hash, no
//     slot, no unaligned k-mer read.  In a set that spells every k-mer once (every built graph) that position is the only one and hence
//     the one a probe reports; in a set with repeated k-mers the neighbour need not be the SMALLEST occurrence, and the host turns
//     extension off (WindowParams::extend, host_window.h).  The state never leaves a lane's run: each run starts with a probe.
//   The sink.  window(p, found, u, o, strand) once per position p of the run, valid or not; fresh(u) before it when the answer came from
//     a probe, so that what a sink keeps per unitig (kmer_off[u]) is loaded once per probe hit, not once per window; finish() behind the
//     run.  Sink::PALINDROME_STRAND0: an extension along strand 1 that lands on a window that is its own reverse complement reports, and
//     goes on from, strand 0 -- the word a probe stores (index_find's compare order).  It is on where hit words leave the kernel and off
//     where only the position counts: there it would change which neighbour the next extension tries.
#pragma once

namespace cdbg {

struct WindowParams {
    const uint8_t* text; uint64_t n_text;   // one batch of the caller's bases
    uint64_t n_out;                         // windows that START in [0, n_out) are this batch's
    const uint32_t* bnd; uint32_t n_bnd;    // the sequence ends inside the batch, ascending; the last one is n_text
    int k; int extend;
    const uint8_t* packed; const uint64_t* unitig_off; const uint32_t* unitig_len; const uint64_t* kmer_off;
    const uint64_t* slots; uint64_t mask;
    uint64_t* out;                          // the kernel's counters
};

// what a lane's run saw: valid windows, those found, those of them answered by extension, slots read
struct WindowTally { uint64_t windows, found, extended, probes; };

// the tile at tile0 and its k - 1 halo as codes: 0 .. 3, 0xFF for a byte outside ACGTacgt (or behind the batch)
template <int TILE, int THREADS>
CDBG_DEV void window_stage(const WindowParams& P, uint64_t tile0, uint8_t (&code)[TILE + QUERY_HALO]) {
    for (int i = (int)threadIdx.x; i < TILE + P.k - 1; i += THREADS) {
        const uint64_t g = tile0 + (uint64_t)i;
        const uint32_t c = g < P.n_text ? P.text[g] : (uint32_t)'\n';
        code[i] = base_valid(c) ? (uint8_t)base_code(c) : (uint8_t)0xFF;
    }
}

// one lane's run: positions [threadIdx.x * RUN, + RUN) of the staged tile
template <int W, int RUN, bool EXTEND, class Sink>
CDBG_DEV WindowTally window_walk(const WindowParams& P, uint64_t tile0, const uint8_t* code, Sink& sink) {
    const int k = P.k, p0 = (int)threadIdx.x * RUN;
    WindowTally t = { 0, 0, 0, 0 };
    if (tile0 + (uint64_t)p0 >= P.n_out) return t;
    uint32_t lo = 0, hi = P.n_bnd - 1;                       // the first sequence end behind p0 (bnd[n_bnd - 1] = n_text is one)
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)P.bnd[mid] > tile0 + (uint64_t)p0) hi = mid; else lo = mid + 1; }
    uint32_t bi = lo; uint64_t seq_end = P.bnd[bi];
    int ok_from = p0;                                       // windows that start before it hold an invalid byte
    Kmer<W> fw = Kmer<W>::zero();
    for (int j = p0; j < p0 + k - 1; ++j) {
        uint32_t c = code[j];
        if (c == 0xFFu) { ok_from = j + 1; c = 0; }
        fw.push_right(k, c);
    }
    Kmer<W> rc = fw.rc(k);                                  // once per run (of 'A' + the first k - 1 bases: the roll below drops the A's complement)
    // the latest hit: its unitig, the arena offset of that unitig, its k-mer positions, the offset in it, the strand
    bool have = false; uint64_t u = 0, u_base = 0; uint32_t u_npos = 0, o = 0, strand = 0;
    for (int i = 0; i < RUN; ++i) {
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
            ++t.windows;
            if constexpr (EXTEND) {
                if (have) {                                 // (the window before this one was valid and found)
                    if (strand == 0) { if (o + 1u < u_npos && packed_base(P.packed, u_base + o + (uint64_t)k) == c) { ++o; found = true; } }
                    else if (o >= 1u && packed_base(P.packed, u_base + o - 1u) == 3u - c) {
                        --o; found = true;
                        if (Sink::PALINDROME_STRAND0 && fw == rc) strand = 0;   // the unitig reads there as the window itself, and a probe says so
                    }
                    t.extended += found ? 1u : 0u;
                }
            }
            if (!found) {
                uint64_t probes;
                const uint64_t at = index_find<W>(fw, rc, k, P.packed, P.unitig_off, P.slots, P.mask, strand, probes);
                t.probes += probes;
                if (at != INDEX_EMPTY) {
                    u = at >> 32; o = (uint32_t)at; found = true;
                    if constexpr (EXTEND) { u_base = P.unitig_off[u]; u_npos = P.unitig_len[u] - (uint32_t)k + 1u; }
                    sink.fresh(u);
                }
            }
            t.found += found ? 1u : 0u;
        }
        sink.window(p, found, u, o, strand);
        if constexpr (EXTEND) have = found && P.extend != 0;
    }
    sink.finish();
    return t;
}

// the sink of the two kernels whose answer is a hit word per position, staged in LDS for a coalesced store
template <bool PALINDROME>
struct HitWordSink {
    static constexpr bool PALINDROME_STRAND0 = PALINDROME;
    uint64_t* hit;                                          // [tile]
    CDBG_DEV void fresh(uint64_t) {}
    CDBG_DEV void window(int p, bool found, uint64_t u, uint32_t o, uint32_t strand) {
        hit[p] = found ? ((u << 33) | ((uint64_t)o << 1) | (uint64_t)strand) : INDEX_EMPTY;
    }
    CDBG_DEV void finish() {}
};

// the staged hit words of a tile to hits[tile0 ..), one 8-byte store per position
template <int TILE, int THREADS>
CDBG_DEV void window_store_hits(const uint64_t* hit, uint64_t tile0, uint64_t n_out, uint64_t* hits) {
    for (int i = (int)threadIdx.x; i < TILE; i += THREADS) {
        const uint64_t g = tile0 + (uint64_t)i;
        if (g < n_out) hits[g] = hit[i];
    }
}

}  // namespace cdbg
