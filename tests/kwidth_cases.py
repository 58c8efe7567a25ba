"""Inputs and case tables for the sweep over every k-mer width and minimizer window (test_hostsim_kwidth.py, test_gpu_kwidth.py).

Every kernel is a template over the key width W = k / 32 + 1, and the host picks kernels and table geometries by W, by k and by
the minimizer window WN = k - m.  The tables below follow that structure:

  * K_EDGES: for every W the k at both ends of its span -- the three shift branches of Kmer<W>::rc (s = 64 W - 2 k: 2 at
    k = 32 W - 1, 64 at k = 32 (W - 1), 66 for the junctions of that k) -- and two k inside it, on edge_text: small reads with the
    shapes that go wrong at a word edge (palindromes, reads of k - 1 / k / k + 1 bases, N, a circle, low complexity);
  * PARTITIONINGS: (abundance-min, log2 partitions) under which K_EDGES runs;
  * LADDER: for every W one partition so full that count and compaction walk through all their tiers;
  * window_cases(): every minimizer window 1 .. 126 and the points where the scan changes kernel, on tile_edge_text: read breaks
    at every distance from the scan's tile edges that a halo rule could get wrong.

The simulator test proves from the launch trace of the simulator build which kernels a case reached; the GPU test runs the same
inputs: partitioning, classification and the choice of kernels are the same host code."""
import random

from test_step_state import _sift_text, _tier_text

COMP = str.maketrans("ACGT", "TGCA")


def _rc(s):
    return s[::-1].translate(COMP)


def words(k):
    return k // 32 + 1


# ---- word-edge k ----
def _k_edges():
    out = [3, 4, 5, 15, 16, 30, 31]
    for w in range(2, 9):
        lo = 32 * (w - 1)
        out += [lo, lo + 1, lo + 15, lo + 16, lo + 30, lo + 31]
    return out


K_EDGES = _k_edges()
assert {192, 193, 222, 223, 224, 225, 254, 255} <= set(K_EDGES) and all(2 < k < 256 for k in K_EDGES)

# (abundance-min, log2 partitions; -1: the library chooses from the input volume)
PARTITIONINGS = [(1, 0), (2, 3), (1, -1)]


def edge_text(k, seed):
    """a few kB of reads of a small genome, with the shapes that go wrong at the edge of a key word"""
    rng = random.Random(1000 * seed + k)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    x = rnd(k + 9)                                           # inverted repeat, longer than k
    g = rnd(2 * k + 200) + x + rnd(2 * k + 200) + _rc(x) + rnd(2 * k + 180)
    reads = []
    for _ in range(30):                                      # both strands, k .. 3 k + 200 bases, 0.4 % substitutions
        L = rng.randrange(k, 3 * k + 201); s = rng.randrange(0, len(g) - L + 1)
        r = g[s:s + L]
        if rng.random() < 0.5:
            r = _rc(r)
        reads.append("".join((rng.choice("ACGT") if rng.random() < 0.004 else c) for c in r))
    h = rnd(k // 2)
    pal = h + _rc(h)                                         # even k: a k-mer that is its own reverse complement; odd k: such a (k-1)-junction
    reads += [rnd(k) + pal + rnd(k), rnd(3) + pal, pal + rnd(2), pal]
    s = rng.randrange(0, len(g) - k - 1)
    reads += [g[s:s + k - 1], g[s + 1:s + 1 + k], g[s:s + k + 1]]
    s = rng.randrange(0, len(g) - 3 * k - 1)
    reads.append(g[s:s + k + 3] + "N" + g[s + k + 3:s + 2 * k + 1] + "N" + g[s + 2 * k + 1:s + 3 * k + 1])   # pieces of k + 3, k - 2 and k
    c = rnd(k + 41)
    reads.append(c + c[:k - 1])                              # a circle
    reads += [("ACG" * k)[:2 * k + 5], "A" * (k + 20)]
    return "\n".join(reads) + "\n"


def minimizer_of(k, log_np):
    """configure() of host_ctx.h: the minimizer length the library picks for this partition count"""
    return max(1, min(min(16, max(6, (log_np + 10) // 2 + 1)), 16, k - 1))


# ---- one full partition per W: every count and compaction tier ----
def ladder_text(k, glen):
    """one genome of glen distinct k-mers (the generator of test_count_tiers), for log2_partitions = 0"""
    return _tier_text(k, glen)


def sift_text(k):
    """mostly once-seen k-mers in one partition under abundance-min 2 (test_count_sift_tier, "sifted")"""
    return _sift_text(k)


# launch texts of the simulator trace (the kernel as the host code names it)
T_COUNT1 = "(k_count_fast<W, TS, Cfg<W>::NTC, false>)"
T_COUNT2 = "(k_count_fast<W, 2 * TS, NT2, 2>)"
T_SIFT = "(k_count_fast<W, TSS, NTS, 2, FSS>)"
T_MULTI = "(k_count<W, TSG, NTG, false>)"
T_HBM = ["k_big_clear<W>", "k_big_insert<W>", "(k_big_sweep<W, 0>)", "(k_big_sweep<W, 1>)"]
T_WAVE1 = "(k_compact_wave<W, Cfg<W>::TSW>)"
T_WAVE2 = "(k_compact_wave<W, Cfg<W>::TSW2>)"
T_WAVE3 = "(k_compact_wave<W, 1024>)"
T_WG1 = "(k_compact<W, TS, false>)"
T_WG2 = "(k_compact<W, Cfg<W>::TSK2, false>)"
T_SPLIT = "(k_split_buckets<W>)"
T_CHBM = "(k_compact<W, TS, true>)"


def ladder_tiers(w):
    """every tier that exists for keys of w words: the union of the launch texts of its ladder rows"""
    t = [T_COUNT1, T_MULTI] + T_HBM + [T_WAVE1, T_WAVE2, T_WG1, T_WG2, T_SPLIT, T_CHBM]
    if w <= 4:
        t.append(T_COUNT2)
    if w >= 3:
        t.append(T_SIFT)
    if 2 <= w <= 4:
        t.append(T_WAVE3)
    return t


# One partition (log2_partitions = 0) per row: (k, abundance-min, glen -- 0: sift_text(k) --, environment, {statistic: lower bound}).
# Per width, k = 32 W - 9 and
#   * the full partition: the smallest glen (in steps of 500) at which the simulator's trace shows tier 1, the second tier (W <= 4) AND the
#     multi-pass kernel for the count, and for the compaction both wave tiers, the 1024-slot tier (W 2 .. 4), k_compact at TS and TSK2 and the
#     split, was 6000 (W = 1), 3500 (W 2 .. 4) and 1000 .. 1200 (W >= 5); the rows take a quarter more, because which tier gives a partition up
#     next to a table's limit may depend on the order its records arrive in on the device (test_count_sift_tier_gpu);
#   * the same partition with one LDS pass allowed and without the split: what then does not fit goes to the tables in HBM, of the count
#     (k_big_*) and of the compaction (k_compact<W, TS, true>) -- W >= 5: from 2000 k-mers, more than one pass of the multi-pass kernel's 2048
#     slots, hence 3000 in both rows.  Without the knobs the count reaches them beyond 16 passes -- from 25 000
#     distinct k-mers for W >= 5 and 70 000 for W = 1: minutes on the simulator for the eight widths;
#   * W >= 3: the sifting tier under abundance-min 2.
# Only lower bounds: tier COUNTS next to a limit depend on arrival order.
_FULL = {1: 7500, 2: 4500, 3: 4500, 4: 4500, 5: 3000, 6: 3000, 7: 3000, 8: 3000}
HBM_ENV = {"CDBG_MAX_PASSES": "1", "CDBG_NO_SPLIT": "1"}
LADDER = []
for _w in range(1, 9):
    _k = 32 * _w - 9
    LADDER.append((_k, 1, _FULL[_w], {}, {"n_multipass_partitions": 1, "n_split_buckets": 1}))
    LADDER.append((_k, 1, _FULL[_w], HBM_ENV, {"n_multipass_partitions": 1, "n_big_partitions": 2}))
    if _w >= 3:
        LADDER.append((_k, 2, 0, {}, {}))


def ladder_id(row):
    return "k%d-amin%d-%s%s" % (row[0], row[1], row[2] or "sift", "-hbm" if row[3] else "")


def ladder_input(row):
    k, amin, glen, _, _ = row
    return ladder_text(k, glen) if glen else sift_text(k)


def check_bounds(st, bounds):
    for name, lo in bounds.items():
        assert st[name] >= lo, (name, st[name], lo)


# ---- minimizer windows ----
SCANF_WNMAX = 48


def scan_is_fast(k, m):
    """host_count.h: the register-window scan (tiles of 4064 junctions) or the generic one (4096)"""
    wn = k - m
    return (k <= 63 and wn <= SCANF_WNMAX) or (k <= 127 and wn > SCANF_WNMAX and wn >= 17)


def scan_tile(k, m):
    return 4064 if scan_is_fast(k, m) else 4096


def scan_variant(k, m):
    """the launch text of the scan kernel that launch_scan_mode picks"""
    wn, w = k - m, words(k)
    if not scan_is_fast(k, m):
        return "(k_scan<W, MODE>)"
    if wn > SCANF_WNMAX:
        return "(k_scan_fast<W, MODE, -1>)"                  # two-level window
    if w == 1 and 15 <= wn <= 19:
        return "(k_scan_fast<W, MODE, W == 1 ? %d : 0>)" % wn
    if w == 2 and wn == 39:
        return "(k_scan_fast<W, MODE, W == 2 ? 39 : 0>)"
    return "(k_scan_fast<W, MODE, 0>)"


WINDOW_SWEEP = [(wn + min(16, (63 if wn <= SCANF_WNMAX else 127) - wn), min(16, (63 if wn <= SCANF_WNMAX else 127) - wn)) for wn in range(1, 127)]
# the compile-time windows 15 .. 19 of one-word k-mers (the sweep above reaches 16 .. 19 with two words) and both neighbours of each
# compile-time window, with one and with two words
WINDOW_NEIGHBOURS = [(31, 16), (31, 15), (31, 14), (31, 13), (31, 12), (55, 16), (30, 16), (31, 11), (36, 16), (54, 16), (56, 16), (55, 15)]
WINDOW_GENERIC = [(64, 16), (128, 16), (128, 1), (191, 8), (223, 16), (255, 16), (255, 1)]


def window_cases():
    seen = set()
    for km in WINDOW_SWEEP + WINDOW_NEIGHBOURS + WINDOW_GENERIC:
        if km not in seen:
            seen.add(km)
            yield km


def tile_edge_distances(k, m):
    return [-k - 1, -k, -k + 1, -(k - m), -m, -17, -16, -15, -1, 0, 1, 15, 16, 17, m, k]


def tile_edge_text(k, m, first=0, n=16):
    """n scan tiles of random bases with a read break at byte T j + d for j = 1 .. n: T is the tile of the scan kernel chosen for (k, m),
    d one of the sixteen distances above per tile edge (from distance number `first` on; the device runs all sixteen, the simulator four
    per case, rotated); the breaks alternate between a newline and an N.  Behind the tiles, the reverse complement of the stretch across
    every tile edge as a read of its own: a k-mer next to an edge that the scan sent to the wrong partition is then counted in two
    places.  No newline at the end"""
    T = scan_tile(k, m)
    rng = random.Random(1000 * k + m)
    t = [rng.choice("ACGT") for _ in range(n * T + 2 * k + 40)]
    clean = "".join(t)
    ds = tile_edge_distances(k, m)
    for j in range(1, n + 1):
        t[T * j + ds[(first + j - 1) % 16]] = "\n" if j & 1 else "N"
    again = [_rc(clean[T * j - k - 20:T * j + k + 20]) for j in range(1, n + 1)]
    return "".join(t) + "\n" + "\n".join(again)
