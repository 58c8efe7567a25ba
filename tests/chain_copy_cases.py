"""Inputs for the tests of k_walk_copy's chunked arena stores (test_hostsim_chain_copy.py, test_gpu_chain_copy.py): a lane collects its
unitig's bytes and stores whole 16-byte-aligned chunks; the ragged ends of the unitig leave as 8-byte stores.

Every case is a row of error-rich texts (glue_batch_cases.rich_text) at abundance-min 1 and must place unitigs at all 16 residues
of `offset % 16` and of `(offset + length) % 16`, and hold a unitig of exactly k bases; a case that does not fails.  The simulator
test also reads the per-piece trace of the simulator build (CDBG_SIM_WALK_TRACE).

Where a unitig lands depends on the order in which workgroups reserve piece ids and arena room.  The simulator runs them in one
order, and there the text of a row's FIRST seed reaches all 32 residues by itself (the simulator test asserts it: 53 .. 243
unitigs).  On the device the order changes from run to run, so the residues of a text of n unitigs are n draws: one of the 16 is
missed with probability 16 * (15/16)^n -- 0.5 for n = 53.  The further seeds of a row bring every case to 300 unitigs and more
(6e-8 per end), and the device test asserts the residues over the row."""
from glue_batch_cases import rich_text

# name -> (k, Graph keywords, genome length, erroneous reads, seeds)
CASES = {
    "k31": (31, dict(log2_partitions=4), 6000, 120, (5, 6)),
    "k32_two_words": (32, dict(log2_partitions=4), 4000, 80, (7, 8)),
    "k21": (21, dict(log2_partitions=3, minimizer_size=16), 1000, 30, (3, 4, 5, 6, 7)),
    "k15_below_one_chunk": (15, dict(log2_partitions=2, minimizer_size=8), 800, 25, (4, 5, 6, 7, 8, 9, 10)),
    "k9": (9, dict(log2_partitions=2, minimizer_size=6), 600, 20, (2, 3, 4, 5, 6, 7, 8)),
    "k8_piecewise_path": (8, dict(log2_partitions=2, minimizer_size=5), 500, 15, (2, 3, 4, 5, 6, 7)),
}
MIN_UNITIGS_PER_ROW = 300

# the two further cases: per-k-mer abundances next to the chunked bases; the walk refused, the ranking path on the same input
ABUNDANCE_CASE = "k21"
RANKING_CASE = "k31"


def texts(name):
    """-> (k, Graph keywords, [text of every seed of the row])"""
    k, kw, glen, nerr, seeds = CASES[name]
    return k, kw, [rich_text(k, glen, s, nerr) for s in seeds]


def assert_dense(off, ln, total):
    """the arena has no hole and no overlap: sorted by offset, every unitig starts where the one before it ends"""
    order = sorted(range(len(off)), key=lambda i: off[i])
    assert order and off[order[0]] == 0
    for a, b in zip(order, order[1:]):
        assert off[b] == off[a] + ln[a], (a, b, off[a], ln[a], off[b])
    assert off[order[-1]] + ln[order[-1]] == total


def assert_conditions(layouts, k):
    """the case reaches what it is in the table for; layouts: [(offsets, lengths)]"""
    heads = {o % 16 for off, _ in layouts for o in off}
    tails = {(o + n) % 16 for off, ln in layouts for o, n in zip(off, ln)}
    assert heads == set(range(16)), sorted(heads)
    assert tails == set(range(16)), sorted(tails)
    assert any(n == k for _, ln in layouts for n in ln), "no unitig of exactly k bases"


def run_case(lib, oracle, text, k, kw, trace=None):
    """parity with the oracle, then the layout of a second run of the same input, every unitig of it from the walk
    (trace: the file that gets the simulator's per-piece trace of that second run) -> (offsets, lengths, stats)"""
    import os
    from bcalm_amd import api
    from parity import assert_parity
    assert_parity(oracle, lib, text, k, 1, **kw)
    g = api.Graph(k, 1, lib=lib, **kw)
    try:
        g.push_text(text)
        if trace is not None:
            os.environ["CDBG_SIM_WALK_TRACE"] = str(trace)
        try:
            g.run()
        finally:
            os.environ.pop("CDBG_SIM_WALK_TRACE", None)
        _, off, ln, _ = g.unitigs_packed()
        st = g.stats()
    finally:
        g.close()
    assert_dense(off, ln, st["unitig_bases"])
    assert st["n_walked_unitigs"] == st["n_unitigs"] == len(off)
    return off, ln, st
