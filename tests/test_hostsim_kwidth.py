"""Every k-mer width and every minimizer window on the simulator (CPU suite): the cases of kwidth_cases.py that test_gpu_kwidth.py
runs on the device, in the subset that keeps this suite quick -- every word-edge k under one of the three partitionings (rotated,
so that every width sees all three), every ladder row, every fifth window (all sixteen unrolled cases of the two-level window
among them) with those whose halo ends on a chunk edge, and every point where the scan changes kernel.

Every case goes through test_step_state.run_case with links and abundances: (k-mer, count) set, canonical unitigs with KC, the
digest formula, the device-side verification with edges, brute-force links and per-k-mer abundances, all against the oracle.
The simulator's launch trace (CDBG_SIM_TRACE, tests/hostsim/hostsim.h) proves what the tables of kwidth_cases.py claim: which
scan kernel a (k, m) pair gets, and that the ladder rows of a width walk through every count and compaction tier it has."""
import collections

import pytest

import hostsim_lib
import kwidth_cases as kc
from test_step_state import run_case


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture
def trace(monkeypatch, tmp_path):
    """the launch texts of everything the test runs -> {text: launches}, read when called"""
    tf = tmp_path / "launches.trace"
    monkeypatch.setenv("CDBG_SIM_TRACE", str(tf))

    def read():
        return collections.Counter(line.rsplit(",", 2)[0] for line in open(tf))
    return read


def check_shape(st, k, m=0):
    assert st["kmer_words"] == kc.words(k), st
    assert st["minimizer_size"] == (m or kc.minimizer_of(k, st["log2_partitions"])), st


@pytest.mark.parametrize("k", kc.K_EDGES)
def test_word_edge_k(oracle, sim, k):
    amin, log_np = kc.PARTITIONINGS[kc.K_EDGES.index(k) % len(kc.PARTITIONINGS)]
    st = run_case(oracle, sim, kc.edge_text(k, 1), k, amin, links=True, abundances=True, log2_partitions=log_np)
    check_shape(st, k)


@pytest.mark.parametrize("w", range(1, 9))
def test_ladder_reaches_every_tier(oracle, sim, trace, w):
    rows = [r for r in kc.LADDER if kc.words(r[0]) == w]
    assert rows
    for row in rows:
        k, amin, glen, env, bounds = row
        with pytest.MonkeyPatch.context() as mp:
            for name, val in env.items():
                mp.setenv(name, val)
            st = run_case(oracle, sim, kc.ladder_input(row), k, amin, links=True, abundances=True, log2_partitions=0)
        check_shape(st, k)
        kc.check_bounds(st, bounds)
    seen = trace()
    missing = [t for t in kc.ladder_tiers(w) if not seen[t]]
    assert not missing, (missing, sorted(seen))


# every fifth window, and the windows of 1, 17 .. 113 keys: the last key of a tile's last window is the first of a 16-key chunk of the halo there
SIM_WINDOWS = [km for i, km in enumerate(kc.WINDOW_SWEEP) if i % 5 == 0 or i % 16 == 0] + kc.WINDOW_NEIGHBOURS + kc.WINDOW_GENERIC
# (windows 51, 56 .. 126: one for each of the sixteen cases R = (WN - 1) & 15 of the two-level window)
assert {(k - m - 1) & 15 for k, m in SIM_WINDOWS if k - m > kc.SCANF_WNMAX and k <= 127} == set(range(16))
assert set(SIM_WINDOWS) <= set(kc.window_cases())


@pytest.mark.parametrize("i,k,m", [(i, k, m) for i, (k, m) in enumerate(SIM_WINDOWS)])
def test_minimizer_windows_across_tile_edges(oracle, sim, trace, i, k, m):
    text = kc.tile_edge_text(k, m, first=4 * i, n=4)         # (four tile edges per case: case i takes the distances 4 i .. 4 i + 3)
    st = run_case(oracle, sim, text, k, 1, links=True, abundances=True, log2_partitions=5, minimizer_size=m)
    check_shape(st, k, m)
    scans = {t for t in trace() if t.startswith(("(k_scan<", "(k_scan_fast<"))}
    assert scans == {kc.scan_variant(k, m)}, scans
    assert st["n_launch_scan"] == -(-len(text) // kc.scan_tile(k, m)), st     # (the tile the table assumes)
