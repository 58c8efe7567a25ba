"""Run-length lookup on the device: the cases of thread_cases.py (as test_hostsim_thread.py runs them on the simulator) on poisoned
memory, and the check the simulator cannot make: thousands of workgroups ranking their heads and tails into one ordered output."""
import os

import pytest

import kwidth_cases as kc
import thread_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_POISON_ALLOC", "0xA5")


@pytest.mark.parametrize("amin", [1, 2])
@pytest.mark.parametrize("k", kc.K_EDGES)
def test_every_key_width(hip, k, amin):
    tc.key_width(hip, k, amin)


@pytest.mark.parametrize("k", [31, 64])
def test_boundaries(hip, k):
    tc.boundaries(hip, k)


def test_long_runs_across_tiles(hip):
    tc.long_runs(hip)


def test_full_density(hip):
    tc.full_density(hip)


@pytest.mark.parametrize("k", [8, 31])
def test_extension_edges(hip, monkeypatch, k):
    tc.extension_edges(hip, monkeypatch, k)


def test_palindrome_cuts_a_reverse_walk(hip, monkeypatch):
    tc.palindrome(hip, monkeypatch)


def test_batches(hip, monkeypatch):
    tc.batches(hip, monkeypatch)


def test_repeated_handmade_three_runs(hip):
    """the same set indexed and threaded three times in one process: which lane wins a slot differs, the fetched bytes must not"""
    tc.repeated_handmade(hip, runs=3)


def test_state(hip):
    tc.state(hip)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(hip, tmp_path, name, k):
    import bcalm_amd
    tc.cli(os.path.join(os.path.dirname(bcalm_amd.api.DEFAULT_LIB), "bcalm"), tmp_path, name, k)


def test_mid_size(hip):
    """generate_reads(200000, 150, 3), k = 31, abundance-min 2: all reads threaded in one call.  found is the graph's KC sum, the lengths
    of the runs add up to it, a read is a handful of runs, and the runs of the first 2000 reads are the fold of g.query() -- which its own
    suite pins against brute force"""
    import bcalm_amd
    k, n_reads = 31, 200000
    g = bcalm_amd.Graph(k, 2, lib=hip)
    try:
        g.generate_reads(n_reads, 150, 3); g.run()
        text = g.read_text(0, n_reads * 151)
        reads = text.split(b"\n")[:n_reads]
        valid = sum(len(p) - k + 1 for r in reads for p in r.upper().replace(b"N", b" ").split() if len(p) >= k)
        tot, run_off, start, place, ln = g.thread_raw(reads)
        print("mid-size: windows %d found %d runs %d extended %d" % (tot["windows"], tot["found"], tot["runs"], tot["extended"]))
        assert tot["found"] == g.digest()["kc_sum"] > 0
        assert tot["windows"] == valid
        assert sum(ln[:tot["runs"]]) == tot["found"]
        assert 0 < tot["runs"] < tot["found"] / 4
        assert list(run_off) == sorted(run_off) and run_off[n_reads] == tot["runs"]
        head = [r.decode() for r in reads[:2000]]
        exp = tc.fold(g.query(head))
        at = 0
        for i, q in enumerate(head):
            got = [(start[r] - at, place[r] >> 33, (place[r] >> 1) & 0xFFFFFFFF, "-" if place[r] & 1 else "+", ln[r]) for r in range(run_off[i], run_off[i + 1])]
            assert got == exp[i], (i, got, exp[i])
            at += len(q)
    finally:
        g.close()
