"""A read set counted against the resident unitigs on the device: the cases of quant_cases.py (as test_hostsim_quant.py runs them on the
simulator) on poisoned memory, and the race check the simulator cannot make (its atomics are plain): one mid-size graph whose own
reads must reproduce the count stage's abundances at every position."""
import itertools
import os

import pytest

import kwidth_cases as kc
import quant_cases as qn

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
    qn.key_width(hip, k, amin)


@pytest.mark.parametrize("k", [31, 64])
def test_boundaries(hip, k):
    qn.boundaries(hip, k)


def test_batches(hip, monkeypatch):
    qn.batches(hip, monkeypatch)


@pytest.mark.parametrize("k", [8, 31])
def test_extension_edges(hip, monkeypatch, k):
    qn.extension_edges(hip, monkeypatch, k)


def test_repeated_handmade_three_runs(hip):
    """the same set indexed and counted three times in one process: which lane wins a slot differs, the fetched bytes must not"""
    qn.repeated_handmade(hip, runs=3)


def test_ceiling_and_clamp(hip, monkeypatch):
    qn.ceiling(hip, monkeypatch)


def test_state(hip):
    qn.state(hip)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(hip, tmp_path, name, k):
    import bcalm_amd
    qn.cli(os.path.join(os.path.dirname(bcalm_amd.api.DEFAULT_LIB), "bcalm"), tmp_path, name, k)


def test_mid_size(hip):
    """generate_reads(200000, 150, 3), k = 31, abundance-min 2, all_abundance_counts: the whole resident text quantified in one call must
    give, at every position, the abundance the count stage found -- real atomics from thousands of waves against the build's numbers"""
    import bcalm_amd
    k, n_reads = 31, 200000
    g = bcalm_amd.Graph(k, 2, lib=hip, all_abundance_counts=True)
    try:
        g.generate_reads(n_reads, 150, 3); g.run()
        text = g.read_text(0, n_reads * 151)
        reads = text.split(b"\n")
        valid = sum(len(p) - k + 1 for r in reads for p in r.upper().replace(b"N", b" ").split() if len(p) >= k)
        assert all(set(r.upper()) <= set(b"ACGTN") for r in reads[:1000])
        r = g.quantify(reads)
        print("mid-size: windows %d found %d extended %d (%.4f of found)" % (r["windows"], r["found"], r["extended"], r["extended"] / r["found"]))
        kcs, cov, ab, off = g.quant_raw()
        n = len(off) - 1
        units = g.unitigs()
        exp = g.unitig_abundances()
        assert n == len(exp) == len(units)
        assert list(off) == [0] + list(itertools.accumulate(len(e) for e in exp))
        pos = 0
        for u, e in enumerate(exp):
            assert ab[pos:pos + len(e)] == e, u
            assert kcs[u] == units[u][1] == sum(e) and cov[u] == len(e), u
            pos += len(e)
        assert r["found"] == g.digest()["kc_sum"] > 0
        assert r["windows"] == valid > r["found"]
        assert r["extended"] > 0.5 * r["found"]
    finally:
        g.close()
