"""k-mer lookup in the resident unitig set on the device: the cases of query_cases.py (as test_hostsim_query.py runs them on the
simulator) on poisoned memory, the race check the simulator cannot make (its atomics are plain), and one mid-size graph."""
import os

import pytest

import kwidth_cases as kc
import query_cases as qc
import test_relink
from test_links import CASES as LINK_CASES
from test_relink import tools  # noqa: F401  (fixture)

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
def test_every_key_width(hip, oracle, k, amin):
    qc.key_width(hip, oracle, k, amin)


@pytest.mark.parametrize("k", [31, 64])
def test_boundaries(hip, k):
    qc.boundaries(hip, k)


def test_batches(hip, monkeypatch):
    qc.batches(hip, monkeypatch)


@pytest.mark.parametrize("name,k", qc.PROBE_CASES)
def test_probe_runs(hip, monkeypatch, name, k):
    qc.probe_runs(hip, monkeypatch, name, k)


def test_repeated_handmade_three_runs(hip):
    """the same set indexed three times in one process: which lane wins a slot differs, the hit bytes must not"""
    qc.repeated_handmade(hip, runs=3)


@pytest.mark.parametrize("name,k,amin", LINK_CASES)
def test_repeated_reads(hip, name, k, amin):
    qc.repeated_reads(hip, name, k)


@pytest.mark.parametrize("name,k,n_pieces,n_links", test_relink.SPLIT_CASES)
def test_repeated_split_pieces(hip, tools, tmp_path, name, k, n_pieces, n_links):  # noqa: F811
    qc.repeated_split(hip, tools, tmp_path, name, k)


def test_state(hip):
    qc.state(hip)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(hip, tmp_path, name, k):
    import bcalm_amd
    qc.cli(os.path.join(os.path.dirname(bcalm_amd.api.DEFAULT_LIB), "bcalm"), tmp_path, name, k)


@pytest.mark.parametrize("k,n_reads", [(31, 200000), (55, 50000)])
def test_mid_size(hip, oracle, k, n_reads):
    """generate_reads(n, 150, 3), abundance-min 2: the first 2 000 reads and their reverse complements against (c) for every hit
    and against (b), the oracle's solid set of the same text"""
    import bcalm_amd
    g = bcalm_amd.Graph(k, 2, lib=hip)
    try:
        g.generate_reads(n_reads, 150, 3); g.run()
        text = g.read_text(0, n_reads * 151).decode()
        solid = qc.solid_set(oracle, text, k, 2)
        ut = [s for s, _ in g.unitigs()]
        reads = text.split("\n")[:2000]
        qs = reads + [qc.rc(r) for r in reads]
        got = g.query(qs)
        n = {"+": 0, "-": 0, None: 0}
        for q, row in zip(qs, got):
            assert len(row) == len(q) - k + 1
            for p, h in enumerate(row):
                x = q[p:p + k]
                assert (h is not None) == (qc.canon(x) in solid), (p, x, h)
                if h is not None:
                    u, o, s = h
                    assert ut[u][o:o + k] == (x if s == "+" else qc.rc(x))
                n[h[2] if h else None] += 1
        assert n["+"] > 0 and n["-"] > 0 and n[None] > 0, n
        info = g.index_info()
        assert info["positions"] == info["distinct"] == g.stats()["n_solid"] == len(solid)
    finally:
        g.close()
