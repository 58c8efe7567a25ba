"""Connected components on the device: the cases of components_cases.py (as test_hostsim_components.py runs them on the simulator) on
poisoned memory, and what the simulator cannot show: thousands of workgroups on eight XCDs hooking into one tree at once (the chains of
200 000 pieces, the star, the mid-size graph), and the same bytes from every run."""
import os

import pytest

import components_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_POISON_ALLOC", "0xA5")


def test_handmade(hip):
    cc.handmade(hip)


@pytest.mark.parametrize("name,k,n_unitigs,n_comp,sizes", cc.FIXTURES, ids=[f[0] for f in cc.FIXTURES])
def test_fixture(hip, name, k, n_unitigs, n_comp, sizes):
    cc.fixture(hip, name, k, n_unitigs, n_comp, sizes)


@pytest.mark.parametrize("amin", [1, 2])
@pytest.mark.parametrize("k", cc.K_WIDTHS)
def test_key_width(hip, k, amin):
    cc.key_width(hip, k, amin)


def test_chains(hip):
    """200 000 pieces: enough workgroups that every XCD hooks into the same tree at once"""
    cc.chains(hip, 200000)


def test_star(hip):
    cc.star(hip)


def test_same_bytes_chain(hip):
    """the shuffled chain labelled three times in one process, after cdbg_reset + reload: which lane wins which hook differs, the bytes must not"""
    cc.same_bytes(hip, cc.shuffled_chain(200000), 31)


def test_same_bytes_star(hip):
    seqs, kcs = cc.star_set()
    cc.same_bytes(hip, seqs, cc.STAR_K, kcs)


def test_state(hip):
    cc.state(hip)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(hip, tmp_path, name, k):
    import bcalm_amd
    cc.cli(os.path.join(os.path.dirname(bcalm_amd.api.DEFAULT_LIB), "bcalm"), tmp_path, name, k)


def test_mid_size(hip):
    """generate_reads(200000, 150, 3), k = 31, abundance-min 2 (the graph test_gpu_thread.py relies on): labels and totals are the model's
    over the fetched links, the k-mers add up to n_solid and the KC to the digest's sum.  The four counts were measured with the model on
    the simulator before cdbg_components existed: 20 391 unitigs, 1 939 components, 18 453 unitigs in the largest, 1 938 singletons"""
    import bcalm_amd
    k = 31
    g = bcalm_amd.Graph(k, 2, lib=hip)
    try:
        g.generate_reads(200000, 150, 3); g.run()
        tot, labels, comps, _ = cc.check(g, k)
        print("mid-size: unitigs %d components %d largest %d singletons %d" % (len(labels), tot["components"], tot["largest"], tot["singletons"]))
        assert sum(d["kmers"] for d in comps) == g.stats()["n_solid"]
        assert sum(d["kc"] for d in comps) == g.digest()["kc_sum"]
        assert (len(labels), tot["components"], tot["largest"], tot["singletons"]) == (20391, 1939, 18453, 1938)
    finally:
        g.close()
