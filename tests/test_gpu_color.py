"""The resident unitigs coloured by sample on the device: the cases of color_cases.py (as test_hostsim_color.py runs them on the simulator)
on poisoned memory, and what the simulator cannot show (its atomics are plain, its lanes run one at a time): the word-edge and class cases
three times in one process -- which lane wins a slot differs, the bytes must not -- and one mid-size graph whose planes must equal what
cdbg_quantify, pinned by its own suite, counts for every sample."""
import os

import pytest

import color_cases as cc
import kwidth_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_POISON_ALLOC", "0xA5")


@pytest.mark.parametrize("k", kc.K_EDGES)
def test_every_key_width(hip, k):
    cc.key_width(hip, k)


def test_word_edges_three_runs(hip, monkeypatch):
    cc.word_edges(hip, monkeypatch, runs=3)


@pytest.mark.parametrize("n_colors", [1, 32, 33, 64, 65])
def test_color_counts(hip, n_colors):
    cc.color_counts(hip, n_colors)


def test_accumulation(hip, monkeypatch):
    cc.accumulation(hip, monkeypatch)


def test_classes_three_runs(hip, monkeypatch):
    cc.classes(hip, monkeypatch, runs=3)


def test_repeated_handmade(hip):
    cc.repeated_handmade(hip)


def test_state(hip):
    cc.state(hip)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(hip, tmp_path, name, k):
    import bcalm_amd
    cc.cli(os.path.join(os.path.dirname(bcalm_amd.api.DEFAULT_LIB), "bcalm"), tmp_path, name, k)


def test_mid_size(hip):
    """generate_reads(60000, 150, 3), k = 31, abundance-min 2, five samples (read i belongs to colours i % 5 and (i // 7) % 5): the planes
    expected are those cdbg_quantify counts per sample (count > 0), runs and classes are folded from them with numpy, and every array the
    library returns must equal that fold -- real atomic ORs, compare-and-swaps and minima from thousands of waves"""
    import numpy as np
    import bcalm_amd
    k, n_reads, N = 31, 60000, 5
    g = bcalm_amd.Graph(k, 2, lib=hip)
    try:
        g.generate_reads(n_reads, 150, 3); g.run()
        reads = g.read_text(0, n_reads * 151).split(b"\n")[:n_reads]
        samples = [[r for i, r in enumerate(reads) if i % 5 == c or (i // 7) % 5 == c] for c in range(N)]
        planes, q_found = [], 0
        for c in range(N):
            g.quant_reset()
            q_found += g.quantify(samples[c])["found"]
            _, _, ab, off = g.quant_raw()
            U = len(off) - 1
            P = off[U]
            planes.append(np.frombuffer(ab, dtype=np.uint32)[:P] > 0)
        off = np.frombuffer(off, dtype=np.uint64).astype(np.int64)
        key = np.zeros(P, dtype=np.int64)
        for c in range(N):
            key |= planes[c].astype(np.int64) << c
        head = np.ones(P, dtype=bool)
        head[1:] = key[1:] != key[:-1]
        head[off[:-1]] = True
        start = np.nonzero(head)[0]
        ln = np.diff(np.append(start, P))
        rkey = key[start]
        uniq, first = np.unique(rkey, return_index=True)
        order = np.argsort(first)                            # classes in the order of their first run
        number = np.zeros(1 << N, dtype=np.int64)
        number[uniq[order]] = np.arange(len(uniq))
        cls = number[rkey]
        unitig = np.searchsorted(off, start, side="right") - 1
        g.color_open(N)
        tot = [g.color(c, samples[c]) for c in range(N)]
        print("mid-size: %d positions, %d runs, %d classes; found %d, extended %d" % (P, len(start), len(uniq), q_found, sum(t["extended"] for t in tot)))
        assert sum(t["found"] for t in tot) == q_found > 0 and sum(t["extended"] for t in tot) > 0
        assert len(uniq) >= 3 and any(bin(int(v)).count("1") >= 2 for v in uniq)
        t, run_off, r_off, r_len, r_cls = g.color_runs_raw()
        R = len(start)
        assert t == {"runs": R, "classes": len(uniq), "colored": int((key != 0).sum()), "single_run_unitigs": int((np.diff(np.searchsorted(start, off)) == 1).sum())}
        assert np.array_equal(np.frombuffer(run_off, dtype=np.uint64).astype(np.int64), np.searchsorted(start, off))
        assert np.array_equal(np.frombuffer(r_off, dtype=np.uint32)[:R], start - off[unitig])
        assert np.array_equal(np.frombuffer(r_len, dtype=np.uint32)[:R], ln)
        assert np.array_equal(np.frombuffer(r_cls, dtype=np.uint32)[:R], cls)
        n, ncol, cruns, kmers, bits, nw = g.color_classes_raw()
        assert n == len(uniq) and nw == 1
        assert np.array_equal(np.frombuffer(bits, dtype=np.uint32)[:n], uniq[order])
        assert list(ncol[:n]) == [bin(int(v)).count("1") for v in uniq[order]]
        assert np.array_equal(np.frombuffer(cruns, dtype=np.uint64)[:n].astype(np.int64), np.bincount(cls, minlength=n))
        assert np.array_equal(np.frombuffer(kmers, dtype=np.uint64)[:n].astype(np.int64), np.bincount(cls, weights=ln, minlength=n).astype(np.int64))
    finally:
        g.close()
