"""Pseudoalignment to the coloured unitigs on the device: the cases of color_query_cases.py (as test_hostsim_color_query.py runs them on the
simulator) on poisoned memory, and what the simulator cannot show (its lanes run one at a time, its atomics are plain): the edge case and
the many-segments case three times in one process with equal bytes, and one mid-size graph whose every returned array must equal a numpy
fold of cdbg_query's hit words and cdbg_fetch_color_runs' runs, each pinned by its own suite."""
import os

import pytest

import color_query_cases as cq
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
    cq.key_width(hip, k)


def test_run_edges_three_runs(hip, monkeypatch):
    cq.run_edges(hip, monkeypatch, runs=3)


@pytest.mark.parametrize("n_colors", [1, 32, 33, 64, 65])
def test_color_counts(hip, n_colors):
    cq.color_counts(hip, n_colors)


def test_thresholds(hip):
    cq.thresholds(hip)


def test_many_segments_three_runs(hip):
    cq.many_segments(hip, runs=3)


def test_batch_seams(hip, monkeypatch):
    cq.batch_seams(hip, monkeypatch)


def test_repeated_handmade(hip):
    cq.repeated_handmade(hip)


def test_state(hip):
    cq.state(hip)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(hip, tmp_path, name, k):
    import bcalm_amd
    cq.cli(hip, os.path.join(os.path.dirname(bcalm_amd.api.DEFAULT_LIB), "bcalm"), tmp_path, name, k)


def test_mid_size(hip):
    mid_size(hip, 60000, 2000)


def mid_size(lib, n_reads, n_sub):
    """generate_reads(60000, 150, 3), k = 31, abundance-min 2, five samples (read i belongs to colours i % 5 and (i // 7) % 5), as
    test_gpu_color.py::test_mid_size sets it up; queries: the 60 000 reads and 2 000 of them with one substitution each.  Expected values are
    folded with numpy from query_raw's hit words and color_runs_raw: a hit's colour run by a search in the runs' first positions, a segment
    head wherever the thread rule or the colour run breaks.  Share 1/1 of all windows: a read with a miss reports nothing."""
    import numpy as np
    import bcalm_amd
    k, N, L = 31, 5, 150
    g = bcalm_amd.Graph(k, 2, lib=lib)
    try:
        g.generate_reads(n_reads, L, 3); g.run()
        reads = g.read_text(0, n_reads * (L + 1)).split(b"\n")[:n_reads]
        g.color_open(N)
        for c in range(N):
            g.color(c, [r for i, r in enumerate(reads) if i % 5 == c or (i // 7) % 5 == c])
        sub = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
        qs = list(reads)
        for i in range(0, n_reads, n_reads // n_sub):        # 2 000 reads with one substitution
            b = bytearray(reads[i]); at = (7 * i) % L
            b[at] = sub.get(b[at], ord("A"))
            qs.append(bytes(b))
        n = len(qs)
        assert n == n_reads + n_sub and all(len(q) == L for q in qs)
        hits, _ = g.query_raw(qs)
        h = np.frombuffer(hits, dtype=np.uint64)[:n * L]
        _, _, ulen, _ = g.unitigs_packed()
        kmer_off = np.concatenate(([0], np.cumsum(np.array(ulen, dtype=np.int64) - k + 1)))
        U = len(kmer_off) - 1
        t, run_off, r_off, r_len, r_cls = g.color_runs_raw()
        R = t["runs"]
        run_off = np.frombuffer(run_off, dtype=np.uint64).astype(np.int64)
        r_first = kmer_off[np.repeat(np.arange(U), np.diff(run_off))] + np.frombuffer(r_off, dtype=np.uint32)[:R]       # ascending
        r_cls = np.frombuffer(r_cls, dtype=np.uint32)[:R]
        nc, _, _, _, bits, nw = g.color_classes_raw()
        assert nw == 1
        bits = np.frombuffer(bits, dtype=np.uint32)[:nc]
        hit = h != np.uint64(2 ** 64 - 1)
        u = (h >> np.uint64(33)).astype(np.int64); o = ((h >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64); st = (h & np.uint64(1)).astype(np.int64)
        cr = np.zeros(n * L, dtype=np.int64)
        cr[hit] = np.searchsorted(r_first, kmer_off[u[hit]] + o[hit], side="right") - 1
        cont = np.zeros(n * L, dtype=bool)
        cont[1:] = hit[1:] & hit[:-1] & (u[1:] == u[:-1]) & (st[1:] == st[:-1]) & (o[1:] == o[:-1] + 1 - 2 * st[:-1])
        cont[::L] = False                                    # (a sequence's last k - 1 positions miss: nothing continues across sequences anyway)
        runs_thread = int((hit & ~cont).sum())
        cont[1:] &= cr[1:] == cr[:-1]
        head = hit & ~cont
        start = np.nonzero(head)[0]
        S = len(start)
        seg_id = np.cumsum(head) - 1
        ln = np.bincount(seg_id[hit], minlength=S)
        cls = r_cls[cr[start]]
        seq = start // L
        found = np.bincount(seq, weights=ln, minlength=n).astype(np.int64)
        counts = np.stack([np.bincount(seq, weights=ln * ((bits[cls] >> c) & 1), minlength=n).astype(np.int64) for c in range(N)], axis=1)
        total = L - k + 1
        rep = (counts >= 1) & (counts >= total)              # share 1/1 of all windows
        raw = g.color_query_raw(qs, (1, 1))
        tot, q_found, q_ncol, q_bits, q_nw, seg_off, s_start, s_place, s_len, s_cls = raw
        print("mid-size: %d sequences, %d thread runs, %d segments, found %d of %d, %d sequences with a colour" % (n, runs_thread, S, tot["found"], tot["windows"], tot["reported"]))
        assert S > runs_thread > 0                            # the colour runs cut thread runs
        assert (rep.sum(axis=1) >= 2).any() and (rep.sum(axis=1) == 0).any()
        assert tot["windows"] == n * total and tot["found"] == int(hit.sum()) and tot["segments"] == S and tot["reported"] == int(rep.any(axis=1).sum())
        assert q_nw == 1
        assert np.array_equal(np.frombuffer(seg_off, dtype=np.uint64).astype(np.int64), np.searchsorted(start, np.arange(n + 1) * L))
        assert np.array_equal(np.frombuffer(s_start, dtype=np.uint64)[:S].astype(np.int64), start)
        assert np.array_equal(np.frombuffer(s_place, dtype=np.uint64)[:S], h[start])
        assert np.array_equal(np.frombuffer(s_len, dtype=np.uint32)[:S], ln)
        assert np.array_equal(np.frombuffer(s_cls, dtype=np.uint32)[:S], cls)
        assert np.array_equal(np.frombuffer(q_found, dtype=np.uint32)[:n], found)
        assert np.array_equal(np.frombuffer(q_bits, dtype=np.uint32)[:n], (rep << np.arange(N)).sum(axis=1))
        assert np.array_equal(np.frombuffer(q_ncol, dtype=np.uint32)[:n], rep.sum(axis=1))
        m, cnt, _ = g.color_query_counts(n // 3, n // 2)
        assert np.array_equal(np.frombuffer(cnt, dtype=np.uint32)[:m * N].reshape(m, N), counts[n // 3:n // 3 + n // 2])
        assert g.thread_raw(qs)[0]["runs"] == runs_thread
    finally:
        g.close()
