"""Timing of cdbg_thread against cdbg_query in the shape of DESIGN.md 5e's table: one MI355X, k = 31, abundance-min 2, the
10 M x 150 bp config-3 graph; the same 1 M of the graph's own reads through both in one process, the two alternating, five repeats,
medians.

  python bench_micro/thread_timing.py [--reads 10000000] [--queries 1000000] [--repeats 5]

Reports (one JSON line at the end):
  * kernels: kernel-only ms (the library's own event timer, printed under CDBG_HOST_MARKS=1) of k_query, of the producer k_thread_hits
    and of the run kernels (count, the two scans, emit, len) behind it;
  * calls: wall ms of Graph.thread_raw against Graph.query_raw plus a numpy fold of its hit words into the same runs -- what a caller
    pays for the walk either way -- and of Graph.query_raw alone;
  * c_calls: wall ms of the C calls alone on prepared buffers (cdbg_query into a caller's array; cdbg_thread + cdbg_fetch_runs);
  * the totals of the call (windows, found, runs, extended), bytes that come back per call, and that both folds agree."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["CDBG_HOST_MARKS"] = "1"                       # (read once per process by the library: set before it is loaded)
import bcalm_amd  # noqa: E402
from bcalm_amd import api  # noqa: E402
from query_timing import Stderr  # noqa: E402
from quant_timing import offsets  # noqa: E402


def numpy_fold(hits, n):
    """the runs of n hit words by the definition of include/cdbg.h -> (start, place, len)"""
    h = np.frombuffer(hits, dtype=np.uint64, count=n)
    hit = h != np.uint64(api.Graph.MISS)
    a, b = h[:-1], h[1:]
    # same unitig, same strand, offset + 1 (strand 0) or - 1 (strand 1): the word moves by 2 (an offset never wraps: it is below 2^32 - k)
    cont = hit[:-1] & hit[1:] & (b == np.where((a & np.uint64(1)) == 1, a - np.uint64(2), a + np.uint64(2)))
    head = hit.copy(); head[1:] &= ~cont
    tail = hit.copy(); tail[:-1] &= ~cont
    start = np.flatnonzero(head)
    return start, h[start], (np.flatnonzero(tail) - start + 1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    lib = bcalm_amd.load(a.lib)
    k, L, n = a.k, a.read_len, a.queries
    res = {"k": k, "reads": a.reads, "queries": n}
    g = api.Graph(k, 2, lib=lib)
    try:
        with Stderr():
            g.generate_reads(a.reads, L, 3); g.run(); g.index()
        res["index_info"] = g.index_info()
        own = g.read_text(0, n * (L + 1))
        seqs = [own[i * (L + 1):(i + 1) * (L + 1)] for i in range(n)]       # (the separator rides at the end of every read: one more broken window)
        off, hits, tot = offsets(n, L), (C.c_uint64 * len(own))(), (C.c_uint64 * 4)()
        run_off = (C.c_uint64 * (n + 1))()
        with Stderr():                                       # warm-up: staging, buffers, the pool
            g._ck(lib.cdbg_query(g._h, own, off, n, hits)); g._ck(lib.cdbg_thread(g._h, own, off, n, tot))
        t = {x: [] for x in ("k_query", "k_thread_hits", "run_kernels", "c_query", "c_thread", "query_raw", "query_raw_fold", "thread_raw")}
        for _ in range(a.repeats):
            with Stderr() as err:
                t0 = time.perf_counter()
                g._ck(lib.cdbg_query(g._h, own, off, n, hits))
                t["c_query"].append((time.perf_counter() - t0) * 1e3)
            t["k_query"].append(float(re.search(r"\[query\] positions \d+ kernel_ms ([0-9.]+)", err.text).group(1)))
            with Stderr() as err:
                t0 = time.perf_counter()
                g._ck(lib.cdbg_thread(g._h, own, off, n, tot))
                start, place, ln = (C.c_uint64 * max(tot[2], 1))(), (C.c_uint64 * max(tot[2], 1))(), (C.c_uint32 * max(tot[2], 1))()
                g._ck(lib.cdbg_fetch_runs(g._h, run_off, start, place, ln))
                t["c_thread"].append((time.perf_counter() - t0) * 1e3)
            m = re.search(r"\[thread\] positions \d+ hits_ms ([0-9.]+) runs_ms ([0-9.]+)", err.text)
            t["k_thread_hits"].append(float(m.group(1))); t["run_kernels"].append(float(m.group(2)))
            with Stderr():
                t0 = time.perf_counter()
                h, o = g.query_raw(seqs)
                t["query_raw"].append((time.perf_counter() - t0) * 1e3)
                folded = numpy_fold(h, o[-1])
                t["query_raw_fold"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                raw = g.thread_raw(seqs)
                t["thread_raw"].append((time.perf_counter() - t0) * 1e3)
        r = raw[0]["runs"]
        res["totals"] = raw[0]
        res["folds_agree"] = bool(len(folded[0]) == r and np.array_equal(folded[0], np.frombuffer(raw[2], dtype=np.uint64, count=r))
                                  and np.array_equal(folded[1], np.frombuffer(raw[3], dtype=np.uint64, count=r))
                                  and np.array_equal(folded[2], np.frombuffer(raw[4], dtype=np.uint32, count=r)))
        res["bytes_back"] = {"query": 8 * len(own), "thread": 20 * r}
        res["median_ms"] = {x: statistics.median(v) for x, v in t.items()}
        res["all_ms"] = t
    finally:
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
