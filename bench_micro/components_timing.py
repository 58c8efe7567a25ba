"""Timing of cdbg_components in the shape of DESIGN.md 5f's table: one MI355X, k = 31, abundance-min 2, the 10 M x 150 bp config-3
graph; the device route and the route a caller had before it -- cdbg_fetch_links and a union-find on the host -- alternating in one
process, five repeats, medians.

  python bench_micro/components_timing.py [--reads 10000000] [--repeats 5]

Reports (one JSON line at the end):
  * kernels: kernel-only ms of the four phases (hook, compress, number, totals: the library's own event timer, printed under
    CDBG_HOST_MARKS=1);
  * device_route: wall ms of cdbg_components + cdbg_fetch_components (labels and all five per-component arrays) on prepared buffers;
  * host_route: wall ms of cdbg_fetch_links + the host labelling (scipy.sparse.csgraph.connected_components, compiled code, where scipy is
    installed; a pure-Python union-find otherwise -- `host_method` says which), split into the copy and the labelling;
  * the totals, the bytes that cross the bus either way, and that both routes give the same labels."""
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

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    HOST_METHOD = "scipy.sparse.csgraph.connected_components"
except ImportError:
    HOST_METHOD = "python union-find"


def host_labels(off, to, U, n_links):
    """the component of every unitig from the fetched link table, numbered in the order of the smallest member"""
    o = np.frombuffer(off, dtype=np.uint64, count=2 * U + 1).astype(np.int64)
    t = np.frombuffer(to, dtype=np.uint32, count=n_links).astype(np.int64) >> 1
    src = np.repeat(np.arange(2 * U, dtype=np.int64) >> 1, np.diff(o))
    if HOST_METHOD.startswith("scipy"):
        _, lab = connected_components(coo_matrix((np.ones(n_links, dtype=np.int8), (src, t)), shape=(U, U)), directed=False)
    else:
        parent = list(range(U))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for a, b in zip(src.tolist(), t.tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        lab = np.array([find(u) for u in range(U)], dtype=np.int64)
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # labels renumbered by first occurrence = by smallest member
    rank = np.empty_like(order); rank[order] = np.arange(len(order))
    return rank[inv].astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    lib = bcalm_amd.load(a.lib)
    u64, u32 = C.c_uint64, C.c_uint32
    res = {"k": a.k, "reads": a.reads, "host_method": HOST_METHOD}
    g = api.Graph(a.k, 2, lib=lib)
    try:
        with Stderr():
            g.generate_reads(a.reads, a.read_len, 3); g.run()
            g._ck(lib.cdbg_link(g._h))
        U = g._num_unitigs()
        nl = u64(); g._ck(lib.cdbg_num_links(g._h, C.byref(nl))); nl = nl.value
        out = (u64 * 4)()
        with Stderr():                                       # warm-up: buffers, the pool, code objects
            g._ck(lib.cdbg_components(g._h, out))
        n = out[0]
        comp, fu = (u32 * max(U, 1))(), (u32 * max(n, 1))()
        nu, ba, km, kc = ((u64 * max(n, 1))() for _ in range(4))
        off, to = (u64 * (2 * U + 1))(), (u32 * max(nl, 1))()
        g._ck(lib.cdbg_fetch_links(g._h, off, to))
        t = {x: [] for x in ("hook", "compress", "number", "totals", "device_route", "host_fetch_links", "host_label", "host_route")}
        lab = None
        for _ in range(a.repeats):
            with Stderr() as err:
                t0 = time.perf_counter()
                g._ck(lib.cdbg_components(g._h, out))
                g._ck(lib.cdbg_fetch_components(g._h, comp, 0, n, fu, nu, ba, km, kc))
                t["device_route"].append((time.perf_counter() - t0) * 1e3)
            m = re.search(r"\[components\] .* hook_ms ([0-9.]+) compress_ms ([0-9.]+) number_ms ([0-9.]+) totals_ms ([0-9.]+)", err.text)
            for x, v in zip(("hook", "compress", "number", "totals"), m.groups()):
                t[x].append(float(v))
            t0 = time.perf_counter()
            g._ck(lib.cdbg_fetch_links(g._h, off, to))
            t1 = time.perf_counter()
            lab = host_labels(off, to, U, nl)
            t2 = time.perf_counter()
            t["host_fetch_links"].append((t1 - t0) * 1e3); t["host_label"].append((t2 - t1) * 1e3); t["host_route"].append((t2 - t0) * 1e3)
        res["unitigs"], res["links"] = U, nl
        res["totals"] = {"components": out[0], "largest": out[1], "largest_id": out[2], "singletons": out[3]}
        res["labels_agree"] = bool(np.array_equal(lab, np.frombuffer(comp, dtype=np.uint32, count=U)))
        res["bytes_back"] = {"device_route": 4 * U + 36 * n, "host_route": 8 * (2 * U + 1) + 4 * nl}
        res["median_ms"] = {x: statistics.median(v) for x, v in t.items()}
        res["all_ms"] = t
    finally:
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
