"""Timing of cdbg_quantify against cdbg_query in the shape of DESIGN.md 5d's table: one MI355X, k = 31, abundance-min 2, the
10 M x 150 bp config-3 graph; the same 1 M of the graph's own reads through both calls in one process, three repeats.

  python bench_micro/quant_timing.py [--reads 10000000] [--queries 1000000] [--repeats 3]

Reports (one JSON line at the end): per repeat the wall and kernel-only ms (the library's own event timer, printed under
CDBG_HOST_MARKS=1) of
  * cdbg_query (the baseline: 8 bytes of hits per base come back to the host),
  * cdbg_quantify with extension,
  * cdbg_quantify in a second context created under CDBG_QUANT_NO_EXTEND=1 (every window probes),
the windows / found / extended of the call and extended / found, and the wall ms of one cdbg_fetch_quant of kc + covered."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["CDBG_HOST_MARKS"] = "1"                       # (read once per process by the library: set before it is loaded)
import bcalm_amd  # noqa: E402
from bcalm_amd import api  # noqa: E402
from query_timing import Stderr  # noqa: E402


def offsets(n, read_len):
    return (C.c_uint64 * (n + 1))(*range(0, (n + 1) * (read_len + 1), read_len + 1))     # (the separator rides at the end of every read: one more broken window)


def time_query(g, text, n, read_len, repeats):
    off, hits, out = offsets(n, read_len), (C.c_uint64 * len(text))(), []
    for _ in range(repeats):
        with Stderr() as err:
            t = time.perf_counter()
            g._ck(g.lib.cdbg_query(g._h, text, off, n, hits))
            wall = time.perf_counter() - t
        m = re.search(r"\[query\] positions (\d+) kernel_ms ([0-9.]+)", err.text)
        out.append({"wall_ms": wall * 1e3, "kernel_ms": float(m.group(2))})
    return out


def time_quantify(g, text, n, read_len, repeats):
    off, tot, out = offsets(n, read_len), (C.c_uint64 * 3)(), []
    g._ck(g.lib.cdbg_quantify(g._h, b"", None, 0, tot))       # (index and counters built outside the timed calls)
    for _ in range(repeats):
        with Stderr() as err:
            t = time.perf_counter()
            g._ck(g.lib.cdbg_quantify(g._h, text, off, n, tot))
            wall = time.perf_counter() - t
        m = re.search(r"\[quant\] positions (\d+) kernel_ms ([0-9.]+)", err.text)
        out.append({"wall_ms": wall * 1e3, "kernel_ms": float(m.group(2)), "windows": tot[0], "found": tot[1], "extended": tot[2],
                    "extended_of_found": tot[2] / tot[1] if tot[1] else None})
    t = time.perf_counter()
    g.quant_raw(per_kmer=False)
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    lib = bcalm_amd.load(a.lib)
    k, L = a.k, a.read_len
    res = {"k": k, "reads": a.reads, "queries": a.queries}
    for name, env in (("extend", None), ("no_extend", "CDBG_QUANT_NO_EXTEND")):
        if env:
            os.environ[env] = "1"                            # (hooks are read when a context is created)
        g = api.Graph(k, 2, lib=lib)
        if env:
            del os.environ[env]
        try:
            with Stderr():
                g.generate_reads(a.reads, L, 3); g.run(); g.index()
            own = g.read_text(0, a.queries * (L + 1))
            if not env:
                res["index_info"] = g.index_info()
                res["query"] = time_query(g, own, a.queries, L, a.repeats)
            res["quantify_" + name], res["fetch_ms_" + name] = time_quantify(g, own, a.queries, L, a.repeats)
        finally:
            g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
