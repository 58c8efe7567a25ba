"""Timing of the colour calls in the shape of DESIGN.md 5g's table: one MI355X, k = 31, abundance-min 2, the 10 M x 150 bp config-3
graph, N = 8 samples of the graph's own reads (sample c = --sample-reads consecutive reads from read c x --sample-reads / 2 on: every
sample shares half of its reads with the next one).

  python bench_micro/color_timing.py [--reads 10000000] [--samples 8] [--sample-reads 250000] [--repeats 3] [--large-n 256]

Reports (one JSON line at the end):
  * mark: per sample, cdbg_color against cdbg_quantify on the same text in the same process -- wall and kernel-only ms (the library's
    own event timer, printed under CDBG_HOST_MARKS=1), windows / found / extended, the atomics k_color_mark issued and atomics per
    found window (k_quant issues exactly one per found window);
  * device_route: wall ms of cdbg_color_classes + cdbg_fetch_color_runs + cdbg_fetch_color_classes on prepared buffers, and the
    kernel-only ms of its three phases;
  * host_route: the emulation the calls replace -- per sample cdbg_quant_reset, cdbg_quantify, cdbg_fetch_quant of the per-position
    counts, then a numpy fold of the N count vectors into runs and classes -- split into the device calls and the fold;
  * the totals, the bytes that cross the bus either way, and that both routes give the same runs and classes;
  * large_n: the same samples marked into --large-n planes (colour c x large-n / samples + large-n / samples - 1: the last plane is one of
    them), the same runs and classes therefore, and cdbg_color_classes alone -- what the class key of --large-n gathered bits costs."""
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


def fold(planes, off, P):
    """runs and classes from N boolean planes, as the definitions of include/cdbg.h have them"""
    key = np.zeros(P, dtype=np.int64)
    for c, p in enumerate(planes):
        key |= p.astype(np.int64) << c
    head = np.ones(P, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    head[off[:-1]] = True
    start = np.nonzero(head)[0]
    ln = np.diff(np.append(start, P))
    rkey = key[start]
    uniq, first, inv = np.unique(rkey, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # classes in the order of their first run
    rank = np.empty_like(order); rank[order] = np.arange(len(order))
    cls = rank[inv]
    unitig = np.searchsorted(off, start, side="right") - 1
    return {"run_off": np.searchsorted(start, off), "offset": start - off[unitig], "len": ln, "cls": cls, "bits": uniq[order],
            "runs": np.bincount(cls, minlength=len(uniq)), "kmers": np.bincount(cls, weights=ln, minlength=len(uniq)).astype(np.int64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sample-reads", type=int, default=250_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--large-n", type=int, default=256, help="0: skip")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    lib = bcalm_amd.load(a.lib)
    u64, u32 = C.c_uint64, C.c_uint32
    N, S, L = a.samples, a.sample_reads, a.read_len
    assert N <= 32 and (N - 1) * (S // 2) + S <= a.reads
    res = {"k": a.k, "reads": a.reads, "samples": N, "sample_reads": S}
    g = api.Graph(a.k, 2, lib=lib)
    try:
        with Stderr():
            g.generate_reads(a.reads, L, 3); g.run(); g.index()
        res["index_info"] = info = g.index_info()
        U, P = g._num_unitigs(), info["positions"]
        texts = [g.read_text(c * (S // 2) * (L + 1), S * (L + 1)) for c in range(N)]
        off = (u64 * (S + 1))(*range(0, (S + 1) * (L + 1), L + 1))       # (the separator rides at the end of every read: one more broken window)
        tot = (u64 * 3)()
        # ---- marking: cdbg_color against cdbg_quantify, sample by sample ----
        with Stderr():                                       # warm-up: planes, counters, the pool, code objects
            g.color_open(N)
            g._ck(lib.cdbg_color(g._h, 0, texts[0], off, S, tot))
            g._ck(lib.cdbg_quantify(g._h, texts[0], off, S, tot))
        mark = []
        for rep in range(a.repeats):
            with Stderr():
                g.color_open(N); g.quant_reset()
            for c in range(N):
                row = {"repeat": rep, "sample": c}
                with Stderr() as err:
                    t = time.perf_counter()
                    g._ck(lib.cdbg_color(g._h, c, texts[c], off, S, tot))
                    row["color_wall_ms"] = (time.perf_counter() - t) * 1e3
                m = re.search(r"\[color\] positions \d+ kernel_ms ([0-9.]+) windows (\d+) found (\d+) extended (\d+) atomics (\d+)", err.text)
                row.update(color_kernel_ms=float(m.group(1)), windows=int(m.group(2)), found=int(m.group(3)), extended=int(m.group(4)), atomics=int(m.group(5)))
                row["atomics_per_found"] = row["atomics"] / row["found"] if row["found"] else None
                with Stderr() as err:
                    t = time.perf_counter()
                    g._ck(lib.cdbg_quantify(g._h, texts[c], off, S, tot))
                    row["quant_wall_ms"] = (time.perf_counter() - t) * 1e3
                row["quant_kernel_ms"] = float(re.search(r"\[quant\] positions \d+ kernel_ms ([0-9.]+)", err.text).group(1))
                assert tot[1] == row["found"]
                mark.append(row)
        res["mark"] = mark
        res["mark_median"] = {x: statistics.median(r[x] for r in mark) for x in ("color_kernel_ms", "quant_kernel_ms", "color_wall_ms", "quant_wall_ms", "atomics_per_found")}
        res["mark_first_repeat_atomics_per_found"] = statistics.median(r["atomics_per_found"] for r in mark if r["repeat"] == 0)
        # ---- classes: the device route ----
        out = (u64 * 4)()
        with Stderr():
            g._ck(lib.cdbg_color_classes(g._h, out))         # warm-up, and the sizes
        R, NC, NW = out[0], out[1], (N + 31) // 32
        run_off, r_off, r_len, r_cls = (u64 * (U + 1))(), (u32 * max(R, 1))(), (u32 * max(R, 1))(), (u32 * max(R, 1))()
        c_ncol, c_bits, c_runs, c_kmers = (u32 * max(NC, 1))(), (u32 * max(NC * NW, 1))(), (u64 * max(NC, 1))(), (u64 * max(NC, 1))()
        t = {x: [] for x in ("device_route", "runs_ms", "table_ms", "totals_ms", "host_device_calls", "host_fold", "host_route")}
        for _ in range(a.repeats):
            with Stderr() as err:
                t0 = time.perf_counter()
                g._ck(lib.cdbg_color_classes(g._h, out))
                g._ck(lib.cdbg_fetch_color_runs(g._h, run_off, r_off, r_len, r_cls))
                g._ck(lib.cdbg_fetch_color_classes(g._h, 0, NC, c_ncol, c_runs, c_kmers, c_bits))
                t["device_route"].append((time.perf_counter() - t0) * 1e3)
            m = re.search(r"\[color_classes\] .* runs_ms ([0-9.]+) table_ms ([0-9.]+) totals_ms ([0-9.]+)", err.text)
            for x, v in zip(("runs_ms", "table_ms", "totals_ms"), m.groups()):
                t[x].append(float(v))
        # ---- the emulation: N x (reset, quantify, fetch) and a numpy fold ----
        kc, cov, ab, ab_off = (u64 * max(U, 1))(), (u32 * max(U, 1))(), (u32 * max(P, 1))(), (u64 * (U + 1))()
        f = None
        for _ in range(a.repeats):
            with Stderr():
                t0 = time.perf_counter()
                planes = []
                for c in range(N):
                    g.quant_reset()
                    g._ck(lib.cdbg_quantify(g._h, texts[c], off, S, tot))
                    g._ck(lib.cdbg_fetch_quant(g._h, 0, U, None, None, ab, ab_off))
                    planes.append(np.frombuffer(ab, dtype=np.uint32, count=P) > 0)
                t1 = time.perf_counter()
                f = fold(planes, np.frombuffer(ab_off, dtype=np.uint64).astype(np.int64), P)
                t2 = time.perf_counter()
            t["host_device_calls"].append((t1 - t0) * 1e3); t["host_fold"].append((t2 - t1) * 1e3); t["host_route"].append((t2 - t0) * 1e3)
        res["totals"] = {"runs": R, "classes": NC, "colored": out[2], "single_run_unitigs": out[3], "unitigs": U, "positions": P}
        res["routes_agree"] = bool(
            np.array_equal(f["run_off"], np.frombuffer(run_off, dtype=np.uint64).astype(np.int64)) and np.array_equal(f["offset"], np.frombuffer(r_off, dtype=np.uint32, count=R))
            and np.array_equal(f["len"], np.frombuffer(r_len, dtype=np.uint32, count=R)) and np.array_equal(f["cls"], np.frombuffer(r_cls, dtype=np.uint32, count=R))
            and np.array_equal(f["bits"], np.frombuffer(c_bits, dtype=np.uint32, count=NC)) and np.array_equal(f["runs"], np.frombuffer(c_runs, dtype=np.uint64, count=NC).astype(np.int64))
            and np.array_equal(f["kmers"], np.frombuffer(c_kmers, dtype=np.uint64, count=NC).astype(np.int64)))
        res["bytes_back"] = {"device_route": 8 * (U + 1) + 12 * R + (20 + 4 * NW) * NC, "host_route": N * (4 * P + 8 * (U + 1))}
        res["plane_bytes"] = {"colours": N * ((P + 31) // 32) * 4, "one_quantify_counter_set": 4 * P}
        res["median_ms"] = {x: statistics.median(v) for x, v in t.items()}
        res["all_ms"] = t
        # ---- the class phase at a large colour count: the same marks, spread over --large-n planes ----
        NL = a.large_n
        if NL:
            assert NL % N == 0 and NL <= 4096
            with Stderr():
                g.color_open(NL)
                for c in range(N):
                    g._ck(lib.cdbg_color(g._h, c * (NL // N) + NL // N - 1, texts[c], off, S, tot))
                g._ck(lib.cdbg_color_classes(g._h, out))     # warm-up
            big = {x: [] for x in ("wall_ms", "runs_ms", "table_ms", "totals_ms")}
            for _ in range(a.repeats):
                with Stderr() as err:
                    t0 = time.perf_counter()
                    g._ck(lib.cdbg_color_classes(g._h, out))
                    big["wall_ms"].append((time.perf_counter() - t0) * 1e3)
                m = re.search(r"\[color_classes\] .* runs_ms ([0-9.]+) table_ms ([0-9.]+) totals_ms ([0-9.]+)", err.text)
                for x, v in zip(("runs_ms", "table_ms", "totals_ms"), m.groups()):
                    big[x].append(float(v))
            res["large_n"] = {"colours": NL, "runs": out[0], "classes": out[1], "same_runs_and_classes": (out[0], out[1]) == (R, NC),
                              "plane_bytes": NL * ((P + 31) // 32) * 4, "median_ms": {x: statistics.median(v) for x, v in big.items()}}
    finally:
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
