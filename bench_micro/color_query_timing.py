"""Timing of the colour query in the shape of DESIGN.md 5h's table: one MI355X, k = 31, abundance-min 2, the 10 M x 150 bp config-3 graph,
N = 8 samples of the graph's own reads (as color_timing.py takes them: sample c = --sample-reads consecutive reads from read
c x --sample-reads / 2 on), queried with --query-reads of its own reads, share 1/2 of all k-mers.

  python bench_micro/color_query_timing.py [--reads 10000000] [--samples 8] [--sample-reads 250000] [--query-reads 1000000] [--repeats 3] [--large-n 256]

Reports (one JSON line at the end), for N = --samples and again for the same marks spread over --large-n planes:
  * device_route: wall ms of cdbg_color_query + cdbg_fetch_color_query (found, n_colors, bits: the answer) on prepared buffers, and the
    kernel-only ms of k_thread_hits, of the run kernels behind it and of k_cq_span (with its scan) / k_cq_emit / k_cq_fold (the library's
    own event timers, printed under CDBG_HOST_MARKS=1);
  * host_route: what the library offered for the same answer before -- cdbg_thread + cdbg_fetch_runs + cdbg_fetch_color_runs +
    cdbg_fetch_color_classes, then a numpy fold: the colour runs under every thread run by two searches, the clipped pieces, one
    weighted bincount per colour, the threshold -- split into the device calls and the fold;
  * the totals, the bytes that come back either way, and that both routes give the same found / bits per sequence."""
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


def host_fold(n, k, L, N, num, den, runs, colour):
    """found and bit rows per sequence from the thread runs and the colour runs, as the definitions of include/cdbg.h have them"""
    run_off, start, place, ln = runs
    kmer_off, kmer_first, r_len, r_cls, bits, NW = colour    # the first global position of every unitig / of every colour run (ascending)
    u = (place >> np.uint64(33)).astype(np.int64); o = ((place >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64); st = (place & np.uint64(1)).astype(np.int64)
    ln = ln.astype(np.int64)
    lo = kmer_off[u] + np.where(st == 1, o - ln + 1, o); hi = lo + ln - 1
    a = np.searchsorted(kmer_first, lo, side="right") - 1; b = np.searchsorted(kmer_first, hi, side="right") - 1
    nseg = b - a + 1
    run = np.repeat(np.arange(len(ln)), nseg)
    cr = a[run] + (np.arange(nseg.sum()) - np.repeat(np.cumsum(nseg) - nseg, nseg))
    c_lo = np.maximum(kmer_first[cr], lo[run]); c_hi = np.minimum(kmer_first[cr] + r_len[cr] - 1, hi[run])
    seg_len = c_hi - c_lo + 1
    seq = np.repeat(np.arange(n), np.diff(run_off))[run]
    found = np.bincount(seq, weights=seg_len, minlength=n).astype(np.int64)
    need = num * (L - k + 1)
    out = np.zeros((n, NW), dtype=np.uint32)
    rows = bits[r_cls[cr]]                                   # [segments][NW]
    for c in range(N):
        cnt = np.bincount(seq, weights=seg_len * ((rows[:, c >> 5] >> np.uint32(c & 31)) & 1), minlength=n).astype(np.int64)
        out[:, c >> 5] |= (((cnt >= 1) & (cnt * den >= need)).astype(np.uint32) << np.uint32(c & 31))
    return found, out, len(cr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sample-reads", type=int, default=250_000)
    ap.add_argument("--query-reads", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--large-n", type=int, default=256, help="0: skip")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    lib = bcalm_amd.load(a.lib)
    u64, u32 = C.c_uint64, C.c_uint32
    N0, S, L, Q, k = a.samples, a.sample_reads, a.read_len, a.query_reads, a.k
    assert (N0 - 1) * (S // 2) + S <= a.reads and Q <= a.reads
    num, den = 1, 2
    res = {"k": k, "reads": a.reads, "samples": N0, "sample_reads": S, "query_reads": Q, "share": [num, den]}
    g = api.Graph(k, 2, lib=lib)
    try:
        with Stderr():
            g.generate_reads(a.reads, L, 3); g.run(); g.index()
        res["index_info"] = info = g.index_info()
        U = g._num_unitigs()
        texts = [g.read_text(c * (S // 2) * (L + 1), S * (L + 1)) for c in range(N0)]
        off = (u64 * (S + 1))(*range(0, (S + 1) * (L + 1), L + 1))       # (the separator rides at the end of every read: one more broken window)
        qtext = g.read_text(0, Q * (L + 1))
        qoff = (u64 * (Q + 1))(*range(0, (Q + 1) * (L + 1), L + 1))
        n_win = L + 1 - k + 1                                # (with the separator: total_i counts one more, broken, window)
        tot = (u64 * 3)()
        for N in [N0] + ([a.large_n] if a.large_n else []):
            assert N % N0 == 0 and N <= 4096
            NW = (N + 31) // 32
            with Stderr():
                g.color_open(N)
                for c in range(N0):
                    g._ck(lib.cdbg_color(g._h, c * (N // N0) + N // N0 - 1, texts[c], off, S, tot))
            out4, out5 = (u64 * 4)(), (u64 * 5)()
            with Stderr():
                g._ck(lib.cdbg_color_classes(g._h, out4))
                g._ck(lib.cdbg_color_query(g._h, qtext, qoff, Q, num, den, 0, out5))      # warm-up, and the sizes
            R, NC, SEG = out4[0], out4[1], out5[2]
            found, ncol, bits = (u32 * Q)(), (u32 * Q)(), (u32 * (Q * NW))()
            t = {x: [] for x in ("device_route", "hits_ms", "runs_ms", "span_ms", "emit_ms", "fold_ms", "host_device_calls", "host_fold", "host_route")}
            for _ in range(a.repeats):
                with Stderr() as err:
                    t0 = time.perf_counter()
                    g._ck(lib.cdbg_color_query(g._h, qtext, qoff, Q, num, den, 0, out5))
                    g._ck(lib.cdbg_fetch_color_query(g._h, found, ncol, bits, None, None, None, None, None))
                    t["device_route"].append((time.perf_counter() - t0) * 1e3)
                m = re.search(r"\[thread\] positions \d+ hits_ms ([0-9.]+) runs_ms ([0-9.]+)", err.text)
                t["hits_ms"].append(float(m.group(1))); t["runs_ms"].append(float(m.group(2)))
                m = re.search(r"\[color_query\] .* span_ms ([0-9.]+) emit_ms ([0-9.]+) fold_ms ([0-9.]+)", err.text)
                for x, v in zip(("span_ms", "emit_ms", "fold_ms"), m.groups()):
                    t[x].append(float(v))
            # ---- what the library offered before: the runs of both kinds to the host, and a numpy fold ----
            agree = None
            for _ in range(a.repeats if N == N0 else 1):
                with Stderr():
                    t0 = time.perf_counter()
                    out = (u64 * 4)()
                    g._ck(lib.cdbg_thread(g._h, qtext, qoff, Q, out))
                    TR = out[2]
                    run_off, start, place, ln = (u64 * (Q + 1))(), (u64 * max(TR, 1))(), (u64 * max(TR, 1))(), (u32 * max(TR, 1))()
                    g._ck(lib.cdbg_fetch_runs(g._h, run_off, start, place, ln))
                    c_off, r_off, r_len, r_cls = (u64 * (U + 1))(), (u32 * max(R, 1))(), (u32 * max(R, 1))(), (u32 * max(R, 1))()
                    c_bits = (u32 * max(NC * NW, 1))()
                    g._ck(lib.cdbg_fetch_color_runs(g._h, c_off, r_off, r_len, r_cls))
                    g._ck(lib.cdbg_fetch_color_classes(g._h, 0, NC, None, None, None, c_bits))
                    t1 = time.perf_counter()
                    c_off_n = np.frombuffer(c_off, dtype=np.uint64).astype(np.int64)
                    r_len_n = np.frombuffer(r_len, dtype=np.uint32, count=R).astype(np.int64)
                    first = np.cumsum(r_len_n) - r_len_n               # (the colour runs partition the positions in order: a run's first global position)
                    kmer_off = first[np.minimum(c_off_n[:-1], R - 1)]   # the first position of every unitig
                    f_found, f_bits, f_seg = host_fold(Q, k, L + 1, N, num, den,
                                                       (np.frombuffer(run_off, dtype=np.uint64).astype(np.int64), np.frombuffer(start, dtype=np.uint64, count=TR),
                                                        np.frombuffer(place, dtype=np.uint64, count=TR), np.frombuffer(ln, dtype=np.uint32, count=TR)),
                                                       (kmer_off, first, r_len_n, np.frombuffer(r_cls, dtype=np.uint32, count=R), np.frombuffer(c_bits, dtype=np.uint32, count=NC * NW).reshape(NC, NW), NW))
                    t2 = time.perf_counter()
                t["host_device_calls"].append((t1 - t0) * 1e3); t["host_fold"].append((t2 - t1) * 1e3); t["host_route"].append((t2 - t0) * 1e3)
                agree = bool(f_seg == SEG and np.array_equal(f_found, np.frombuffer(found, dtype=np.uint32)) and np.array_equal(f_bits.reshape(-1), np.frombuffer(bits, dtype=np.uint32)))
            res["n%d" % N] = {"colours": N, "colour_runs": R, "classes": NC, "windows": out5[0], "found": out5[1], "thread_runs": TR, "segments": SEG, "reported": out5[3],
                              "windows_per_sequence": n_win, "routes_agree": agree,
                              "bytes_back": {"device_route": Q * (8 + 4 * NW), "host_route": 8 * (Q + 1) + 20 * TR + 8 * (U + 1) + 12 * R + 4 * NW * NC},
                              "median_ms": {x: statistics.median(v) for x, v in t.items()}, "all_ms": t}
    finally:
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
