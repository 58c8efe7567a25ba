"""Timing of the k-mer lookup (cdbg_index / cdbg_query) in the shape of DESIGN.md's timing tables: one MI355X, k = 31, abundance-min 2,
the 10 M x 150 bp config-3 graph; host wall time around each call, three repeats.

  python bench_micro/query_timing.py [--reads 10000000] [--queries 1000000] [--lib <libcdbg.so built with -DCDBG_PROFILE_PHASES>] [--host-map]

Reports (one JSON line at the end):
  * cdbg_index: ms, table bytes;
  * cdbg_query of --queries of the graph's own reads and of the same reads complemented without reversal (as good as random: misses): M k-mers/s including the
    copies, and kernel-only (the library's own event timer, printed under CDBG_HOST_MARKS=1);
  * mean slots read per looked-up k-mer, when --lib names a build with the counter compiled in (CDBG_PROFILE_PHASES);
  * --host-map: the same lookup on the host, single thread, with the structure bcalm_tools keeps its end k-mers in
    (std::unordered_map<std::string, ...>; bench_micro/query_host_map.cpp, built on first use): map over every k-mer of the unitigs,
    lookup timed over the first --host-queries reads and reported per k-mer."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CDBG_HOST_MARKS"] = "1"                       # (read once per process by the library: set before it is loaded)
import bcalm_amd  # noqa: E402
from bcalm_amd import api  # noqa: E402


class Stderr:
    """what the library writes to file descriptor 2 inside the block"""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0); self.text = self.tmp.read().decode(errors="replace"); self.tmp.close()


def time_query(g, text, n, read_len, k, repeats):
    off = (C.c_uint64 * (n + 1))(*range(0, (n + 1) * (read_len + 1), read_len + 1))     # (the separator rides at the end of every read: one more broken window)
    hits = (C.c_uint64 * len(text))()
    kmers = n * (read_len - k + 1)                            # (the window that holds the separator is not looked up)
    out = []
    for _ in range(repeats):
        with Stderr() as err:
            t = time.perf_counter()
            g._ck(g.lib.cdbg_query(g._h, text, off, n, hits))
            wall = time.perf_counter() - t
        m = re.search(r"\[query\] positions (\d+) kernel_ms ([0-9.]+) looked_up (\d+) slots_read (\d+)", err.text)
        kernel_ms, looked, slots = float(m.group(2)), int(m.group(3)), int(m.group(4))
        out.append({"wall_ms": wall * 1e3, "mkmers_s": kmers / wall / 1e6, "kernel_ms": kernel_ms, "kernel_mkmers_s": kmers / kernel_ms / 1e3,
                    "slots_per_kmer": slots / looked if looked else None})
    found = sum(1 for i in range(0, min(len(text), 2000 * (read_len + 1))) if hits[i] != api.Graph.MISS)
    return out, found / (min(n, 2000) * (read_len - k + 1))


def host_map(g, text, n, read_len, k):
    exe = os.path.join(ROOT, "bench_micro", "variants", "query_host_map")
    src = os.path.join(ROOT, "bench_micro", "query_host_map.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe])
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "u.txt"), "w") as f:
            for s, _ in g.unitigs():
                f.write(s + "\n")
        with open(os.path.join(d, "q.txt"), "wb") as f:
            f.write(text[:n * (read_len + 1)])
        r = subprocess.run([exe, os.path.join(d, "u.txt"), os.path.join(d, "q.txt"), str(k)], capture_output=True, text=True, check=True)
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--host-map", action="store_true")
    ap.add_argument("--host-queries", type=int, default=100_000)
    a = ap.parse_args()
    lib = bcalm_amd.load(a.lib)
    k, L = a.k, a.read_len
    res = {"k": k, "reads": a.reads, "queries": a.queries, "index": []}
    g = api.Graph(k, 2, lib=lib)
    try:
        g.generate_reads(a.reads, L, 3)
        for _ in range(a.repeats):
            with Stderr():
                g.reset(); g.run()
                t = time.perf_counter(); g.index(); res["index"].append((time.perf_counter() - t) * 1e3)
        res["index_info"] = g.index_info()
        res["unitigs"] = g.stats()["n_unitigs"]
        own = g.read_text(0, a.queries * (L + 1))
        res["own"], res["own_found"] = time_query(g, own, a.queries, L, k, a.repeats)
        # reads the graph does not hold.  (Not "another seed": the generator's genome of seed s is the genome of seed 0 shifted by s bases,
        # k_scan.h gen_genome_base, so its reads hit.)  The own reads complemented WITHOUT reversal: as good as random to the graph
        other = own.translate(bytes.maketrans(b"ACGT", b"TGCA"))
        res["other"], res["other_found"] = time_query(g, other, a.queries, L, k, a.repeats)
        if a.host_map:
            res["host_map_own"] = host_map(g, own, min(a.queries, a.host_queries), L, k)
    finally:
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
