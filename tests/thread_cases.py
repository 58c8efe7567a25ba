"""Shared helpers, inputs and test bodies of the run-length lookup tests (test_hostsim_thread.py on the simulator, test_gpu_thread.py on the
device): cdbg_thread / cdbg_fetch_runs / `bcalm -thread`.

Expected runs never come from the code under test: they are fold(), a Python run-length fold of query_cases.expected() -- the brute-force
index over g.unitigs() or over the loaded sequences -- that follows the definition of a run in include/cdbg.h.  Every check also asserts,
for every run, that its unitig spells the query's bases (strand +) or their reverse complement (strand -)."""
import gzip
import os
import random
import subprocess

import kwidth_cases as kc
import oracle_lib
import quant_cases as qn
import query_cases as qc
from bcalm_amd import api

E_STATE = qc.E_STATE
rc = qc.rc


def fold(rows):
    """per query the runs (q, unitig, offset, strand, n) of its per-position expectations (as query_cases.expected() returns them): a hit
    continues the hit one position before it on the same unitig and strand at offset + 1 (strand +) or offset - 1 (strand -)"""
    out = []
    for row in rows:
        runs, prev = [], None
        for p, h in enumerate(row):
            if h is not None:
                if prev is not None and (h[0], h[2]) == (prev[0], prev[2]) and h[1] == prev[1] + (1 if h[2] == "+" else -1):
                    runs[-1][4] += 1
                else:
                    runs.append([p, h[0], h[1], h[2], 1])
            prev = h
        out.append([tuple(r) for r in runs])
    return out


def runs_of(raw, queries):
    """the ctypes arrays of thread_raw as the per-sequence lists Graph.thread() returns"""
    _, run_off, start, place, ln = raw
    out, at = [], 0
    for i, q in enumerate(queries):
        out.append([(start[r] - at, place[r] >> 33, (place[r] >> 1) & 0xFFFFFFFF, "-" if place[r] & 1 else "+", ln[r]) for r in range(run_off[i], run_off[i + 1])])
        at += len(q)
    return out


def run_bytes(raw):
    tot, run_off, start, place, ln = raw
    r = tot["runs"]
    return bytes(run_off) + bytes(start)[:8 * r] + bytes(place)[:8 * r] + bytes(ln)[:4 * r]


def check(g, seqs, k, queries, idx=None, **kw):
    """thread `queries` and compare runs and totals with the fold of the brute-force index over `seqs` (the resident set); every run must
    be spelled by its unitig; -> (totals, runs per query, the raw arrays)"""
    idx = qc.brute_index(seqs, k) if idx is None else idx
    rows = qc.expected(seqs, idx, k, queries)
    exp = fold(rows)
    raw = g.thread_raw(queries, **kw)
    tot = raw[0]
    got = runs_of(raw, queries)
    assert raw[1][0] == 0 and raw[1][len(queries)] == tot["runs"] == sum(len(r) for r in exp)
    up = [s.upper() for s in seqs]
    for qi, (q, gr, er) in enumerate(zip(queries, got, exp)):
        assert gr == er, (qi, gr[:5], er[:5])
        for p, u, o, s, n in gr:
            span = q[p:p + n + k - 1].upper()
            assert len(span) == n + k - 1
            if s == "+":
                assert up[u][o:o + n + k - 1] == span, (qi, p, u, o, s, n)
            else:
                assert o - n + 1 >= 0 and up[u][o - n + 1:o + k] == rc(span), (qi, p, u, o, s, n)
    assert tot["windows"] == sum(1 for q in queries for _ in qn.windows_of(q, k))
    assert tot["found"] == sum(1 for row in rows for h in row if h is not None) == sum(n for r in got for *_, n in r)
    assert tot["extended"] <= tot["found"]
    if not kw:
        assert g.thread(queries) == got
    return tot, got, raw


def refused(call, what):
    try:
        call()
        raise AssertionError("no error: " + what)
    except api.CdbgError as e:
        assert e.code == E_STATE and what in str(e), e


# ---------------------------------------------------------------- 1. every key width
def key_width(lib, k, amin, extends=True):
    text = kc.edge_text(k, 1)
    g = qc.built(lib, text, k, amin)
    try:
        ut = [s for s, _ in g.unitigs()]
        reads = text.split("\n")
        tot, got, _ = check(g, ut, k, qc.variants(reads, k, k))
        flat = [r for rs in got for r in rs]
        if k >= 5:
            assert any(n > 1 and s == "+" for *_, s, n in flat) and any(n > 1 and s == "-" for *_, s, n in flat)
            assert any(n == 1 for *_, n in flat)
            assert tot["windows"] > tot["found"] > 0
        else:                                                # (the reads spell every k-mer there is: every unitig is ONE k-mer)
            assert all(len(s) == k for s in ut)
            assert tot["runs"] == tot["found"] > 0 and tot["extended"] == 0
        can_extend = any(len(s) > k for s in ut)
        assert (tot["extended"] > 0) == (can_extend and extends), tot
    finally:
        g.close()


# ---------------------------------------------------------------- 2. boundaries
def boundaries(lib, k):
    text = kc.edge_text(k, 2)
    g = qc.built(lib, text, k, 1)
    try:
        ut = [s for s, _ in g.unitigs()]
        idx = qc.brute_index(ut, k)
        U = max(ut, key=len)
        assert len(U) >= 2 * k + 5
        V = U[:2 * k + 5]
        qs = [V[:k - 1], V[:k], V[:k + 1], "", "", rc(V[:k + 1]), "ACGT" * k]
        cuts = list(range(1, len(V)))
        for c in cuts:                                       # V cut at every offset into two adjacent sequences
            qs += [V[:c], V[c:]]
        tot, got, raw = check(g, ut, k, qs, idx=idx)
        assert got[0] == [] and len(got[1]) == 1 and got[1][0][4] == 1 and got[2][0][4] == 2 and got[3] == got[4] == []
        assert got[5][0][3] != got[2][0][3] and got[5][0][4] == 2
        whole = check(g, ut, k, [V], idx=idx)[1][0]
        assert len(whole) == 1 and whole[0][4] == len(V) - k + 1     # the uncut bytes are ONE run ...
        for j, c in enumerate(cuts):                                 # ... and each cut gives two runs, never one
            a, b = got[7 + 2 * j], got[7 + 2 * j + 1]
            assert [n for *_, n in a] == ([c - k + 1] if c >= k else []), (c, a)
            assert [n for *_, n in b] == ([len(V) - c - k + 1] if len(V) - c >= k else []), (c, b)
        assert run_bytes(g.thread_raw(qs, first_offset=37)) == run_bytes(raw)      # offsets[0] != 0
    finally:
        g.close()


# ---------------------------------------------------------------- 3. tile seams and density
TILE = 8192                                                  # every power-of-two tile up to it has an edge at its multiples


def seam_set(k=31):
    rng = random.Random(31)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    return [rnd(3 * TILE + 200), rnd(300)]


def _sub(s, i):
    return s[:i] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s[i]] + s[i + 1:]


def long_runs(lib, k=31):
    seqs = seam_set(k)
    A = seqs[0]
    idx = qc.brute_index(seqs, k)
    g = qc.loaded(lib, seqs, k)
    try:
        info = g.index_info()
        assert info["positions"] == info["distinct"]
        tot, got, _ = check(g, seqs, k, [A], idx=idx)
        assert got == [[(0, 0, 0, "+", len(A) - k + 1)]] and tot["extended"] > 0
        assert check(g, seqs, k, [rc(A)], idx=idx)[1] == [[(0, 0, len(A) - k, "-", len(A) - k + 1)]]
        for j in (1, 2):                                     # each in a call of its own: the query position is the tile position
            got = check(g, seqs, k, [_sub(A, TILE * j - 1)], idx=idx)[1][0]
            assert any(q == TILE * j for q, *_ in got) and len(got) == 2, got          # a head exactly at the tile's first position
            got = check(g, seqs, k, [_sub(A, TILE * j + k - 1)], idx=idx)[1][0]
            assert any(q + n - 1 == TILE * j - 1 for q, *_, n in got) and len(got) == 2, got   # a tail exactly at the last position of the tile before
    finally:
        g.close()


def full_density(lib):
    k = 4
    g = qc.built(lib, kc.edge_text(k, 1), k, 1)
    try:
        ut = [s for s, _ in g.unitigs()]
        assert len(ut) == 136 and all(len(s) == k for s in ut)       # every 4-mer there is, each a unitig of its own
        rng = random.Random(4)
        q = "".join(rng.choice("ACGT") for _ in range(3 * TILE + 100))
        for at in (5000, TILE - 1, 20000):
            q = q[:at] + "N" + q[at + 1:]
        tot, got, _ = check(g, ut, k, [q])
        assert tot["runs"] == tot["found"] == tot["windows"] == len(q) - k + 1 - 3 * k     # every lane of every tile holds a head and a tail
        assert tot["extended"] == 0
    finally:
        g.close()


def extension_edges(lib, monkeypatch, k):
    """quant_cases.edge_text: a genome longer than a tile as one read, branches, a unitig of exactly k bases -- walked on both strands with
    and without extension: the same bytes, and those of the fold"""
    reads = qn.edge_text(k)
    g = qc.built(lib, "\n".join(reads) + "\n", k, 1)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    qs = list(reads) + [rc(r) for r in reads]
    by_len = sorted(ut, key=len)
    for s in by_len[-6:]:
        if len(s) > k + 2:
            qs += [_sub(s, k), _sub(rc(s), k), _sub(s, len(s) - 1), rc(s) + "ACGT"]
    idx = qc.brute_index(ut, k)
    got = []
    for env in ({}, {"CDBG_QUANT_NO_EXTEND": "1"}):
        g = qn._fresh(lib, ut, k, monkeypatch, env)
        try:
            tot, _, raw = check(g, ut, k, qs, idx=idx)
            assert (tot["extended"] == 0) if env else (tot["extended"] > 0), tot
            got.append(run_bytes(raw))
        finally:
            g.close()
    assert got[0] == got[1]


def palindrome(lib, monkeypatch, k=16):
    """a loaded sequence with a k-mer that is its own reverse complement in its middle, every k-mer spelled once (so the producer extends):
    the k-mer reports strand + and cuts the strand - walk of the reverse complement in three, with and without extension"""
    rng = random.Random(16)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    h = rnd(k // 2)
    X, Y = rnd(50), rnd(50)
    while rc(X[-1]) == Y[0]:                                 # (the k-mers beside the palindrome must not be each other's reverse complement)
        Y = rnd(50)
    P = X + h + rc(h) + Y
    seqs = [rnd(60), P]
    idx = qc.brute_index(seqs, k)
    got = []
    for env in ({}, {"CDBG_QUANT_NO_EXTEND": "1"}):
        g = qn._fresh(lib, seqs, k, monkeypatch, env)
        try:
            info = g.index_info()
            assert info["positions"] == info["distinct"]
            tot, runs, raw = check(g, seqs, k, [P, rc(P)], idx=idx)
            assert runs[0] == [(0, 1, 0, "+", len(P) - k + 1)]
            assert [(s, n) for *_, s, n in runs[1]] == [("-", 50), ("+", 1), ("-", 50)] and runs[1][1][2] == 50, runs[1]
            assert (tot["extended"] == 0) if env else (tot["extended"] > 0), tot
            got.append(run_bytes(raw))
        finally:
            g.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------- 4. batches: the result must not depend on the batch size
def batches(lib, monkeypatch, k=31):
    text = oracle_lib.read_input("rand_b")
    g = qc.built(lib, text, k, 2)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    batch = max(4 * k, 256)                                  # the floor of CDBG_QUERY_BATCH
    reads = [r for r in text.split("\n") if r]
    rng = random.Random(5)
    long = "".join(ut)                                       # one sequence of 20 batches and more
    while len(long) < 20 * batch:
        long += rc(long)
    long = long[:20 * batch + 17]
    many = []
    for i in range(200):
        r = reads[i % len(reads)]
        n = rng.randrange(k, 3 * k + 1)
        s = rng.randrange(0, max(1, len(r) - n))
        many.append(r[s:s + n] if i % 3 else rc(r[s:s + n]))
    qs = [long] + many + ["", long[5:9 * batch]] + many[:50]
    idx = qc.brute_index(ut, k)
    got = []
    for env in ({}, {"CDBG_QUERY_BATCH": "1"}):
        g = qn._fresh(lib, ut, k, monkeypatch, env)
        try:
            tot, runs, raw = check(g, ut, k, qs, idx=idx)
            assert any(n > batch for *_, n in runs[0])       # runs that span many seams
            got.append(run_bytes(raw))
        finally:
            g.close()
    assert got[0] == got[1]
    seqs = seam_set(k)                                       # the single 24 k run of long_runs(), cut by ~100 seams, is still one run
    A = seqs[0]
    g = qn._fresh(lib, seqs, k, monkeypatch, {"CDBG_QUERY_BATCH": "1"})
    try:
        raw = g.thread_raw([A])
        assert runs_of(raw, [A]) == [[(0, 0, 0, "+", len(A) - k + 1)]] and raw[0]["runs"] == 1
    finally:
        g.close()


# ---------------------------------------------------------------- 5. repeated k-mers (loaded sets)
def repeated_handmade(lib, runs=1):
    k = 8
    seqs, qs, pal = qc.handmade(k)
    qs = qs + [s for s in seqs[-45:]]                        # the LATER copies of the records as queries: placed at the first copy
    idx = qc.brute_index(seqs, k)
    ref = None
    for _ in range(runs):
        g = qc.loaded(lib, seqs, k)
        try:
            tot, got, raw = check(g, seqs, k, qs, idx=idx)
            assert tot["extended"] == 0                      # a set that repeats k-mers: every window probes
            info = g.index_info()
            assert info["distinct"] < info["positions"]
            assert any(n > 1 for r in got for *_, n in r)
            b = run_bytes(raw)
        finally:
            g.close()
        assert ref is None or b == ref
        ref = b


# ---------------------------------------------------------------- 6. state
def state(lib):
    k = 15
    ta, tb = oracle_lib.read_input("rand_a"), oracle_lib.read_input("rand_b")
    reads_a = [r for r in ta.split("\n") if r][:30]
    reads_b = [r for r in tb.split("\n") if r][:30]
    A = reads_a + [rc(r) for r in reads_a[:10]] + ["ACGT" * 10]
    B = reads_b + reads_a[5:15] + ["N" + reads_a[0]]
    u64, u32 = api.C.c_uint64, api.C.c_uint32
    g = api.Graph(k, 2, lib=lib)
    fetch = lambda *a: g._ck(lib.cdbg_fetch_runs(g._h, *a))
    try:
        refused(lambda: g.thread(A), "cdbg_thread before cdbg_glue")
        refused(lambda: fetch(None, None, None, None), "cdbg_fetch_runs before cdbg_glue")
        g.push_text(ta); g.count()
        refused(lambda: g.thread(A), "before cdbg_glue")
        g.compact(); g.glue()
        ua = [s for s, _ in g.unitigs()]
        refused(lambda: fetch(None, None, None, None), "cdbg_fetch_runs before cdbg_thread")
        hits = g.query(A)
        ta_, ra, raw_a = check(g, ua, k, A)
        assert g.query(A) == hits                            # the lookup is what it was
        tb_, rb, raw_b = check(g, ua, k, B)                  # a second call replaces the first result
        assert ra != rb
        n = tb_["runs"]
        off, start, place, ln = (u64 * (len(B) + 1))(), (u64 * n)(), (u64 * n)(), (u32 * n)()
        fetch(None, None, None, None)                        # NULL outputs: any of them
        fetch(off, None, None, None); fetch(None, start, None, ln); fetch(None, None, place, None)
        assert bytes(off) + bytes(start) + bytes(place) + bytes(ln) == run_bytes(raw_b)
        fetch(off, start, place, ln)                         # ... and the result stays until the next call
        assert bytes(off) + bytes(start) + bytes(place) + bytes(ln) == run_bytes(raw_b)
        zero = {"windows": 0, "found": 0, "runs": 0, "extended": 0}
        raw = g.thread_raw([])                               # n = 0 succeeds: zeros and no runs
        assert raw[0] == zero and list(raw[1]) == [0]
        raw = g.thread_raw(["", ""])
        assert raw[0] == zero and list(raw[1]) == [0, 0, 0] and g.thread(["", ""]) == [[], []]
        out = (u64 * 4)()
        g._ck(lib.cdbg_thread(g._h, None, None, 0, out))
        assert list(out) == [0, 0, 0, 0]
        check(g, ua, k, A)
        g.reset()                                            # reset forgets the result
        refused(lambda: fetch(None, None, None, None), "cdbg_fetch_runs before cdbg_glue")
        g.run()                                              # (the reads stay resident: the same graph, rebuilt)
        refused(lambda: fetch(None, None, None, None), "cdbg_fetch_runs before cdbg_thread")
        check(g, [s for s, _ in g.unitigs()], k, A)
    finally:
        g.close()
    g = api.Graph(k, 2, lib=lib)
    try:
        g.push_text(tb); g.run()
        ub = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    # load -> thread -> reset -> load of another set: the result goes with the set, and the runs follow the second set
    g = api.Graph(k, 1, lib=lib)
    fetch = lambda *a: g._ck(lib.cdbg_fetch_runs(g._h, *a))
    try:
        g.load_unitigs(ua)
        check(g, ua, k, A + B)
        g.reset()
        g.load_unitigs(ub)
        refused(lambda: fetch(None, None, None, None), "cdbg_fetch_runs before cdbg_thread")
        check(g, ub, k, A + B)
    finally:
        g.close()


def state_two_ranks(lib, monkeypatch, memcpy):
    """a rank that holds a share of the unitigs cannot answer for the graph: world_size = 2, and one rank sent through the multi-rank
    path (CDBG_FORCE_MULTI, in-process loop-back transport) up to a glued graph"""
    import loopback
    qs = ["ACGTACGTACGTACGTACGT"]

    def all_refused(g):
        refused(lambda: g.thread(qs), "cdbg_thread: one rank only")
        refused(lambda: g._ck(lib.cdbg_fetch_runs(g._h, None, None, None, None)), "cdbg_fetch_runs: one rank only")
    g = api.Graph(15, 2, lib=lib, world_size=2, rank=0)
    try:
        all_refused(g)
    finally:
        g.close()
    monkeypatch.setenv("CDBG_FORCE_MULTI", "1")
    g = api.Graph(15, 2, lib=lib)
    try:
        hub = loopback.Loopback(1, memcpy)
        hub.memcpy_d2h = hub.memcpy_h2d = memcpy
        hub.endpoint(0).attach(g)
        g.push_text(oracle_lib.read_input("rand_a")); g.run()
        assert g.stats()["n_unitigs"] > 0
        all_refused(g)
    finally:
        g.close()
        monkeypatch.delenv("CDBG_FORCE_MULTI")


# ---------------------------------------------------------------- 7. CLI
def cli(exe, tmp_path, name, k):
    """<prefix>.thread.tsv must be byte-identical to the <prefix>.query.tsv that -query folds on the host from the same files"""
    text = oracle_lib.read_input(name)
    refs = [r for r in text.split("\n") if r]
    d = tmp_path / ("cli_" + name); d.mkdir()
    with open(d / "reads.fa", "w") as f:
        for i, r in enumerate(refs):
            f.write(">r%d\n%s\n" % (i, r))
    run = lambda args: subprocess.run([exe] + args, cwd=d, capture_output=True, text=True, timeout=600)
    r = run(["-in", "reads.fa", "-kmer-size", str(k), "-abundance-min", "1", "-out", "g"])
    assert r.returncode == 0, r.stdout + r.stderr
    fa = (d / "g.unitigs.fa").read_bytes()
    rng = random.Random(k)
    queries = refs[:60] + [rc(r) for r in refs[:20] if set(r) <= qc.ACGT] + ["".join(rng.choice("ACGT") for _ in range(2 * k + 9)), "ACG", refs[0][:k] + "N" + refs[0][k:]]
    with gzip.open(d / "q.fa.gz", "wt") as f:                # gzip FASTA, sequences wrapped at 50 columns, a description behind every name
        for i, q in enumerate(queries):
            f.write(">q%d some description\n" % i)
            for j in range(0, len(q), 50):
                f.write(q[j:j + 50] + "\n")
    with open(d / "q.fq", "w") as f:
        for i, q in enumerate(queries):
            f.write("@q%d/1 x\n%s\n+\n%s\n" % (i, q, "I" * len(q)))
    base = ["-in", "g.unitigs.fa", "-kmer-size", str(k)]
    for qf in ("q.fa.gz", "q.fq"):
        r = run(base + ["-query", qf])
        assert r.returncode == 0, r.stdout + r.stderr
        exp = (d / "g.query.tsv").read_bytes()
        assert b":+:" in exp and b":-:" in exp and b"\t*\n" in exp and exp.count(b"\n") == len(queries)
        r = run(base + ["-thread", qf])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "thread: %d sequences, " % len(queries) in r.stdout and "runs written to g.thread.tsv" in r.stdout, r.stdout
        assert (d / "g.thread.tsv").read_bytes() == exp
        assert (d / "g.unitigs.fa").read_bytes() == fa       # untouched
        assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa", "g.query.tsv", "g.thread.tsv", "q.fa.gz", "q.fq"])
        os.remove(d / "g.query.tsv"); os.remove(d / "g.thread.tsv")
    for args, msg in ((base + ["-thread", "q.fq", "-nb-gpus", "2"], "-nb-gpus must be 1"),
                      (base + ["-thread", "q.fq", "-query", "q.fq"], "separate modes"),
                      (base + ["-thread", "q.fq", "-quantify", "q.fq"], "separate modes"),
                      (base + ["-thread", "q.fq", "-redo-links"], "separate modes"),
                      (base + ["-thread"], "needs a value"),
                      (base + ["-thread", "nothing.fa"], "cannot open query file"),
                      (["-in", "absent.unitigs.fa", "-kmer-size", str(k), "-thread", "q.fq"], "cannot open")):
        r = run(args)
        assert r.returncode == 1 and msg in r.stdout + r.stderr, (args, r.stdout, r.stderr)
    assert (d / "g.unitigs.fa").read_bytes() == fa
    assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa", "q.fa.gz", "q.fq"])
