"""Shared helpers, inputs and test bodies of the k-mer lookup tests (test_hostsim_query.py on the simulator, test_gpu_query.py on the
device): cdbg_index / cdbg_query / `bcalm -query`.

Expected values never come from the code under test.  Three independent sources:
  (a) brute_index(): a Python dict canonical k-mer -> smallest (unitig, offset) over the sequences the graph reports through
      g.unitigs() (pinned against the oracle by the other suites), or over the sequences handed to load_unitigs;
  (b) the oracle's solid set: for a built graph a k-mer of any text is found <=> it is a solid k-mer of oracle.run(text, k, amin);
  (c) self-consistency: for every hit, unitigs[u][o:o + k] is the query k-mer (strand +) or its reverse complement (strand -).
check() asserts that its queries produced a hit on each strand and a miss: a kernel that answers "miss" everywhere cannot pass."""
import ctypes as C
import gzip
import os
import random
import subprocess

import kwidth_cases as kc
import oracle_lib
from bcalm_amd import api

COMP = str.maketrans("ACGTacgt", "TGCAtgca")
MISS = 0xFFFFFFFFFFFFFFFF
E_STATE = -4
ACGT = set("ACGT")


def rc(s):
    return s[::-1].translate(COMP)


def canon(x):
    r = rc(x)
    return r if r < x else x


def brute_index(seqs, k):
    """(a): canonical k-mer -> the smallest (unitig, offset) at which `seqs` spell it or its reverse complement"""
    idx = {}
    for u, s in enumerate(seqs):
        s = s.upper()
        for o in range(len(s) - k + 1):
            idx.setdefault(canon(s[o:o + k]), (u, o))
    return idx


def expected(seqs, idx, k, queries):
    """per query the list g.query() must return"""
    seqs = [s.upper() for s in seqs]
    out = []
    for q in queries:
        q = q.upper()
        row = []
        for p in range(len(q) - k + 1):
            x = q[p:p + k]
            e = None
            if set(x) <= ACGT:
                at = idx.get(canon(x))
                if at is not None:
                    e = (at[0], at[1], "+" if seqs[at[0]][at[1]:at[1] + k] == x else "-")
            row.append(e)
        out.append(row)
    return out


def check(g, seqs, k, queries, solid=None, idx=None):
    """g.query(queries) against (a) over `seqs` (the resident set), (c) for every hit and -- solid given -- (b); -> (hits +, hits -, misses)"""
    idx = brute_index(seqs, k) if idx is None else idx
    got = g.query(queries)
    exp = expected(seqs, idx, k, queries)
    n = {"+": 0, "-": 0, None: 0}
    up = [s.upper() for s in seqs]
    for qi, (q, gr, er) in enumerate(zip(queries, got, exp)):
        assert len(gr) == max(0, len(q) - k + 1), (qi, len(q), len(gr))
        for p, (h, e) in enumerate(zip(gr, er)):
            assert h == e, (qi, p, h, e, q[p:p + k])
            x = q[p:p + k].upper()
            if h is not None:
                u, o, s = h
                assert up[u][o:o + k] == (x if s == "+" else rc(x))                       # (c)
            if solid is not None:
                assert (h is not None) == (set(x) <= ACGT and canon(x) in solid), (qi, p, x)   # (b)
            n[h[2] if h else None] += 1
    assert n["+"] > 0 and n["-"] > 0 and n[None] > 0, n
    return n["+"], n["-"], n[None]


def variants(reads, k, seed):
    """the queries of the key-width sweep: the reads, their reverse complements, each with one substitution every ~k bases, a lower-case copy, and reads with
    N at offsets 0, k - 1 and k"""
    rng = random.Random(seed)
    reads = [r for r in reads if r]
    out = list(reads) + [rc(r) for r in reads if set(r) <= ACGT]
    for r in reads:
        t = list(r)
        for i in range(rng.randrange(0, k), len(t), k):
            t[i] = rng.choice([c for c in "ACGT" if c != t[i].upper()])
        out.append("".join(t))
    out += [r.lower() for r in reads]
    long = [r for r in reads if len(r) > 2 * k and set(r) <= ACGT]
    for j, at in enumerate((0, k - 1, k)):
        r = long[j % len(long)]
        out.append(r[:at] + "N" + r[at + 1:])
    return out


def built(lib, text, k, amin, **kw):
    g = api.Graph(k, amin, lib=lib, **kw)
    g.push_text(text); g.run()
    return g


def loaded(lib, seqs, k):
    g = api.Graph(k, 1, lib=lib)
    g.load_unitigs(seqs)
    return g


def solid_set(oracle, text, k, amin):
    return {x for x, _ in oracle.run(text, k, amin, want_solid=True)["solid"]}


def hit_bytes(g, queries, **kw):
    hits, off = g.query_raw(queries, **kw)
    return bytes(hits)[:8 * off[-1]]


# ---------------------------------------------------------------- 1. every key width
def key_width(lib, oracle, k, amin):
    text = kc.edge_text(k, 1)
    g = built(lib, text, k, amin)
    try:
        ut = [s for s, _ in g.unitigs()]
        reads = text.split("\n")
        check(g, ut, k, variants(reads, k, k), solid=solid_set(oracle, text, k, amin) if amin == 2 else None)
        info = g.index_info()
        assert info["positions"] == info["distinct"] == g.stats()["n_solid"], (info, g.stats()["n_solid"])
        assert info["slots"] & (info["slots"] - 1) == 0 and info["slots"] >= 1.5 * info["positions"] + 64 > info["slots"] / 2
        assert info["bytes"] == 8 * info["slots"]
    finally:
        g.close()


# ---------------------------------------------------------------- 2. boundaries
def boundaries(lib, k):
    text = kc.edge_text(k, 2)
    g = built(lib, text, k, 1)
    try:
        ut = [s for s, _ in g.unitigs()]
        idx = brute_index(ut, k)
        U = max(ut, key=len)
        assert len(U) >= 2 * k + 5
        V = U[:2 * k + 5]
        qs = [V[:k - 1], V[:k], V[:k + 1], "", "", rc(V[:k + 1]), "ACGT" * k]
        for c in range(1, len(V)):                           # V cut at every offset into two adjacent sequences
            qs += [V[:c], V[c:]]
        check(g, ut, k, qs, idx=idx)
        hits, off = g.query_raw(qs)
        for i in range(len(qs)):                             # the last k - 1 windows of every sequence miss, whatever the bytes behind them spell
            for p in range(max(off[i], off[i + 1] - k + 1), off[i + 1]):
                assert hits[p] == MISS, (i, p)
        assert hits[off[1]] != MISS and hits[off[2]] != MISS and hits[off[2] + 1] != MISS       # (the k and k + 1 base sequences themselves hit)
        whole = g.query([V])[0]
        assert all(h is not None for h in whole)             # ... and the uncut bytes do spell present k-mers
        assert hit_bytes(g, qs, first_offset=37) == hit_bytes(g, qs)                             # offsets[0] != 0
    finally:
        g.close()


# ---------------------------------------------------------------- 3. batches / 4. probe runs: the same set under a test hook
def _same_under(lib, monkeypatch, seqs, k, queries, env):
    """hits of `queries` against the loaded set `seqs`, with and without the environment `env` (read when a context is created)"""
    g = loaded(lib, seqs, k)
    try:
        check(g, seqs, k, queries)
        ref = hit_bytes(g, queries)
        ref_info = g.index_info()
    finally:
        g.close()
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    g = loaded(lib, seqs, k)
    try:
        got = hit_bytes(g, queries)
        info = g.index_info()
    finally:
        g.close()
        for name in env:
            monkeypatch.delenv(name)
    assert got == ref
    return ref_info, info


def batches(lib, monkeypatch, k=31):
    text = oracle_lib.read_input("rand_b")
    g = built(lib, text, k, 2)
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
    _same_under(lib, monkeypatch, ut, k, [long] + many + ["", long[5:9 * batch]] + many[:50], {"CDBG_QUERY_BATCH": "1"})


PROBE_CASES = [("rand_a", 15), ("rand_b", 31), ("edge127", 127)]


def probe_runs(lib, monkeypatch, name, k):
    text = kc.edge_text(k, 1) if name == "edge127" else oracle_lib.read_input(name)
    g = built(lib, text, k, 1 if name == "edge127" else 2)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    reads = [r for r in text.split("\n") if r]
    qs = variants(reads[:40], k, 3)
    ref_info, info = _same_under(lib, monkeypatch, ut, k, qs, {"CDBG_INDEX_LOG2_SLOTS": "0"})
    forced = 1
    while forced <= info["distinct"]:                        # the smallest power of two > distinct k-mers
        forced *= 2
    assert info["slots"] == forced <= ref_info["slots"], (info, ref_info)
    assert (info["positions"], info["distinct"]) == (ref_info["positions"], ref_info["distinct"])


# ---------------------------------------------------------------- 5. repeated k-mers (loaded sets)
def handmade(k=8, seed=11):
    """(sequences, queries): records three times over, records beside their reverse complements, and a k-mer that is its own reverse complement"""
    rng = random.Random(seed)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    R = [rnd(rng.randrange(k, 40)) for _ in range(40)]
    S = [rnd(rng.randrange(k, 30)) for _ in range(10)]
    h = rnd(k // 2)
    pal = h + rc(h)
    seqs = []
    for r in R:
        seqs += [r]
    seqs += [pal]
    for s in S:
        seqs += [s, rc(s)]
    seqs += R + [rc(s).lower() for s in S] + R + [pal]
    qs = R[:10] + [rc(r) for r in R[:10]] + S + [rc(s) for s in S] + [pal, rc(pal), rnd(60), "N" + R[0], pal[:k - 1]]
    return seqs, qs, pal


def repeated_handmade(lib, runs=1):
    k = 8
    seqs, qs, pal = handmade(k)
    ref = None
    for _ in range(runs):
        g = loaded(lib, seqs, k)
        try:
            check(g, seqs, k, qs)
            at = g.query([pal])[0][0]
            assert at is not None and at[2] == "+" and seqs[at[0]].upper()[at[1]:at[1] + k] == pal     # its own reverse complement: strand +
            info = g.index_info()
            assert info["distinct"] < info["positions"] == sum(len(s) - k + 1 for s in seqs)
            assert info["distinct"] == len(brute_index(seqs, k))
            b = hit_bytes(g, qs)
        finally:
            g.close()
        assert ref is None or b == ref
        ref = b


def repeated_reads(lib, name, k):
    """the reads of a golden input as a loaded set: a foreign FASTA that spells most k-mers many times"""
    text = oracle_lib.read_input(name)
    seqs = []
    for line in text.split("\n"):
        cur = ""
        for c in line + "N":
            if c.upper() in ACGT:
                cur += c
            else:
                if len(cur) >= k:
                    seqs.append(cur)
                cur = ""
    seqs = seqs[:400]
    rng = random.Random(k)
    qs = seqs[:30] + [rc(s) for s in seqs[:30]] + ["".join(rng.choice("ACGT") for _ in range(3 * k + 20)), seqs[0][:k - 1]]
    g = loaded(lib, seqs, k)
    try:
        check(g, seqs, k, qs)
        info = g.index_info()
        assert info["distinct"] == len(brute_index(seqs, k)) <= info["positions"] == sum(len(s) - k + 1 for s in seqs)
    finally:
        g.close()


def repeated_split(lib, tools, tmp_path, name, k):
    import test_relink
    _, pieces = test_relink._split_pieces(lib, tools, name, k, tmp_path)
    seqs = pieces + pieces[:20]                              # (the split pieces share no k-mer: a few of them once more)
    rng = random.Random(k)
    qs = pieces[:40] + [rc(s) for s in pieces[:40]] + ["".join(rng.choice("ACGT") for _ in range(3 * k + 20))]
    g = loaded(lib, seqs, k)
    try:
        check(g, seqs, k, qs)
        info = g.index_info()
        assert info["distinct"] < info["positions"]
    finally:
        g.close()


# ---------------------------------------------------------------- 6. state
def state(lib, multi_lib=None):
    k = 15
    ta, tb = oracle_lib.read_input("rand_a"), oracle_lib.read_input("rand_b")
    reads_a = [r for r in ta.split("\n") if r][:30]
    reads_b = [r for r in tb.split("\n") if r][:30]
    qs = reads_a + [rc(r) for r in reads_a] + reads_b + ["ACGT" * 10]
    g = api.Graph(k, 2, lib=lib)
    try:
        for call in (lambda: g.query(qs), g.index, g.index_info):                  # before glue
            try:
                call()
                raise AssertionError("no error before cdbg_glue")
            except api.CdbgError as e:
                assert e.code == E_STATE and "before cdbg_glue" in str(e), e
        g.push_text(ta); g.count()
        try:
            g.query(qs)
            raise AssertionError("no error before cdbg_glue")
        except api.CdbgError as e:
            assert e.code == E_STATE
        g.compact(); g.glue()
        ua = [s for s, _ in g.unitigs()]
        check(g, ua, k, qs)
        info = g.index_info()
        g.index(); g.index()                                 # a no-op on an indexed context
        assert g.index_info() == info
        check(g, ua, k, qs)
    finally:
        g.close()
    # one context run, queried, reset and run again, then a context over input B on the blocks the first handed to the pool: every index is built
    # in dirty memory, and the second answers are B's alone
    g = api.Graph(k, 2, lib=lib)
    try:
        g.push_text(ta); g.run()
        check(g, [s for s, _ in g.unitigs()], k, qs)
        g.reset()
        try:
            g.query(qs)
            raise AssertionError("the index survived cdbg_reset")
        except api.CdbgError as e:
            assert e.code == E_STATE
        g.run()                                              # (the reads stay resident: the same graph, rebuilt)
        check(g, [s for s, _ in g.unitigs()], k, qs)
    finally:
        g.close()
    g = api.Graph(k, 2, lib=lib)
    try:
        g.push_text(tb); g.run()
        ub = [s for s, _ in g.unitigs()]
        check(g, ub, k, qs)
    finally:
        g.close()
    # load -> reset -> load of another set: the answers follow the second set
    g = api.Graph(k, 1, lib=lib)
    try:
        g.load_unitigs(ua)
        check(g, ua, k, qs)
        ia = g.index_info()
        g.reset()
        g.load_unitigs(ub)
        check(g, ub, k, qs)
        assert g.index_info() != ia
        hits, off = g.query_raw([])                          # no sequences: nothing written
        assert off == [0] and hits[0] == 0
        assert g.query(["", ""]) == [[], []]
    finally:
        g.close()


def state_two_ranks(lib, monkeypatch, memcpy):
    """a rank that holds a share of the unitigs cannot answer for the graph: world_size = 2, and one rank sent through the multi-rank
    path (CDBG_FORCE_MULTI, in-process loop-back transport) up to a glued graph"""
    import loopback
    qs = ["ACGTACGTACGTACGTACGT"]

    def refused(g):
        for call in (g.index, g.index_info, lambda: g.query(qs)):
            try:
                call()
                raise AssertionError("no error on a rank of several")
            except api.CdbgError as e:
                assert e.code == E_STATE and "one rank only" in str(e), e
    g = api.Graph(15, 2, lib=lib, world_size=2, rank=0)
    try:
        refused(g)
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
        refused(g)
    finally:
        g.close()
        monkeypatch.delenv("CDBG_FORCE_MULTI")


# ---------------------------------------------------------------- 7. CLI
def fold_tsv(names, queries, rows, k):
    """the <prefix>.query.tsv `bcalm -query` must write, folded from per-position expectations `rows` (as expected() returns them)"""
    out = []
    for name, q, row in zip(names, queries, rows):
        runs, cur = [], None                                 # cur: [qpos, len, unitig, strand, upos, last offset]
        for p, h in enumerate(row):
            if h is not None and cur and (h[0], h[2]) == (cur[2], cur[3]) and h[1] == cur[5] + (1 if h[2] == "+" else -1):
                cur[1] += 1; cur[5] = h[1]
                continue
            if cur:
                runs.append(cur)
            cur = [p, 1, h[0], h[2], h[1], h[1]] if h is not None else None
        if cur:
            runs.append(cur)
        found = sum(1 for h in row if h is not None)
        out.append("%s\t%d\t%d\t%s\n" % (name, len(row), found, ",".join("%d:%d:%d:%s:%d" % tuple(r[:5]) for r in runs) or "*"))
    return "".join(out)


def cli(exe, tmp_path, name, k):
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
    lines = fa.decode().split("\n")
    ut = [lines[i + 1] for i in range(0, len(lines) - 1, 2)]
    idx = brute_index(ut, k)
    rng = random.Random(k)
    queries = refs[:60] + [rc(r) for r in refs[:20] if set(r) <= ACGT] + ["".join(rng.choice("ACGT") for _ in range(2 * k + 9)), "ACG", refs[0][:k] + "N" + refs[0][k:]]
    names = ["q%d" % i for i in range(len(queries))]
    exp = fold_tsv(names, queries, expected(ut, idx, k, queries), k)
    assert any(":+:" in l for l in exp.split("\n")) and any(":-:" in l for l in exp.split("\n")) and "\t*\n" in exp
    with gzip.open(d / "q.fa.gz", "wt") as f:                # gzip FASTA, sequences wrapped at 50 columns, a description behind every name
        for n, q in zip(names, queries):
            f.write(">%s some description\n" % n)
            for i in range(0, len(q), 50):
                f.write(q[i:i + 50] + "\n")
    with open(d / "q.fq", "w") as f:
        for n, q in zip(names, queries):
            f.write("@%s/1 x\n%s\n+\n%s\n" % (n, q, "I" * len(q)))
    for qf, fix in (("q.fa.gz", lambda s: s), ("q.fq", lambda s: s.replace("\t", "/1\t", 1))):
        r = run(["-in", "g.unitigs.fa", "-kmer-size", str(k), "-query", qf])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "query: %d sequences" % len(queries) in r.stdout, r.stdout
        got = (d / "g.query.tsv").read_text()
        assert got == "".join(fix(l) + "\n" for l in exp.split("\n") if l)
        assert (d / "g.unitigs.fa").read_bytes() == fa       # untouched
        assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa", "g.query.tsv", "q.fa.gz", "q.fq"])
        os.remove(d / "g.query.tsv")
    # -in <prefix> -out <prefix> names the same files
    r = run(["-in", "whatever.h5", "-out", "g", "-kmer-size", str(k), "-query", "q.fq"])
    assert r.returncode == 0 and (d / "g.query.tsv").exists(), r.stdout + r.stderr
    for args, msg in ((["-in", "g.unitigs.fa", "-kmer-size", str(k), "-query", "q.fq", "-nb-gpus", "2"], "-nb-gpus must be 1"),
                      (["-in", "g.unitigs.fa", "-kmer-size", str(k), "-query", "q.fq", "-redo-links"], "-query and -redo-links"),
                      (["-in", "g.unitigs.fa", "-kmer-size", str(k), "-query"], "needs a value"),
                      (["-in", "g.unitigs.fa", "-kmer-size", str(k), "-query", "nothing.fa"], "cannot open query file"),
                      (["-in", "absent.unitigs.fa", "-kmer-size", str(k), "-query", "q.fq"], "cannot open")):
        r = run(args)
        assert r.returncode == 1 and msg in r.stdout + r.stderr, (args, r.stdout, r.stderr)
    assert (d / "g.unitigs.fa").read_bytes() == fa
