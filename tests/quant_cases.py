"""Shared helpers, inputs and test bodies of the quantification tests (test_hostsim_quant.py on the simulator, test_gpu_quant.py on the
device): cdbg_quantify / cdbg_fetch_quant / cdbg_quant_reset / `bcalm -quantify`.

Expected values never come from the code under test.  Two sources:
  (a) brute force: query_cases.brute_index over g.unitigs() (or over the loaded sequences) gives the smallest-occurrence position of
      every canonical k-mer; the valid windows of the queries are counted per position in Python, the saturation rule
      (count if count < ceiling else 2147483647) applied, and kc / covered / the totals follow;
  (b) the build's own abundances: a graph built with all_abundance_counts from text T, quantified with T's reads, must report
      g.unitig_abundances() per position, the KC of g.unitigs() per unitig and digest()["kc_sum"] windows found -- numbers the other
      suites pin against the oracle.
Every case asserts found > 0 and windows > found: a kernel that counts nothing, or counts everything, cannot pass."""
import gzip
import os
import random
import subprocess

import kwidth_cases as kc
import oracle_lib
import query_cases as qc
from bcalm_amd import api

SAT = 2147483647
CEILING = 2 ** 31 - 4096
E_STATE = qc.E_STATE
rc = qc.rc


def windows_of(q, k):
    """(offset, k-mer in upper case) of every window of q that holds only ACGTacgt"""
    q = q.upper()
    bad = -1
    for i, ch in enumerate(q):
        if ch not in qc.ACGT:
            bad = i
        if i >= k - 1 and bad < i - k + 1:
            yield i - k + 1, q[i - k + 1:i + 1]


def brute(seqs, k, queries, ceiling=CEILING, idx=None):
    """(a) -> (reported counts per unitig position, raw counts, windows, found)"""
    idx = qc.brute_index(seqs, k) if idx is None else idx
    raw = [[0] * (len(s) - k + 1) for s in seqs]
    windows = found = 0
    for q in queries:
        for _, x in windows_of(q, k):
            windows += 1
            at = idx.get(qc.canon(x))
            if at is not None:
                found += 1
                raw[at[0]][at[1]] += 1
    rep = [[v if v < ceiling else SAT for v in row] for row in raw]
    return rep, raw, windows, found


def quant_bytes(g):
    kcs, cov, ab, off = g.quant_raw()
    n = len(off) - 1
    return bytes(kcs)[:8 * n] + bytes(cov)[:4 * n] + bytes(ab)[:4 * off[n]] + bytes(off)


def check_fetch(g, rep, raw):
    """everything cdbg_fetch_quant reports against the per-position expectation: counts, kc = sum of the reported values, covered"""
    per = g.quant(per_kmer=True)
    assert len(per) == len(rep)
    for u, ((kcu, cov, ab), er, rr) in enumerate(zip(per, rep, raw)):
        assert ab == er, (u, ab, er)
        assert kcu == sum(er), (u, kcu, sum(er))
        assert cov == sum(1 for v in rr if v), (u, cov)
    assert g.quant() == [(a, b) for a, b, _ in per]          # kc and covered alone (ab = NULL)
    return per


def check(g, seqs, k, queries, ceiling=CEILING, idx=None, **kw):
    """quantify `queries` into zeroed counters and compare everything with (a); -> the totals of the call"""
    rep, raw, windows, found = brute(seqs, k, queries, ceiling, idx)
    r = g.quantify(queries, **kw)
    assert (r["windows"], r["found"]) == (windows, found), (r, windows, found)
    n_canonical = (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2
    if len(qc.brute_index(seqs, k) if idx is None else idx) == n_canonical:
        assert k <= 4 and windows == found > 0               # (tiny k: the set spells every k-mer there is -- nothing can miss)
    else:
        assert found > 0 and windows > found, (windows, found)
    assert r["extended"] <= r["found"]
    check_fetch(g, rep, raw)
    return r


def zeros(g, seqs, k):
    assert g.quant(per_kmer=True) == [(0, 0, [0] * (len(s) - k + 1)) for s in seqs]


def refused(call, what):
    try:
        call()
        raise AssertionError("no error: " + what)
    except api.CdbgError as e:
        assert e.code == E_STATE and what in str(e), e


# ---------------------------------------------------------------- 1. every key width
def key_width(lib, k, amin):
    text = kc.edge_text(k, 1)
    g = qc.built(lib, text, k, amin, all_abundance_counts=True)
    try:
        units = g.unitigs()
        ut = [s for s, _ in units]
        reads = text.split("\n")
        r = g.quantify(reads)                                # (b): the graph's own reads
        per = g.quant(per_kmer=True)
        assert [p[2] for p in per] == g.unitig_abundances()
        assert [p[0] for p in per] == [kcu for _, kcu in units]
        assert [p[1] for p in per] == [len(s) - k + 1 for s in ut]       # every position of the graph is one of its reads' k-mers
        assert r["found"] == g.digest()["kc_sum"] > 0
        assert r["windows"] == sum(1 for q in reads for _ in windows_of(q, k))
        every = len(qc.brute_index(ut, k)) == (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2    # tiny k: the graph holds every k-mer there is
        assert k <= 4 or not every
        assert r["windows"] > r["found"] if amin == 2 and not every else r["windows"] == r["found"]   # abundance-min 1: every window of the text is solid
        # (k = 3, 4: the reads spell every k-mer there is, every unitig is ONE k-mer and no hit has a neighbour to extend into -- a property of
        #  the input, read from g.unitigs(): there the shortcut must stay silent)
        can_extend = any(len(s) > k for s in ut)
        assert k <= 4 or can_extend
        assert (r["extended"] > 0) == can_extend, r
        g.quant_reset()
        r = check(g, ut, k, qc.variants(reads, k, k))        # (a)
        assert (r["extended"] > 0) == can_extend, r
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
        for c in range(1, len(V)):                           # V cut at every offset into two adjacent sequences
            qs += [V[:c], V[c:]]
        check(g, ut, k, qs, idx=idx)                         # (nothing is counted across two adjacent sequences: (a) counts per sequence)
        ref = quant_bytes(g)
        g.quant_reset()
        check(g, ut, k, qs, idx=idx, first_offset=37)        # offsets[0] != 0
        assert quant_bytes(g) == ref
    finally:
        g.close()


# ---------------------------------------------------------------- 3. batches: the k - 1 overlap must not count twice
def _fresh(lib, seqs, k, monkeypatch, env):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    g = qc.loaded(lib, seqs, k)                              # (the hooks are read when a context is created)
    for name in env:
        monkeypatch.delenv(name)
    return g


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
        g = _fresh(lib, ut, k, monkeypatch, env)
        try:
            check(g, ut, k, qs, idx=idx)
            got.append(quant_bytes(g))
        finally:
            g.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------- 4. extension edges
def edge_text(k, seed=7):
    """reads of a handmade graph: a genome longer than a tile of the kernel as ONE read, a branch off it, a k-mer on its own (a unitig of exactly
    k bases), an even-k k-mer that is its own reverse complement inside a read"""
    rng = random.Random(100 * k + seed)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    G = rnd(9000)
    reads = [G, G[300:300 + 3 * k] + rnd(2 * k), rc(G[700:700 + 2 * k]) + rnd(k + 3), rnd(k)]
    h = rnd(k // 2)
    if k % 2 == 0:
        reads.append(rnd(k) + h + rc(h) + rnd(k))
    return reads


def extension_edges(lib, monkeypatch, k):
    reads = edge_text(k)
    g = qc.built(lib, "\n".join(reads) + "\n", k, 1)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    assert len(ut) > 3 and any(len(s) == k for s in ut) and len(reads[0]) > 8192 + k
    rng = random.Random(k)
    sub = lambda s, i: s[:i] + rng.choice([c for c in "ACGT" if c != s[i]]) + s[i + 1:]
    qs = list(reads) + [rc(r) for r in reads]                # along every unitig to its last k-mer and into the neighbour, on both strands
    by_len = sorted(ut, key=len)
    for s in by_len[-6:]:
        if len(s) > k + 2:
            qs += [sub(s, k), sub(rc(s), k), sub(s, len(s) - 1), rc(s) + "ACGT"]   # a substitution one base behind a hit; strand - down to offset 0 and beyond
    qs += [s for s in by_len[:4]] + [rc(s) for s in by_len[:4]]
    for d in range(1, 70, 3):                                # short reads at every distance from a lane's run boundary
        qs.append(reads[0][1000 + d:1000 + d + k + d % 40])
    idx = qc.brute_index(ut, k)
    got = []
    for env in ({}, {"CDBG_QUANT_NO_EXTEND": "1"}):
        g = _fresh(lib, ut, k, monkeypatch, env)
        try:
            r = check(g, ut, k, qs, idx=idx)
            assert (r["extended"] == 0) if env else (r["extended"] > 0), r
            got.append(quant_bytes(g))
        finally:
            g.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------- 5. repeated k-mers (loaded sets)
def repeated_handmade(lib, runs=1):
    k = 8
    seqs, qs, pal = qc.handmade(k)
    qs = qs + [s for s in seqs[-45:]]                        # the LATER copies of the records as queries: counted at the first copy
    ref = None
    for _ in range(runs):
        g = qc.loaded(lib, seqs, k)
        try:
            r = check(g, seqs, k, qs)
            assert r["extended"] == 0                        # a set that repeats k-mers: every window probes
            info = g.index_info()
            assert info["distinct"] < info["positions"]
            first = set(qc.brute_index(seqs, k).values())
            for u, (_, _, ab) in enumerate(g.quant(per_kmer=True)):
                for o, v in enumerate(ab):
                    assert v == 0 or (u, o) in first, (u, o, v)      # nothing at an occurrence that is not the smallest
            b = quant_bytes(g)
        finally:
            g.close()
        assert ref is None or b == ref
        ref = b


# ---------------------------------------------------------------- 6. ceiling and clamp
def ceiling(lib, monkeypatch, k=21):
    rng = random.Random(6)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    seqs = [rnd(60) for _ in range(5)]
    qs = [seqs[0]] * 4 + [seqs[1]] * 3 + [rc(seqs[1])] * 2 + [seqs[2]] * 6 + [seqs[3], rc(seqs[3])] * 5 + [seqs[3][7:40]] + [rnd(80), seqs[0][:k + 5] + "N"]
    rng.shuffle(qs)
    rep, raw, windows, found = brute(seqs, k, qs, 5)
    vals = {v for row in raw for v in row}
    assert {0, 4, 5, 6, 10, 11} <= vals and {v for row in rep for v in row} == {0, 4, SAT}
    got = []
    for env in ({}, {"CDBG_QUERY_BATCH": "1", "CDBG_QUANT_CLAMP_WINDOWS": "300"}):
        env = dict(env, CDBG_QUANT_CEILING="5")
        g = _fresh(lib, seqs, k, monkeypatch, env)
        try:
            half = len(qs) // 2                              # two calls: the tally of windows since the last clamp lives across calls
            a, b = g.quantify(qs[:half]), g.quantify(qs[half:])
            assert (a["windows"] + b["windows"], a["found"] + b["found"]) == (windows, found) and windows > found > 0
            per = check_fetch(g, rep, raw)
            assert any(kcu >= SAT for kcu, _, _ in per)      # kc sums the reported values
            got.append(quant_bytes(g))
        finally:
            g.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------- 7. state
def state(lib):
    k = 15
    ta, tb = oracle_lib.read_input("rand_a"), oracle_lib.read_input("rand_b")
    reads_a = [r for r in ta.split("\n") if r][:30]
    reads_b = [r for r in tb.split("\n") if r][:30]
    A = reads_a + [rc(r) for r in reads_a[:10]] + ["ACGT" * 10]
    B = reads_b + reads_a[5:15] + ["N" + reads_a[0]]
    g = api.Graph(k, 2, lib=lib)
    try:
        calls = ((lambda: g.quantify(A), "cdbg_quantify"), (g.quant, "cdbg_fetch_quant"), (g.quant_reset, "cdbg_quant_reset"))
        for call, name in calls:
            refused(call, name + " before cdbg_glue")
        g.push_text(ta); g.count()
        refused(calls[0][0], "before cdbg_glue")
        g.compact(); g.glue()
        ua = [s for s, _ in g.unitigs()]
        zeros(g, ua, k)                                      # a fetch before any quantify
        hits = g.query(A)
        check(g, ua, k, A)
        assert g.query(A) == hits                            # the lookup is what it was
        r = g.quantify(B)                                    # accumulation: A, then B, equals A + B
        rep, raw, windows, found = brute(ua, k, A + B)
        assert r["found"] == found - brute(ua, k, A)[3]
        check_fetch(g, rep, raw)
        ref = quant_bytes(g)
        info = g.index_info()
        g.quant_reset()
        zeros(g, ua, k)
        assert g.index_info() == info
        assert g.quantify([]) == {"windows": 0, "found": 0, "extended": 0} == g.quantify(["", ""])
        zeros(g, ua, k)
        check(g, ua, k, A + B)
        assert quant_bytes(g) == ref
        g.reset()
        for call, name in calls:
            refused(call, name + " before cdbg_glue")
        g.run()                                              # (the reads stay resident: the same graph, rebuilt) -- and it starts from zeros
        zeros(g, [s for s, _ in g.unitigs()], k)
        check(g, [s for s, _ in g.unitigs()], k, A)
    finally:
        g.close()
    g = api.Graph(k, 2, lib=lib)
    try:
        g.push_text(tb); g.run()
        ub = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    # load -> reset -> load of another set: the counts follow the second set; quantify([]) alone builds index and counters
    g = api.Graph(k, 1, lib=lib)
    try:
        g.load_unitigs(ua)
        assert g.quantify([]) == {"windows": 0, "found": 0, "extended": 0}
        zeros(g, ua, k)
        check(g, ua, k, A + B)
        g.reset()
        refused(g.quant, "before cdbg_glue")
        g.load_unitigs(ub)
        zeros(g, ub, k)
        check(g, ub, k, A + B)
    finally:
        g.close()


def state_two_ranks(lib, monkeypatch, memcpy):
    """a rank that holds a share of the unitigs cannot count for the graph: world_size = 2, and one rank sent through the multi-rank
    path (CDBG_FORCE_MULTI, in-process loop-back transport) up to a glued graph"""
    import loopback
    qs = ["ACGTACGTACGTACGTACGT"]

    def all_refused(g):
        for call in (lambda: g.quantify(qs), g.quant, g.quant_reset):
            refused(call, "one rank only")
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


# ---------------------------------------------------------------- 8. CLI
def fold_tsv(seqs, k, rep, raw, per_kmer):
    """the <prefix>.quant.tsv `bcalm -quantify` must write"""
    out = []
    for u, (s, er, rr) in enumerate(zip(seqs, rep, raw)):
        n, kcu = len(s) - k + 1, sum(er)
        row = "%d\t%d\t%d\t%d\t%.1f" % (u, n, kcu, sum(1 for v in rr if v), kcu / n)
        out.append(row + ("\t" + ",".join(str(v) for v in er) if per_kmer else "") + "\n")
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
    rng = random.Random(k)
    sample = refs[:60] + [rc(r) for r in refs[:20] if set(r) <= qc.ACGT] + refs[:7] + ["".join(rng.choice("ACGT") for _ in range(2 * k + 9)), "ACG", refs[0][:k] + "N" + refs[0][k:]]
    rep, raw, windows, found = brute(ut, k, sample)
    assert windows > found > 0 and len({v for row in raw for v in row}) > 2
    with gzip.open(d / "s.fa.gz", "wt") as f:                # gzip FASTA, sequences wrapped at 50 columns
        for i, q in enumerate(sample):
            f.write(">s%d some description\n" % i)
            for j in range(0, len(q), 50):
                f.write(q[j:j + 50] + "\n")
    with open(d / "s.fq", "w") as f:
        for i, q in enumerate(sample):
            f.write("@s%d/1 x\n%s\n+\n%s\n" % (i, q, "I" * len(q)))
    for sf in ("s.fa.gz", "s.fq"):
        for per_kmer in (False, True):
            r = run(["-in", "g.unitigs.fa", "-kmer-size", str(k), "-quantify", sf] + (["-all-abundance-counts"] if per_kmer else []))
            assert r.returncode == 0, r.stdout + r.stderr
            assert "quantify: %d sequences, %d k-mers, %d found, " % (len(sample), windows, found) in r.stdout, r.stdout
            assert "counts written to g.quant.tsv" in r.stdout
            assert (d / "g.quant.tsv").read_text() == fold_tsv(ut, k, rep, raw, per_kmer)
            assert (d / "g.unitigs.fa").read_bytes() == fa   # untouched
            assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa", "g.quant.tsv", "s.fa.gz", "s.fq"])
            os.remove(d / "g.quant.tsv")
    base = ["-in", "g.unitigs.fa", "-kmer-size", str(k)]
    for args, msg in ((base + ["-quantify", "s.fq", "-nb-gpus", "2"], "-nb-gpus must be 1"),
                      (base + ["-quantify", "s.fq", "-redo-links"], "separate modes"),
                      (base + ["-quantify", "s.fq", "-query", "s.fq"], "separate modes"),
                      (base + ["-quantify"], "needs a value"),
                      (base + ["-quantify", "nothing.fa"], "cannot open sample file"),
                      (["-in", "absent.unitigs.fa", "-kmer-size", str(k), "-quantify", "s.fq"], "cannot open")):
        r = run(args)
        assert r.returncode == 1 and msg in r.stdout + r.stderr, (args, r.stdout, r.stderr)
    assert (d / "g.unitigs.fa").read_bytes() == fa
    assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa", "s.fa.gz", "s.fq"])
