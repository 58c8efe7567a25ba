"""Shared helpers, inputs and test bodies of the colour tests (test_hostsim_color.py on the simulator, test_gpu_color.py on the device):
cdbg_color_open / cdbg_color / cdbg_color_classes / cdbg_fetch_color_runs / cdbg_fetch_color_classes / `bcalm -colors`.

Expected values never come from the code under test: query_cases.brute_index gives the smallest-occurrence position of every canonical
k-mer of the resident sequences, quant_cases.windows_of the valid windows of the samples, and brute() / fold() below build colour sets,
runs and classes straight from the definitions of include/cdbg.h.

check() asserts about its own input that windows > found > 0, that there are at least three classes, a class of two or more colours and
an empty-set run: a kernel that marks nothing, or marks everything, cannot pass.  Three kinds of input cannot have all of that, by the
definitions themselves, and say so where they call check(): a built graph marked with ALL of its own reads has no position without a
colour (key_width() therefore colours every graph a second time, with its first ten reads alone); one colour alone makes two classes
at the most (color_counts() with N = 1); and at k <= 4 the graph spells every k-mer there is (windows == found: the one relaxation
quant_cases.check makes, made here under the same condition) and so does every sample of reads, so that all positions share one colour
set -- key_width() therefore colours such a graph the second time with samples made of its own unitigs, and there every assertion holds."""
import gzip
import itertools
import os
import random
import subprocess

import kwidth_cases as kc
import oracle_lib
import query_cases as qc
import quant_cases as qn
from bcalm_amd import api

E_PARAM = -1
E_STATE = qc.E_STATE
MAX_COLORS = 4096
QUANT_TILE = 8192                                            # bcalm_amd/csrc/k_quant.h
rc = qc.rc


def brute(seqs, k, marks, idx=None):
    """marks: [(colour, [sequences])] in call order -> (the colour set of every position of every sequence, (windows, found) per call)"""
    idx = qc.brute_index(seqs, k) if idx is None else idx
    sets = [[set() for _ in range(len(s) - k + 1)] for s in seqs]
    totals = []
    for c, qs in marks:
        windows = found = 0
        for q in qs:
            for _, x in qn.windows_of(q, k):
                windows += 1
                at = idx.get(qc.canon(x))
                if at is not None:
                    found += 1
                    sets[at[0]][at[1]].add(c)
        totals.append((windows, found))
    return sets, totals


def fold(sets):
    """-> (per sequence its runs (offset, len, class), the classes in the order of their first run)"""
    runs, number, table = [], {}, []
    for row in sets:
        mine, o = [], 0
        while o < len(row):
            e = o + 1
            while e < len(row) and row[e] == row[o]:
                e += 1
            key = frozenset(row[o])
            if key not in number:
                number[key] = len(table)
                table.append({"colors": sorted(key), "runs": 0, "kmers": 0})
            c = number[key]
            table[c]["runs"] += 1
            table[c]["kmers"] += e - o
            mine.append((o, e - o, c))
            o = e
        runs.append(mine)
    return runs, table


def color_bytes(g):
    """everything the two fetches return, as bytes"""
    tot, run_off, off, ln, cls = g.color_runs_raw()
    R = tot["runs"]
    n, ncol, runs, kmers, bits, nw = g.color_classes_raw()
    assert n == tot["classes"]
    return (repr(sorted(tot.items())).encode() + bytes(run_off) + bytes(off)[:4 * R] + bytes(ln)[:4 * R] + bytes(cls)[:4 * R]
            + bytes(ncol)[:4 * n] + bytes(runs)[:8 * n] + bytes(kmers)[:8 * n] + bytes(bits)[:4 * n * nw])


def mark(g, n_colors, marks, **kw):
    g.color_open(n_colors)
    return [g.color(c, qs, **kw) for c, qs in marks]


def check_result(g, n_colors, sets):
    """both fetches against the fold of `sets`; -> (runs, classes) as folded"""
    runs, table = fold(sets)
    tot, run_off, off, ln, cls = g.color_runs_raw()
    R = sum(len(r) for r in runs)
    assert tot == {"runs": R, "classes": len(table), "colored": sum(1 for row in sets for s in row if s),
                   "single_run_unitigs": sum(1 for r in runs if len(r) == 1)}, tot
    assert list(run_off) == [sum(len(r) for r in runs[:u]) for u in range(len(runs) + 1)]
    assert [(off[r], ln[r], cls[r]) for r in range(R)] == [t for r in runs for t in r]
    assert g.color_runs() == runs
    assert g.color_classes() == table
    n, ncol, cruns, kmers, bits, nw = g.color_classes_raw()
    assert n == len(table) and nw == (n_colors + 31) // 32
    for i, e in enumerate(table):
        assert ncol[i] == len(e["colors"])
        row = sum(bits[i * nw + j] << (32 * j) for j in range(nw))
        assert row == sum(1 << c for c in e["colors"]) and row >> n_colors == 0      # (padding bits zero)
    assert sum(cruns[i] for i in range(n)) == R and sum(kmers[i] for i in range(n)) == sum(len(row) for row in sets)
    return runs, table


def check(g, seqs, k, n_colors, marks, idx=None, empty_run=True, min_classes=3, multi=True, classes=True, **kw):
    """colour a freshly opened set with `marks` and compare everything with the fold of the definitions; -> (runs, classes, totals)"""
    sets, totals = brute(seqs, k, marks, idx)
    got = mark(g, n_colors, marks, **kw)
    assert [(r["windows"], r["found"]) for r in got] == totals, (got, totals)
    windows, found = sum(t[0] for t in totals), sum(t[1] for t in totals)
    n_canonical = (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2
    if len(qc.brute_index(seqs, k) if idx is None else idx) == n_canonical:
        assert k <= 4 and windows == found > 0               # (tiny k: the set spells every k-mer there is -- nothing can miss)
    else:
        assert windows > found > 0, (windows, found)
    assert all(r["extended"] <= r["found"] for r in got)
    runs, table = check_result(g, n_colors, sets)
    if classes:                                              # (off only where key_width() says why)
        assert len(table) >= min_classes, table
        assert not multi or any(len(e["colors"]) >= 2 for e in table), table
        assert any(not e["colors"] for e in table) == empty_run, table
    return runs, table, {"windows": windows, "found": found, "extended": sum(r["extended"] for r in got)}


def refused(call, what, code=E_STATE):
    try:
        call()
        raise AssertionError("no error: " + what)
    except api.CdbgError as e:
        assert e.code == code and what in str(e), e


# ---------------------------------------------------------------- 1. every key width
def key_width(lib, k):
    text = kc.edge_text(k, 1)
    g = qc.built(lib, text, k, 2)
    try:
        ut = [s for s, _ in g.unitigs()]
        idx = qc.brute_index(ut, k)
        reads = text.split("\n")
        s0, s1, s2 = reads[0::2], reads[1::2], [rc(r) for r in reads[0::3]]      # (rc() leaves an N where it is)
        # every read is in colour 0 or 1 and every k-mer of the graph is one of a read: no position without a colour, by construction
        # tiny k: a few kB of reads spell every k-mer there is, in every sample -- one colour set everywhere, whichever reads are taken
        tiny = k <= 4
        _, _, r = check(g, ut, k, 3, [(0, s0), (1, s1), (2, s2)], idx=idx, empty_run=False, classes=not tiny)
        can_extend = any(len(s) > k for s in ut)
        assert k <= 4 or can_extend
        assert (r["extended"] > 0) == can_extend, r
        if not tiny:
            # ... so once more with the first ten reads alone: what only the later reads spell are runs of the empty set
            head = reads[:10]
            check(g, ut, k, 3, [(0, head[0::2]), (1, head[1::2]), (2, [rc(r) for r in head[0::3]])], idx=idx, empty_run=True)
        else:
            # ... and there once more with whole unitigs as samples (a built graph spells every k-mer once, so a unitig marks its own
            # positions only): unitig i gets {0, 1, 2}, {}, {1}, {0}, {1}, {} by i mod 6 -- four classes, one of three colours, the empty
            # set -- and a k-mer the graph does not spell, where there is one, is the window that misses
            assert len(ut) >= 6
            absent = [x for x in ("".join(t) for t in itertools.product("ACGT", repeat=k)) if qc.canon(x) not in idx][:1]
            check(g, ut, k, 3, [(0, ut[0::3] + absent), (1, ut[0::2]), (2, [rc(s) for s in ut[0::6]])], idx=idx)
    finally:
        g.close()


# ---------------------------------------------------------------- 2. word edges
def distinct_seqs(k, lengths, seed):
    """sequences of the given numbers of k-mer positions that spell every canonical k-mer at most once between them, none its own reverse complement"""
    rng = random.Random(seed)
    used, out = set(), []
    for n in lengths:
        while True:
            s = "".join(rng.choice("ACGT") for _ in range(k))
            if qc.canon(s) in used or s == rc(s):
                continue
            mine = {qc.canon(s)}
            stuck = False
            while len(s) < n + k - 1 and not stuck:
                for b in rng.sample("ACGT", 4):
                    x = (s + b)[-k:]
                    if qc.canon(x) not in used and qc.canon(x) not in mine and x != rc(x):
                        s += b; mine.add(qc.canon(x))
                        break
                else:
                    stuck = True
            if not stuck:
                break
        used |= mine
        out.append(s)
    return out


WORD_K = 8
WORD_POS = [31, 1, 1, 30, 1, 1, 100, 40, 23, 1, 64, 32, 5, 77, 9]      # k-mer positions per unitig: kmer_off = 0, 31, 32, 33, 63, 64, 65, 165, ...
BIG = 6                                                      # the unitig of 100 positions: 65 .. 164, across the word edges at 96, 128 and 160


def word_edge_input(seed=4):                               # (a seed whose random and substituted bases spell no k-mer of the big unitig: word_edges() asserts it)
    k = WORD_K
    seqs = distinct_seqs(k, WORD_POS, 21)
    off = [sum(WORD_POS[:u]) for u in range(len(WORD_POS) + 1)]
    assert off[1:7] == [31, 32, 33, 63, 64, 65] and len(seqs[1]) == len(seqs[2]) == k and WORD_POS[BIG] > 64
    assert off[1] % 32 == 31 and off[2] % 32 == 0 and off[4] % 32 == 31 and off[5] % 32 == 0      # unitigs of exactly k bases at bit 31 and at bit 0
    rng = random.Random(seed)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    sub = lambda s, i: s[:i] + rng.choice([c for c in "ACGT" if c != s[i]]) + s[i + 1:]
    V = seqs[7]
    cuts = []
    for c in range(1, 41):                                   # V cut every c bases into adjacent sequences
        cuts += [V[i:i + c] for i in range(0, len(V), c)]
    long = ""
    while len(long) <= QUANT_TILE + 3 * k:                   # longer than a tile of the kernel and its halo
        long += seqs[10] + "N" + rc(seqs[13]) + "n" + seqs[11] + "N" + rc(seqs[10]) + "-"
    marks = [(0, [seqs[BIG], seqs[1], seqs[4], seqs[0], seqs[3][:k + 11], ""]),
             (1, [rc(seqs[BIG]), rc(seqs[2]), rc(seqs[5]), rc(seqs[0])[3:], rc(seqs[3])] + cuts),
             (2, [long, sub(seqs[8], k), sub(rc(seqs[8]), k), sub(seqs[13], len(seqs[13]) - 1), rnd(50), seqs[12][:k - 1], "ACGTN" + seqs[9]])]
    return k, seqs, marks


def word_edges(lib, monkeypatch, runs=1):
    k, seqs, marks = word_edge_input()
    idx = qc.brute_index(seqs, k)
    ref = None
    for _ in range(runs):
        got = []
        for env in ({}, {"CDBG_QUANT_NO_EXTEND": "1"}):
            g = qn._fresh(lib, seqs, k, monkeypatch, env)
            try:
                runs_, table, r = check(g, seqs, k, 3, marks, idx=idx)
                info = g.index_info()
                assert info["distinct"] == info["positions"] == sum(WORD_POS)
                assert (r["extended"] == 0) if env else (r["extended"] > 0), r
                assert runs_[BIG] == [(0, WORD_POS[BIG], runs_[BIG][0][2])]          # one run across two word edges: no head at bit 0
                assert table[runs_[BIG][0][2]]["colors"] == [0, 1]
                assert len(runs_[1]) == len(runs_[2]) == 1 and runs_[1][0][2] != runs_[2][0][2]
                got.append(color_bytes(g))
            finally:
                g.close()
        assert got[0] == got[1]
        assert ref is None or got[0] == ref
        ref = got[0]


# ---------------------------------------------------------------- 3. colour-count edges
def color_counts(lib, n_colors):
    k = WORD_K
    seqs = distinct_seqs(k, [20 + 3 * (i % 7) for i in range(24)], 33)
    rng = random.Random(n_colors)
    junk = "".join(rng.choice("ACGT") for _ in range(40))
    used = sorted({c for c in (0, 31, 32, n_colors - 1) if c < n_colors})
    spans = {0: seqs[0:10], 31: seqs[5:15], 32: seqs[8:13]}
    spans[n_colors - 1] = spans.get(n_colors - 1, []) + seqs[15:19]
    marks = [(c, spans[c] + [junk]) for c in used]
    g = qc.loaded(lib, seqs, k)
    try:
        refused(lambda: g.color_open(0), "cdbg_color_open", E_PARAM)
        refused(lambda: g.color_open(MAX_COLORS + 1), "cdbg_color_open", E_PARAM)
        # one colour alone: the empty set and {0}, nothing else can exist
        runs, table, _ = check(g, seqs, k, n_colors, marks, min_classes=3 if n_colors > 1 else 2, multi=n_colors > 1)
        assert {c for e in table for c in e["colors"]} == set(used)
        if n_colors > 32:                                    # two sets that differ only in colour 32 are two classes
            a, b = table[runs[6][0][2]]["colors"], table[runs[9][0][2]]["colors"]
            assert a == [0, 31] and b == [0, 31, 32] and runs[6][0][2] != runs[9][0][2], (a, b)
        refused(lambda: g.color(n_colors, [seqs[0]]), "cdbg_color", E_PARAM)
        refused(lambda: g.color(2 ** 32 - 1, [seqs[0]]), "cdbg_color", E_PARAM)
        check_result(g, n_colors, brute(seqs, k, marks)[0])  # (a refused call marked nothing ...)
    finally:
        g.close()


# ---------------------------------------------------------------- 4. accumulation and idempotence
def accumulation(lib, monkeypatch, k=31):
    text = oracle_lib.read_input("rand_b")
    g = qc.built(lib, text, k, 2)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    batch = max(4 * k, 256)                                  # the floor of CDBG_QUERY_BATCH
    reads = [r for r in text.split("\n") if r]
    rng = random.Random(5)
    long = "".join(ut[:2 * len(ut) // 3])                    # one sequence of 20 batches and more; the last third of the unitigs is not in it
    while len(long) < 20 * batch:
        long += rc(long)
    long = long[:20 * batch + 17]
    many = []
    for i in range(120):
        r = reads[i % len(reads)]
        n = rng.randrange(k, 3 * k + 1)
        s = rng.randrange(0, max(1, len(r) - n))
        many.append(r[s:s + n] if i % 3 else rc(r[s:s + n]))
    A, B, C_ = [long] + many[:60], many[40:] + [""], [long[5:9 * batch], "N" * 5 + many[7]]
    marks = [(0, A), (1, B), (2, C_)]
    idx = qc.brute_index(ut, k)
    sets = brute(ut, k, marks, idx)[0]
    got = []
    for env in ({}, {"CDBG_QUERY_BATCH": "1"}):
        g = qn._fresh(lib, ut, k, monkeypatch, env)
        try:
            check(g, ut, k, 3, marks, idx=idx)
            got.append(color_bytes(g))
            if not env:
                check(g, ut, k, 3, marks, idx=idx, first_offset=37)          # offsets[0] != 0
                assert color_bytes(g) == got[0]
                mark(g, 3, [(0, A), (1, B), (0, A), (2, C_), (1, B)])        # the same sample twice
                check_result(g, 3, sets)
                assert color_bytes(g) == got[0]
                mark(g, 3, [(1, B[:30]), (0, A), (1, B[30:70]), (2, C_), (1, B[70:])])   # one sample over three calls
                check_result(g, 3, sets)
                assert color_bytes(g) == got[0]
        finally:
            g.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------- 5. classes
def class_input():
    k = WORD_K
    seqs = distinct_seqs(k, [12 + (7 * i) % 45 for i in range(60)], 55)
    rng = random.Random(8)
    n_colors = 5
    marks = []
    for c in range(n_colors):
        qs = []
        for u, s in enumerate(seqs[:50]):                    # (the last ten unitigs stay without a colour)
            if (u * 7 + c * 3) % 5 < 2:
                qs.append(s if u % 2 else rc(s))
            elif rng.random() < 0.3:
                a = rng.randrange(0, len(s) - k + 1)
                qs.append(s[a:a + k + rng.randrange(0, 12)])
        marks.append((c, qs + ["".join(rng.choice("ACGT") for _ in range(30))]))
    return k, seqs, n_colors, marks


def classes(lib, monkeypatch, runs=1):
    k, seqs, n_colors, marks = class_input()
    idx = qc.brute_index(seqs, k)
    ref = None
    for _ in range(runs):
        got = []
        for env in ({}, {"CDBG_COLOR_LOG2_SLOTS": "1"}):     # the floor applies: the smallest power of two > runs, probe chains are long
            g = qn._fresh(lib, seqs, k, monkeypatch, env)
            try:
                runs_, table, _ = check(g, seqs, k, n_colors, marks, idx=idx)
                assert len(table) >= 8
                # equal sets in far-apart unitigs share a class; classes are numbered by their first run
                first = {}
                for u, ur in enumerate(runs_):
                    for o, n, c in ur:
                        first.setdefault(c, u)
                assert any(any(c == c2 and u - first[c] >= 20 for _, _, c2 in ur) for c in first for u, ur in enumerate(runs_))
                seen = [c for ur in runs_ for _, _, c in ur]
                assert [c for i, c in enumerate(seen) if c not in seen[:i]] == list(range(len(table)))
                # a range fetch equals a slice of the full fetch
                n, ncol, cruns, kmers, bits, nw = g.color_classes_raw()
                for a, m in ((0, 0), (2, 3), (n - 1, 1), (n, 0), (1, n - 1)):
                    n2, ncol2, cruns2, kmers2, bits2, _ = g.color_classes_raw(a, m)
                    assert n2 == m and list(ncol2[:m]) == list(ncol[a:a + m]) and list(cruns2[:m]) == list(cruns[a:a + m])
                    assert list(kmers2[:m]) == list(kmers[a:a + m]) and list(bits2[:m * nw]) == list(bits[a * nw:(a + m) * nw])
                refused(lambda: g.color_classes_raw(n, 1), "cdbg_fetch_color_classes", E_PARAM)
                refused(lambda: g.color_classes_raw(n + 1, 0), "cdbg_fetch_color_classes", E_PARAM)
                got.append(color_bytes(g))
            finally:
                g.close()
        assert got[0] == got[1]
        assert ref is None or got[0] == ref
        ref = got[0]


# ---------------------------------------------------------------- 6. repeated k-mers (loaded sets)
def repeated_handmade(lib):
    k = 8
    seqs, qs, pal = qc.handmade(k)
    marks = [(0, qs), (1, [s for s in seqs[-45:]]), (2, [rc(s) for s in seqs[40:52]] + qs[:5])]    # the LATER copies as samples: marked at the first copy
    g = qc.loaded(lib, seqs, k)
    try:
        runs, table, r = check(g, seqs, k, 3, marks)
        assert r["extended"] == 0                            # a set that repeats k-mers: every window probes
        info = g.index_info()
        assert info["distinct"] < info["positions"]
        first = set(qc.brute_index(seqs, k).values())
        n_marked = 0
        for u, ur in enumerate(runs):
            for o, n, c in ur:
                if table[c]["colors"]:
                    n_marked += n
                    assert all((u, o + i) in first for i in range(n)), (u, o, n)      # nothing at an occurrence that is not the smallest
        assert 0 < n_marked < info["positions"]
    finally:
        g.close()


# ---------------------------------------------------------------- 7. state
def state(lib):
    k = 15
    ta, tb = oracle_lib.read_input("rand_a"), oracle_lib.read_input("rand_b")
    reads_a = [r for r in ta.split("\n") if r][:40]
    reads_b = [r for r in tb.split("\n") if r][:30]
    A = reads_a[:20] + [rc(r) for r in reads_a[:6]] + ["ACGT" * 10]
    B = reads_a[12:30] + reads_b[:5] + ["N" + reads_a[0]]
    marks = [(0, A), (1, B)]
    g = api.Graph(k, 2, lib=lib)
    try:
        calls = ((lambda: g.color_open(2), "cdbg_color_open"), (lambda: g.color(0, A), "cdbg_color"), (g.color_runs_raw, "cdbg_color_classes"),
                 (lambda: g._ck(g.lib.cdbg_fetch_color_runs(g._h, None, None, None, None)), "cdbg_fetch_color_runs"),
                 (lambda: g._ck(g.lib.cdbg_fetch_color_classes(g._h, 0, 0, None, None, None, None)), "cdbg_fetch_color_classes"))
        for call, name in calls:
            qn.refused(call, name + " before cdbg_glue")
        g.push_text(ta); g.count()
        qn.refused(calls[0][0], "before cdbg_glue")
        g.compact(); g.glue()
        ua = [s for s, _ in g.unitigs()]
        qn.refused(calls[1][0], "cdbg_color before cdbg_color_open")
        qn.refused(calls[2][0], "cdbg_color_classes before cdbg_color_open")
        hits = g.query(A)
        g.quantify(A)
        quant = qn.quant_bytes(g)
        g.color_open(2)
        qn.refused(calls[3][0], "cdbg_fetch_color_runs before cdbg_color_classes")       # a fetch without classes
        qn.refused(calls[4][0], "cdbg_fetch_color_classes before cdbg_color_classes")
        check(g, ua, k, 2, marks)
        ref = color_bytes(g)
        assert g.query(A) == hits and qn.quant_bytes(g) == quant                         # the lookup and the counters are what they were
        g.quant_reset(); g.quantify(A)
        assert qn.quant_bytes(g) == quant and color_bytes(g) == ref                      # ... and counting touches no colour
        g.color(1, [reads_a[35]])
        qn.refused(calls[3][0], "cdbg_fetch_color_runs before cdbg_color_classes")       # ... and again after a further cdbg_color
        qn.refused(calls[4][0], "cdbg_fetch_color_classes before cdbg_color_classes")
        check_result(g, 2, brute(ua, k, marks + [(1, [reads_a[35]])])[0])
        assert color_bytes(g) != ref
        g.color_open(2)                                      # a re-open forgets
        assert g.color(0, []) == {"windows": 0, "found": 0, "extended": 0} == g.color(1, ["", ""])
        check_result(g, 2, brute(ua, k, [])[0])
        assert g.color_classes() == [{"colors": [], "runs": len(ua), "kmers": sum(len(s) - k + 1 for s in ua)}]
        check(g, ua, k, 2, marks)
        assert color_bytes(g) == ref
        g.reset()
        for call, name in calls:
            qn.refused(call, name + " before cdbg_glue")
        g.run()                                              # (the reads stay resident: the same graph, rebuilt) -- and nothing of the colours is left
        qn.refused(calls[1][0], "cdbg_color before cdbg_color_open")
        qn.refused(calls[3][0], "before cdbg_color_classes")
        check(g, [s for s, _ in g.unitigs()], k, 2, marks)   # (against its own unitigs: a rebuilt graph may number them differently)
    finally:
        g.close()
    g = api.Graph(k, 2, lib=lib)
    try:
        g.push_text(tb); g.run()
        ub = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    # load -> load of another set: the colours follow the second set; an empty set gives zeros
    g = api.Graph(k, 1, lib=lib)
    try:
        g.load_unitigs(ua)
        check(g, ua, k, 2, marks)
        g.reset()
        qn.refused(g.color_runs_raw, "before cdbg_glue")
        g.load_unitigs(ub)
        qn.refused(lambda: g.color(0, A), "cdbg_color before cdbg_color_open")
        check(g, ub, k, 2, [(0, B + reads_b), (1, A + reads_b[3:9])])
        g.reset()
        g.load_unitigs([])
        g.color_open(3)
        assert g.color(2, A)["found"] == 0
        tot, run_off, _, _, _ = g.color_runs_raw()
        assert tot == {"runs": 0, "classes": 0, "colored": 0, "single_run_unitigs": 0} and list(run_off) == [0]
        assert g.color_classes() == []
    finally:
        g.close()


def state_two_ranks(lib, monkeypatch, memcpy):
    """a rank that holds a share of the unitigs cannot colour the graph: world_size = 2, and one rank sent through the multi-rank
    path (CDBG_FORCE_MULTI, in-process loop-back transport) up to a glued graph"""
    import loopback
    qs = ["ACGTACGTACGTACGTACGT"]

    def all_refused(g):
        for call in (lambda: g.color_open(2), lambda: g.color(0, qs), g.color_runs_raw, g.color_classes_raw):
            qn.refused(call, "one rank only")
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
def fold_tsvs(sets):
    """the <prefix>.colors.tsv and <prefix>.color_classes.tsv `bcalm -colors` must write"""
    runs, table = fold(sets)
    a = "".join("%d\t%d\t%d\t%d\n" % (u, o, n, c) for u, ur in enumerate(runs) for o, n, c in ur)
    b = "".join("%d\t%d\t%d\t%d\t%s\n" % (i, len(e["colors"]), e["runs"], e["kmers"], ",".join(str(c) for c in e["colors"]) or "-") for i, e in enumerate(table))
    return a, b, runs, table


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
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    a = max(1, len(refs) // 4)                               # (the last refs stay without a colour; pufferize_refs has three)
    samples = [refs[:a] + [rnd(2 * k + 9), "ACG", refs[0][:k] + "N" + refs[0][k:]],
               [rc(r) for r in refs[a // 2:2 * a] if set(r) <= qc.ACGT] + [rnd(3 * k)],
               [r[3:k + 9] for r in refs[max(0, a - 1):2 * a + 1]] + [rnd(k + 1)]]
    sets, totals = brute(ut, k, list(enumerate(samples)))
    exp_runs, exp_classes, runs, table = fold_tsvs(sets)
    windows, found = sum(t[0] for t in totals), sum(t[1] for t in totals)
    assert windows > found > 0 and len(table) >= 3 and any(len(e["colors"]) >= 2 for e in table) and any(not e["colors"] for e in table)
    with gzip.open(d / "s0.fa.gz", "wt") as f:               # gzip FASTA, sequences wrapped at 50 columns
        for i, q in enumerate(samples[0]):
            f.write(">s%d some description\n" % i)
            for j in range(0, len(q), 50):
                f.write(q[j:j + 50] + "\n")
    with open(d / "s1.fq", "w") as f:
        for i, q in enumerate(samples[1]):
            f.write("@s%d/1 x\n%s\n+\n%s\n" % (i, q, "I" * len(q)))
    with open(d / "s2.fa", "w") as f:
        for i, q in enumerate(samples[2]):
            f.write(">s%d\n%s\n" % (i, q))
    (d / "list.txt").write_text("s0.fa.gz\n\ns1.fq\ns2.fa\n\n")       # one sample per non-empty line
    inputs = ["reads.fa", "g.unitigs.fa", "s0.fa.gz", "s1.fq", "s2.fa", "list.txt"]
    r = run(["-in", "g.unitigs.fa", "-kmer-size", str(k), "-colors", "list.txt"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "colors: 3 samples, %d k-mers, %d found, %d runs, %d classes" % (windows, found, sum(len(x) for x in runs), len(table)) in r.stdout, r.stdout
    assert "colours written to g.colors.tsv and g.color_classes.tsv" in r.stdout
    assert (d / "g.colors.tsv").read_text() == exp_runs
    assert (d / "g.color_classes.tsv").read_text() == exp_classes
    assert (d / "g.unitigs.fa").read_bytes() == fa           # untouched
    assert sorted(os.listdir(d)) == sorted(inputs + ["g.colors.tsv", "g.color_classes.tsv"])
    os.remove(d / "g.colors.tsv"); os.remove(d / "g.color_classes.tsv")
    (d / "empty.txt").write_text("\n\n")
    (d / "bad.txt").write_text("s0.fa.gz\nnothing.fa\n")
    (d / "many.txt").write_text("s2.fa\n" * (MAX_COLORS + 1))
    inputs += ["empty.txt", "bad.txt", "many.txt"]
    base = ["-in", "g.unitigs.fa", "-kmer-size", str(k)]
    for args, msg in ((base + ["-colors", "list.txt", "-nb-gpus", "2"], "-nb-gpus must be 1"),
                      (base + ["-colors", "list.txt", "-query", "s1.fq"], "separate modes"),
                      (base + ["-colors", "list.txt", "-quantify", "s1.fq"], "separate modes"),
                      (base + ["-colors", "list.txt", "-thread", "s1.fq"], "separate modes"),
                      (base + ["-colors", "list.txt", "-components"], "separate modes"),
                      (base + ["-colors", "list.txt", "-redo-links"], "separate modes"),
                      (base + ["-colors"], "needs a value"),
                      (base + ["-colors", "absent.txt"], "cannot open sample list"),
                      (base + ["-colors", "bad.txt"], "cannot open sample file"),
                      (base + ["-colors", "empty.txt"], "no samples"),
                      (base + ["-colors", "many.txt"], str(MAX_COLORS))):
        r = run(args)
        assert r.returncode == 1 and msg in r.stdout + r.stderr, (args, r.stdout, r.stderr)
        assert sorted(os.listdir(d)) == sorted(inputs), args
    assert (d / "g.unitigs.fa").read_bytes() == fa
