"""Shared helpers, inputs and test bodies of the colour-query tests (test_hostsim_color_query.py on the simulator, test_gpu_color_query.py on
the device): cdbg_color_query / cdbg_fetch_color_query / cdbg_fetch_color_query_counts / `bcalm -colors -color-query`.

Expected values never come from the code under test.  brute() restates the definitions of include/cdbg.h: query_cases.brute_index gives the
smallest-occurrence position of every canonical k-mer, color_cases.brute the colour set of every position from the marks, color_cases.fold
the colour runs and classes of those sets, query_cases.expected the hit of every window -- and then every window is taken by itself: it is
found or not, it adds one to the count of every colour of its position's set, and it continues the window before it when cdbg_thread's rule
says so and both positions lie in the same colour run.  reported() applies the threshold in Python integers."""
import gzip
import os
import random
import subprocess

import color_cases as cc
import kwidth_cases as kc
import oracle_lib
import quant_cases as qn
import query_cases as qc
import thread_cases as tc
from bcalm_amd import api

E_PARAM = cc.E_PARAM
E_STATE = cc.E_STATE
THREAD_TILE = 1024                                           # bcalm_amd/csrc/k_thread.h
rc = qc.rc
refused = cc.refused


def brute(seqs, k, n_colors, marks, queries, idx=None):
    """-> per query {"windows", "found", "counts": [per colour], "segments": [(q, unitig, offset, strand, n, class)]}, and the classes"""
    idx = qc.brute_index(seqs, k) if idx is None else idx
    sets, _ = cc.brute(seqs, k, marks, idx)
    runs, table = cc.fold(sets)
    run_of = []                                              # per unitig, per position: (the colour run's number in the unitig, its class)
    for ur, row in zip(runs, sets):
        ids = [None] * len(row)
        for j, (o, n, c) in enumerate(ur):
            for p in range(o, o + n):
                ids[p] = (j, c)
        run_of.append(ids)
    out = []
    for q, row in zip(queries, qc.expected(seqs, idx, k, queries)):
        segs, prev, counts, found = [], None, [0] * n_colors, 0
        for p, h in enumerate(row):
            if h is not None:
                found += 1
                j, c = run_of[h[0]][h[1]]
                for col in table[c]["colors"]:
                    counts[col] += 1
                if (prev is not None and (h[0], h[2]) == (prev[0], prev[2]) and h[1] == prev[1] + (1 if h[2] == "+" else -1)
                        and run_of[prev[0]][prev[1]][0] == j):
                    segs[-1][4] += 1
                else:
                    segs.append([p, h[0], h[1], h[2], 1, c])
            prev = h
        out.append({"windows": max(0, len(q) - k + 1), "found": found, "counts": counts, "segments": [tuple(s) for s in segs]})
    return out, table


def reported(e, num, den, of_found):
    base = e["found"] if of_found else e["windows"]
    if base == 0:
        return []
    return [c for c, x in enumerate(e["counts"]) if x >= 1 and x * den >= num * base]


def segments_of(raw, queries):
    _, _, _, _, _, seg_off, start, place, ln, cls = raw
    out, at = [], 0
    for i, q in enumerate(queries):
        out.append([(start[s] - at, place[s] >> 33, (place[s] >> 1) & 0xFFFFFFFF, "-" if place[s] & 1 else "+", ln[s], cls[s]) for s in range(seg_off[i], seg_off[i + 1])])
        at += len(q)
    return out


def query_bytes(raw, n, totals=True):
    """everything cdbg_fetch_color_query returns, as bytes (behind the call's totals)"""
    tot, found, ncol, bits, nw, seg_off, start, place, ln, cls = raw
    S = tot["segments"]
    return ((repr(sorted(tot.items())).encode() if totals else b"") + bytes(found)[:4 * n] + bytes(ncol)[:4 * n] + bytes(bits)[:4 * n * nw] + bytes(seg_off)
            + bytes(start)[:8 * S] + bytes(place)[:8 * S] + bytes(ln)[:4 * S] + bytes(cls)[:4 * S])


def check(g, k, n_colors, exp, queries, share=(0, 1), of_found=False, dicts=False, counts=True, **kw):
    """one colour query against brute()'s `exp`: totals, segments, found, bit rows (padding zero), colours per sequence, the counts matrix;
    -> the raw arrays"""
    raw = g.color_query_raw(queries, share, of_found, **kw)
    tot, found, ncol, bits, nw, seg_off, start, place, ln, cls = raw
    n = len(queries)
    assert nw == (n_colors + 31) // 32
    got = segments_of(raw, queries)
    n_rep, cols = 0, []
    for i, e in enumerate(exp):
        assert got[i] == e["segments"], (i, got[i][:4], e["segments"][:4])
        assert found[i] == e["found"] == sum(s[4] for s in got[i]), (i, found[i], e["found"])
        cols.append(reported(e, share[0], share[1], of_found))
        row = sum(bits[i * nw + j] << (32 * j) for j in range(nw))
        assert row == sum(1 << c for c in cols[i]) and row >> n_colors == 0, (i, bin(row), cols[i])      # (padding bits zero)
        assert ncol[i] == len(cols[i])
        n_rep += 1 if cols[i] else 0
    assert seg_off[0] == 0 and seg_off[n] == tot["segments"] == sum(len(e["segments"]) for e in exp)
    assert tot["windows"] == sum(1 for q in queries for _ in qn.windows_of(q, k))
    assert tot["found"] == sum(e["found"] for e in exp) and tot["reported"] == n_rep and tot["extended"] <= tot["found"]
    if counts:
        m, cnt, N = g.color_query_counts()
        assert (m, N) == (n, n_colors) and list(cnt[:n * N]) == [x for e in exp for x in e["counts"]]
    if dicts:
        assert g.color_query(queries, share, of_found) == [{"windows": e["windows"], "found": e["found"], "colors": c, "segments": e["segments"]} for e, c in zip(exp, cols)]
    return raw


# ---------------------------------------------------------------- 1. every key width
def key_width(lib, k):
    text = kc.edge_text(k, 1)
    g = qc.built(lib, text, k, 2)
    try:
        ut = [s for s, _ in g.unitigs()]
        idx = qc.brute_index(ut, k)
        reads = [r for r in text.split("\n") if r]
        head = reads[:10]                                    # (the later reads alone spell runs of the empty set; color_cases.key_width says why)
        marks = [(0, head[0::2]), (1, head[1::2] + reads[10::4]), (2, [rc(r) for r in head[0::3]])]
        cc.mark(g, 3, marks)
        qs = qc.variants(reads, k, k)
        exp, table = brute(ut, k, 3, marks, qs, idx)
        raw = check(g, k, 3, exp, qs, (1, 3), dicts=k in (31, 32))
        if k >= 5:
            assert raw[0]["windows"] > raw[0]["found"] > 0 and 0 < raw[0]["reported"] < len(qs)
            assert any(s[3] == "+" for e in exp for s in e["segments"]) and any(s[3] == "-" for e in exp for s in e["segments"])
        check(g, k, 3, exp, qs, (1, 1), True, counts=False)
    finally:
        g.close()


# ---------------------------------------------------------------- 2. run and word edges
def run_edges(lib, monkeypatch, runs=1):
    """color_cases.word_edge_input(): kmer_off 0, 31, 32, 33, 63, 64, 65, 165 ...; the unitig of 100 positions (65 .. 164) coloured so that its
    colour set changes exactly at positions 95/96, 127/128 and 159/160 -- offsets 31, 63 and 95 of the unitig"""
    k, seqs, _ = cc.word_edge_input()
    B, BIG = seqs[cc.BIG], cc.BIG
    piece = lambda a, b: B[a:b + k - 1]                      # the bases that spell the positions [a, b) of B
    marks = [(0, [piece(0, 31), piece(95, 100), seqs[1], seqs[0], seqs[3][:k + 11]]),
             (1, [rc(piece(31, 63)), rc(seqs[2]), seqs[7], rc(seqs[0])[3:]]),
             (2, [piece(63, 95), seqs[0][:k + 5], "ACGTN" + seqs[9]])]
    qs = [piece(30, 40),                                     # starts on the last position of a colour run
          piece(20, 32),                                     # ends on the first position of the next
          piece(31, 63),                                     # covers exactly one colour run
          B, rc(B),                                          # the whole unitig, forwards and backwards
          rc(piece(62, 96)), seqs[1], rc(seqs[2]), seqs[0] + "N" + seqs[7], seqs[4] + seqs[5], "", piece(0, 100)[:k - 1], "N" * 30,
          "".join(random.Random(9).choice("ACGT") for _ in range(60))]
    idx = qc.brute_index(seqs, k)
    exp, table = brute(seqs, k, 3, marks, qs, idx)
    c = [s[5] for s in exp[3]["segments"]]
    assert exp[3]["segments"] == [(0, BIG, 0, "+", 31, c[0]), (31, BIG, 31, "+", 32, c[1]), (63, BIG, 63, "+", 32, c[2]), (95, BIG, 95, "+", 5, c[0])]
    assert [table[x]["colors"] for x in c[:3]] == [[0], [1], [2]]
    # the reverse complement: the same colour runs in reverse order, place walking down
    assert exp[4]["segments"] == [(0, BIG, 99, "-", 5, c[0]), (5, BIG, 94, "-", 32, c[2]), (37, BIG, 62, "-", 32, c[1]), (69, BIG, 30, "-", 31, c[0])]
    assert exp[0]["segments"] == [(0, BIG, 30, "+", 1, c[0]), (1, BIG, 31, "+", 9, c[1])]
    assert exp[1]["segments"] == [(0, BIG, 20, "+", 11, c[0]), (11, BIG, 31, "+", 1, c[1])]
    assert exp[2]["segments"] == [(0, BIG, 31, "+", 32, c[1])]
    assert exp[13]["found"] == 0 and exp[10]["windows"] == exp[11]["windows"] == 0
    ref = None
    for _ in range(runs):
        got = []
        for env in ({}, {"CDBG_QUANT_NO_EXTEND": "1"}):
            g = qn._fresh(lib, seqs, k, monkeypatch, env)
            try:
                cc.mark(g, 3, marks)
                assert g.color_runs()[BIG] == [(0, 31, c[0]), (31, 32, c[1]), (63, 32, c[2]), (95, 5, c[0])]
                raw = check(g, k, 3, exp, qs, (1, 2), dicts=not env)
                assert (raw[0]["extended"] == 0) if env else (raw[0]["extended"] > 0), raw[0]
                got.append(query_bytes(raw, len(qs), totals=False))      # (without extension `extended` differs, and nothing else)
                assert query_bytes(check(g, k, 3, exp, qs, (1, 2), first_offset=37), len(qs), totals=False) == got[-1]      # offsets[0] != 0
            finally:
                g.close()
        assert got[0] == got[1]
        assert ref is None or got[0] == ref
        ref = got[0]


# ---------------------------------------------------------------- 3. colour-count edges
def count_input(n_colors):
    k = cc.WORD_K
    seqs = cc.distinct_seqs(k, [20 + 3 * (i % 7) for i in range(24)], 33)
    rng = random.Random(n_colors)
    junk = "".join(rng.choice("ACGT") for _ in range(40))
    used = sorted({c for c in (0, 31, 32, n_colors - 1) if c < n_colors})
    spans = {0: seqs[0:10], 31: seqs[5:15], 32: seqs[8:13]}
    spans[n_colors - 1] = spans.get(n_colors - 1, []) + seqs[15:19] + [seqs[3][:k + 4]]
    marks = [(c, spans[c] + [junk]) for c in used]
    qs = seqs[:21] + [seqs[6] + seqs[9], rc(seqs[12]) + "N" + seqs[16], junk, seqs[16][:k + 3], "", seqs[3] + seqs[20] + rc(seqs[8])]
    return k, seqs, marks, qs


def color_counts(lib, n_colors):
    k, seqs, marks, qs = count_input(n_colors)
    g = qc.loaded(lib, seqs, k)
    try:
        cc.mark(g, n_colors, marks)
        exp, _ = brute(seqs, k, n_colors, marks, qs)
        assert any(0 < x < e["found"] for e in exp for x in e["counts"]) and any(e["found"] and not any(e["counts"]) for e in exp)
        assert n_colors == 1 or any(sum(1 for x in e["counts"] if x) >= 2 for e in exp)
        check(g, k, n_colors, exp, qs, (1, 2), dicts=True)
        check(g, k, n_colors, exp, qs, (0, 1))
        n, N = len(qs), n_colors
        _, full, _ = g.color_query_counts()
        for a, m in ((0, 0), (3, 4), (n - 1, 1), (n, 0), (1, n - 1)):       # a range equals a slice of the whole matrix
            m2, part, _ = g.color_query_counts(a, m)
            assert m2 == m and list(part[:m * N]) == list(full[a * N:(a + m) * N])
        refused(lambda: g.color_query_counts(n, 1), "cdbg_fetch_color_query_counts", E_PARAM)
        refused(lambda: g.color_query_counts(n + 1, 0), "cdbg_fetch_color_query_counts", E_PARAM)
    finally:
        g.close()


# ---------------------------------------------------------------- 4. threshold edges
def thresholds(lib):
    k, seqs, marks, qs = count_input(33)
    N = 33
    qs = qs + [seqs[0][:k - 1], "N" * 25, "ACGT" * 6]        # shorter than k, only N, no hit (with the empty sequence and the junk of count_input)
    g = qc.loaded(lib, seqs, k)
    try:
        cc.mark(g, N, marks)
        exp, _ = brute(seqs, k, N, marks, qs)
        nothing = [i for i, e in enumerate(exp) if e["found"] == 0]
        assert {len(qs) - 3, len(qs) - 2, len(qs) - 1, qs.index("")} <= set(nothing) and exp[-1]["windows"] > 0 and exp[-2]["windows"] > 0
        pairs = []                                           # (sequence, colour, count x, base, of_found): four with x < base, two with x == base per mode
        for of_found in (False, True):
            lt, eq = {}, {}
            for i, e in enumerate(exp):
                b = e["found"] if of_found else e["windows"]
                for c, x in enumerate(e["counts"]):
                    if x:
                        (lt if x < b else eq).setdefault((x, b), (i, c, x, b, of_found))
            pairs += list(lt.values())[:4] + list(eq.values())[:2]
        assert any(x < b for _, _, x, b, _ in pairs) and any(x == b for _, _, x, b, _ in pairs)
        row = lambda raw, i, c: (raw[3][i * raw[4] + (c >> 5)] >> (c & 31)) & 1
        for i, c, x, b, of_found in pairs:
            raw = check(g, k, N, exp, qs, (x, b), of_found, counts=False)
            assert row(raw, i, c) == 1                       # count * den >= num * base holds with equality
            assert all(raw[2][j] == 0 for j in nothing)
            if x < b:
                raw = check(g, k, N, exp, qs, (x + 1, b), of_found, counts=False)
                assert row(raw, i, c) == 0
        i, c, x, b, of_found = next(p for p in pairs if p[2] < p[3])
        den = 2 ** 32 - 5                                    # x * den needs 64 bits: a 32-bit product would compare garbage
        num = x * den // b
        assert x * den >= 2 ** 32 and (num + 1) * b > x * den >= num * b
        assert row(check(g, k, N, exp, qs, (num, den), of_found, counts=False), i, c) == 1
        assert row(check(g, k, N, exp, qs, (num + 1, den), of_found, counts=False), i, c) == 0
        raw = check(g, k, N, exp, qs, (0, 1))                # the union of the colours seen
        assert all(raw[2][j] == sum(1 for v in e["counts"] if v) for j, e in enumerate(exp))
        raw = check(g, k, N, exp, qs, (1, 1), True)          # the intersection over the k-mers found
        assert all(raw[2][j] == sum(1 for v in e["counts"] if v and v == e["found"]) for j, e in enumerate(exp))
        assert any(raw[2][j] for j in range(len(qs))) and all(raw[2][j] == 0 for j in nothing)
        check(g, k, N, exp, qs, (2 ** 32 - 1, 2 ** 32 - 1), False)
    finally:
        g.close()


# ---------------------------------------------------------------- 5. one thread run, many segments
def many_segments(lib, runs=1):
    k = 31
    rng = random.Random(3000)
    A = "".join(rng.choice("ACGT") for _ in range(3000))
    idx = qc.brute_index([A], k)
    assert len(idx) == len(A) - k + 1                        # its k-mers are distinct: the unitig threaded by itself is ONE thread run
    marks, p = [(0, []), (1, [])], 0
    while p < len(A) - k + 1:                                # two colours in alternating pieces of 1 to 5 positions
        n = min(rng.choice([1, 1, 2, 2, 3, 4, 5]), len(A) - k + 1 - p)
        marks[len(marks[0][1]) > len(marks[1][1])][1].append(A[p:p + n + k - 1])
        p += n
    qs = [A, rc(A)]
    exp, table = brute([A], k, 2, marks, qs, idx)
    S = len(exp[0]["segments"])
    assert S == len(exp[1]["segments"]) == len(marks[0][1]) + len(marks[1][1]) > THREAD_TILE > 64
    assert [s[4] for s in exp[1]["segments"]] == [s[4] for s in exp[0]["segments"]][::-1]
    ref = None
    for _ in range(runs):
        g = qc.loaded(lib, [A], k)
        try:
            cc.mark(g, 2, marks)
            raw = check(g, k, 2, exp, qs, (1, 2))
            assert raw[0]["segments"] == 2 * S
            off = (api.C.c_uint64 * 3)()                     # (cdbg_fetch_runs now reports the runs of the same sequences: one each)
            g._ck(lib.cdbg_fetch_runs(g._h, off, None, None, None))
            assert list(off) == [0, 1, 2]
            b = query_bytes(raw, 2)
        finally:
            g.close()
        assert ref is None or b == ref
        ref = b


# ---------------------------------------------------------------- 6. batch seams
def batch_seams(lib, monkeypatch, k=31):
    text = oracle_lib.read_input("rand_b")
    g = qc.built(lib, text, k, 2)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    reads = [r for r in text.split("\n") if r]
    rng = random.Random(6)
    long = "".join(ut[:2 * len(ut) // 3])
    while len(long) < 10 * 256:
        long += rc(long)
    long = long[:10 * 256 + 17]                              # one sequence of 10 batches and more
    many = []
    for i in range(60):
        r = reads[i % len(reads)]
        n = rng.randrange(k, 3 * k + 1)
        s = rng.randrange(0, max(1, len(r) - n))
        many.append(r[s:s + n] if i % 3 else rc(r[s:s + n]))
    marks = [(0, [long[:1000]] + many[:30]), (1, many[20:] + [long[800:1700]]), (2, [long[400:2200], "N" * 5 + many[7]])]
    qs = [long] + many[:40] + ["", long[5:3 * 256]] + [rc(m) for m in many[:12]] + [long[100:160] + "N" + long[160:400]]
    idx = qc.brute_index(ut, k)
    exp, _ = brute(ut, k, 3, marks, qs, idx)
    assert len(exp[0]["segments"]) > 5 and any(s[4] > 256 for s in exp[0]["segments"])      # segments that span batch seams
    got = []
    for env in ({}, {"CDBG_QUERY_BATCH": "256"}, {"CDBG_QUERY_BATCH": "256", "CDBG_QUANT_NO_EXTEND": "1"}):
        g = qn._fresh(lib, ut, k, monkeypatch, env)
        try:
            cc.mark(g, 3, marks)
            raw = check(g, k, 3, exp, qs, (1, 3), counts=not got)
            _, cnt, N = g.color_query_counts()
            assert (raw[0]["extended"] == 0) == ("CDBG_QUANT_NO_EXTEND" in env), raw[0]
            got.append(query_bytes(raw, len(qs), totals=False) + bytes(cnt)[:4 * len(qs) * N])      # (every array; `extended` alone may differ)
        finally:
            g.close()
    assert got[0] == got[1] == got[2]


# ---------------------------------------------------------------- 7. repeated k-mers (loaded sets)
def repeated_handmade(lib):
    k = 8
    seqs, qs, pal = qc.handmade(k)
    marks = [(0, qs), (1, [s for s in seqs[-45:]]), (2, [rc(s) for s in seqs[40:52]] + qs[:5])]
    queries = qs + [s for s in seqs[-45:]] + [rc(s) for s in seqs[38:50]]
    g = qc.loaded(lib, seqs, k)
    try:
        info = g.index_info()
        assert info["distinct"] < info["positions"]
        cc.mark(g, 3, marks)
        exp, _ = brute(seqs, k, 3, marks, queries)
        raw = check(g, k, 3, exp, queries, (1, 2), True, dicts=True)
        assert raw[0]["extended"] == 0                       # a set that repeats k-mers: every window probes, the smallest occurrence answers
        first = set(qc.brute_index(seqs, k).values())
        for e in exp:
            for q, u, o, s, n, c in e["segments"]:
                assert all((u, o + (i if s == "+" else -i)) in first for i in range(n))
    finally:
        g.close()


# ---------------------------------------------------------------- 8. state
def state(lib):
    k = 15
    u64, u32 = api.C.c_uint64, api.C.c_uint32
    ta, tb = oracle_lib.read_input("rand_a"), oracle_lib.read_input("rand_b")
    reads_a = [r for r in ta.split("\n") if r][:40]
    reads_b = [r for r in tb.split("\n") if r][:30]
    A = reads_a[:20] + [rc(r) for r in reads_a[:6]] + ["ACGT" * 10]
    B = reads_a[12:30] + reads_b[:5] + ["N" + reads_a[0]]
    marks = [(0, A), (1, B)]
    qs = reads_a[5:25] + [rc(reads_a[1]), "", "ACGT" * 10]
    text = "".join(qs).encode()
    offs = (u64 * (len(qs) + 1))(*[sum(len(q) for q in qs[:i]) for i in range(len(qs) + 1)])
    g = api.Graph(k, 2, lib=lib)
    out = (u64 * 5)()
    query = lambda num=0, den=1, off=offs, n=len(qs): g._ck(lib.cdbg_color_query(g._h, text, off, n, num, den, 0, out))
    fetch = lambda *a: g._ck(lib.cdbg_fetch_color_query(g._h, *(a or (None,) * 8)))
    counts = lambda first=0, n=0, p=None: g._ck(lib.cdbg_fetch_color_query_counts(g._h, first, n, p))

    def none_left(why="before cdbg_color_query"):
        refused(fetch, "cdbg_fetch_color_query " + why)
        refused(counts, "cdbg_fetch_color_query_counts " + why)
    try:
        for call, name in ((query, "cdbg_color_query"), (fetch, "cdbg_fetch_color_query"), (counts, "cdbg_fetch_color_query_counts")):
            refused(call, name + " before cdbg_glue")
        g.push_text(ta); g.count(); g.compact(); g.glue()
        ua = [s for s, _ in g.unitigs()]
        refused(query, "cdbg_color_query before cdbg_color_classes")
        g.color_open(2)
        refused(query, "cdbg_color_query before cdbg_color_classes")
        g.color(0, A); g.color(1, B)
        refused(query, "cdbg_color_query before cdbg_color_classes")      # marked, not folded
        none_left()
        exp, _ = brute(ua, k, 2, marks, qs)
        raw = check(g, k, 2, exp, qs, (1, 2), dicts=True)
        ref = query_bytes(raw, len(qs))
        n, S = len(qs), raw[0]["segments"]
        # a colour query replaces cdbg_fetch_runs by the runs of its own sequences ...
        R = sum(len(r) for r in tc.fold(qc.expected(ua, qc.brute_index(ua, k), k, qs)))
        r_off, r_start, r_place, r_len = (u64 * (n + 1))(), (u64 * max(R, 1))(), (u64 * max(R, 1))(), (u32 * max(R, 1))()
        g._ck(lib.cdbg_fetch_runs(g._h, r_off, r_start, r_place, r_len))
        assert r_off[n] == R > 0
        mine = bytes(r_off) + bytes(r_start) + bytes(r_place) + bytes(r_len)
        # ... and a later cdbg_thread leaves the colour query's fetches intact
        other = g.thread_raw(B)
        assert tc.run_bytes(other) != mine
        assert tc.run_bytes(g.thread_raw(qs)) == mine
        g.thread_raw(B)

        def fetched():
            found, ncol, bits = (u32 * n)(), (u32 * n)(), (u32 * n)()
            seg_off, start, place, ln, cls = (u64 * (n + 1))(), (u64 * S)(), (u64 * S)(), (u32 * S)(), (u32 * S)()
            fetch(None, None, None, None, None, None, None, None)        # NULL outputs: any of them
            fetch(found, None, bits, None, start, None, ln, None); fetch(None, ncol, None, seg_off, None, place, None, cls)
            return (bytes(found) + bytes(ncol) + bytes(bits) + bytes(seg_off) + bytes(start) + bytes(place) + bytes(ln) + bytes(cls))
        assert ref.endswith(fetched())
        m, cnt, N = g.color_query_counts()
        assert list(cnt[:m * N]) == [x for e in exp for x in e["counts"]]
        counts(n, 0)                                         # the empty range at the end is a range
        refused(lambda: counts(n, 1, cnt), "cdbg_fetch_color_query_counts", E_PARAM)
        refused(lambda: counts(n + 1, 0), "cdbg_fetch_color_query_counts", E_PARAM)
        # refused parameters, each with its code; a failed call leaves no result behind
        for bad in (lambda: query(2, 1), lambda: query(0, 0), lambda: query(1, 0)):
            refused(bad, "cdbg_color_query: share", E_PARAM)
            none_left()
            query(1, 2)
            assert ref.endswith(fetched())
        huge = (u64 * 2)(0, 2 ** 32 + k - 1)                 # 2^32 windows: refused before a base is read
        refused(lambda: query(0, 1, huge, 1), "more than the 4294967295", E_PARAM)
        none_left()
        down = (u64 * 3)(10, 40, 30)
        refused(lambda: query(0, 1, down, 2), "offsets not monotone", E_PARAM)
        none_left()
        g._ck(lib.cdbg_color_query(g._h, None, None, 0, 0, 1, 0, out))       # no sequences: success and zeros
        assert list(out) == [0, 0, 0, 0, 0]
        so = (u64 * 1)(7)
        fetch(None, None, None, so, None, None, None, None)
        assert so[0] == 0
        # everything that forgets the classes forgets the query result too
        check(g, k, 2, exp, qs, (1, 2))
        g.color(1, [reads_a[35]])                            # a further cdbg_color
        refused(query, "cdbg_color_query before cdbg_color_classes")
        none_left()
        exp2, _ = brute(ua, k, 2, marks + [(1, [reads_a[35]])], qs)
        check(g, k, 2, exp2, qs, (1, 2))
        g.color_open(2)                                      # a re-open
        refused(query, "cdbg_color_query before cdbg_color_classes")
        none_left()
        cc.mark(g, 2, marks)
        assert query_bytes(check(g, k, 2, exp, qs, (1, 2)), n) == ref
        g.reset()                                            # cdbg_reset
        for call, name in ((query, "cdbg_color_query"), (fetch, "cdbg_fetch_color_query"), (counts, "cdbg_fetch_color_query_counts")):
            refused(call, name + " before cdbg_glue")
        g.run()                                              # cdbg_run (count, compact, cdbg_glue): the same graph rebuilt, nothing of the colours left
        refused(query, "cdbg_color_query before cdbg_color_classes")
        none_left()
        ur = [s for s, _ in g.unitigs()]
        cc.mark(g, 2, marks)
        check(g, k, 2, brute(ur, k, 2, marks, qs)[0], qs, (1, 2))
    finally:
        g.close()
    g = api.Graph(k, 1, lib=lib)                             # cdbg_load_unitigs: the result goes with the set it was folded from
    try:
        g.load_unitigs(ua)
        cc.mark(g, 2, marks)
        assert query_bytes(check(g, k, 2, exp, qs, (1, 2)), n) == ref
        g.reset()
        g.load_unitigs(ua[: len(ua) // 2])
        refused(query, "cdbg_color_query before cdbg_color_classes")
        none_left()
        cc.mark(g, 2, marks)
        check(g, k, 2, brute(ua[: len(ua) // 2], k, 2, marks, qs)[0], qs, (1, 2))
        g.reset()
        g.load_unitigs([])                                   # an empty set: nothing is found, nothing reported
        cc.mark(g, 2, marks)
        raw = g.color_query_raw(qs)
        assert raw[0]["found"] == raw[0]["segments"] == raw[0]["reported"] == 0 and raw[0]["windows"] > 0 and list(raw[5]) == [0] * (n + 1)
    finally:
        g.close()


# ---------------------------------------------------------------- 9. CLI
def cli(lib, exe, tmp_path, name, k):
    """<prefix>.color_query.tsv must equal the fold of the API's answer for the same unitigs, samples and queries"""
    text = oracle_lib.read_input(name)
    refs = [r for r in text.split("\n") if r]
    d = tmp_path / ("cli_" + name); d.mkdir()
    with open(d / "reads.fa", "w") as f:
        for i, r in enumerate(refs):
            f.write(">r%d\n%s\n" % (i, r))
    run = lambda args: subprocess.run([exe] + args, cwd=d, capture_output=True, text=True, timeout=600)
    r = run(["-in", "reads.fa", "-kmer-size", str(k), "-abundance-min", "1", "-out", "g"])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = (d / "g.unitigs.fa").read_text().split("\n")
    ut = [lines[i + 1] for i in range(0, len(lines) - 1, 2)]
    rng = random.Random(k)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    a = max(1, len(refs) // 4)
    samples = [refs[:a] + [rnd(2 * k + 9), "ACG"], [rc(r) for r in refs[a // 2:2 * a] if set(r) <= qc.ACGT] + [rnd(3 * k)], [r[3:k + 9] for r in refs[max(0, a - 1):2 * a + 1]]]
    queries = refs[:40] + [rc(r) for r in refs[:10] if set(r) <= qc.ACGT] + [rnd(2 * k + 9), "ACG", refs[0][:k] + "N" + refs[0][k:]]
    for i, s in enumerate(samples):
        with open(d / ("s%d.fa" % i), "w") as f:
            for j, q in enumerate(s):
                f.write(">s%d\n%s\n" % (j, q))
    (d / "list.txt").write_text("s0.fa\ns1.fa\ns2.fa\n")
    with gzip.open(d / "q.fa.gz", "wt") as f:                # gzip FASTA, sequences wrapped at 50 columns, a description behind every name
        for i, q in enumerate(queries):
            f.write(">q%d some description\n" % i)
            for j in range(0, len(q), 50):
                f.write(q[j:j + 50] + "\n")
    inputs = ["reads.fa", "g.unitigs.fa", "s0.fa", "s1.fa", "s2.fa", "list.txt", "q.fa.gz"]
    g = qc.loaded(lib, ut, k)
    try:
        cc.mark(g, 3, list(enumerate(samples)))
        tsv = {}
        for share, of_found in (((0, 1), False), ((1, 2), True)):
            ans = g.color_query(queries, share, of_found)
            tsv[share] = "".join("q%d\t%d\t%d\t%d\t%s\n" % (i, e["windows"], e["found"], len(e["colors"]), ",".join(str(c) for c in e["colors"]) or "*") for i, e in enumerate(ans))
            assert any(len(e["colors"]) >= 2 for e in ans) and any(not e["colors"] for e in ans)
        assert tsv[(0, 1)] != tsv[(1, 2)]
    finally:
        g.close()
    base = ["-in", "g.unitigs.fa", "-kmer-size", str(k)]
    for extra, share in (([], (0, 1)), (["-color-share", "1/2", "-color-share-of-found"], (1, 2))):
        r = run(base + ["-colors", "list.txt", "-color-query", "q.fa.gz"] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "color-query: %d sequences, " % len(queries) in r.stdout and "colour query written to g.color_query.tsv" in r.stdout, r.stdout
        assert (d / "g.color_query.tsv").read_text() == tsv[share]
        assert sorted(os.listdir(d)) == sorted(inputs + ["g.colors.tsv", "g.color_classes.tsv", "g.color_query.tsv"])
        for f in ("g.colors.tsv", "g.color_classes.tsv", "g.color_query.tsv"):
            os.remove(d / f)
    r = run(base + ["-colors", "list.txt"])                  # -colors alone writes the two files it always wrote
    assert r.returncode == 0 and sorted(os.listdir(d)) == sorted(inputs + ["g.colors.tsv", "g.color_classes.tsv"]), r.stdout + r.stderr
    os.remove(d / "g.colors.tsv"); os.remove(d / "g.color_classes.tsv")
    for args, msg in ((base + ["-color-query", "q.fa.gz"], "-color-query needs -colors"),
                      (base + ["-colors", "list.txt", "-color-query", "q.fa.gz", "-color-share", "3/2"], "malformed -color-share"),
                      (base + ["-colors", "list.txt", "-color-query", "q.fa.gz", "-color-share", "1/0"], "malformed -color-share"),
                      (base + ["-colors", "list.txt", "-color-query", "q.fa.gz", "-color-share", "half"], "malformed -color-share"),
                      (base + ["-colors", "list.txt", "-color-query", "q.fa.gz", "-color-share", "1/"], "malformed -color-share"),
                      (base + ["-colors", "list.txt", "-color-query"], "needs a value"),
                      (base + ["-colors", "list.txt", "-color-query", "absent.fa"], "cannot open query file")):
        r = run(args)
        assert r.returncode == 1 and msg in r.stdout + r.stderr, (args, r.stdout, r.stderr)
        assert sorted(os.listdir(d)) == sorted(inputs), args
