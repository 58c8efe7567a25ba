"""Shared inputs and the test body of the consumer-agreement tests (test_hostsim_walk.py on the simulator, test_gpu_walk.py on the device):
cdbg_query, cdbg_quantify, cdbg_thread and cdbg_color walk the same text with one window walker (k_window.h) and must give one answer.

The truth is what cdbg_query reports -- it never extends, and its own suite pins it against brute force: the counters of cdbg_quantify are
the multiplicities of (unitig, offset) among its hit words, the runs of cdbg_thread are thread_cases.fold() of them, the positions one
colour marks are the set of them, and every consumer counts the windows quant_cases.windows_of() counts and finds as many as the hit words
hold."""
import collections
import random

import quant_cases as qn
import query_cases as qc
import thread_cases as tc

rc = qc.rc
TILE = 8192                                                  # the quant / colour tile; the query / thread tile is half of it
KS = [8, 31, 32]                                             # W = 1; W = 1 with odd k; W = 2 with even k (palindromes exist at 8 and 32)
ENVS = [{}, {"CDBG_QUANT_NO_EXTEND": "1"}, {"CDBG_QUERY_BATCH": "1"}]      # the last: the floor, max(4 k, 256) bases per batch

_inputs = {}


def palindrome_seq(k, taken, rng):
    """X + h + rc(h) + Y: a k-mer that is its own reverse complement between two flanks of 5 bases; no k-mer of it is in `taken` (canonical
    k-mers) or spelled twice, and the k-mers beside the palindrome are not each other's reverse complement"""
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    while True:
        h = rnd(k // 2)
        X, Y = rnd(5), rnd(5)
        P = X + h + rc(h) + Y
        own = [qc.canon(P[i:i + k]) for i in range(len(P) - k + 1)]
        if rc(X[-1]) != Y[0] and len(set(own)) == len(own) and not taken & set(own):
            return P


def inputs(lib, k):
    """-> (the set to load, the queries, the palindromic sequence or None), built once per library and k"""
    key = (id(lib), k)
    if key in _inputs:
        return _inputs[key]
    rng = random.Random(1000 + k)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    g = qc.built(lib, "\n".join(rnd(rng.randrange(200, 601)) for _ in range(20)) + "\n", k, 1)
    try:
        ut = [s for s, _ in g.unitigs()]
    finally:
        g.close()
    assert any(len(s) > k + 2 for s in ut)
    pal = None
    if k % 2 == 0:
        pal = palindrome_seq(k, set(qc.brute_index(ut, k)), rng)
    seqs = ut + ([pal] if pal else [])
    qs = []
    for s in seqs:                                           # every unitig, forward and reverse-complemented
        qs += [s, rc(s)]
    for s in sorted(ut, key=len)[-8:]:                       # reads cut from them with an N inside
        a = rng.randrange(0, max(1, len(s) - k - 2))
        r = s[a:a + rng.randrange(k + 2, 3 * k + 2)]
        at = rng.randrange(1, len(r) - 1)
        qs += [r[:at] + "N" + r[at + 1:], rc(r)[:at] + "n" + rc(r)[at + 1:]]
    qs += [ut[0][:k - 1], "", "", "", rc(ut[-1])[:k - 1], "", ""]      # sequences of k - 1 bases, runs of empty sequences
    long = ""                                                # one concatenation that takes the text past two quant tiles (four query tiles)
    i, rest = 0, sum(len(q) for q in qs)
    while len(long) < 2000 or rest + len(long) <= 2 * TILE + k:
        long += ut[i % len(ut)] if (i // len(ut)) % 2 == 0 else rc(ut[i % len(ut)])
        i += 1
    qs.append(long)
    assert sum(len(q) for q in qs) > 2 * TILE + k
    _inputs[key] = (seqs, qs, pal)
    return _inputs[key]


def agree(lib, monkeypatch, k, env):
    seqs, qs, pal = inputs(lib, k)
    g = qn._fresh(lib, seqs, k, monkeypatch, env)
    try:
        info = g.index_info()
        assert info["positions"] == info["distinct"]         # every k-mer spelled once: extension is on unless the environment turns it off
        rows = g.query(qs)                                   # the truth: one probe per window
        windows = sum(1 for q in qs for _ in qn.windows_of(q, k))
        mult = collections.Counter((h[0], h[1]) for row in rows for h in row if h is not None)
        found = sum(mult.values())
        assert 0 < found < windows
        assert any(h[2] == "+" for row in rows for h in row if h) and any(h[2] == "-" for row in rows for h in row if h)
        if pal:                                              # rc(pal) walks pal downwards on strand -; the palindrome itself reports strand +
            u, row = len(seqs) - 1, rows[2 * len(seqs) - 1]
            assert [h[2] for h in row] == ["-"] * 5 + ["+"] + ["-"] * 5 and all(h[0] == u for h in row), row
            assert [h[1] for h in row] == list(range(10, -1, -1))
        # cdbg_quantify: the counter of a position is its multiplicity among the hit words
        q = g.quantify(qs)
        per = g.quant(per_kmer=True)
        assert len(per) == len(seqs)
        for u, (_, _, ab) in enumerate(per):
            assert ab == [mult.get((u, o), 0) for o in range(len(seqs[u]) - k + 1)], u
        # cdbg_thread: the runs are the fold of the hit words
        raw = g.thread_raw(qs)
        t = raw[0]
        assert tc.runs_of(raw, qs) == tc.fold(rows)
        # cdbg_color, one colour: the coloured positions are the positions hit
        g.color_open(1)
        c = g.color(0, qs)
        classes = g.color_classes()
        coloured = {(u, o + i) for u, runs in enumerate(g.color_runs()) for o, n, cl in runs if classes[cl]["colors"] for i in range(n)}
        assert coloured == set(mult)
        for name, r in (("quantify", q), ("thread", t), ("color", c)):
            assert (r["windows"], r["found"]) == (windows, found), (name, r, windows, found)
            assert (r["extended"] == 0) if "CDBG_QUANT_NO_EXTEND" in env else (0 < r["extended"] <= found), (name, r)
    finally:
        g.close()
