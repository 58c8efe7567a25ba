"""Shared helpers, inputs and test bodies of the connected-component tests (test_hostsim_components.py on the simulator,
test_gpu_components.py on the device): cdbg_components / cdbg_fetch_components / `bcalm -components`.

Expected partitions never come from the code under test: they are model(), a pure-Python union-find over Graph.links() -- which
test_links.py / test_relink.py pin -- renumbered by smallest member; for the hand-made set they are written out by hand.  The totals come
from g.unitigs() lengths and KC.  Every check also asserts the sums over all components, that first_unitig is the smallest member and
strictly ascending, that out[] agrees with the arrays, and that a sub-range fetch equals the slice of the full fetch."""
import os
import random
import subprocess

import kwidth_cases as kc
import oracle_lib
import query_cases as qc
from bcalm_amd import api

E_PARAM, E_STATE = -1, -4
rc = qc.rc
C = api.C


# ---------------------------------------------------------------- the model
def union_find(n, pairs):
    """-> labels of 0 .. n - 1 under the given pairs, components numbered in the order of their smallest member"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    ids, labels = {}, []
    for u in range(n):                                       # (a root is the smallest member of its tree: met before every other member)
        r = find(u)
        if r not in ids:
            assert r == u
            ids[r] = len(ids)
        labels.append(ids[r])
    return labels


def model(links, lens, kcs, k):
    """labels and per-component totals from Graph.links() and the unitigs' lengths and KC"""
    labels = union_find(len(links), ((u, v) for u, l in enumerate(links) for _, v, _ in l))
    comps = []
    for u, c in enumerate(labels):
        if c == len(comps):
            comps.append({"first_unitig": u, "unitigs": 0, "bases": 0, "kmers": 0, "kc": 0})
        d = comps[c]
        d["unitigs"] += 1; d["bases"] += lens[u]; d["kmers"] += lens[u] - k + 1; d["kc"] += kcs[u]
    return labels, comps


def totals_of(comps):
    """what cdbg_components reports, from a list of per-component dicts"""
    big = max(range(len(comps)), key=lambda c: (comps[c]["unitigs"], -c)) if comps else 0
    return {"components": len(comps), "largest": comps[big]["unitigs"] if comps else 0, "largest_id": big,
            "singletons": sum(1 for d in comps if d["unitigs"] == 1)}


def raw_bytes(raw, U):
    tot, comp, fu, nu, bases, kmers, kcs = raw
    n = tot["components"]
    return bytes(comp)[:4 * U] + bytes(fu)[:4 * n] + b"".join(bytes(a)[:8 * n] for a in (nu, bases, kmers, kcs))


def check(g, k, labels=None, comps=None, links=None):
    """label the resident set and compare with the model over g.links() (and with `labels` / `comps` where the caller wrote them out);
    -> (totals, labels, components, the raw arrays)"""
    raw = g.components_raw()
    tot, comp, fu, nu, bases, kmers, kcs = raw
    links = g.links() if links is None else links
    ut = g.unitigs()
    U = len(ut)
    lens, ukc = [len(s) for s, _ in ut], [c for _, c in ut]
    exp_labels, exp_comps = model(links, lens, ukc, k)
    if labels is not None:
        assert exp_labels == labels and exp_comps == comps   # the model itself, against what was written out by hand
    n = tot["components"]
    got_labels = list(comp[:U])
    got_comps = [{"first_unitig": fu[i], "unitigs": nu[i], "bases": bases[i], "kmers": kmers[i], "kc": kcs[i]} for i in range(n)]
    assert n == len(exp_comps), (n, len(exp_comps))
    assert got_labels == exp_labels, [(u, a, b) for u, (a, b) in enumerate(zip(got_labels, exp_labels)) if a != b][:5]
    assert got_comps == exp_comps, [(i, a, b) for i, (a, b) in enumerate(zip(got_comps, exp_comps)) if a != b][:5]
    # the sums over all components
    assert sum(d["unitigs"] for d in got_comps) == U
    assert sum(d["bases"] for d in got_comps) == sum(lens)
    assert sum(d["kmers"] for d in got_comps) == sum(x - k + 1 for x in lens)
    assert sum(d["kc"] for d in got_comps) == sum(ukc)
    # first_unitig: the smallest member, strictly ascending
    seen = {}
    for u, c in enumerate(got_labels):
        seen.setdefault(c, u)
    assert [seen[c] for c in range(n)] == [d["first_unitig"] for d in got_comps]
    assert all(a["first_unitig"] < b["first_unitig"] for a, b in zip(got_comps, got_comps[1:]))
    assert tot == totals_of(got_comps), (tot, totals_of(got_comps))
    # a sub-range equals the slice of the full fetch; the ends of the range are legal
    for first, cnt in ((0, 0), (n, 0), (n // 3, n - n // 3), (0, min(n, 1)), (max(n - 1, 0), min(n, 1))):
        sub = g.components_raw(first, cnt)
        assert sub[0] == tot and bytes(sub[1])[:4 * U] == bytes(comp)[:4 * U]
        assert bytes(sub[2])[:4 * cnt] == bytes(fu)[4 * first:4 * (first + cnt)]
        for a, b in zip(sub[3:], raw[3:]):
            assert bytes(a)[:8 * cnt] == bytes(b)[8 * first:8 * (first + cnt)]
    assert g.components() == (got_labels, got_comps)
    return tot, got_labels, got_comps, raw


def refused(call, what, code=E_STATE):
    try:
        call()
        raise AssertionError("no error: " + what)
    except api.CdbgError as e:
        assert e.code == code and what in str(e), e


def loaded(lib, seqs, k, kcs=None):
    g = api.Graph(k, 1, lib=lib)
    g.load_unitigs(seqs, kcs)
    return g


# ---------------------------------------------------------------- 1. the hand-made loaded set
HAND_K = 5
HAND = [                # (sequence, KC)
    ("TCAGAGT", 3),     # 0  chain: ..GAGT
    ("CTGGGT", 1),      # 1  isolated
    ("GAGTATGTA", 4),   # 2  chain: GAGT.. ..TGTA
    ("AGGATAAGGA", 1),  # 3  its only link is to itself (AGGA .. AGGA)
    ("TGTATACCA", 5),   # 4  chain: TGTA..
    ("CGGCGGAG", 9),    # 5  a record ...
    ("CGGCGGAG", 2),    # 6  ... listed twice: no link between the two, each links to 7
    ("GGAGGGC", 6),     # 7  GGAG..
    ("ACGACGT", 5),     # 8  ..ACGT, a (k - 1)-mer that is its own reverse complement: linked to itself and to 9 ...
    ("TCAATACGT", 3),   # 9  ..ACGT: ... which it enters through the end it leaves by
    ("ACGGTTC", 5),     # 10 ..GTTC
    ("AATGGAAC", 8),    # 11 ..GAAC = rc(GTTC): linked end to end on opposite strands
]
HAND_LABELS = [0, 1, 0, 2, 0, 3, 3, 3, 4, 4, 5, 5]
HAND_COMPS = [
    {"first_unitig": 0, "unitigs": 3, "bases": 25, "kmers": 13, "kc": 12},
    {"first_unitig": 1, "unitigs": 1, "bases": 6, "kmers": 2, "kc": 1},
    {"first_unitig": 3, "unitigs": 1, "bases": 10, "kmers": 6, "kc": 1},
    {"first_unitig": 5, "unitigs": 3, "bases": 23, "kmers": 11, "kc": 17},
    {"first_unitig": 8, "unitigs": 2, "bases": 16, "kmers": 8, "kc": 8},
    {"first_unitig": 10, "unitigs": 2, "bases": 15, "kmers": 7, "kc": 13},
]


def handmade(lib):
    g = loaded(lib, [s for s, _ in HAND], HAND_K, [c for _, c in HAND])
    try:
        links = g.links()
        assert {v for _, v, _ in links[3]} == {3} and links[1] == []
        assert 6 not in [v for _, v, _ in links[5]] and [v for _, v, _ in links[5]] == [v for _, v, _ in links[6]] == [7]
        assert sorted(v for _, v, _ in links[8]) == [8, 9]
        tot, labels, comps, _ = check(g, HAND_K, HAND_LABELS, HAND_COMPS, links=links)
        assert labels == HAND_LABELS and comps == HAND_COMPS
        assert tot == {"components": 6, "largest": 3, "largest_id": 0, "singletons": 2}     # (components 0 and 3 tie: the smaller id)
    finally:
        g.close()


# ---------------------------------------------------------------- 2. fixtures
# name, k, unitigs, components, unitigs of the largest components (descending; as many as are pinned)
FIXTURES = [("rand_a", 31, 335, 11, [325]), ("rand_b", 31, 401, 6, [396]), ("palin4", 4, 5, 2, [3, 2]), ("pufferize_refs", 9, 3, 1, [3]),
            ("spec_gtatac", 3, 2, 1, [2]), ("tiny_read", 21, 1, 1, [1])]


def fixture(lib, name, k, n_unitigs, n_comp, sizes):
    g = qc.built(lib, oracle_lib.read_input(name), k, 1)
    try:
        tot, labels, comps, _ = check(g, k)
        assert (len(labels), tot["components"]) == (n_unitigs, n_comp)
        assert sorted((d["unitigs"] for d in comps), reverse=True)[:len(sizes)] == sizes and tot["largest"] == sizes[0]
        if name == "tiny_read":
            assert g.links() == [[]]
    finally:
        g.close()


# ---------------------------------------------------------------- 3. key widths
K_WIDTHS = [3, 32, 33, 255]


def key_width(lib, k, amin):
    g = qc.built(lib, kc.edge_text(k, 1), k, amin)
    try:
        tot, labels, _, _ = check(g, k)
        assert len(labels) > 0 and tot["components"] >= 1
    finally:
        g.close()


# ---------------------------------------------------------------- 4. chains
def chain_pieces(n, k, seed):
    """one random sequence cut into n pieces of k + 5 bases that overlap by k - 1: a path of n unitigs"""
    rng = random.Random(seed)
    step = 6
    s = "".join(rng.choices("ACGT", k=step * (n - 1) + k + 5))
    return [s[step * i:step * i + k + 5] for i in range(n)]


def chains(lib, n, k=31):
    pieces = chain_pieces(n, k, 41)
    shuffled = list(pieces); random.Random(7).shuffle(shuffled)
    for seqs in (pieces, pieces[::-1], shuffled):
        g = loaded(lib, seqs, k)
        try:
            tot, labels, comps, _ = check(g, k)
            assert tot == {"components": 1, "largest": n, "largest_id": 0, "singletons": 0} and set(labels) == {0}
            assert comps == [{"first_unitig": 0, "unitigs": n, "bases": n * (k + 5), "kmers": 6 * n, "kc": 0}]
        finally:
            g.close()
    m = n // 4
    four = [chain_pieces(m, k, 50 + j) for j in range(4)]
    seqs = [four[j][i] for i in range(m) for j in range(4)]             # interleaved record by record
    g = loaded(lib, seqs, k, list(range(len(seqs))))
    try:
        tot, labels, comps, _ = check(g, k)
        assert tot == {"components": 4, "largest": m, "largest_id": 0, "singletons": 0}
        assert labels == [u % 4 for u in range(4 * m)]
        assert [d["kc"] for d in comps] == [sum(range(j, 4 * m, 4)) for j in range(4)]
    finally:
        g.close()


def shuffled_chain(n, k=31):
    seqs = chain_pieces(n, k, 41); random.Random(7).shuffle(seqs)
    return seqs


# ---------------------------------------------------------------- 5. star
STAR_K = 15


def star_set(spokes=3000, spokes2=120, isolated=5):
    """one hub whose last k - 1 bases begin `spokes` records with distinct continuations, a second, smaller star and a few isolated
    records, in a seeded shuffle; -> (sequences, KC)"""
    k = STAR_K
    rng = random.Random(15)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))

    def one(ns):
        hub = rnd(40)
        tails = set()
        while len(tails) < ns:
            tails.add(rnd(9))
        return [hub] + [hub[-(k - 1):] + t for t in sorted(tails)]
    seqs = one(spokes) + one(spokes2) + [rnd(25) for _ in range(isolated)]
    rng.shuffle(seqs)
    return seqs, [1 + (i % 7) for i in range(len(seqs))]


def star(lib):
    k = STAR_K
    seqs, kcs = star_set()
    g = loaded(lib, seqs, k, kcs)
    try:
        links = g.links()
        assert max(sum(1 for s, _, _ in l if s == sg) for l in links for sg in "+-") >= 3000      # one end carries all the spokes
        tot, labels, comps, _ = check(g, k, links=links)
        assert tot == {"components": 7, "largest": 3001, "largest_id": tot["largest_id"], "singletons": 5}
        assert sorted(d["unitigs"] for d in comps) == [1, 1, 1, 1, 1, 121, 3001]
    finally:
        g.close()


# ---------------------------------------------------------------- 6. the same bytes on every run (device)
def same_bytes(lib, seqs, k, kcs=None, runs=3):
    g = api.Graph(k, 1, lib=lib)
    try:
        ref = None
        for i in range(runs):
            if i:
                g.reset()
            g.load_unitigs(seqs, kcs)
            b = raw_bytes(g.components_raw(), len(seqs))
            assert ref is None or b == ref
            ref = b
        check(g, k)
    finally:
        g.close()


# ---------------------------------------------------------------- 7. state
def state(lib):
    k = 15
    text = oracle_lib.read_input("rand_a")
    u64, u32 = C.c_uint64, C.c_uint32
    g = api.Graph(k, 2, lib=lib)
    fetch = lambda *a: g._ck(lib.cdbg_fetch_components(g._h, *a))
    nothing = (None, 0, 0, None, None, None, None, None)
    try:
        refused(g.components_raw, "cdbg_components before cdbg_glue")
        refused(lambda: fetch(*nothing), "cdbg_fetch_components before cdbg_glue")
        g.push_text(text); g.count()
        refused(g.components_raw, "before cdbg_glue")
        g.compact(); g.glue()
        refused(lambda: fetch(*nothing), "cdbg_fetch_components before cdbg_components")
        tot, labels, comps, raw = check(g, k)
        n, U = tot["components"], len(labels)
        fetch(*nothing)                                      # all-NULL output pointers are legal
        fetch(None, 0, n, None, None, None, None, None)
        comp, nu = (u32 * U)(), (u64 * n)()
        fetch(comp, 0, 0, None, None, None, None, None); fetch(None, 0, n, None, nu, None, None, None)
        assert list(comp) == labels and list(nu) == [d["unitigs"] for d in comps]
        for first, cnt in ((n + 1, 0), (0, n + 1), (n, 1), (1, 2 ** 64 - 1), (2 ** 64 - 1, 2)):
            refused(lambda: fetch(None, first, cnt, None, None, None, None, None), "cdbg_fetch_components: components", E_PARAM)
        before = raw_bytes(raw, U)
        g._ck(lib.cdbg_link(g._h))                           # a repeated cdbg_link does not invalidate the labels
        fu, ba, km, kk = (u32 * n)(), (u64 * n)(), (u64 * n)(), (u64 * n)()
        fetch(comp, 0, n, fu, nu, ba, km, kk)
        assert bytes(comp) + bytes(fu) + bytes(nu) + bytes(ba) + bytes(km) + bytes(kk) == before
        g.reset()                                            # reset forgets them
        refused(lambda: fetch(*nothing), "cdbg_fetch_components before cdbg_glue")
        g.run()                                              # (the reads stay resident: the same graph, rebuilt)
        refused(lambda: fetch(*nothing), "cdbg_fetch_components before cdbg_components")
        assert raw_bytes(check(g, k)[3], U) == before
        ua = g.unitigs()
    finally:
        g.close()
    # a freshly loaded set with no cdbg_link yet: the call builds the links itself; another set after a reset: the labels go with the set
    g = api.Graph(k, 1, lib=lib)
    fetch = lambda *a: g._ck(lib.cdbg_fetch_components(g._h, *a))
    try:
        g.load_unitigs([s for s, _ in ua], [c for _, c in ua])
        nl = u64()
        refused(lambda: g._ck(lib.cdbg_num_links(g._h, C.byref(nl))), "cdbg_num_links before cdbg_link")
        out = (u64 * 4)()
        g._ck(lib.cdbg_components(g._h, out))
        g._ck(lib.cdbg_num_links(g._h, C.byref(nl)))
        assert nl.value == sum(len(l) for l in g.links()) > 0
        assert check(g, k)[0] == tot and list(out) == [tot["components"], tot["largest"], tot["largest_id"], tot["singletons"]]
        g.reset()
        g.load_unitigs([s for s, _ in ua[::2]])
        refused(lambda: fetch(*nothing), "cdbg_fetch_components before cdbg_components")
        assert len(check(g, k)[1]) == len(ua[::2])
    finally:
        g.close()
    g = loaded(lib, [], k)                                   # an empty loaded set gives zeros
    try:
        raw = g.components_raw()
        assert raw[0] == {"components": 0, "largest": 0, "largest_id": 0, "singletons": 0}
        assert g.components() == ([], [])
        g._ck(lib.cdbg_fetch_components(g._h, None, 0, 0, None, None, None, None, None))
        refused(lambda: g._ck(lib.cdbg_fetch_components(g._h, None, 0, 1, None, None, None, None, None)), "cdbg_fetch_components: components", E_PARAM)
    finally:
        g.close()


def state_two_ranks(lib, monkeypatch, memcpy):
    """a rank that holds a share of the unitigs cannot answer for the graph (the loop-back pattern of thread_cases.state_two_ranks)"""
    import loopback

    def all_refused(g):
        refused(g.components_raw, "cdbg_components: one rank only")
        refused(lambda: g._ck(lib.cdbg_fetch_components(g._h, None, 0, 0, None, None, None, None, None)), "cdbg_fetch_components: one rank only")
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
def parse_unitigs_fa(path):
    """-> [(sequence, KC, [target of every L: token])] of a unitigs file, in file order"""
    recs = []
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith(">"):
            toks = line.split(" ")
            kcv = [int(t[5:]) for t in toks if t.startswith("KC:i:")]
            recs.append(["", kcv[0] if kcv else 0, [int(t.split(":")[2]) for t in toks if t.startswith("L:")]])
        elif line:
            recs[-1][0] += line
    return recs


def cli(exe, tmp_path, name, k):
    """both tables must be what the model gives for the file's records, with the links the construction run wrote into the headers"""
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
    recs = parse_unitigs_fa(d / "g.unitigs.fa")
    assert sum(c for _, c, _ in recs) > 0
    labels = union_find(len(recs), ((u, v) for u, (_, _, l) in enumerate(recs) for v in l))
    _, comps = model([[(None, v, None) for v in l] for _, _, l in recs], [len(s) for s, _, _ in recs], [c for _, c, _ in recs], k)
    exp_c = "#component\tunitigs\tbases\tkmers\tKC\tfirst_unitig\n" + "".join(
        "%d\t%d\t%d\t%d\t%d\t%d\n" % (i, c["unitigs"], c["bases"], c["kmers"], c["kc"], c["first_unitig"]) for i, c in enumerate(comps))
    exp_u = "#unitig\tcomponent\n" + "".join("%d\t%d\n" % (u, c) for u, c in enumerate(labels))
    base = ["-in", "g.unitigs.fa", "-kmer-size", str(k)]
    r = run(base + ["-components", "-verbose"])
    assert r.returncode == 0, r.stdout + r.stderr
    t = totals_of(comps)
    assert "components: %d components, %d unitigs in the largest (component %d), %d components of one unitig" % (
        t["components"], t["largest"], t["largest_id"], t["singletons"]) in r.stdout, r.stdout
    assert "components written to g.components.tsv and g.unitig_components.tsv" in r.stdout, r.stdout
    assert (d / "g.components.tsv").read_text() == exp_c
    assert (d / "g.unitig_components.tsv").read_text() == exp_u
    assert (d / "g.unitigs.fa").read_bytes() == fa           # untouched
    assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa", "g.components.tsv", "g.unitig_components.tsv"])
    r = run(["-in", "g", "-kmer-size", str(k), "-components", "-out", "h"])     # -out names another prefix: there is no h.unitigs.fa
    assert r.returncode == 1 and "cannot open" in r.stdout + r.stderr
    os.remove(d / "g.components.tsv"); os.remove(d / "g.unitig_components.tsv")
    for args, msg in ((base + ["-components", "-nb-gpus", "2"], "-nb-gpus must be 1"),
                      (base + ["-components", "-query", "x"], "separate modes"),
                      (base + ["-components", "-redo-links"], "separate modes"),
                      (base + ["-components", "-thread", "x"], "separate modes"),
                      (base + ["-components", "-quantify", "x"], "separate modes"),
                      (["-in", "absent.unitigs.fa", "-kmer-size", str(k), "-components"], "cannot open")):
        r = run(args)
        assert r.returncode == 1 and msg in r.stdout + r.stderr, (args, r.stdout, r.stderr)
    assert (d / "g.unitigs.fa").read_bytes() == fa
    assert sorted(os.listdir(d)) == sorted(["reads.fa", "g.unitigs.fa"])
