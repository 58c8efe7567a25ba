"""Links recomputed for a unitig set the caller supplies: Graph.load_unitigs + links() (bcalm_amd/csrc/k_relink.h, the junction join
without a degree bound) and the `bcalm ... -redo-links` mode.  Expected links always come from the brute force over all pairs of ends
(oracle_py.links), never from the code under test.  CPU tests run the kernel-logic simulator and its build of the CLI; the GPU tests
run the product."""
import os
import shutil
import subprocess
import sys

import pytest

import oracle_lib

sys.path.insert(0, os.path.join(oracle_lib.ROOT, "oracle"))
import oracle_py as op  # noqa: E402
from bcalm_amd import api  # noqa: E402
from test_links import CASES  # noqa: E402

ROOT = oracle_lib.ROOT
FLIP = {"+": "-", "-": "+"}
SPLIT_CASES = [("pufferize_refs", 9, 5, 8), ("rand_a", 15, 918, 2072), ("rand_b", 31, 1031, 2126)]   # name, k, pieces, links


# ---------------------------------------------------------------- helpers
def _sim():
    import hostsim_lib
    return hostsim_lib.load()


def _sim_cli():
    _sim()
    return os.path.join(ROOT, "tests", "hostsim", "_build", "bcalm_hostsim")


@pytest.fixture(scope="module")
def tools():
    import __graft_entry__ as ge
    ge.build_host_tools()
    return os.path.join(ROOT, "bcalm_amd", "_build", "bcalm_tools")


def _built(lib, text, k, amin):
    """-> ([(seq, kc)], set digest, link set) of the graph built from `text`"""
    g = api.Graph(k, amin, lib=lib)
    try:
        g.push_text(text); g.run()
        ut = g.unitigs()
        dig = g.digest()["set_digest"]
        ls = _link_set(g.links())
    finally:
        g.close()
    return ut, dig, ls


def _link_set(per_unitig):
    got = set()
    for u, ls in enumerate(per_unitig):
        for fs, v, ts in ls:
            assert (u, fs, v, ts) not in got, "duplicate link"
            got.add((u, fs, v, ts))
    return got


def _raw_links(g):
    """(end_off[], link_to[]) exactly as cdbg_fetch_links returns them"""
    import ctypes as C
    g._ck(g.lib.cdbg_link(g._h))
    n, nl = C.c_uint64(), C.c_uint64()
    g._ck(g.lib.cdbg_num_unitigs(g._h, C.byref(n), None))
    g._ck(g.lib.cdbg_num_links(g._h, C.byref(nl)))
    off = (C.c_uint64 * (2 * n.value + 1))(); to = (C.c_uint32 * max(nl.value, 1))()
    g._ck(g.lib.cdbg_fetch_links(g._h, off, to))
    return list(off), list(to)[:nl.value]


def _check_loaded(lib, seqs, k, exp=None):
    """load `seqs` into a fresh graph: links == brute force, mirror property, ascending targets; -> the link set"""
    g = api.Graph(k, 1, lib=lib)
    try:
        g.load_unitigs(seqs)
        got = _link_set(g.links())
        off, to = _raw_links(g)
    finally:
        g.close()
    exp = op.links([s.upper() for s in seqs], k) if exp is None else exp
    assert got == exp, (sorted(got - exp)[:5], sorted(exp - got)[:5])
    for (u, fs, v, ts) in got:                               # mirror constraint, as tests/test_links.py::_check
        assert (v, FLIP[ts], u, FLIP[fs]) in got
    assert off[-1] == len(to) == len(exp)
    for e in range(len(off) - 1):                            # layout: every end's targets ascending
        run = to[off[e]:off[e + 1]]
        assert run == sorted(run)
    return got


def _split_pieces(lib, tools, name, k, tmp_path):
    """bcalm_tools split_unitigs on the references (input lines of length >= k) and the unitigs `lib` builds -> (split FASTA path, pieces)"""
    text = oracle_lib.read_input(name)
    refs = [l for l in text.split("\n") if len(l) >= k]
    ut, _, _ = _built(lib, text, k, 1)
    d = tmp_path / ("split_" + name); d.mkdir()
    (d / "refs.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(refs)))
    (d / "u.fa").write_text("".join(">%d LN:i:%d\n%s\n" % (i, len(s), s) for i, (s, _) in enumerate(ut)))
    r = subprocess.run([tools, "split_unitigs", "refs.fa", "u.fa", str(k)], cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = d / "u.fa.split.fa"
    lines = out.read_text().split("\n")
    pieces = [lines[i + 1] for i in range(0, len(lines) - 1, 2)]
    assert all(lines[i] == ">unitig%d" % (i // 2) for i in range(0, len(lines) - 1, 2))
    return out, pieces


def _parse_fa(path):
    """[(header line without '>', sequence)] of a one-line-per-sequence FASTA"""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    recs = []
    for i in range(0, len(lines) - 1, 2):
        assert lines[i].startswith(">")
        recs.append((lines[i][1:], lines[i + 1]))
    return recs


def _header_links(recs):
    out = set()
    for u, (h, _) in enumerate(recs):
        assert h.split(" ")[0] == str(u)
        for t in h.split(" "):
            if t.startswith("L:"):
                _, fs, v, ts = t.split(":")
                assert (u, fs, int(v), ts) not in out
                out.add((u, fs, int(v), ts))
    return out


def _run_cli(cli, args, cwd):
    return subprocess.run([cli] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def _reads_fasta(path, text):
    with open(path, "w") as f:
        for i, l in enumerate(x for x in text.split("\n") if x):
            f.write(">r%d\n%s\n" % (i, l))


# ---------------------------------------------------------------- shared test bodies (simulator and GPU)
def _round_trip(lib, name, k, amin):
    ut, _, _ = _built(lib, oracle_lib.read_input(name), k, amin)
    got = _check_loaded(lib, [s for s, _ in ut], k)
    if name in ("pufferize_refs", "rand_a"):
        assert got


def _tripled(lib, name, k, amin, first=None):
    ut, _, _ = _built(lib, oracle_lib.read_input(name), k, amin)
    seqs = [s for s, _ in ut][:first] * 3
    exp = op.links(seqs, k)
    per_end = {}
    for (u, fs, v, ts) in exp:
        per_end[(u, fs)] = per_end.get((u, fs), 0) + 1
    assert max(per_end.values()) >= 9                          # more than the six ends a join of one graph's unitigs keeps
    _check_loaded(lib, seqs, k, exp)


# Runs longer than a wave (64 ends), which the ordering and the fill hand to whole waves.  At k = 5 every copy of ACGTACGTACGTA begins
# with the palindromic junction ACGT, so the left ends of all copies link to each other (one run, linked to itself); AAAAAAA at k = 4
# puts all right ends on AAA+ and all left ends on AAA-: two runs linked to each other.  The mixed set keeps 70 copies (every other one in
# lower case) among sequences of degree 1 -- GGTTGACGT joins the long run, CGTATTGCC follows every copy, GGCATTCAGG -> CAGGTTTAC -- so that
# one wave holds ends of long and of short runs, and ends of short runs with long targets.
_COPY = "ACGTACGTACGTA"
_MIXED = (["GGCATTCAGG", "GGTTGACGT"] + [_COPY, _COPY.lower()] * 17 + ["CAGGTTTAC", "CGTATTGCC"] + [_COPY.lower(), _COPY] * 18)
LONG_RUNS = {"palindromic_150": ([_COPY] * 150, 5, 150 * 150), "two_runs_200": (["AAAAAAA"] * 200, 4, 2 * 200 * 200), "mixed_70": (_MIXED, 5, None)}


def _long_runs(lib, case):
    seqs, k, n_links = LONG_RUNS[case]
    exp = op.links([s.upper() for s in seqs], k)
    deg = {}
    for (u, fs, v, ts) in exp:
        deg[(u, fs)] = deg.get((u, fs), 0) + 1
    assert len(exp) > 0 and max(deg.values()) > 64             # (of the input: the brute force says a run is longer than a wave)
    if n_links is not None:
        assert len(exp) == n_links
    else:                                                      # ends 0 .. 63 share a wave: degree 1 and degree > 64 among them
        first = [d for (u, _), d in deg.items() if u < 32]
        assert min(first) == 1 and max(first) > 64
    got = _check_loaded(lib, seqs, k, exp)
    assert len(got) > 0


def _deterministic(lib, name, k, amin):
    ut, _, _ = _built(lib, oracle_lib.read_input(name), k, amin)
    seqs = [s for s, _ in ut] * 2
    res = []
    for _ in range(2):
        g = api.Graph(k, 1, lib=lib)
        try:
            g.load_unitigs(seqs)
            res.append(_raw_links(g))
        finally:
            g.close()
    assert res[0] == res[1]
    off, to = res[0]
    for e in range(len(off) - 1):
        assert to[off[e]:off[e + 1]] == sorted(to[off[e]:off[e + 1]])


def _cli_own_output(cli, tmp_path, reads_text, k, amin):
    """test 7: -redo-links on the CLI's own output keeps every record but for the order of its L: tokens, and is idempotent"""
    _reads_fasta(tmp_path / "f.fa", reads_text)
    r = _run_cli(cli, ["-in", "f.fa", "-kmer-size", str(k), "-abundance-min", str(amin)], tmp_path)
    assert r.returncode == 0, r.stdout
    fa = tmp_path / "f.unitigs.fa"
    before = _parse_fa(fa)
    r = _run_cli(cli, ["-in", "f.h5", "-kmer-size", str(k), "-skip-bcalm", "-skip-bglue", "-redo-links"], tmp_path)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1] == "unitigs written to f.unitigs.fa"
    first = fa.read_bytes()
    after = _parse_fa(fa)
    assert len(before) == len(after) > 0
    for (hb, sb), (ha, sa) in zip(before, after):
        assert sb == sa
        tb, ta = hb.split(" "), ha.split(" ")
        assert [t for t in tb if not t.startswith("L:")] == [t for t in ta if not t.startswith("L:")]
        assert sorted(t for t in tb if t.startswith("L:")) == sorted(t for t in ta if t.startswith("L:"))
        assert len(tb) == len(ta)
    r = _run_cli(cli, ["-in", "f.unitigs.fa", "-kmer-size", str(k), "-redo-links"], tmp_path)
    assert r.returncode == 0, r.stdout
    assert fa.read_bytes() == first
    assert sorted(os.listdir(tmp_path)) == ["f.fa", "f.unitigs.fa"]


def _cli_split_file(cli, tools, split_fa, pieces, k, tmp_path, n_links):
    """test 8: a split file with >unitigN headers relinked, with -gfa"""
    d = tmp_path / "cli_split"; d.mkdir()
    shutil.copy(split_fa, d / "x.unitigs.fa")
    r = _run_cli(cli, ["-in", "x.unitigs.fa", "-kmer-size", str(k), "-redo-links", "-gfa"], d)
    assert r.returncode == 0, r.stdout
    recs = _parse_fa(d / "x.unitigs.fa")
    assert [s for _, s in recs] == pieces
    exp = op.links(pieces, k)
    assert len(exp) == n_links
    assert _header_links(recs) == exp
    for h, _ in recs:
        assert h.endswith(" ")                                 # the writer's trailing blank, as in a normal run
    r = subprocess.run([tools, "convertToGFA", "x.unitigs.fa", "conv.gfa", str(k)], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (d / "conv.gfa").read_bytes() == (d / "x.unitigs.gfa").read_bytes()
    assert sorted(os.listdir(d)) == ["conv.gfa", "x.unitigs.fa", "x.unitigs.gfa"]


# ---------------------------------------------------------------- CPU: the library on the simulator
@pytest.mark.parametrize("name,k,amin", CASES)
def test_round_trip_sim(name, k, amin):
    """1: the unitigs of a built graph, loaded into a fresh one, link as the brute force says"""
    _round_trip(_sim(), name, k, amin)


@pytest.mark.parametrize("name,k,n_pieces,n_links", SPLIT_CASES)
def test_split_pieces_sim(tools, tmp_path, name, k, n_pieces, n_links):
    """2: pieces cut by bcalm_tools split_unitigs"""
    _, pieces = _split_pieces(_sim(), tools, name, k, tmp_path)
    assert len(pieces) == n_pieces
    assert len(_check_loaded(_sim(), pieces, k)) == n_links


def test_no_degree_bound_rand_a_sim():
    """3: nine ends on one oriented junction"""
    _tripled(_sim(), "rand_a", 15, 2)


def test_no_degree_bound_rand_b_sim():
    _tripled(_sim(), "rand_b", 31, 2, first=300)


def test_no_degree_bound_one_sequence_forty_times_sim():
    """3: forty copies of one sequence whose ends overlap each other (ACGTACGT...: every copy follows every copy)"""
    seqs = ["ACGTACGTACGTA"] * 40
    got = _check_loaded(_sim(), seqs, 5)
    assert len(got) >= 40 * 40


@pytest.mark.parametrize("case", sorted(LONG_RUNS))
def test_long_runs_sim(case):
    """runs longer than a wave: the wave-cooperative ordering and fill"""
    _long_runs(_sim(), case)


@pytest.mark.parametrize("name,k,amin", [("rand_a", 15, 2), ("even_k8", 8, 1)])
def test_deterministic_sim(name, k, amin):
    """4: two loads of one set give the same end_off / link_to arrays, every end's targets ascending"""
    _deterministic(_sim(), name, k, amin)


def test_adopted_set_sim():
    """5: the loaded context describes the set it was given"""
    lib = _sim()
    ut, dig, _ = _built(lib, oracle_lib.read_input("rand_b"), 31, 2)
    seqs = [s if i % 2 else s.lower() for i, (s, _) in enumerate(ut)]
    kcs = [kc for _, kc in ut]
    g = api.Graph(31, 2, lib=lib)
    try:
        g.load_unitigs(seqs, kc=kcs)
        assert g.unitigs() == ut
        assert g.unitigs(3, 4) == ut[3:7]
        packed, off, ln, kc = g.unitigs_packed()
        assert kc == kcs and ln == [len(s) for s, _ in ut]
        for (s, _), o, n in zip(ut, off, ln):
            assert "".join("ACGT"[(packed[(o + j) >> 2] >> (2 * ((o + j) & 3))) & 3] for j in range(n)) == s
        d = g.digest()
        assert d["set_digest"] == dig
        assert d["solid_count_sum"] == 2 ** 64 - 1
        assert d["kc_sum"] == sum(kcs) and d["kmers_in_unitigs"] == sum(len(s) - 30 for s, _ in ut)
        st = g.stats()
        assert st["n_unitigs"] == len(ut) and st["unitig_bases"] == sum(len(s) for s, _ in ut)
        g.links()
        assert g.unitig_id_base() == (0, len(ut))
    finally:
        g.close()
    g = api.Graph(31, 2, lib=lib)                              # no KC given: all 0
    try:
        g.load_unitigs([s for s, _ in ut[:5]])
        assert g.unitigs() == [(s, 0) for s, _ in ut[:5]]
    finally:
        g.close()


def test_refusals_sim():
    """6: what a loaded context, or a context that is not fresh, must refuse -- and reset() makes it a builder again"""
    lib = _sim()
    E_PARAM, E_STATE = -1, -4
    ok = ["ACGTTGCATGC", "TTGCATGCAAA"]

    def refused(code, fn):
        with pytest.raises(api.CdbgError) as ei:
            fn()
        assert ei.value.code == code, str(ei.value)
        return str(ei.value)

    g = api.Graph(7, 1, lib=lib)
    try:
        assert "unitig 1" in refused(E_PARAM, lambda: g.load_unitigs(["ACGTTGCATGC", "ACGTAC"]))       # shorter than k
        assert "unitig 1" in refused(E_PARAM, lambda: g.load_unitigs(["ACGTTGCATGC", "TTGCANGCAAA"]))  # a byte outside ACGTacgt
        g.load_unitigs(ok)                                                                            # (the failed loads left it fresh)
        for fn in (g.count, g.compact, g.glue, g.run, g.verify, g.verify_edges, g.solid_kmers, g.unitig_abundances,
                   lambda: g.verify_unitigs(ok), lambda: g.push_text("ACGTACGTAC"), lambda: g.push_reads(["ACGTACGTAC"]),
                   lambda: g.stage_text("ACGTACGTAC\n"), lambda: g.generate_reads(10, 50, 3), lambda: g.expect_input(100),
                   lambda: g.load_unitigs(ok)):
            assert "loaded" in refused(E_STATE, fn)
        assert _link_set(g.links()) == op.links(ok, 7)
        g.reset()
        refused(E_STATE, g.links)
        text = oracle_lib.read_input("pufferize_refs")
        g.push_text(text); g.run()
        got = oracle_lib.canonical_set(oracle_lib.load(), g.unitigs(), 7)
    finally:
        g.close()
    assert got == oracle_lib.load().run(text, 7, 1)["unitigs"]
    g = api.Graph(7, 1, lib=lib)
    try:
        g.push_text("ACGTACGTAC")
        refused(E_STATE, lambda: g.load_unitigs(ok))                                                  # text was pushed
    finally:
        g.close()


# ---------------------------------------------------------------- CPU: the command line (simulator build of bcalm)
def test_cli_own_output_sim(tmp_path):
    """7"""
    _cli_own_output(_sim_cli(), tmp_path, oracle_lib.read_input("rand_a"), 15, 1)


@pytest.mark.parametrize("name,k,n_pieces,n_links", SPLIT_CASES)
def test_cli_split_file_sim(tools, tmp_path, name, k, n_pieces, n_links):
    """8"""
    split_fa, pieces = _split_pieces(_sim(), tools, name, k, tmp_path)
    _cli_split_file(_sim_cli(), tools, split_fa, pieces, k, tmp_path, n_links)


def test_cli_many_slices_keep_record_order_sim(tools, tmp_path):
    """the file parsed in many slices by several threads gives the bytes of the one-slice run"""
    split_fa, pieces = _split_pieces(_sim(), tools, "rand_a", 15, tmp_path)
    outs = []
    for env in ({}, {"BCALM_SLICE_BYTES": "300"}):
        d = tmp_path / ("slices%d" % len(outs)); d.mkdir()
        wrapped = "".join(">unitig%d\n%s\n" % (i, "\n".join(p[j:j + 20] for j in range(0, len(p), 20))) for i, p in enumerate(pieces))
        (d / "x.unitigs.fa").write_text(wrapped)
        r = subprocess.run([_sim_cli(), "-in", "x.unitigs.fa", "-kmer-size", "15", "-redo-links", "-nb-cores", "4"], cwd=d, capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout
        outs.append((d / "x.unitigs.fa").read_bytes())
    assert outs[0] == outs[1]
    recs = _parse_fa(tmp_path / "slices1" / "x.unitigs.fa")
    assert [s for _, s in recs] == pieces and _header_links(recs) == op.links(pieces, 15)


def test_cli_stale_links_and_kept_tokens_sim(tmp_path):
    """9: wrong L: tokens go, every other header token stays verbatim and in order; wrapped, lower-case sequence lines are joined"""
    seqs = ["ACGTTGCATGC", "TTGCATGCAAA", "GGGGGGGGGGG"]
    k = 7
    (tmp_path / "s.unitigs.fa").write_text(
        ">7 LN:i:11 KC:i:22 km:f:4.4 L:+:2:- L:-:0:+ \n" + seqs[0] + "\n"
        ">zz LN:i:11 ab:Z:3 4 5 6 7 L:+:0:+\n" + seqs[1][:5].lower() + "\n" + seqs[1][5:] + "\n"
        ">2\n" + seqs[2] + "\n")
    r = _run_cli(_sim_cli(), ["-in", "whatever.h5", "-out", "s", "-kmer-size", str(k), "-skip-bcalm", "-skip-bglue", "-redo-links",
                              "-abundance-min", "3", "-nb-cores", "2", "-max-memory", "100"], tmp_path)
    assert r.returncode == 0, r.stdout
    recs = _parse_fa(tmp_path / "s.unitigs.fa")
    assert [s for _, s in recs] == seqs
    exp = op.links(seqs, k)
    assert _header_links(recs) == exp and exp
    assert recs[0][0] == "0 LN:i:11 KC:i:22 km:f:4.4 " + " ".join(t for t in recs[0][0].split(" ") if t.startswith("L:")) + " "
    assert recs[1][0].startswith("1 LN:i:11 ab:Z:3 4 5 6 7 ")
    assert recs[2][0].startswith("2 ")
    assert "L:+:2:-" not in recs[0][0]


def test_cli_errors_sim(tmp_path):
    """10: usage errors and bad files end with EXCEPTION: and status 1, and leave the file as it was"""
    cli = _sim_cli()
    good = ">0 LN:i:11\nACGTTGCATGC\n>1 LN:i:11\nTTGCATGCAAA\n"
    short = ">0 LN:i:11\nACGTTGCATGC\n>1 LN:i:4\nTTGC\n"
    badbase = ">0 LN:i:11\nACGTTGCATGC\n>1 LN:i:11\nTTGCANGCAAA\n"
    (tmp_path / "g.unitigs.fa").write_text(good)
    (tmp_path / "sh.unitigs.fa").write_text(short)
    (tmp_path / "bb.unitigs.fa").write_text(badbase)

    def fails(args, word=None):
        r = _run_cli(cli, args, tmp_path)
        assert r.returncode == 1 and "EXCEPTION:" in r.stdout, (args, r.stdout)
        if word:
            assert word in r.stdout, r.stdout
    fails(["-in", "g.unitigs.fa", "-kmer-size", "7", "-skip-bcalm"], "only supported together with -redo-links")
    fails(["-in", "g.unitigs.fa", "-kmer-size", "7", "-skip-bglue"], "only supported together with -redo-links")
    fails(["-in", "g.unitigs.fa", "-kmer-size", "7", "-nb-gpus", "2", "-redo-links"], "-nb-gpus")
    fails(["-in", "nothing.h5", "-kmer-size", "7", "-redo-links"], "nothing.unitigs.fa")
    fails(["-in", "sh.unitigs.fa", "-kmer-size", "7", "-redo-links"], "record 1")
    fails(["-in", "bb.unitigs.fa", "-kmer-size", "7", "-redo-links", "-gfa"], "record 1")
    assert (tmp_path / "g.unitigs.fa").read_text() == good
    assert (tmp_path / "sh.unitigs.fa").read_text() == short
    assert (tmp_path / "bb.unitigs.fa").read_text() == badbase
    assert sorted(os.listdir(tmp_path)) == ["bb.unitigs.fa", "g.unitigs.fa", "sh.unitigs.fa"]
    r = _run_cli(cli, ["-in", "g.unitigs.fa", "-kmer-size", "7", "-redo-links"], tmp_path)
    assert r.returncode == 0 and _header_links(_parse_fa(tmp_path / "g.unitigs.fa")) == op.links(["ACGTTGCATGC", "TTGCATGCAAA"], 7)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,amin", CASES)
def test_round_trip_gpu(hip, name, k, amin):
    """11: tests 1, 3 and 4 on the device for every case"""
    _round_trip(hip, name, k, amin)
    ut, _, _ = _built(hip, oracle_lib.read_input(name), k, amin)
    seqs = [s for s, _ in ut][:120] * 3
    _check_loaded(hip, seqs, k)
    _deterministic(hip, name, k, amin)


@pytest.mark.gpu
def test_no_degree_bound_gpu(hip):
    """11: the degree-9 sets of test 3 and forty copies of one sequence"""
    _tripled(hip, "rand_a", 15, 2)
    _tripled(hip, "rand_b", 31, 2, first=300)
    assert len(_check_loaded(hip, ["ACGTACGTACGTA"] * 40, 5)) >= 1600


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LONG_RUNS))
def test_long_runs_gpu(hip, case):
    """11: runs longer than a wave on the device"""
    _long_runs(hip, case)


@pytest.mark.gpu
def test_synthetic_reads_gpu(hip, oracle):
    """12: 3000 synthetic reads, k = 31, abundance-min 2"""
    ut, dig, built_links = _built(hip, oracle.synth_reads(3000, 150, 3).decode(), 31, 2)
    got = _check_loaded(hip, [s for s, _ in ut], 31)
    assert got == built_links


@pytest.mark.gpu
def test_one_million_reads_gpu(hip, oracle_1m):
    """13: beyond the brute force -- the loaded graph's links against the built graph's own (the capped join, pinned elsewhere)"""
    text, _ = oracle_1m
    g = api.Graph(31, 2, lib=hip)
    try:
        g.push_text(text); g.run()
        ut = g.unitigs(); dig = g.digest()["set_digest"]
        off_b, to_b = _raw_links(g)
    finally:
        g.close()
    g = api.Graph(31, 2, lib=hip)
    try:
        g.load_unitigs([s for s, _ in ut], kc=[kc for _, kc in ut])
        assert g.digest()["set_digest"] == dig
        off_l, to_l = _raw_links(g)
    finally:
        g.close()
    assert off_b == off_l and len(to_b) == len(to_l) > 0
    for e in range(len(off_b) - 1):
        a = to_l[off_l[e]:off_l[e + 1]]
        assert a == sorted(to_b[off_b[e]:off_b[e + 1]])


@pytest.mark.gpu
def test_cli_gpu(hip, oracle, tools, tmp_path):
    """14: the real bcalm binary -- test 7 on 20 000 synthetic reads, test 8 on rand_b"""
    cli = os.path.join(ROOT, "bcalm_amd", "_build", "bcalm")
    assert os.path.exists(cli)
    own = tmp_path / "own"; own.mkdir()
    _cli_own_output(cli, own, oracle.synth_reads(20000, 150, 3).decode(), 31, 2)
    split_fa, pieces = _split_pieces(hip, tools, "rand_b", 31, tmp_path)
    _cli_split_file(cli, tools, split_fa, pieces, 31, tmp_path, 2126)
