"""No result may depend on what device memory held before (CPU suite, through the simulator).

  * poisoned allocations: every block the simulator's allocator hands out (CDBG_SIM_POISON) and every block the library takes fresh
    or from its pool (CDBG_POISON_ALLOC) filled with 0xFF -- the all-ones EMPTY / sentinel words and full cursors -- or with 0xA5,
    plain garbage; fresh pages of the simulator (and of the driver, in practice) are zero and would hide a kernel that reads a
    counter, cursor, flag or table slot it never wrote;
  * repeated steps: reset() + run() three times on one context, the way bench.py times its steps, with the state that survives
    reset() on purpose (the learned partition count, the deferred-placement switch, every buffer);
  * a dirty pool: a context runs on the buffers that another context of the same shape has just handed back;
  * Graph.verify(): only a capacity failure of the edge pass becomes edges = None.

Every result is compared with the oracle -- (k-mer, count) set, canonical unitig set with KC, statistics, device digest, device
verify with edges, links and abundance vectors where the case asks for them -- never with another run of the library."""
import os
import random
import re
import subprocess
import sys

import pytest

import hostsim_lib
import oracle_lib
from bcalm_amd import api
from parity import kmer_set_sums, set_digest

sys.path.insert(0, os.path.join(oracle_lib.ROOT, "oracle"))
import oracle_py as op  # noqa: E402

POISONS = ["0xFF", "0xA5"]
COMP = str.maketrans("ACGT", "TGCA")
PLAN = ("count_slices", "n_deferred_records", "n_records", "log2_partitions", "n_multipass_partitions", "n_big_partitions")


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(params=POISONS)
def poison(request, monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", request.param)
    monkeypatch.setenv("CDBG_POISON_ALLOC", request.param)
    return request.param


def expected(oracle, text, k, amin):
    exp = oracle.run(text, k, amin, want_solid=True)
    exp["kmer_sums"] = kmer_set_sums([s for s, _ in exp["solid"]], k)
    exp["count_sum"] = sum(c for _, c in exp["solid"])
    return exp


def check_graph(oracle, g, exp, k, solid, links=False, abundances=False):
    """everything a finished graph reports, against the oracle -> stats"""
    st = g.stats()
    es = exp["stats"]
    assert (st["n_occurrences"], st["n_distinct"], st["n_solid"], st["n_unitigs"]) == (es["occurrences"], es["distinct"], es["solid"], es["unitigs"]), (st, es)
    assert solid == exp["solid"], "(k-mer, count) set differs"
    ut = g.unitigs()
    canon = oracle_lib.canonical_set(oracle, ut, k)
    if canon != exp["unitigs"]:
        raise AssertionError(f"unitig sets differ: only got {sorted(set(canon) - set(exp['unitigs']))[:3]}, only expected {sorted(set(exp['unitigs']) - set(canon))[:3]}")
    d = g.digest()
    # (the formula on the unitigs fetched -- the oracle's set, as checked above; a unitig that closes on itself, ACACACACACAC at k = 11,
    #  may be emitted in another rotation than the oracle's canonical one, and the digest is not rotation-invariant)
    assert d["set_digest"] == set_digest(ut), d
    assert d["kc_sum"] == d["solid_count_sum"] == exp["count_sum"], d
    assert d["kmers_in_unitigs"] == es["solid"], d
    v = g.verify()
    assert v["unitig_kmers"] == v["solid_kmers"] == exp["kmer_sums"], v
    assert v["mergeable_ends"] == 0 and v["edges"] is not None and "edges_error" not in v and api.Graph.edges_conserved(v), v
    if links:                                             # the brute force of tests/test_links.py over all pairs of unitig ends
        got = {(u, fs, v_, ts) for u, ls in enumerate(g.links()) for fs, v_, ts in ls}
        want = op.links([s for s, _ in ut], k)
        assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    if abundances:                                        # -all-abundance-counts: the oracle's count of every k-mer, in the emitted orientation
        counts = dict(exp["solid"])
        for (s, kc), a in zip(ut, g.unitig_abundances()):
            want = [counts[min(s[i:i + k], s[i:i + k].translate(COMP)[::-1])] for i in range(len(s) - k + 1)]
            assert a == want and sum(a) == kc
    return st


def push(g, text, ingest):
    if ingest == "stage":
        g.stage_text(text)
    elif ingest == "expect":                              # announced input: the scan runs on the tiles that have landed while the rest arrives
        b = text.encode() if isinstance(text, str) else text
        reads = b.split(b"\n")
        g.expect_input(len(b))
        for i in range(0, len(reads), 97):
            chunk = b"\n".join(reads[i:i + 97])
            if chunk:
                g.push_text(chunk)
    else:
        g.push_text(text)


def step(g):
    """one step as cdbg_run takes it, with the stage-1 surface fetched between count and compaction"""
    g.count()
    solid = g.solid_kmers()
    g.compact(); g.glue()
    return solid


def run_case(oracle, lib, text, k, amin, ingest="push", links=False, abundances=False, **kw):
    exp = expected(oracle, text, k, amin)
    g = api.Graph(k, amin, lib=lib, all_abundance_counts=abundances, **kw)
    try:
        push(g, text, ingest)
        return check_graph(oracle, g, exp, k, step(g), links, abundances)
    finally:
        g.close()


# ---- inputs ----
def _reads_of(genome, n, rng, lo, hi, err=0.0):
    out = []
    for _ in range(n):
        L = rng.randrange(lo, hi); s = rng.randrange(0, len(genome) - L)
        r = genome[s:s + L]
        if rng.random() < 0.5:
            r = r.translate(COMP)[::-1]
        out.append("".join((rng.choice("ACGT") if rng.random() < err else c) for c in r))
    return "\n".join(out) + "\n"


def _wide_text(seed):
    """reads of both strands with errors (tests/test_hostsim_pipeline.py test_wide_kmers_beyond_the_default_span_list)"""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(5000))
    return _reads_of(g, 40, rng, 200, 900, 0.004)


def _tier_text(k, glen):
    """ONE partition whose distinct k-mers overflow the one-pass count table (test_count_tiers)"""
    rng = random.Random(glen + k)
    g = "".join(rng.choice("ACGT") for _ in range(glen))
    return g + "\n" + g[100:100 + 2 * k] + "\n"


def _sift_text(k):
    """mostly once-seen k-mers of four words in one partition under abundance-min 2: the sifting tier (test_count_sift_tier, "sifted")"""
    rng = random.Random(k * 7 + len("sifted"))
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    g = rnd(250 + k)
    reads = [g, g, g[5:], g[::-1].translate(COMP)] + [rnd(k + 99) for _ in range(26)]
    reads.append(g[:k + 10] + rnd(1) + g[k + 11:2 * k + 30])
    return "\n".join(reads) + "\n"


def _split_text(k, glen):
    """buckets no LDS compaction tier takes (test_second_level_bucket_split)"""
    rng = random.Random(glen + k)
    g = "".join(rng.choice("ACGT") for _ in range(glen))
    low = "".join(rng.choice("AT") for _ in range(glen // 3))
    return "\n".join([g, low, g[300:300 + 3 * k][::-1].translate(COMP) + "A" * (2 * k) + g[700:700 + 2 * k], g[100:100 + 2 * k]]) + "\n"


def _golden(name):
    return lambda oracle: oracle_lib.read_input(name)


def _synth(n, L, cfg, extra=None):
    return lambda oracle: (oracle_lib.read_input(extra) if extra else "") + oracle.synth_reads(n, L, cfg).decode()


STREAM_ENV = {"CDBG_STAGE_BYTES": "16384", "CDBG_STREAM_MIN_BYTES": "40000", "CDBG_STREAM_BATCH_TILES": "4", "CDBG_PREWARM_MIN_BYTES": "1"}
# id: (text(oracle), k, amin, Graph keywords, environment, ingest, links, abundances) -- a sample of every family of tests/test_hostsim_pipeline.py
CASES = {
    "golden_even_k8": (_golden("even_k8"), 8, 1, dict(log2_partitions=3), {}, "push", True, True),
    "golden_palin4": (_golden("palin4"), 4, 1, dict(log2_partitions=0), {}, "push", True, False),
    "golden_cycles": (_golden("circ_test3"), 7, 1, dict(log2_partitions=3), {}, "push", True, False),
    "golden_even_k64": (_golden("even_k64"), 64, 1, dict(log2_partitions=5), {}, "push", True, False),
    "w1": (_golden("rand_b"), 31, 2, dict(log2_partitions=5), {}, "push", False, True),
    "w2": (_golden("rand_w2"), 55, 2, dict(log2_partitions=4), {}, "push", True, False),
    "w4": (_golden("rand_w4"), 127, 1, dict(log2_partitions=2), {}, "push", False, False),
    "w8": (lambda oracle: _wide_text(255), 255, 1, dict(log2_partitions=4, minimizer_size=16), {}, "push", False, False),
    "scan_exact": (_golden("rand_a"), 15, 2, dict(log2_partitions=4), {"CDBG_SCAN_MODE": "exact"}, "push", False, False),
    "scan_capped_spills": (_golden("minitip"), 21, 1, dict(log2_partitions=4), {"CDBG_SCAN_MODE": "capped", "CDBG_PART_CAP": "1"}, "push", False, False),
    "scan_var_spills": (_synth(1500, 150, 3 | 0x100), 21, 2, dict(log2_partitions=6), {"CDBG_SCAN_MODE": "var", "CDBG_PART_CAP": "1", "CDBG_VAR_SCALE": "0.02"}, "push", False, False),
    "deferred_spills": (_synth(60, 150, 3, "rand_b"), 31, 2, dict(log2_partitions=10),
                        {"CDBG_SCAN_MODE": "capped", "CDBG_DEFER_SLICES": "4", "CDBG_PART_CAP": "1", "CDBG_DEFER_CAP": "3"}, "push", False, False),
    "count_second_tier": (lambda oracle: _tier_text(31, 3800), 31, 1, dict(log2_partitions=0), {}, "push", False, False),
    "count_multipass": (lambda oracle: _tier_text(55, 6000), 55, 1, dict(log2_partitions=0), {"CDBG_MAX_PASSES": "1"}, "push", False, False),
    "count_sift": (lambda oracle: _sift_text(127), 127, 2, dict(log2_partitions=0), {}, "push", False, False),
    "bucket_split": (lambda oracle: _split_text(31, 9000), 31, 1, dict(log2_partitions=1), {}, "push", False, False),
    "bucket_no_split": (lambda oracle: _split_text(31, 9000), 31, 1, dict(log2_partitions=1), {"CDBG_NO_SPLIT": "1"}, "push", False, False),
    "glue_log": (_golden("rand_a"), 15, 2, dict(log2_partitions=5), {"CDBG_GLUE_LOG": "1"}, "push", True, False),
    "glue_table": (_golden("rand_a"), 15, 2, dict(log2_partitions=5), {"CDBG_GLUE_TABLE": "1"}, "push", False, False),
    "glue_overflow": (_synth(400, 150, 3, "rand_a"), 15, 2, dict(log2_partitions=5), {"CDBG_JOIN_LOG_JB": "0"}, "push", False, False),
    "glue_rank": (_golden("circ_test3"), 7, 1, dict(log2_partitions=5), {"CDBG_GLUE_RANK": "1"}, "push", True, False),
    "glue_walkmax": (_golden("rand_a"), 15, 2, dict(log2_partitions=5), {"CDBG_WALK_MAX": "0"}, "push", False, False),
    "ingest_stage_text": (_synth(600, 150, 3), 31, 2, dict(log2_partitions=4), {"CDBG_STAGE_BYTES": "16384"}, "stage", False, False),
    "ingest_expect_input": (_synth(3000, 150, 3), 31, 2, dict(log2_partitions=6), STREAM_ENV, "expect", False, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_poisoned_parity(oracle, sim, poison, case, monkeypatch):
    """every new block (simulator allocator and library pool alike) full of 0xFF / 0xA5: the same result as the oracle on every path"""
    text, k, amin, kw, env, ingest, links, abundances = CASES[case]
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    st = run_case(oracle, sim, text(oracle), k, amin, ingest=ingest, links=links, abundances=abundances, **kw)
    # (the forced path was taken)
    if case == "deferred_spills":
        assert st["count_slices"] == 4 and st["n_deferred_records"] > 0, st
    elif case == "count_second_tier":
        assert st["n_multipass_partitions"] == 0, st
    elif case in ("count_multipass", "count_sift"):
        assert st["n_multipass_partitions"] == (1 if case == "count_multipass" else 0), st
    elif case.startswith("bucket_"):
        assert (st["n_split_buckets"] >= 1) == (case == "bucket_split"), st
    elif case == "ingest_expect_input":
        assert st["n_tiles_overlapped"] > 0, st


def _parse_cli_fa(path):
    lines = open(path).read().split("\n")
    out = []
    for i in range(0, len(lines) - 1, 2):
        m = re.match(r">\d+ LN:i:(\d+) KC:i:(\d+) ", lines[i])
        assert m and int(m.group(1)) == len(lines[i + 1]), lines[i]
        out.append((lines[i + 1], int(m.group(2))))
    return out


def test_poisoned_cli(oracle, sim, poison, tmp_path):
    """the simulator build of the bcalm CLI, file to file, with poisoned allocations (the variables reach the child process)"""
    exe = os.path.join(oracle_lib.ROOT, "tests", "hostsim", "_build", "bcalm_hostsim")
    text = oracle.synth_reads(500, 150, 3 | 0x100).decode()
    (tmp_path / "reads.fa").write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(x for x in text.split("\n") if x)))
    for inp, name, k, amin, ref in ((os.path.join(oracle_lib.ROOT, "tests", "golden", "inputs", "minitip.fa"), "minitip", 21, 1, oracle_lib.read_input("minitip")),
                                    (str(tmp_path / "reads.fa"), "reads", 31, 2, text)):
        r = subprocess.run([exe, "-in", inp, "-kmer-size", str(k), "-abundance-min", str(amin)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        got = oracle_lib.canonical_set(oracle, _parse_cli_fa(tmp_path / (name + ".unitigs.fa")), k)
        assert got == oracle.run(ref, k, amin)["unitigs"]


# ---- repeated steps ----
def _recount_text(seed):
    """one copy of a random genome at abundance-min 1: the partition count chosen for the count table leaves thousands of solid k-mers
    per compaction bucket, and cdbg_count counts again with more partitions -- the learned count (log_np_override) survives reset()"""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(20000))
    return g + "\n" + g[5000:5300] + "\n"


STEP_CASES = {
    # (text(oracle), k, amin, Graph keywords, environment)
    "learned_partition_count": (lambda oracle: _recount_text(11), 31, 1, {}, {}),
    # deferred placement whose placement kernel spills more than the spill list holds (79 K records into regions of one record; the scan places
    # 2/16 of the partitions and spills less than the list's 64 K, k_place the other 14/16).  Whichever check sees the overflow first -- the one
    # behind the scan (the simulator's k_place has run by then) or the one behind the first count tier, which runs the step again with deferral
    # off (allow_defer, count_impl in host_count.h) -- the step ends in the exact layout, and steps 2 and 3 must take the same path
    "deferred_spill_overflow": (_synth(560, 150, 3), 11, 2, dict(log2_partitions=10),
                                {"CDBG_SCAN_MODE": "capped", "CDBG_DEFER_SLICES": "2,14", "CDBG_PART_CAP": "1"}),
    "var_overflow_regions": (_synth(1500, 150, 3 | 0x100), 31, 2, dict(log2_partitions=6), {"CDBG_SCAN_MODE": "var", "CDBG_PART_CAP": "8"}),
    "multipass_count": (lambda oracle: _tier_text(31, 11000), 31, 1, dict(log2_partitions=0), {}),
}


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_repeated_steps(oracle, sim, case, monkeypatch):
    """three reset() + run() steps on one context, each against the oracle; steps 2 and 3 (the first may learn) report the same plan"""
    text, k, amin, kw, env = STEP_CASES[case]
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    text = text(oracle)
    exp = expected(oracle, text, k, amin)
    g = api.Graph(k, amin, lib=sim, **kw)
    plans = []
    try:
        g.push_text(text)
        for i in range(3):
            if i:
                g.reset()
            st = check_graph(oracle, g, exp, k, step(g))
            plans.append({x: st[x] for x in PLAN})
    finally:
        g.close()
    assert plans[1] == plans[2], plans
    if case == "learned_partition_count":
        assert plans[0]["log2_partitions"] == plans[1]["log2_partitions"] >= 6, plans
    elif case == "deferred_spill_overflow":               # (the count that was kept placed every record itself; without the tiny regions the same input is deferred)
        assert all(p["count_slices"] == 1 and p["n_deferred_records"] == 0 for p in plans), plans
        monkeypatch.delenv("CDBG_PART_CAP")
        g = api.Graph(k, amin, lib=sim, **kw)
        try:
            g.push_text(text); g.count()
            assert g.stats()["count_slices"] == 2 and g.stats()["n_deferred_records"] > 0, g.stats()
        finally:
            g.close()
    elif case == "multipass_count":
        assert all(p["n_multipass_partitions"] == 1 for p in plans), plans


# ---- dirty pool ----
def _hostile(oracle):
    return dict(text=oracle.synth_reads(400, 150, 3 | 0x100).decode(), amin=1, abundances=True, links=True)


def _uniform(oracle):
    return dict(text=oracle.synth_reads(150, 150, 3).decode(), amin=2, abundances=False, links=False)


@pytest.mark.parametrize("order", ["hostile_then_uniform", "uniform_then_hostile", "released_between"])
def test_dirty_pool_handover(oracle, sim, order):
    """context A runs and is destroyed -- its buffers go to the process's pool -- then context B with the same k and partition count runs
    on them; both against the oracle.  released_between: cdbg_release_cached() between the two (the control)"""
    a, b = (_uniform(oracle), _hostile(oracle)) if order == "uniform_then_hostile" else (_hostile(oracle), _uniform(oracle))
    sim.cdbg_release_cached()
    for i, c in enumerate((a, b)):
        if i and order == "released_between":
            sim.cdbg_release_cached()
        run_case(oracle, sim, c["text"], 31, c["amin"], links=c["links"], abundances=c["abundances"], log2_partitions=6)


# ---- Graph.verify() ----
class _EdgePassFails:
    """the simulator library, except that cdbg_verify_edges answers `code`"""
    def __init__(self, lib, code):
        self._lib, self._code = lib, code

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def cdbg_verify_edges(self, h, out):
        return self._code

    def cdbg_last_error(self):
        return b"edge pass failed (stub)"


@pytest.mark.parametrize("code", [api.E_INTERNAL, api.E_NOMEM])
def test_verify_reports_only_a_capacity_failure_as_missing_edges(sim, code):
    """CDBG_E_NOMEM (no room for the junction table, or more k-mers than its 32-bit slots) -> edges None with the reason; any other failure
    of the edge pass (here CDBG_E_INTERNAL) must fail verify() instead of dropping the check"""
    g = api.Graph(15, 2, lib=_EdgePassFails(sim, code), log2_partitions=3)
    try:
        g.push_text(oracle_lib.read_input("rand_a")); g.run()
        if code == api.E_NOMEM:
            v = g.verify()
            assert v["edges"] is None and "(stub)" in v["edges_error"] and v["unitig_kmers"] == v["solid_kmers"], v
        else:
            with pytest.raises(api.CdbgError) as e:
                g.verify()
            assert e.value.code == code
    finally:
        g.close()
