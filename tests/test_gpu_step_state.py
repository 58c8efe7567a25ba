"""The device side (-m gpu) of tests/test_step_state.py: no result may depend on zeroed, pooled or previous-step memory.

  * the bench's kernel instantiation (k = 31, m = 16, 2^20 partitions, capped single-pass scan; the 1 M-read input of
    test_config3_instantiation_parity) and the config-4 / -5 shapes through three reset() + run() steps on one context, the way bench.py
    times its steps, each step against the oracle; then the same with every new device block -- fresh or from the process's pool --
    filled with 0xFF or 0xA5 (CDBG_POISON_ALLOC);
  * a dirty pool: a context runs on the buffers that another context of the same shape has just handed back;
  * poisoned parity on a sample of the families of tests/test_gpu_parity.py."""
import json
import os
import random

import pytest

import oracle_lib
from parity import assert_parity, assert_verified, set_digest

pytestmark = pytest.mark.gpu
ROOT = oracle_lib.ROOT
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
POISONS = ["0xFF", "0xA5"]
PLAN = ("count_slices", "n_deferred_records", "n_records", "log2_partitions", "n_multipass_partitions", "n_big_partitions")
COMP = str.maketrans("ACGT", "TGCA")
CPU_THREADS = 16


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()


@pytest.fixture(scope="module")
def digest_1m(oracle_1m):
    """(the cdbg_digest formula on the oracle's unitigs, their KC sum) of the 1 M-read input"""
    _, exp = oracle_1m
    return set_digest(exp["unitigs"]), sum(kc for _, kc in exp["unitigs"])


def _check(g, exp, digest=None, kc_sum=None, oracle=None, k=None):
    """a finished graph against the oracle: counts, set digest (formula on the oracle's unitigs, or the canonical unitig set itself when
    `oracle` is given), KC sum, and the device-side definition check with edges -> stats"""
    st = g.stats(); d = g.digest(); es = exp["stats"]
    assert (st["n_occurrences"], st["n_distinct"], st["n_solid"], st["n_unitigs"]) == (es["occurrences"], es["distinct"], es["solid"], es["unitigs"]), (st, es)
    if oracle is not None:
        ut = g.unitigs()
        assert oracle_lib.canonical_set(oracle, ut, k) == exp["unitigs"]
        digest, kc_sum = set_digest(ut), sum(kc for _, kc in exp["unitigs"])
    assert d["set_digest"] == digest and d["kc_sum"] == d["solid_count_sum"] == kc_sum and d["kmers_in_unitigs"] == st["n_solid"], d
    v = assert_verified(g)
    assert v["edges"] is not None and "edges_error" not in v, v
    return st


def _steps(g, check, plan=PLAN):
    plans = []
    for i in range(3):
        if i:
            g.reset()
        g.run()
        st = check(g)
        plans.append({x: st[x] for x in plan})
    assert plans[1] == plans[2], plans
    return plans


@pytest.mark.parametrize("poison", [None] + POISONS)
def test_bench_kernels_three_steps(oracle_1m, digest_1m, hip, poison, monkeypatch):
    """the bench line's instantiation through three steps on one context: every step has the oracle's counts, set digest and KC sum"""
    import bcalm_amd
    monkeypatch.setenv("CDBG_SCAN_MODE", "capped")
    if poison:
        monkeypatch.setenv("CDBG_POISON_ALLOC", poison)
    text, exp = oracle_1m
    g = bcalm_amd.Graph(31, 2, lib=hip, minimizer_size=16, log2_partitions=20)
    try:
        g.push_text(text)
        plans = _steps(g, lambda g: _check(g, exp, *digest_1m))
    finally:
        g.close()
    assert plans[0]["log2_partitions"] == 20


# the config-4 / -5 shapes of test_synthetic_parity, and two whose first step learns or falls back (tests/test_step_state.py): the partition
# count chosen again after a first count (log_np_override), and deferred placement whose placement kernel spills more than the spill list holds
STEP_CASES = {
    "config4_k55": (55, 2, 30000, 150, 4, {}, {}),
    "config5_k127": (127, 2, 4000, 1000, 5, {}, {}),
    "learned_partition_count": (31, 1, 300000, 150, 3, {}, {}),
    "deferred_spill_overflow": (31, 2, 60000, 150, 3, dict(log2_partitions=12), {"CDBG_SCAN_MODE": "capped", "CDBG_DEFER_SLICES": "1,15", "CDBG_PART_CAP": "1"}),
}


@pytest.mark.parametrize("case,poison", [(c, p) for c in ("config4_k55", "config5_k127") for p in [None] + POISONS] +
                         [("learned_partition_count", None), ("deferred_spill_overflow", None)])
def test_three_steps(oracle, hip, case, poison, monkeypatch):
    import bcalm_amd
    k, amin, n, L, cfg, kw, env = STEP_CASES[case]
    for x, v in env.items():
        monkeypatch.setenv(x, v)
    if poison:
        monkeypatch.setenv("CDBG_POISON_ALLOC", poison)
    text = oracle.synth_reads(n, L, cfg)
    exp = oracle.run(text, k, amin)
    # (k-mers of three words and more under an abundance filter: which count tier takes a partition near the admission limit of the sifting tier
    #  depends on the order in which its records landed -- device atomics, not step state -- so n_multipass_partitions may differ by one or two
    #  between identical steps, with the same result (see test_count_sift_tier_gpu); the simulator, in order, checks these counts too)
    plan = PLAN if k < 64 else tuple(x for x in PLAN if x not in ("n_multipass_partitions", "n_big_partitions"))
    g = bcalm_amd.Graph(k, amin, lib=hip, **kw)
    try:
        g.push_text(text)
        plans = _steps(g, lambda g: _check(g, exp, oracle=oracle, k=k), plan)
    finally:
        g.close()
    if case == "learned_partition_count":
        assert plans[0]["log2_partitions"] == plans[1]["log2_partitions"], plans
    elif case == "deferred_spill_overflow":                 # (the count that was kept placed every record itself)
        assert all(p["count_slices"] == 1 and p["n_deferred_records"] == 0 for p in plans), plans


def test_dirty_pool_handover_on_device(oracle, oracle_1m, digest_1m, hip):
    """A runs and is destroyed (its buffers go to the process's pool), then B -- same k, same partition count -- runs on them:
    2 M hostile reads at abundance-min 1 (abundance vectors and links on) hand over to the 1 M uniform reads, compared with the oracle;
    then 1 M uniform reads hand over to 400 K hostile reads, compared with oracle/cpu_mt.cpp"""
    import bcalm_amd
    text, exp = oracle_1m
    kw = dict(minimizer_size=16, log2_partitions=20)
    hip.cdbg_release_cached()
    a = bcalm_amd.Graph(31, 1, lib=hip, all_abundance_counts=True, **kw)
    try:
        a.generate_reads(2_000_000, 150, 3 | 0x100); a.run(); assert_verified(a)      # (verify builds the links)
    finally:
        a.close()
    b = bcalm_amd.Graph(31, 2, lib=hip, **kw)
    try:
        b.push_text(text); b.run(); _check(b, exp, *digest_1m)
    finally:
        b.close()
    hip.cdbg_release_cached()
    a = bcalm_amd.Graph(31, 2, lib=hip, **kw)
    try:
        a.push_text(text); a.run()
    finally:
        a.close()
    b = bcalm_amd.Graph(31, 1, lib=hip, **kw)
    try:
        b.generate_reads(400_000, 150, 3 | 0x100)
        cpu = oracle_lib.cpu_mt_run(b.read_text(0, 400_000 * 151), 31, 1, CPU_THREADS)
        b.run(); st = b.stats(); d = b.digest(); assert_verified(b)
    finally:
        b.close()
    assert st["n_occurrences"] == cpu["occurrences"] == 400_000 * 120
    assert (st["n_distinct"], st["n_solid"], st["n_unitigs"], st["unitig_bases"]) == (cpu["distinct"], cpu["solid"], cpu["unitigs"], cpu["unitig_bases"])
    assert d["kc_sum"] == cpu["kc_sum"] and d["set_digest"] == cpu["set_digest"]


# ---- poisoned parity: a sample of the families of tests/test_gpu_parity.py ----
@pytest.fixture(params=POISONS)
def poison(request, monkeypatch):
    monkeypatch.setenv("CDBG_POISON_ALLOC", request.param)
    return request.param


@pytest.mark.parametrize("key", sorted(GOLD))
@pytest.mark.parametrize("log_np", [-1, 10])
def test_golden_parity_poisoned(oracle, hip, poison, key, log_np):
    name, k, amin = key.split("/")
    k, amin = int(k), int(amin)
    got = assert_parity(oracle, hip, oracle_lib.read_input(name), k, amin, log2_partitions=log_np)
    assert oracle_lib.canonical_set(oracle, got["unitigs"], k) == [tuple(u) for u in GOLD[key]["unitigs"]]
    assert oracle_lib.solid_sha256(got["solid"]) == GOLD[key]["solid"]["sha256"]


@pytest.mark.parametrize("k,cfg,n_reads,read_len,log_np", [(31, 3, 60000, 150, 12), (255, 5, 1500, 1000, 10)])
@pytest.mark.parametrize("part_cap,defer_cap", [("260", None), (None, "16")])
def test_deferred_record_placement_poisoned(oracle, hip, poison, k, cfg, n_reads, read_len, log_np, part_cap, defer_cap, monkeypatch):
    """the shapes of test_deferred_record_placement_gpu with four slices: regions small enough for k_place to spill, streams small enough to fill up"""
    monkeypatch.setenv("CDBG_SCAN_MODE", "capped"); monkeypatch.setenv("CDBG_DEFER_SLICES", "4")
    if part_cap:
        monkeypatch.setenv("CDBG_PART_CAP", part_cap)
    if defer_cap:
        monkeypatch.setenv("CDBG_DEFER_CAP", defer_cap)
    st = assert_parity(oracle, hip, oracle.synth_reads(n_reads, read_len, cfg), k, 2, log2_partitions=log_np)["stats"]
    assert st["count_slices"] == 4 and st["n_deferred_records"] > 0


@pytest.mark.parametrize("case", ["sifted", "solid_overflow", "fingerprint_overflow", "many_members"])
def test_count_sift_tier_poisoned(oracle, hip, poison, case):
    """test_count_sift_tier_gpu at k = 127: the sifting tier, and the multi-pass kernel behind it"""
    k = 127
    rng = random.Random(k * 7 + len(case))
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    g = rnd({"sifted": 250, "solid_overflow": 1500, "fingerprint_overflow": 250, "many_members": 300}[case] + k)
    reads = [g, g, g[5:], g[::-1].translate(COMP)] + [rnd(k + 99) for _ in range({"sifted": 26, "solid_overflow": 8, "fingerprint_overflow": 90, "many_members": 45}[case])]
    if case == "many_members":
        reads += [g] * 24
    reads.append(g[:k + 10] + rnd(1) + g[k + 11:2 * k + 30])
    got = assert_parity(oracle, hip, "\n".join(reads) + "\n", k, 2, log2_partitions=0)
    assert got["stats"]["n_multipass_partitions"] == (0 if case in ("sifted", "many_members") else 1), got["stats"]


@pytest.mark.parametrize("mode", ["log", "table", "overflow", "rank", "walkmax"])
def test_glue_record_paths_poisoned(oracle, hip, poison, mode, monkeypatch):
    """test_glue_record_paths_gpu at k = 31"""
    monkeypatch.setenv({"log": "CDBG_GLUE_LOG", "table": "CDBG_GLUE_TABLE", "overflow": "CDBG_JOIN_LOG_JB", "rank": "CDBG_GLUE_RANK", "walkmax": "CDBG_WALK_MAX"}[mode],
                       "0" if mode in ("overflow", "walkmax") else "1")
    st = assert_parity(oracle, hip, oracle.synth_reads(100000, 150, 3), 31, 2)["stats"]
    assert st["n_walked_unitigs"] == (0 if mode in ("rank", "walkmax") else st["n_unitigs"])


@pytest.mark.parametrize("k,glen,log_np", [(31, 400000, 10), (55, 400000, 10)])
@pytest.mark.parametrize("tier2", ["1", "0"])
def test_second_wave_tier_poisoned(oracle, hip, poison, k, glen, log_np, tier2, monkeypatch):
    """test_second_wave_tier_one_word_gpu at k = 31 and 55"""
    import bcalm_amd
    from test_hostsim_pipeline import _mid_bucket_text
    if k <= 31:
        monkeypatch.setenv("CDBG_CW_TIER2", tier2)
    elif tier2 == "0":
        monkeypatch.setenv("CDBG_CW_TIER3", "off")
    text = _mid_bucket_text(k, glen, glen + k)
    assert_parity(oracle, hip, text, k, 1, log2_partitions=log_np)
    gg = bcalm_amd.Graph(k, 1, lib=hip, log2_partitions=log_np)
    try:
        gg.push_text(text); gg.run(); assert_verified(gg)
    finally:
        gg.close()
