"""k_compact_wave's batched glue records on the simulator: one compact list of the ends that post a record, the join-bucket place
reserved early for the first step of 64, the store at the end of the bucket.  Every case proves from the simulator's per-bucket
trace (glue_batch_cases.py) that it reached the condition it is named after, then checks the result against the oracle and with
the device-side verification."""
import collections

import pytest

import hostsim_lib
import oracle_lib
from bcalm_amd import api
from glue_batch_cases import BATCH_CASES, SHAPE_CASES, SINK_CASE
from parity import assert_parity, assert_verified


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


def _rows(path):
    out = []
    for line in open(path):
        f = [int(x) for x in line.split()]
        assert len(f) == 6 + f[5], line
        out.append((f[0], f[1], f[2], f[3], f[4], f[5], f[6:]))
    return out


def _traced(oracle, sim, monkeypatch, tmp_path, text, k, amin, kw, env=None, tag="t"):
    """parity + verification of one input with the bucket trace on -> (trace rows of the parity run, its stats)"""
    for name, val in (env or {}).items():
        monkeypatch.setenv(name, val)
    tf = tmp_path / (tag + ".trace")
    monkeypatch.setenv("CDBG_SIM_CW_TRACE", str(tf))
    st = assert_parity(oracle, sim, text, k, amin, **kw)["stats"]
    rows = _rows(tf) if tf.exists() else []
    monkeypatch.delenv("CDBG_SIM_CW_TRACE")
    g = api.Graph(k, amin, lib=sim, **kw)
    try:
        g.push_text(text); g.run(); assert_verified(g)
    finally:
        g.close()
    return rows, st


@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_batch_edges_and_record_kinds(oracle, sim, monkeypatch, tmp_path, name):
    """buckets of 0, 1, 63, 64, 65 and more than 128 glue records; CONFIRM records only, open ends only, both"""
    text, k, kw, conds = BATCH_CASES[name]
    rows, st = _traced(oracle, sim, monkeypatch, tmp_path, text, k, 1, kw)
    for what, pred in conds.items():
        assert pred(rows), (name, what, [r[:6] for r in rows])
    # every open end on a list was posted, once (a bucket beyond the wave tiers posts its own and is not traced)
    assert st["n_glue_open_ends"] >= sum(r[3] - r[4] for r in rows)
    if all(r[2] <= 256 for r in rows) and len(rows) == 1 << kw["log2_partitions"]:
        assert st["n_glue_open_ends"] == sum(r[3] - r[4] for r in rows)


def test_both_sinks_agree(oracle, sim, monkeypatch, tmp_path):
    """the join buckets (single rank) and the sequential log (CDBG_GLUE_LOG: what several ranks exchange): the same buckets post the
    same records, and the unitig sets are equal"""
    text, k, kw = SINK_CASE
    rows_d, st_d = _traced(oracle, sim, monkeypatch, tmp_path, text, k, 1, kw, tag="direct")
    rows_l, st_l = _traced(oracle, sim, monkeypatch, tmp_path, text, k, 1, kw, env={"CDBG_GLUE_LOG": "1"}, tag="log")
    assert any(r[3] > 128 for r in rows_d) and any(0 < r[4] < r[3] for r in rows_d)
    assert sorted(r[:6] for r in rows_d) == sorted(r[:6] for r in rows_l)
    assert st_d["n_glue_open_ends"] == st_l["n_glue_open_ends"] == sum(r[3] - r[4] for r in rows_d)
    assert st_d["n_unitigs"] == st_l["n_unitigs"]                             # (both sets equal the oracle's: assert_parity)


def test_overflow_after_reservation(oracle, sim, monkeypatch, tmp_path):
    """CDBG_JOIN_LOG_JB=0: ONE join bucket of 256 places for a few thousand records.  Places are reserved and abandoned (error 8),
    compaction runs again through the log: every bucket is traced twice, and the result is the oracle's"""
    text, k, kw = SINK_CASE
    rows, st = _traced(oracle, sim, monkeypatch, tmp_path, text, k, 1, kw, env={"CDBG_JOIN_LOG_JB": "0"})
    assert sum(r[3] for r in rows) // 2 > 256
    seen = collections.Counter(r[:6] for r in rows)
    assert seen and all(n == 2 for n in seen.values()), seen


@pytest.mark.parametrize("name", sorted(SHAPE_CASES))
def test_piece_shapes(oracle, sim, monkeypatch, tmp_path, name):
    """what the record passes sit between: pieces of 1, 2 and k - m + 1 k-mers, an isolated cycle inside a bucket, an even k with
    a palindromic k-mer, k < 9 (byte prefix path), k = 55 and k = 127, the 1024-slot tier, all abundance counts"""
    text, k, amin, kw, env, conds = SHAPE_CASES[name]
    if "\n" not in text:
        text = oracle_lib.read_input(text)
    rows, st = _traced(oracle, sim, monkeypatch, tmp_path, text, k, amin, kw, env=env)
    for what, pred in conds.items():
        assert pred(rows), (name, what, [r[:6] for r in rows])
    if name in ("cycle_in_bucket_1", "cycle_in_bucket_3"):
        assert st["n_cycles"] == 1 and st["n_unitigs"] == 1
    if kw.get("all_abundance_counts"):
        from test_abundance import _check
        _check(sim, oracle, text, k, amin, **{x: y for x, y in kw.items() if x != "all_abundance_counts"})
