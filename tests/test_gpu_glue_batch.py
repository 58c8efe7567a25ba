"""k_compact_wave's batched glue records on the GPU (-m gpu): the inputs of test_hostsim_glue_batch.py, which proves on the
simulator -- same partitioning, same classification code -- that each of them reaches the condition it is named after (buckets
of 0, 1, 63, 64, 65 and more than 128 records, CONFIRM-only / open-only / mixed buckets, the 1024-slot tier, ...).  Here: the
unitig set against the oracle and the device-side verification, through the join buckets, the log, and the overflow fallback."""
import pytest

import oracle_lib
from bcalm_amd import api
from glue_batch_cases import BATCH_CASES, SHAPE_CASES, SINK_CASE
from parity import assert_parity, assert_verified

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()          # fails loudly when the extension is missing


def _run(oracle, hip, text, k, amin, kw):
    st = assert_parity(oracle, hip, text, k, amin, **kw)["stats"]
    g = api.Graph(k, amin, lib=hip, **kw)
    try:
        g.push_text(text); g.run(); assert_verified(g)
    finally:
        g.close()
    return st


@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_batch_edges_and_record_kinds(oracle, hip, name):
    text, k, kw, _ = BATCH_CASES[name]
    _run(oracle, hip, text, k, 1, kw)


def test_both_sinks_agree(oracle, hip, monkeypatch):
    text, k, kw = SINK_CASE
    st_d = _run(oracle, hip, text, k, 1, kw)
    monkeypatch.setenv("CDBG_GLUE_LOG", "1")
    st_l = _run(oracle, hip, text, k, 1, kw)
    assert st_d["n_glue_open_ends"] == st_l["n_glue_open_ends"] > 128
    assert st_d["n_unitigs"] == st_l["n_unitigs"]


def test_overflow_after_reservation(oracle, hip, monkeypatch):
    text, k, kw = SINK_CASE
    monkeypatch.setenv("CDBG_JOIN_LOG_JB", "0")
    _run(oracle, hip, text, k, 1, kw)


@pytest.mark.parametrize("name", sorted(SHAPE_CASES))
def test_piece_shapes(oracle, hip, monkeypatch, name):
    text, k, amin, kw, env, _ = SHAPE_CASES[name]
    if "\n" not in text:
        text = oracle_lib.read_input(text)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    st = _run(oracle, hip, text, k, amin, kw)
    if name in ("cycle_in_bucket_1", "cycle_in_bucket_3"):
        assert st["n_cycles"] == 1 and st["n_unitigs"] == 1
    if kw.get("all_abundance_counts"):
        from test_abundance import _check
        _check(hip, oracle, text, k, amin, **{x: y for x, y in kw.items() if x != "all_abundance_counts"})
