"""k_walk_copy's chunked arena stores on the GPU (-m gpu): the inputs of test_hostsim_chain_copy.py, which proves on the simulator
-- same kernel source, every store checked against the lane's unitig -- that they reach the shapes the copy distinguishes.  Here:
the unitig set against the oracle, a dense arena, every residue of the unitigs' two ends modulo 16 (over the seeds of a row: the
device's placement order is not the simulator's, chain_copy_cases.py), a unitig of exactly k bases; the per-k-mer abundances next
to the chunked bases; the ranking path on the same input."""
import pytest

from chain_copy_cases import ABUNDANCE_CASE, CASES, RANKING_CASE, assert_conditions, run_case, texts
from parity import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()          # fails loudly when the extension is missing


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(oracle, hip, name):
    k, kw, tx = texts(name)
    assert_conditions([run_case(hip, oracle, text, k, kw)[:2] for text in tx], k)


def test_abundances_next_to_chunked_bases(oracle, hip):
    from test_abundance import _check
    k, kw, tx = texts(ABUNDANCE_CASE)
    _check(hip, oracle, tx[0], k, 1, **kw)


def test_ranking_fallback_same_set(oracle, hip, monkeypatch):
    k, kw, tx = texts(RANKING_CASE)
    monkeypatch.setenv("CDBG_WALK_MAX", "0")
    st = assert_parity(oracle, hip, tx[0], k, 1, **kw)["stats"]
    assert st["n_walked_unitigs"] == 0 and st["n_unitigs"] > 0
