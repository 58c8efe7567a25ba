"""Every k-mer width and every minimizer window on the GPU (-m gpu): the tables of kwidth_cases.py in full -- every word-edge k under
all three partitionings, every ladder row, every minimizer window 1 .. 126 with the points where the scan changes kernel, each
across all sixteen tile-edge distances.  test_hostsim_kwidth.py proves on the simulator, from its launch trace, which kernels these
inputs reach (same host code); here they run as the instantiations the device compiler made of them: register and LDS budgets
against __launch_bounds__, wave-synchronous code, memory ordering, occupancy-derived grids.

Every case goes through test_step_state.run_case with links and abundances: (k-mer, count) set, canonical unitigs with KC, the
digest formula, the device-side verification with edges, brute-force links and per-k-mer abundances, all against the oracle."""
import pytest

import kwidth_cases as kc
from test_step_state import run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()          # fails loudly when the extension is missing


def check_shape(st, k, m=0):
    assert st["kmer_words"] == kc.words(k), st
    assert st["minimizer_size"] == (m or kc.minimizer_of(k, st["log2_partitions"])), st


@pytest.mark.parametrize("amin,log_np", kc.PARTITIONINGS)
@pytest.mark.parametrize("k", kc.K_EDGES)
def test_word_edge_k(oracle, hip, k, amin, log_np):
    st = run_case(oracle, hip, kc.edge_text(k, 1), k, amin, links=True, abundances=True, log2_partitions=log_np)
    check_shape(st, k)


@pytest.mark.parametrize("row", kc.LADDER, ids=kc.ladder_id)
def test_ladder(oracle, hip, row, monkeypatch):
    k, amin, glen, env, bounds = row
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    st = run_case(oracle, hip, kc.ladder_input(row), k, amin, links=True, abundances=True, log2_partitions=0)
    check_shape(st, k)
    kc.check_bounds(st, bounds)


@pytest.mark.parametrize("k,m", list(kc.window_cases()))
def test_minimizer_windows_across_tile_edges(oracle, hip, k, m):
    text = kc.tile_edge_text(k, m)
    st = run_case(oracle, hip, text, k, 1, links=True, abundances=True, log2_partitions=5, minimizer_size=m)
    check_shape(st, k, m)
    assert st["n_launch_scan"] == -(-len(text) // kc.scan_tile(k, m)), st
