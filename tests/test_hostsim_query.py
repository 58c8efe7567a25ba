"""k-mer lookup in the resident unitig set on the simulator (CPU suite): cdbg_index / cdbg_query / `bcalm -query` through the cases
of query_cases.py, which test_gpu_query.py runs on the device.  Every new block of the simulator is poisoned (CDBG_SIM_POISON):
the table must not depend on what its memory held before."""
import ctypes
import os

import pytest

import hostsim_lib
import kwidth_cases as kc
import query_cases as qc
import test_relink
from test_links import CASES as LINK_CASES
from test_relink import tools  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", "0xA5")


@pytest.mark.parametrize("amin", [1, 2])
@pytest.mark.parametrize("k", kc.K_EDGES)
def test_every_key_width(sim, oracle, k, amin):
    qc.key_width(sim, oracle, k, amin)


@pytest.mark.parametrize("k", [31, 64])
def test_boundaries(sim, k):
    qc.boundaries(sim, k)


def test_batches(sim, monkeypatch):
    qc.batches(sim, monkeypatch)


@pytest.mark.parametrize("name,k", qc.PROBE_CASES)
def test_probe_runs(sim, monkeypatch, name, k):
    qc.probe_runs(sim, monkeypatch, name, k)


def test_repeated_handmade(sim):
    qc.repeated_handmade(sim)


@pytest.mark.parametrize("name,k,amin", LINK_CASES)
def test_repeated_reads(sim, name, k, amin):
    qc.repeated_reads(sim, name, k)


@pytest.mark.parametrize("name,k,n_pieces,n_links", test_relink.SPLIT_CASES)
def test_repeated_split_pieces(sim, tools, tmp_path, name, k, n_pieces, n_links):  # noqa: F811
    qc.repeated_split(sim, tools, tmp_path, name, k)


def test_state(sim):
    qc.state(sim)


def test_state_two_ranks(sim, monkeypatch):
    qc.state_two_ranks(sim, monkeypatch, lambda dst, src, n: ctypes.memmove(dst, src, n))


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(sim, tmp_path, name, k):
    qc.cli(os.path.join(os.path.dirname(hostsim_lib.SO), "bcalm_hostsim"), tmp_path, name, k)
