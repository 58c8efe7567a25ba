"""A read set counted against the resident unitigs on the simulator (CPU suite): cdbg_quantify / cdbg_fetch_quant / cdbg_quant_reset /
`bcalm -quantify` through the cases of quant_cases.py, which test_gpu_quant.py runs on the device.  Every new block of the simulator is
poisoned (CDBG_SIM_POISON): the counters must not depend on what their memory held before."""
import ctypes
import os

import pytest

import hostsim_lib
import kwidth_cases as kc
import quant_cases as qn


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", "0xA5")


@pytest.mark.parametrize("amin", [1, 2])
@pytest.mark.parametrize("k", kc.K_EDGES)
def test_every_key_width(sim, k, amin):
    qn.key_width(sim, k, amin)


@pytest.mark.parametrize("k", [31, 64])
def test_boundaries(sim, k):
    qn.boundaries(sim, k)


def test_batches(sim, monkeypatch):
    qn.batches(sim, monkeypatch)


@pytest.mark.parametrize("k", [8, 31])
def test_extension_edges(sim, monkeypatch, k):
    qn.extension_edges(sim, monkeypatch, k)


def test_repeated_handmade(sim):
    qn.repeated_handmade(sim)


def test_ceiling_and_clamp(sim, monkeypatch):
    qn.ceiling(sim, monkeypatch)


def test_state(sim):
    qn.state(sim)


def test_state_two_ranks(sim, monkeypatch):
    qn.state_two_ranks(sim, monkeypatch, lambda dst, src, n: ctypes.memmove(dst, src, n))


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(sim, tmp_path, name, k):
    qn.cli(os.path.join(os.path.dirname(hostsim_lib.SO), "bcalm_hostsim"), tmp_path, name, k)
