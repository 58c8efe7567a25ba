"""Connected components on the simulator (CPU suite): cdbg_components / cdbg_fetch_components / `bcalm -components` through the cases of
components_cases.py, which test_gpu_components.py runs on the device.  Every new block of the simulator is poisoned (CDBG_SIM_POISON): the
labels must not depend on what their memory held before.  The simulator runs one lane at a time: the racing hooks are the device's part."""
import ctypes
import os

import pytest

import components_cases as cc
import hostsim_lib


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", "0xA5")


def test_handmade(sim):
    cc.handmade(sim)


@pytest.mark.parametrize("name,k,n_unitigs,n_comp,sizes", cc.FIXTURES, ids=[f[0] for f in cc.FIXTURES])
def test_fixture(sim, name, k, n_unitigs, n_comp, sizes):
    cc.fixture(sim, name, k, n_unitigs, n_comp, sizes)


@pytest.mark.parametrize("amin", [1, 2])
@pytest.mark.parametrize("k", cc.K_WIDTHS)
def test_key_width(sim, k, amin):
    cc.key_width(sim, k, amin)


def test_chains(sim):
    """5 000 pieces in order, reversed, shuffled, and four interleaved chains: a fixed number of launches, so seconds on the simulator"""
    cc.chains(sim, 5000)


def test_star(sim):
    cc.star(sim)


def test_state(sim):
    cc.state(sim)


def test_state_two_ranks(sim, monkeypatch):
    cc.state_two_ranks(sim, monkeypatch, lambda dst, src, n: ctypes.memmove(dst, src, n))


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(sim, tmp_path, name, k):
    cc.cli(os.path.join(os.path.dirname(hostsim_lib.SO), "bcalm_hostsim"), tmp_path, name, k)
