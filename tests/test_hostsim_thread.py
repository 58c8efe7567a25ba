"""Run-length lookup on the simulator (CPU suite): cdbg_thread / cdbg_fetch_runs / `bcalm -thread` through the cases of thread_cases.py,
which test_gpu_thread.py runs on the device.  Every new block of the simulator is poisoned (CDBG_SIM_POISON): the runs must not depend on
what their memory held before."""
import ctypes
import os

import pytest

import hostsim_lib
import kwidth_cases as kc
import thread_cases as tc


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", "0xA5")


@pytest.mark.parametrize("amin", [1, 2])
@pytest.mark.parametrize("k", kc.K_EDGES)
def test_every_key_width(sim, k, amin):
    tc.key_width(sim, k, amin)


@pytest.mark.parametrize("k", [31, 64])
def test_boundaries(sim, k):
    tc.boundaries(sim, k)


def test_long_runs_across_tiles(sim):
    tc.long_runs(sim)


def test_full_density(sim):
    tc.full_density(sim)


@pytest.mark.parametrize("k", [8, 31])
def test_extension_edges(sim, monkeypatch, k):
    tc.extension_edges(sim, monkeypatch, k)


def test_palindrome_cuts_a_reverse_walk(sim, monkeypatch):
    tc.palindrome(sim, monkeypatch)


def test_batches(sim, monkeypatch):
    tc.batches(sim, monkeypatch)


def test_repeated_handmade(sim):
    tc.repeated_handmade(sim)


def test_state(sim):
    tc.state(sim)


def test_state_two_ranks(sim, monkeypatch):
    tc.state_two_ranks(sim, monkeypatch, lambda dst, src, n: ctypes.memmove(dst, src, n))


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(sim, tmp_path, name, k):
    tc.cli(os.path.join(os.path.dirname(hostsim_lib.SO), "bcalm_hostsim"), tmp_path, name, k)
