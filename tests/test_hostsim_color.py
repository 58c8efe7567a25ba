"""The resident unitigs coloured by sample on the simulator (CPU suite): cdbg_color_open / cdbg_color / cdbg_color_classes / the two fetches /
`bcalm -colors` through the cases of color_cases.py, which test_gpu_color.py runs on the device.  Every new block of the simulator is
poisoned (CDBG_SIM_POISON): planes, table and results must not depend on what their memory held before."""
import ctypes
import os

import pytest

import color_cases as cc
import hostsim_lib
import kwidth_cases as kc


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", "0xA5")


@pytest.mark.parametrize("k", kc.K_EDGES)
def test_every_key_width(sim, k):
    cc.key_width(sim, k)


def test_word_edges(sim, monkeypatch):
    cc.word_edges(sim, monkeypatch)


@pytest.mark.parametrize("n_colors", [1, 32, 33, 64, 65])
def test_color_counts(sim, n_colors):
    cc.color_counts(sim, n_colors)


def test_accumulation(sim, monkeypatch):
    cc.accumulation(sim, monkeypatch)


def test_classes(sim, monkeypatch):
    cc.classes(sim, monkeypatch)


def test_repeated_handmade(sim):
    cc.repeated_handmade(sim)


def test_state(sim):
    cc.state(sim)


def test_state_two_ranks(sim, monkeypatch):
    cc.state_two_ranks(sim, monkeypatch, lambda dst, src, n: ctypes.memmove(dst, src, n))


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(sim, tmp_path, name, k):
    cc.cli(os.path.join(os.path.dirname(hostsim_lib.SO), "bcalm_hostsim"), tmp_path, name, k)
