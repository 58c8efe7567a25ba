"""Pseudoalignment to the coloured unitigs on the simulator (CPU suite): cdbg_color_query / cdbg_fetch_color_query /
cdbg_fetch_color_query_counts / `bcalm -colors -color-query` through the cases of color_query_cases.py, which test_gpu_color_query.py runs
on the device.  Every new block of the simulator is poisoned (CDBG_SIM_POISON): no result may depend on what its memory held before."""
import os

import pytest

import color_query_cases as cq
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
    cq.key_width(sim, k)


def test_run_edges(sim, monkeypatch):
    cq.run_edges(sim, monkeypatch)


@pytest.mark.parametrize("n_colors", [1, 32, 33, 64, 65])
def test_color_counts(sim, n_colors):
    cq.color_counts(sim, n_colors)


def test_thresholds(sim):
    cq.thresholds(sim)


def test_many_segments(sim):
    cq.many_segments(sim)


def test_batch_seams(sim, monkeypatch):
    cq.batch_seams(sim, monkeypatch)


def test_repeated_handmade(sim):
    cq.repeated_handmade(sim)


def test_state(sim):
    cq.state(sim)


@pytest.mark.parametrize("name,k", [("pufferize_refs", 9), ("rand_b", 31)])
def test_cli(sim, tmp_path, name, k):
    cq.cli(sim, os.path.join(os.path.dirname(hostsim_lib.SO), "bcalm_hostsim"), tmp_path, name, k)
