"""The four consumers of the index give one answer, on the simulator (CPU suite): the cases of walk_cases.py, which test_gpu_walk.py runs on
the device.  Every new block of the simulator is poisoned (CDBG_SIM_POISON)."""
import pytest

import hostsim_lib
import walk_cases as wc


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_SIM_POISON", "0xA5")


@pytest.mark.parametrize("env", wc.ENVS, ids=lambda e: "-".join(e) or "default")
@pytest.mark.parametrize("k", wc.KS)
def test_consumers_agree(sim, monkeypatch, k, env):
    wc.agree(sim, monkeypatch, k, env)
