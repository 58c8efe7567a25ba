"""The four consumers of the index give one answer, on the device: the cases of walk_cases.py (as test_hostsim_walk.py runs them on the
simulator) on poisoned memory."""
import pytest

import walk_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import bcalm_amd
    return bcalm_amd.load()


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CDBG_POISON_ALLOC", "0xA5")


@pytest.mark.parametrize("env", wc.ENVS, ids=lambda e: "-".join(e) or "default")
@pytest.mark.parametrize("k", wc.KS)
def test_consumers_agree(hip, monkeypatch, k, env):
    wc.agree(hip, monkeypatch, k, env)
