"""k_walk_copy's chunked arena stores on the simulator: parity with the oracle, a dense arena, and -- from the per-piece trace of
the simulator build (CDBG_SIM_WALK_TRACE: unitig, its offset, first new byte, new bytes, forward?, chunks that left inside the
piece, last piece?) -- proof that the inputs reach the shapes the copy distinguishes.  The simulator build checks every arena
store of the kernel against the lane's unitig (device error 10), so a store into a neighbour fails the run itself."""
import pytest

import hostsim_lib
from chain_copy_cases import ABUNDANCE_CASE, CASES, MIN_UNITIGS_PER_ROW, RANKING_CASE, assert_conditions, run_case, texts
from parity import assert_parity


@pytest.fixture(scope="module")
def sim():
    return hostsim_lib.load()


@pytest.fixture(scope="module")
def runs(oracle, sim, tmp_path_factory):
    """name -> [(offsets, lengths, stats, trace rows of the layout run) of every seed], each case run once for all tests of this file"""
    done = {}
    tdir = tmp_path_factory.mktemp("walk_trace")

    def get(name):
        if name not in done:
            k, kw, tx = texts(name)
            out = []
            for i, text in enumerate(tx):
                tf = tdir / ("%s_%d.trace" % (name, i))
                off, ln, st = run_case(sim, oracle, text, k, kw, trace=tf)
                rows = [tuple(int(x) for x in line.split()) for line in open(tf)] if tf.exists() else []
                assert all(len(r) == 7 for r in rows)
                out.append((off, ln, st, rows))
            done[name] = out
        return done[name]
    return get


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(runs, name):
    k = CASES[name][0]
    res = runs(name)
    assert_conditions([res[0][:2]], k)                            # the first seed by itself, in the simulator's one order
    assert sum(len(off) for off, _, _, _ in res) >= MIN_UNITIGS_PER_ROW      # (what the device test's residues rest on)
    for off, ln, st, rows in res:
        if k < 9:
            assert not rows                                       # (copied piece by piece: not traced)
            continue
        # the trace speaks of this layout: one row per piece, every unitig's last row ends where the unitig does
        assert len(rows) == st["n_pieces"]
        last = [r for r in rows if r[6]]
        assert len(last) == len(off)
        for uid, uoff, at, new, _, _, _ in last:
            assert uoff == off[uid] and at + new == ln[uid]


def test_trace_reaches_every_shape(runs):
    rows = [r for name in sorted(CASES) for res in runs(name) for r in res[3]]
    for fwd in (0, 1):
        assert {r[3] for r in rows if r[4] == fwd} >= set(range(1, 18)), (fwd, sorted({r[3] for r in rows if r[4] == fwd}))
    assert any(r[5] == 2 for r in rows), "no piece with two chunks leaving inside it"
    assert any(r[5] == 0 for r in rows), "no piece without a chunk leaving"
    ends = {(r[1] + r[2] + r[3]) % 16 for r in rows if r[6]}
    assert 0 in ends and 1 in ends, sorted(ends)


def test_abundances_next_to_chunked_bases(oracle, sim):
    from test_abundance import _check
    k, kw, tx = texts(ABUNDANCE_CASE)
    _check(sim, oracle, tx[0], k, 1, **kw)


def test_ranking_fallback_same_set(oracle, sim, monkeypatch):
    k, kw, tx = texts(RANKING_CASE)
    monkeypatch.setenv("CDBG_WALK_MAX", "0")
    st = assert_parity(oracle, sim, tx[0], k, 1, **kw)["stats"]
    assert st["n_walked_unitigs"] == 0 and st["n_unitigs"] > 0
