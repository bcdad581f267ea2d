"""The fused rollout kernels' per-lane bookkeeping against the oracle: what a lane still owes, its step serial, the count of good steps
the epilogue reconstructs from `owed`, the games counter and the showdown queue's slots -- k_rollout, k_rollout_tab, k_rollout_allin(_tab)
and k_rollout_call on one full wave plus one ragged wave of 36 lanes, in deferred launches of 16 + 25 + 7 steps (the last one below the
table-evaluator kernels' threshold), with and without auto-reset.  Without it finished games leave lanes that cannot step any more with steps
still requested, and a table in error stops for the rest of its call: the oracle makes the same calls.

Compared: every state array of the snapshot, State::owed, State::terr (through the snapshot blob) and the four device counters against the
oracle's own counts.  State::mid (hands rolled inside a step in flight) has no getter: it is covered through what it governs, the hand-cap
case, whose capped step spans the deferred launches' bookkeeping."""
import numpy as np
import pytest

import golden_util as GU
import snapshot_spec as SS

pytestmark = pytest.mark.gpu

T = 100               # 64 + 36 lanes
PLAN = (16, 25, 7)


@pytest.fixture(scope="module")
def HB():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    from hip_backend import HipBackend
    return HipBackend


@pytest.fixture(scope="module")
def O():
    from oracle import loader
    loader.lib()
    return loader


def assert_same(a, b, where):
    for k in GU.SNAP_FIELDS:
        assert GU.bits_equal(a[k], b[k]), "%s: field %s differs" % (where, k)


def run_case(HB, O, monkeypatch, N, policy, auto, tab=None, cfg=(100, 2, 1), seed=7100, base=0, dealer=0):
    if tab is not None:
        monkeypatch.setenv("PK_ROLLOUT_TAB", tab)
    monkeypatch.setenv("PK_TPB", "64")                  # full-width waves: a small batch would otherwise be spread one table per wave
    o = O.OracleGame(T, N, *cfg, seed=seed, table_id_base=base)
    h = HB(T, N, *cfg, seed=seed, table_id_base=base)
    where = "N=%d policy=%d auto=%s tab=%s" % (N, policy, auto, tab)
    try:
        o.reset(dealer=dealer); h.reset(dealer=dealer)
        h.g.set_coalesce(0)                             # one launch per call
        h.g.launch_stats(reset=True)
        co = np.zeros(4, np.uint64)
        for k in PLAN:
            co += o.rollout(k, policy, auto)[0]
            h.g.rollout(k, policy, auto, True, counters=False)          # asynchronous, may defer its stragglers
        owed_mid = h.g.owed                             # (diagnostic getter: completes nothing)
        assert (owed_mid <= sum(PLAN)).all(), where
        ch = h.rollout(0, policy, auto)                 # completes everything, fetches the counters
        st = h.g.launch_stats()
        assert st["steps"] == sum(PLAN) and st["launches"] >= len(PLAN), (where, st)
        print(where, "counters oracle", co.tolist(), "hip", ch.tolist(), "owed in flight max", int(owed_mid.max()))
        assert ch.tolist() == co.tolist(), where + ": counters (steps, hands, evals, games)"
        if auto:
            assert ch[0] == T * sum(PLAN), where
        assert (h.g.owed == 0).all(), where + ": owed after completion"
        so, sh = o.snapshot(), h.snapshot()
        assert_same(so, sh, where)
        if auto:
            assert (sh["step_serial"] == sum(PLAN)).all(), where
        else:                                           # (with auto-reset a capped table's bits are kept as `seen`, the oracle clears them)
            terr = SS.view(h.g.save(), N, T, "terr")
            assert np.array_equal(terr, o.errs()), where + ": terr"
        return co, o.errs()
    finally:
        h.g.close()


@pytest.mark.parametrize("auto", [True, False], ids=["autoreset", "noreset"])
@pytest.mark.parametrize("N,policy", [(2, 0), (6, 0), (2, 1), (6, 1), (9, 1), (2, 2), (6, 2)],
                         ids=lambda v: str(v))
def test_rollout_bookkeeping_vs_oracle(HB, O, monkeypatch, N, policy, auto):
    """k_rollout_tab / k_rollout_allin_tab (launches of 16 and 25 steps), k_rollout / k_rollout_allin (the 7-step launch) and k_rollout_call.
    The all-in agents at nine seats on the full wave put 9 x 64 = 576 hands into the showdown queue: more than one hand per lane, in the
    lane-major slot order, across the two-hands-per-lane rounds and the single-hand remainder."""
    run_case(HB, O, monkeypatch, N, policy, auto)


@pytest.mark.parametrize("N,policy", [(6, 0), (9, 1)], ids=["random6", "allin9"])
def test_rollout_bookkeeping_without_the_table_evaluator(HB, O, monkeypatch, N, policy):
    """PK_ROLLOUT_TAB=0: every launch takes k_rollout / k_rollout_allin (the queue's results come back through lds.res)."""
    run_case(HB, O, monkeypatch, N, policy, True, tab="0")


@pytest.mark.parametrize("auto", [True, False], ids=["autoreset", "noreset"])
def test_hand_cap_table_keeps_its_step_count(HB, O, monkeypatch, auto):
    """The configuration of the committed game_n6_hand_cap fixture (tests/golden/make_golden.py CAP_SETS) as table 0 of the batch: its ninth
    step rolls past PK_HAND_CAP hands and ends with PK_TERR_HAND_CAP.  Without auto-reset the table's `owed` is zeroed there and its count
    of good steps freezes: `steps` must still be the oracle's.  With auto-reset the capped step counts as a finished game."""
    cfg = ([37.5, 5, 1, 2, 2, 0.5], 0.5, 250)
    co, errs = run_case(HB, O, monkeypatch, 6, 0, auto, cfg=cfg, seed=3107974733015276566, base=551120854, dealer=5)
    if auto:
        assert co[0] == T * sum(PLAN)
    else:
        assert co[0] < T * sum(PLAN)
