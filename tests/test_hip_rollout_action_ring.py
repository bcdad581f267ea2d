"""The fused random-agent rollout's action draws against the oracle, aimed at the action ring (ActionRing in pk_device.hpp: two Philox blocks of
eight 16-bit draws per lane in LDS, refilled for every lane at once when some lane runs short) and at the Philox block itself, which the ring,
the deal and k_pick share.  Every state byte of the snapshot, State::owed and the four counters, on 165 tables in waves of 64, 64 and 37 lanes
(PK_TPB=64), at 2 and 6 seats, with the table-evaluator kernels (PK_ROLLOUT_TAB=1: k_rollout_tab for the launches of 16 steps and more) and
without (k_rollout for every launch).

The ring is rebuilt from the step serial at every launch, so the calls are short and many -- 1, 2, 3, 5, 16, 25, 7 and 40 steps -- once as one
launch per call (set_coalesce(0)) and once merged as the host merges them by default.  The configurations:

  pos567   step serials set before the first reset so that the lanes of a wave start at positions 5, 6 and 7 of an action block: the first
           ensure() of a launch must fetch the current block AND the next one for some lanes and not for their neighbours
  wrap     step serial 2^35 - 5 (block index 2^32 - 1) and hand serial 2^32 - 2: the block index crosses 2^32 after five steps, the ring's
           32-bit `filled` wraps while the Philox counter takes the index's high word
  short    per-seat stacks of a few big blinds: games end within a few hands, so lanes auto-reset (and are dealt a fresh game) in the middle of
           a block while their neighbours play on
  idle     the same stacks without auto-reset, behind a call of no steps at all: first every lane owes nothing, later more and more lanes sit
           on a finished game with steps still requested and never draw again"""
import numpy as np
import pytest

import golden_util as GU

pytestmark = pytest.mark.gpu

T = 165                          # 64 + 64 + 37 lanes
PLAN = (1, 2, 3, 5, 16, 25, 7, 40)
SHORT = [3, 5, 2, 7.5, 4, 2.5]
KINDS = ("pos567", "wrap", "short", "idle")


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


def config(kind, N):
    """(start credits, big blind, small blind), (hand serials, step serials) or None, auto_reset, seed, table id base"""
    if kind == "pos567":
        pos = np.array([5, 6, 7], np.uint64)[np.arange(T) % 3]
        return (100, 2, 1), (np.zeros(T, np.uint64), np.uint64(8 * 4000) + pos), True, 8100 + N, 0
    if kind == "wrap":
        return (100, 2, 1), (2 ** 32 - 2, 2 ** 35 - 5), True, 8200 + N, 0xffffff9c     # (table ids wrap 2^32 inside the batch as well)
    return (SHORT[:N], 2, 1), None, kind == "short", 8300 + N, 77


def assert_same(a, b, where):
    for k in GU.SNAP_FIELDS:
        assert GU.bits_equal(a[k], b[k]), "%s: field %s differs" % (where, k)


def run_case(HB, O, kind, N, coalesce):
    cfg, serials, auto, seed, base = config(kind, N)
    where = "%s N=%d coalesce=%s" % (kind, N, coalesce)
    o = O.OracleGame(T, N, *cfg, seed=seed, table_id_base=base)
    h = HB(T, N, *cfg, seed=seed, table_id_base=base)
    try:
        assert h.g.wave_shape[0] == 64, where
        if serials is not None:
            o.set_serials(*serials); h.set_serials(*serials)
        o.reset(); h.reset()
        if coalesce is not None:
            h.g.set_coalesce(coalesce)
        co = np.zeros(4, np.uint64)
        if kind == "idle":                                  # a launch in which no table owes anything
            co += o.rollout(0, 0, auto)[0]
            ch0 = h.rollout(0, 0, auto)
            assert ch0.tolist() == [0, 0, 0, 0], where
            assert_same(o.snapshot(), h.snapshot(), where + " after a call of no steps")
        s0 = np.asarray(o.snapshot()["step_serial"], np.uint64)
        for k in PLAN:
            co += o.rollout(k, 0, auto)[0]
            h.g.rollout(k, 0, auto, True, counters=False)   # asynchronous: may defer its stragglers, may be merged with the next call
        ch = h.rollout(0, 0, auto)                          # completes everything, fetches the counters
        assert ch.tolist() == co.tolist(), where + ": counters (steps, hands, evals, games)"
        assert (h.g.owed == 0).all(), where + ": owed after completion"
        so, sh = o.snapshot(), h.snapshot()
        assert_same(so, sh, where)
        s1 = np.asarray(so["step_serial"], np.uint64)
        if auto:
            assert ch[0] == T * sum(PLAN) and (s1 - s0 == sum(PLAN)).all(), where
        if kind == "wrap":                                  # the case is about the crossing: it must have happened on every table
            assert ((s0 >> np.uint64(3)) < 2 ** 32).all() and ((s1 >> np.uint64(3)) >= 2 ** 32).all(), where
        if kind == "short":
            assert ch[3] >= T, where + ": every table should have finished a game or more"
        if kind == "idle":
            assert 0 < ch[0] < T * sum(PLAN), where + ": some lanes must have stopped on a finished game"
    finally:
        h.g.close()


@pytest.mark.parametrize("coalesce", [0, None], ids=["launch_per_call", "merged"])
@pytest.mark.parametrize("tab", ["1", "0"], ids=["tab", "notab"])
@pytest.mark.parametrize("N", [2, 6])
def test_action_draws_of_the_fused_rollout_vs_oracle(HB, O, monkeypatch, N, tab, coalesce):
    monkeypatch.setenv("PK_ROLLOUT_TAB", tab)
    monkeypatch.setenv("PK_TPB", "64")                      # full-width waves: a small batch would otherwise be spread one table per wave
    for kind in KINDS:
        run_case(HB, O, kind, N, coalesce)
