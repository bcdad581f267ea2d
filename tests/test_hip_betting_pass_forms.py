"""The fused random-agent rollout against the oracle, every state byte, aimed at what a betting pass computes with seat and serial arithmetic
(pk_device.hpp): ActionRing::half_of (the 16-bit draw taken by one bit-field extract at offset `serial << 4`), begin_step<PK_MONEY_BLOCK>
(`pending[a] = bet` as a block on the lanes where money moves) and the cyclic seat walks of scan_first / next_turns / first_playing (the seat
mask twice over, windows by bit-field extract, wrap-arounds by unsigned minimum).

67 tables in waves of 64 and 3 lanes (PK_TPB=64), at 2, 3 and 6 seats, 48 steps: as launches of 16 + 25 + 7 (PK_ROLLOUT_TAB=1: the
table-evaluator kernel k_rollout_tab runs all three), compared after every launch, and as 48 launches of one step (k_rollout_single).  The other
rollout kernels' form, begin_step<PK_MONEY_SEAT>, is the parent's and stays with the older tests.  Once more at six seats with the serials
resumed at (2^32 - 2, 2^35 - 5): the step serial's low word carries into the high word five steps into the run, and `serial << 4` drops all but
the parity either way.

Before the device runs, a pre-flight on the oracle alone (one Game.step at a time on the rollout's own draws, which must end in the rollout's
state) shows that the run exercises what it is aimed at: at six seats every seat index acts with a money action (CALL, a raise, ALL_IN) and
with FOLD or CHECK, draws are taken at odd and at even step serials, and a next_turn follows each of the turns 0, 1 and 2."""
import numpy as np
import pytest

import golden_util as GU

pytestmark = pytest.mark.gpu

T = 67                           # 64 + 3 lanes
PLAN = (16, 25, 7)
K_STEPS = sum(PLAN)
SEATS = (2, 3, 6)
SEED = 0x62657473                # "bets"
RESUMED = (2 ** 32 - 2, 2 ** 35 - 5)
MV_CALL = 2                      # FOLD 0, CHECK 1 | CALL 2, RAISE_* 3..5, ALL_IN 6: money moves


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


def oracle(O, N, serials):
    o = O.OracleGame(T, N, seed=SEED + N)
    if serials is not None:
        o.set_serials(*serials)
    o.reset()
    return o


_REF = {}


def reference(O, N, serials):
    """The oracle's snapshots after 16, 41 and 48 steps, computed once per configuration and shared by the tests (never modified), behind the
    pre-flight: the same 48 steps one Game.step at a time."""
    key = (N, serials)
    if key in _REF:
        return _REF[key]
    where = "pre-flight N=%d%s" % (N, "" if serials is None else " resumed")
    o = oracle(O, N, serials)
    snaps, counters = [], np.zeros(4, np.uint64)
    for k in PLAN:
        counters += o.rollout(k, 0, True)[0]
        snaps.append(o.snapshot())
    p = oracle(O, N, serials)
    money, quiet = np.zeros(N, bool), np.zeros(N, bool)
    parity, turns = set(), set()
    for _ in range(K_STEPS):
        s = p.snapshot()
        a = p.pick_actions(0)
        parity.update((np.asarray(s["step_serial"], np.uint64) & np.uint64(1)).tolist())
        for seat, act in zip(s["active"].tolist(), a.tolist()):
            (money if act >= MV_CALL else quiet)[seat] = True
        flags, err = p.step(a)
        assert not err.any(), where
        s1 = p.snapshot()
        same_hand = (s1["hand"] == s["hand"]) & (s1["hand_serial"] == s["hand_serial"])
        turns.update(s["turn"][same_hand & (s1["turn"] > s["turn"])].tolist())
        over = (flags & 1).astype(np.uint8)                 # PK_FLAG_GAME_OVER: the rollout resets such a table on the spot
        if over.any():
            p.reset(mask=over)
    assert_same(snaps[-1], p.snapshot(), where + ": step by step against the rollout")
    if N == 6:
        assert money.all() and quiet.all(), (where, money.tolist(), quiet.tolist())
    assert parity == {0, 1}, (where, parity)
    assert {0, 1, 2} <= turns, (where, turns)
    if serials is not None:                                 # the case is about the carry: every table's low word must have wrapped
        s0 = np.uint64(serials[1])
        assert int(s0) % 2 ** 32 > 2 ** 32 - K_STEPS and ((np.asarray(snaps[-1]["step_serial"], np.uint64) >> np.uint64(32)) > (s0 >> np.uint64(32))).all(), where
    _REF[key] = (snaps, counters)
    return _REF[key]


def device(HB, N, serials):
    h = HB(T, N, seed=SEED + N)
    assert h.g.wave_shape[0] == 64
    if serials is not None:
        h.set_serials(*serials)
    h.reset()
    h.g.set_coalesce(0)                                     # one launch per call
    return h


def run_fused(HB, O, N, serials):
    snaps, counters = reference(O, N, serials)
    where = "N=%d%s" % (N, "" if serials is None else " resumed")
    h = device(HB, N, serials)
    try:
        got = np.zeros(4, np.uint64)
        for k, want in zip(PLAN, snaps):
            got += np.asarray(h.rollout(k, 0, True), np.uint64)
            assert_same(want, h.snapshot(), "%s after the launch of %d steps" % (where, k))
        assert got.tolist() == counters.tolist(), where + ": counters (steps, hands, evals, games)"
        assert (h.g.owed == 0).all(), where
    finally:
        h.g.close()


def run_single(HB, O, N, serials):
    snaps, counters = reference(O, N, serials)
    where = "N=%d%s, launches of one step" % (N, "" if serials is None else " resumed")
    h = device(HB, N, serials)
    try:
        got = np.zeros(4, np.uint64)
        done = 0
        for k, want in zip(PLAN, snaps):
            for _ in range(k):
                got += np.asarray(h.rollout(1, 0, True), np.uint64)
            done += k
            assert_same(want, h.snapshot(), "%s, after %d" % (where, done))
        assert got.tolist() == counters.tolist(), where + ": counters (steps, hands, evals, games)"
    finally:
        h.g.close()


@pytest.mark.parametrize("N", SEATS)
def test_fused_launches_of_16_25_7_steps_vs_oracle(HB, O, monkeypatch, N):
    monkeypatch.setenv("PK_TPB", "64")                      # full-width waves: a small batch would otherwise be spread one table per wave
    monkeypatch.setenv("PK_ROLLOUT_TAB", "1")
    run_fused(HB, O, N, None)


@pytest.mark.parametrize("N", SEATS)
def test_one_step_launches_vs_oracle(HB, O, monkeypatch, N):
    monkeypatch.setenv("PK_TPB", "64")
    monkeypatch.setenv("PK_ROLLOUT_TAB", "1")
    run_single(HB, O, N, None)


def test_resumed_serials_carry_in_the_low_word_fused(HB, O, monkeypatch):
    monkeypatch.setenv("PK_TPB", "64")
    monkeypatch.setenv("PK_ROLLOUT_TAB", "1")
    run_fused(HB, O, 6, RESUMED)


def test_resumed_serials_carry_in_the_low_word_one_step_launches(HB, O, monkeypatch):
    monkeypatch.setenv("PK_TPB", "64")
    monkeypatch.setenv("PK_ROLLOUT_TAB", "1")
    run_single(HB, O, 6, RESUMED)
