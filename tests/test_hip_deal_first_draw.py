"""The decks the device kernels leave in game.deck against the RNG spec (oracle/rng_spec.py), aimed at the Lehmer decode of
Table<N>::deal_cards: where 5 + 2 N = 4 k + 1 (every even seat count) the FIRST draw stays out of the packed words and the decoded words are
shifted into deck order; elsewhere every draw is packed.  A table's deck is deck_permutation(seed, table id, hand_serial - 1)[:5 + 2 N] mapped
through canonical_deck_values(): the deal of hand_serial h is the one before the serial moved on to h + 1.

67 tables in waves of 64 and 3 lanes (PK_TPB=64), at 2, 4 and 6 seats (K = 9, 13, 17; k_rollout_tab for the fused run), 8 and 16 seats
(K = 21 and 37 -- the only K = 4 k + 1 with three Philox blocks) and, as controls on the other path, 3 and 9 seats.  Runs: after reset() (k_reset), after 48
fused steps (one launch), after 48 launches of one step (k_rollout), after 48 Game.steps on picked actions (k_pick + k_step, finished games
reset by mask), and the first three once more with table ids that wrap 2^32 inside the batch and the serials resumed at (2^32 - 2, 2^35 - 5), so that
the hand serial's high word -- a Philox counter word of its own -- comes into play during the run."""
import numpy as np
import pytest

from oracle import rng_spec as R

pytestmark = pytest.mark.gpu

T = 67                           # 64 + 3 lanes
K_STEPS = 48
SEATS = (2, 4, 6, 8, 16, 3, 9)
SEED = 0x6669727374              # "first"
RESUMED = dict(base=2 ** 32 - 40, serials=(2 ** 32 - 2, 2 ** 35 - 5))
CANON = R.canonical_deck_values()


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def spec_decks(N, base, serials):
    """u8 [T, 5 + 2 N]: the deck the spec deals table t at hand serial serials[t]"""
    k = 5 + 2 * N
    return np.array([[CANON[i] for i in R.deck_permutation(SEED, (base + t) % 2 ** 32, int(serials[t]), k)[:k]] for t in range(T)], np.uint8)


def check(g, N, base, where, at_least=None):
    hs = np.asarray(g.hand_serial, np.uint64)
    assert (hs >= 1).all(), where
    if at_least is not None:                                # the run is about deals that happened inside it
        assert (hs > at_least).sum() >= T // 2, (where, "tables that dealt again", int((hs > at_least).sum()))
    got, want = np.asarray(g.deck), spec_decks(N, base, hs - np.uint64(1))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (where, bad[:4].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist(), hs[bad[:4]].tolist())
    return hs


def game(PK, N, base=0, serials=None):
    g = PK.VecGame(T, num_players=N, seed=SEED, table_id_base=base)
    assert g.wave_shape[0] == 64
    if serials is not None:
        g.set_serials(*serials)
    g.reset()
    return g


def run_reset_fused_single(PK, N, base, serials, where):
    g = game(PK, N, base, serials)
    try:
        hs0 = check(g, N, base, where + " after reset()")
        if serials is not None:
            assert (hs0 == serials[0] + 1).all(), where
        c = g.rollout(K_STEPS, policy=0, auto_reset=True, fused=True)
        assert c["steps"] == T * K_STEPS, where
        hs1 = check(g, N, base, where + " after %d fused steps" % K_STEPS, at_least=hs0)
        g.set_coalesce(0)
        for _ in range(K_STEPS):
            g.rollout(1, policy=0, auto_reset=True, fused=True)
        hs2 = check(g, N, base, where + " after %d launches of one step" % K_STEPS, at_least=hs1)
        if serials is not None:                             # the case is about the crossing
            assert (hs2 > 2 ** 32).sum() >= T // 2, (where, "tables that dealt hand serial 2^32")
    finally:
        g.close()


@pytest.mark.parametrize("N", SEATS)
def test_decks_after_reset_fused_and_single_step_launches(PK, monkeypatch, N):
    monkeypatch.setenv("PK_TPB", "64")                      # full-width waves: a small batch would otherwise be spread one table per wave
    monkeypatch.setenv("PK_ROLLOUT_TAB", "1")
    run_reset_fused_single(PK, N, 0, None, "N=%d" % N)


@pytest.mark.parametrize("N", SEATS)
def test_decks_of_resumed_streams_and_wrapping_table_ids(PK, monkeypatch, N):
    monkeypatch.setenv("PK_TPB", "64")
    monkeypatch.setenv("PK_ROLLOUT_TAB", "1")
    run_reset_fused_single(PK, N, RESUMED["base"], RESUMED["serials"], "N=%d resumed" % N)


@pytest.mark.parametrize("N", SEATS)
def test_decks_after_game_steps(PK, monkeypatch, N):
    """k_step's end_block (the whole side-pot loop per call, a lone table's stock of decks dealt ahead) deals through the same decode"""
    monkeypatch.setenv("PK_TPB", "64")
    g = game(PK, N)
    try:
        hs0 = np.asarray(g.hand_serial, np.uint64)
        for _ in range(K_STEPS):
            over = g.step(g.pick_actions(0), strict=False)[0]
            if over.any():
                g.reset(mask=over.astype(np.uint8))
        check(g, N, 0, "N=%d after %d Game.steps" % (N, K_STEPS), at_least=hs0)
    finally:
        g.close()
