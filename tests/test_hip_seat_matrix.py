"""Every table-kernel family at every seat count 2 .. 16 (one template instantiation of pk_tables.hip each) against the CPU oracle, through
the shared drivers of tests/seat_matrix.py: one case per (seat count, family, wave shape), so a failure names the instantiation and the shape.

Wave shapes (seat_matrix.WAVE_SHAPES): pk_create spreads a small batch over the chip -- 64 tables per wave halved while the batch fits 1 024
waves of half as many -- so the matrix's 165 tables run ONE table per wave (`spread`: 63 dead lanes, no cross-lane code sees two live lanes)
unless PK_TPB says otherwise.  `full` (PK_TPB=64) makes them two full wavefronts and a ragged one of 37 lanes; `part` (PK_TPB=8) twenty
waves of 8 live lanes and one of 5, the other lanes dead inside the wave -- what a caller between 1 025 and 32 768 tables gets.  Every driver
asserts VecGame.wave_shape on every handle it makes, so a case cannot silently run narrow.  The ids of the `spread` cases are the ones the
matrix had before it knew shapes ("N-family"); every other id ends in its shape.

Batches: 165 tables, one table for the step and env families (under `spread` only: it is the same launch under any shape), 197 tables in
two sub-batches.  Configurations per case: default, ladder (N-way showdowns with up to N - 1 side-pot levels) and top_seat (table ids that
wrap inside the batch, seat N - 1 wherever the family takes a seat) -- seat_matrix.matrix_config; tests/test_seat_matrix_host.py shows on the
CPU that each of them contains what it is there for and stays below the caps.  A fourth configuration, resumed (RNG streams resumed so that
hand_serial and the action-block index step_serial >> 3 both cross 2^32 inside the run), has cases of its own: full waves (plus the lone
table of game_step and env_step, whose deals come from a stock of four decks) at 2, 6, 9, 13 and 16 seats.  A fifth, deep (the never-fold
caller of oracle/rng_spec.py on per-seat fractional stacks: raises on every street, all-ins on different streets, multi-way river
showdowns that pay several amounts; the device is handed the oracle's actions), runs every family at every seat count on full waves,
game_step and env_step also under `spread` and `part` at 2, 6, 9, 13 and 16 seats, and rollout_from_deep: the call agents' fused rollout
finishing such hands."""
import pytest

import seat_matrix as M

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def HB():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    from hip_backend import HipBackend
    return HipBackend


def game_step(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        K = M.k_of("game_step", kind, N)
        for T in (M.T_MATRIX, 1) if shape == "spread" or kind == M.RESUMED else (M.T_MATRIX,):
            st = M.game_step(HB, M.matrix_config(kind, N, T, shape), K)
            assert st["rows"] == 3 * T * K and st["views"] == 6 * T * K, (kind, T, st)


def game_step_async(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        K = M.k_of("game_step_async", kind, N)
        for T, budget in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[-1])] * (shape == "spread"):
            st = M.game_step_async(HB, M.matrix_config(kind, N, T, shape), K, max_hands=budget)
            # (the pre-flight shows that no matrix configuration meets game.py:473, so the twin runs to the drain and its state is compared)
            assert st["drained"] and st["async_steps"] > 0 and st["rows"] == st["async_steps"], (kind, T, budget, st)


def env_opps(kind, N):
    """The opponents' policy of the env families, one run each.  deep: call agents (every hand an N-way river showdown raised on every
    street), and random agents up to six seats (more of them fold too often to see late streets)."""
    return {"ladder": (1,), M.DEEP: (2, 0) if N <= 6 else (2,)}.get(kind, (0,))


def env_step(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        K = M.k_of("env_step", kind, N)
        for opp in env_opps(kind, N):
            for T, passes in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[-1])] * (shape == "spread" or kind == M.RESUMED):
                st = M.env_step(M.env_config(kind, N, T, shape), opp, K, passes)
                assert st["delivered"] == T * K, (kind, T, st)


def env_batches(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        K = M.k_of("env_step", kind, N)
        for opp in env_opps(kind, N):
            st = M.env_step(M.env_config(kind, N, M.T_BATCHES, shape), opp, K, 3, B=2)
            assert st["sub"] == 1 and st["delivered"] == M.T_BATCHES * K, (kind, st)


def env_multi(HB, N, shape="spread", kinds=M.KINDS):
    if kinds == (M.DEEP,):
        for mixed in (False, True):             # every seat played by the caller by the deep rule; then in-kernel call agents among them
            for T, passes in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[0])] * (shape == "spread"):
                cfg = M.matrix_config(M.DEEP, N, T, shape)
                pols, external = M.deep_multi_seats(N, mixed)
                st = M.env_multi(cfg, pols, external, M.K_MULTI, passes)
                assert st["delivered"] == T * M.K_MULTI and (not external or st["yields"] > 0), (mixed, T, st)
        return
    for kind in kinds:
        for T, passes in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[0])] * (shape == "spread"):
            cfg = M.matrix_config(kind, N, T, shape)
            pols, external = M.multi_seats(cfg)
            st = M.env_multi(cfg, pols, external, M.K_MULTI, passes)
            assert st["delivered"] == T * M.K_MULTI, (kind, T, st)
            if kind == "top_seat" and T > 1:
                assert st["yields_by_seat"][N - 1] > 0, (kind, st)       # the top nibble was played by the caller
    cfg = M.matrix_config("top_seat", N, shape=shape)
    M.env_in_kernel_seats(cfg, M.in_kernel_seats(cfg), M.K_MULTI)


def rollout_call(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        K = M.k_of("rollout_call", kind, N)
        c = M.rollout_call(HB, M.matrix_config(kind, N, shape=shape), K)
        assert c[0] == M.T_MATRIX * K and c[1] > 0, (kind, c)


def rollout(HB, N, shape="spread", kinds=M.KINDS):
    """The fused rollout of the configuration's own agents (random; all-in for the ladder) in deferred launches of K // 3 and K - K // 3 - 7
    steps (16 and 25 at K = 48) and a completing one of 7, then ten lockstep steps.  Launches of at least 16 steps are k_rollout_tab up to six
    seats and k_rollout_allin_tab up to ten; k_rollout / k_rollout_allin beyond."""
    for kind in kinds:
        K = M.k_of("rollout", kind, N)
        assert K >= 48 and K // 3 >= 16 and K - K // 3 - 7 >= 16
        assert M.rollout_then_lockstep(HB, M.matrix_config(kind, N, shape=shape), K, lock=10, split=True) == M.T_MATRIX * (K + 10)


def rollout_from_deep(HB, N, shape="spread", kinds=(M.DEEP,)):
    """K_DEEP lockstep steps of the deep caller, then the call agents' fused rollout (launches of 16, 25 and 7 steps) finishes the hands."""
    for kind in kinds:
        deep_tables, c = M.rollout_from_deep(HB, M.matrix_config(kind, N, shape=shape), M.k_of("played", kind, N))
        assert deep_tables > 0 or N == 2, (kind, deep_tables)
        assert c[0] == M.T_MATRIX * M.K_ROLLOUT and c[1] > 0 and c[2] > 0, (kind, c)


def played_k(kind, N):
    return M.k_of("played", kind, N) if kind == M.DEEP else M.K_PLAYED


def snapshots(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        M.snapshots(HB, M.matrix_config(kind, N, shape=shape), played_k(kind, N), extra_call=M.extra_call(kind, N), observer=N - 1 if kind == "top_seat" else "active")


def equity(HB, N, shape="spread", kinds=M.KINDS):
    for kind in kinds:
        st = M.equity(HB, M.matrix_config(kind, N, shape=shape), played_k(kind, N), extra_call=M.extra_call(kind, N),
                      observer={"default": -2, "ladder": -1, "top_seat": N - 1, M.DEEP: -2}[kind])
        assert st["tables"] == M.EQUITY_FIRST and st["samples"] == 65 * M.EQUITY_FIRST, (kind, st)


FAMILIES = [game_step, game_step_async, env_step, env_batches, env_multi, rollout_call, snapshots, equity]
PART_FAMILIES = [rollout, game_step, env_step]
RESUMED_FAMILIES = [rollout, rollout_call, game_step, game_step_async, env_step]
DEEP_FAMILIES = [game_step, game_step_async, env_step, env_batches, env_multi, rollout_from_deep, snapshots, equity]
DEEP_SHAPE_FAMILIES = [game_step, env_step]


def _cases():
    """(id, N, family, shape, configurations), by seat count as before."""
    for N in M.SEATS:
        for f in FAMILIES:
            yield "%d-%s" % (N, f.__name__), N, f, "spread", M.KINDS
        yield "%d-rollout-spread" % N, N, rollout, "spread", M.KINDS
        for f in FAMILIES + [rollout]:
            yield "%d-%s-full" % (N, f.__name__), N, f, "full", M.KINDS
        for f in PART_FAMILIES:
            yield "%d-%s-part" % (N, f.__name__), N, f, "part", M.KINDS
        if N in M.RESUMED_SEATS:
            for f in RESUMED_FAMILIES:
                yield "%d-%s-full-resumed" % (N, f.__name__), N, f, "full", (M.RESUMED,)
        for f in DEEP_FAMILIES:
            yield "%d-%s-full-deep" % (N, f.__name__), N, f, "full", (M.DEEP,)
        if N in M.DEEP_SHAPE_SEATS:
            for shape in ("spread", "part"):
                for f in DEEP_SHAPE_FAMILIES:
                    yield "%d-%s-%s-deep" % (N, f.__name__, shape), N, f, shape, (M.DEEP,)


CASES = list(_cases())


@pytest.mark.parametrize("N,family,shape,kinds", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_family_at_every_seat_count(HB, monkeypatch, N, family, shape, kinds):
    M.use_shape(monkeypatch, shape)
    family(HB, N, shape, kinds)


def test_wave_shape_accessor(HB, monkeypatch):
    """pk_get_wave_shape / VecGame.wave_shape: pk_create's rule without a knob, PK_TPB and PK_ENV_TPB with one (the env kernels follow
    PK_TPB unless PK_ENV_TPB names a power of two), NULL arguments refused with the outputs untouched."""
    import ctypes as C
    from pokerl_amd import _lib as L
    for tpb, env_tpb, T, want in ((None, None, 1025, (2, 2)), (None, None, 1024, (1, 1)), ("64", None, 5, (64, 64)), ("8", "4", 165, (8, 4)), ("8", "3", 165, (8, 8)),
                                  (None, "16", 165, (1, 16))):
        for name, v in (("PK_TPB", tpb), ("PK_ENV_TPB", env_tpb)):
            monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, v)
        h = HB(T, 3)
        assert h.g.wave_shape == want and h.env.game.wave_shape == want, (tpb, env_tpb, T, h.g.wave_shape, want)
        a = C.c_int(-7)
        for args in ((h.g._h, None, C.byref(a)), (h.g._h, C.byref(a), None), (None, C.byref(a), C.byref(a))):
            assert L.lib().pk_get_wave_shape(*args) == L.PK_E_INVALID_ARG and a.value == -7, args
        h.g.close()
