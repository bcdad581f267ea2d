"""Every table-kernel family at every seat count 2 .. 16 (one template instantiation of pk_tables.hip each) against the CPU oracle, through
the shared drivers of tests/seat_matrix.py: one case per (seat count, family), so a failure names the instantiation.

Shapes: 165 tables (two full wavefronts and a ragged one of 37 lanes), one table for the step and env families, 197 tables in two
sub-batches.  Configurations per case: default, ladder (N-way showdowns with up to N - 1 side-pot levels) and top_seat (table ids that
wrap inside the batch, seat N - 1 wherever the family takes a seat) -- seat_matrix.matrix_config; tests/test_seat_matrix_host.py shows on the
CPU that each of them contains what it is there for and stays below the caps."""
import pytest

import seat_matrix as M

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def HB():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    from hip_backend import HipBackend
    return HipBackend


def game_step(HB, N):
    for kind in M.KINDS:
        for T in (M.T_MATRIX, 1):
            st = M.game_step(HB, M.matrix_config(kind, N, T), M.K_GAME)
            assert st["rows"] == 3 * T * M.K_GAME and st["views"] == 6 * T * M.K_GAME, (kind, T, st)


def game_step_async(HB, N):
    for kind in M.KINDS:
        for T, budget in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[-1])]:
            st = M.game_step_async(HB, M.matrix_config(kind, N, T), M.K_GAME, max_hands=budget)
            # (the pre-flight shows that no matrix configuration meets game.py:473, so the twin runs to the drain and its state is compared)
            assert st["drained"] and st["async_steps"] > 0 and st["rows"] == st["async_steps"], (kind, T, budget, st)


def env_step(HB, N):
    for kind in M.KINDS:
        opp = 1 if kind == "ladder" else 0
        for T, passes in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[-1])]:
            st = M.env_step(M.matrix_config(kind, N, T), opp, M.K_ENV, passes)
            assert st["delivered"] == T * M.K_ENV, (kind, T, st)


def env_batches(HB, N):
    for kind in M.KINDS:
        st = M.env_step(M.matrix_config(kind, N, M.T_BATCHES), 1 if kind == "ladder" else 0, M.K_ENV, 3, B=2)
        assert st["sub"] == 1 and st["delivered"] == M.T_BATCHES * M.K_ENV, (kind, st)


def env_multi(HB, N):
    for kind in M.KINDS:
        for T, passes in [(M.T_MATRIX, b) for b in M.BUDGETS] + [(1, M.BUDGETS[0])]:
            cfg = M.matrix_config(kind, N, T)
            pols, external = M.multi_seats(cfg)
            st = M.env_multi(cfg, pols, external, M.K_MULTI, passes)
            assert st["delivered"] == T * M.K_MULTI, (kind, T, st)
            if kind == "top_seat" and T > 1:
                assert st["yields_by_seat"][N - 1] > 0, (kind, st)       # the top nibble was played by the caller
    cfg = M.matrix_config("top_seat", N)
    M.env_in_kernel_seats(cfg, M.in_kernel_seats(cfg), M.K_MULTI)


def rollout_call(HB, N):
    for kind in M.KINDS:
        c = M.rollout_call(HB, M.matrix_config(kind, N), M.k_call(N))
        assert c[0] == M.T_MATRIX * M.k_call(N) and c[1] > 0, (kind, c)


def snapshots(HB, N):
    for kind in M.KINDS:
        M.snapshots(HB, M.matrix_config(kind, N), M.K_PLAYED, extra_call=M.extra_call(kind, N), observer=N - 1 if kind == "top_seat" else "active")


def equity(HB, N):
    for kind in M.KINDS:
        st = M.equity(HB, M.matrix_config(kind, N), M.K_PLAYED, extra_call=M.extra_call(kind, N),
                      observer={"default": -2, "ladder": -1, "top_seat": N - 1}[kind])
        assert st["tables"] == M.EQUITY_FIRST and st["samples"] == 65 * M.EQUITY_FIRST, (kind, st)


FAMILIES = [game_step, game_step_async, env_step, env_batches, env_multi, rollout_call, snapshots, equity]


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("N", M.SEATS)
def test_family_at_every_seat_count(HB, N, family):
    family(HB, N)
