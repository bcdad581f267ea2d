"""The equity seat matrix on the GPU: every seat-templated equity kernel -- k_equity<N>, k_eqs<N>, k_eqw<N, RC>, k_ev<N> with k_ev_prep<N, TABLE>,
k_evw<N> with its prep kernel -- and the table forms of the five at every seat count 2 .. 16, through the host forms of pokerl_amd.judger
and of VecGame, every output against the numpy restatements of the definitions: integers equal, every f64 byte for byte.  The cases and
their comparisons live in tests/equity_seat_matrix.py (one copy); tests/test_equity_seat_matrix_host.py holds their inputs, on the CPU, to
what they are there for.  At five seat counts (the word edges of the packed range rows, both level groupings) the device forms run once
more on a caller's non-blocking stream and must give the host forms' bytes.
Measured on the MI355X, first run: 2.6 s for the module's 90 cases, specs included (the slowest case 0.16 s; a table-forms case 0.04 - 0.09 s)."""
import pytest

import equity_seat_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def spot_family(family, N):
    want = M.want(family, N)
    got = M.device_host(family, N)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        M.assert_same(family, g, w, M.where_of(family, N, "host form v spec, call %d" % k))
    if family in ("equity", "ev"):
        M.assert_royal(family, N, got[0], M.where_of(family, N, "host form"))
    if N in M.STREAM_SEATS:
        for k, (s, g) in enumerate(zip(M.device_stream(family, N), got)):
            M.assert_same_bytes(family, s, g, M.where_of(family, N, "device form on a caller's stream v host form, call %d" % k))


def table_forms(N):
    b = M.table_backend(N)
    g = b.g
    snap = M.table_state(b)
    assert sorted(set(snap["turn"].tolist())) == [1, 2, 3] and ((snap["states"] == 0).any() or N == 2), M.where_of("table_forms", N, "the table state")
    before = g.save()
    want = M.table_want(N, g.deck, g.player_states, g.turn, g.active_player, g.bets, g.pending_bets)
    got = M.table_device(g, N)
    assert sorted(got) == sorted(want) == sorted(M.TABLE_PARTS)
    for name, fam in M.TABLE_PARTS.items():
        assert not got[name]["status"].any(), M.where_of("table_forms", N, name)
        M.assert_same(fam, got[name], want[name], M.where_of("table_forms", N, "%s v spec fed from the getters" % name))
    if N in M.STREAM_SEATS:
        on_stream = M.table_device_stream(g, N)
        for name, fam in M.TABLE_PARTS.items():
            M.assert_same_bytes(fam, on_stream[name], got[name], M.where_of("table_forms", N, "%s_d on a caller's stream v host form" % name))
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    g.close()


@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("N", M.SEATS)
def test_equity_seat_matrix(PK, N, family):
    if family == "table_forms":
        table_forms(N)
    else:
        spot_family(family, N)
