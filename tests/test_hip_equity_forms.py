"""GPU tests of what the four call forms of the equity family share (pk_X_d, pk_X, pk_table_X_d, pk_table_X for the seven spot families;
pk_api.hip writes each form once): with no spot a call returns PK_OK and writes nothing, a call that asks only for the outputs it must
(status; EV: status and ev) gives those byte for byte as the call that asks for all of them, and the table forms refuse bad arguments of a
live handle with the texts they always had.  What the forms compute is pinned per family by tests/test_hip_equity*.py, test_hip_rvr.py and
test_hip_hist.py (all four forms against the spec and each other; test_hip_equity.py::test_repeatable_and_stream_forms_agree also asks
pk_equity_d for `share` alone)."""
import numpy as np
import pytest

import equity_spec as ES

pytestmark = pytest.mark.gpu
H = 1326                       # holdings
NBINS, SAMPLES = 4, 64
PATTERN = 0xA5
# family -> (outputs in ABI order as (name, bytes per spot), the outputs a call must ask for); N: seats
FAMILIES = {
    "equity": (lambda N: [("win", 4 * N), ("tie", 4 * N), ("share", 8 * N), ("boards", 4), ("status", 1)], ("status",)),
    "equity_ev": (lambda N: [("share", 8 * N * N), ("level_seat", N), ("amount", 8 * N), ("ev", 8 * N), ("boards", 4), ("status", 1)], ("ev", "status")),
    "equity_sampled": (lambda N: [("win", 4 * N), ("tie", 4 * N), ("share", 8 * N), ("samples", 4), ("status", 1)], ("status",)),
    "equity_ranged": (lambda N: [("win", 4 * N), ("tie", 4 * N), ("share", 8 * N), ("accepted", 4), ("status", 1)], ("status",)),
    "equity_range": (lambda N: [("agg", 24), ("win", 4 * H), ("tie", 4 * H), ("boards", 4), ("status", 1)], ("status",)),
    "equity_rvr": (lambda N: [("win", 8 * H), ("tie", 8 * H), ("tot", 8 * H), ("boards", 4), ("status", 1)], ("status",)),
    "equity_hist": (lambda N: [("hist", 2 * H * NBINS), ("void", 2 * H), ("completions", 4), ("status", 1)], ("status",)),
}
FORMS = ("d", "host", "table_d", "table")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def middle(family, table, p):
    """The arguments between m and the outputs.  p: name -> pointer of an explicit form's input arrays (host or device)."""
    if table:
        return {"equity": [], "equity_ev": [], "equity_sampled": [0, SAMPLES, 5], "equity_ranged": [0, SAMPLES, 5, None, 0, None, 0],
                "equity_range": [0, None, 0], "equity_rvr": [None, 0], "equity_hist": [None, 0, NBINS]}[family]
    spots = [p["holes"], p["board"], p["nboard"], p["live"]]
    return {"equity": spots, "equity_ev": spots + [p["bets"]], "equity_sampled": spots + [None, SAMPLES, 7, 5],
            "equity_ranged": spots + [None, SAMPLES, 7, 5, None, 0, None], "equity_range": [p["hero"], p["board"], p["nboard"], None, None, 0],
            "equity_rvr": [p["board"], p["nboard"], None, None, 0], "equity_hist": [p["board"], p["nboard"], None, None, 0, NBINS]}[family]


class Caller:
    """One handle of 4 tables at n seats -- tables 0 and 1 on the turn, 2 and 3 on the river, nobody folded -- and the same spots as explicit
    arrays; call() runs one form of one family on `m` of them with the wanted outputs pre-filled with PATTERN and returns their bytes."""

    def __init__(self, PK, n):
        from pokerl_amd import _lib, hipmem
        self.L, self.hipmem, self.n = _lib, hipmem, n
        self.g = g = PK.VecGame(4, num_players=n, seed=40 + n)
        g.reset()
        turn_blob = None
        for _ in range(8 * n):                                               # everybody calls or checks: the tables move in lockstep
            if turn_blob is None and (g.turn == 2).all():
                turn_blob = g.save([0, 1])
            if (g.turn == 3).all():
                break
            g.step(g.pick_actions(policy=2))
        g.load(turn_blob, [0, 1])
        assert g.turn.tolist() == [2, 2, 3, 3]
        self.tables = np.array([3, 0, 2], np.int32)
        holes, board, nboard, live = ES.table_spots(g.deck, g.player_states, g.turn)
        assert (live == (1 << n) - 1).all()
        t = self.tables
        self.inputs = dict(holes=holes[t], board=board[t], nboard=nboard[t], live=live[t], bets=np.full((3, n), 10.0), hero=holes[t][:, 0])
        self.inputs = {k: np.ascontiguousarray(v) for k, v in self.inputs.items()}
        self.inputs_d = {k: hipmem.DeviceBuffer(v.nbytes).upload(v) for k, v in self.inputs.items()}
        self.tables_d = hipmem.DeviceBuffer(t.nbytes).upload(t)

    def close(self):
        for b in list(self.inputs_d.values()) + [self.tables_d]:
            b.free()
        self.g.close()

    def call(self, family, form, m, wanted):
        L, n = self.L, self.n
        outputs = FAMILIES[family][0](n)
        table, device = form.startswith("table"), form.endswith("d")
        host = {name: np.full(max(m, 1) * size, PATTERN, np.uint8) for name, size in outputs if name in wanted}
        dev = {name: self.hipmem.DeviceBuffer(a.nbytes).upload(a) for name, a in host.items()} if device else {}
        outs = [(dev[name].ptr if device else L.ptr(host[name])) if name in wanted else None for name, _ in outputs]
        fn = getattr(L.lib(), "pk_%s%s%s" % ("table_" if table else "", family, "_d" if device else ""))
        if table:
            head = [self.g._h, self.tables_d.ptr if device else L.ptr(self.tables), m]
        else:
            head = [0] + ([n] if family in ("equity", "equity_ev", "equity_sampled", "equity_ranged") else []) + [m]
        p = {k: b.ptr for k, b in self.inputs_d.items()} if device else {k: L.ptr(a) for k, a in self.inputs.items()}
        L.check(fn(*head, *middle(family, table, p), *outs, *([None] if device and not table else [])), self.g._h if table else None)
        if device:
            self.g.sync()                                                    # (the handle's stream; an explicit call ran on the NULL stream, which the copy below follows)
            for name, b in dev.items():
                host[name] = b.download(np.uint8, b.nbytes)
                b.free()
        return host


@pytest.fixture(scope="module", params=[2, 3])
def caller(PK, request):
    c = Caller(PK, request.param)
    yield c
    c.close()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_no_spot_is_ok_and_writes_nothing(caller, family):
    names = [name for name, _ in FAMILIES[family][0](caller.n)]
    for form in FORMS:
        got = caller.call(family, form, 0, names)
        assert all((a == PATTERN).all() for a in got.values()), (family, form)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_required_outputs_alone_equal_the_full_call(caller, family):
    outputs, required = FAMILIES[family]
    names = [name for name, _ in outputs(caller.n)]
    for form in FORMS:
        full = caller.call(family, form, 3, names)
        assert not full["status"].any(), (family, form, full["status"].tolist())
        assert all((a != PATTERN).any() for a in full.values()), (family, form)      # (every output was written)
        alone = caller.call(family, form, 3, required)
        assert sorted(alone) == sorted(required)
        for name in required:
            assert alone[name].tobytes() == full[name].tobytes(), (family, form, name)


def test_table_forms_refuse_with_their_texts(caller):
    """The argument checks of the table forms on a live handle, in the order they are made (they need a handle, so no CPU test sees them)."""
    L, g = caller.L, caller.g
    lib, h, N = L.lib(), g._h, caller.n
    one = np.zeros(64, np.uint8)
    p = L.ptr(one)
    for d in ("_d", ""):
        def refused(family, middle_args, outs, text):
            name = "pk_table_%s%s" % (family, d)
            assert getattr(lib, name)(h, None, middle_args[0], *middle_args[1:], *outs) == L.PK_E_INVALID_ARG, name
            assert lib.pk_last_error(h).decode() == name + text, name
        big = 2 ** 31
        refused("equity", [big], [None] * 5, ": m >= 2^31")
        refused("equity", [2 ** 31 - 1], [None] * 5, ": too many spots for one call (the worst-case task count must fit 32 bits: split the batch)")
        refused("equity_ev", [big], [None] * 6, ": m >= 2^31")
        refused("equity_ev", [1], [None] * 6, ": NULL status")
        refused("equity_ev", [2 ** 31 - 1], [None] * 5 + [p], ": too many spots for one call (the worst-case task count must fit 32 bits: split the batch)")
        refused("equity_sampled", [big, 0, 64, 0], [None] * 5, ": m >= 2^31")
        for samples in (0, 2 ** 24 + 1):
            refused("equity_sampled", [1, 0, samples, 0], [None] * 5, ": samples outside 1 .. 2^24")
        for observer in (-3, N):
            refused("equity_sampled", [1, observer, 64, 0], [None] * 5, ": observer outside {-2, -1, 0 .. N-1}")
        refused("equity_sampled", [2 ** 14, 0, 2 ** 24, 0], [None] * 5, ": m * ceil(samples / 64) must fit 32 bits: split the batch")
        refused("equity_ranged", [big, 0, 64, 0, None, 0, None, 0], [None] * 5, ": m >= 2^31")
        refused("equity_ranged", [1, 0, 0, 0, None, 0, None, 0], [None] * 5, ": samples outside 1 .. 2^24")
        for observer in (-1, -3, N):
            refused("equity_ranged", [1, observer, 64, 0, None, 0, None, 0], [None] * 5,
                    ": observer outside {-2, 0 .. N-1} (PK_OBSERVER_NONE: nothing would be hidden)")
        refused("equity_ranged", [1, 0, 64, 0, p, 17, None, 0], [None] * 5, ": num_ranges above PK_EQW_MAX_RANGES (16)")
        refused("equity_ranged", [1, 0, 64, 0, None, 2, None, 0], [None] * 5, ": NULL weights with num_ranges > 0")
        refused("equity_ranged", [2 ** 14, 0, 2 ** 24, 0, None, 0, None, 0], [None] * 5, ": m * ceil(samples / 64) must fit 32 bits: split the batch")
        refused("equity_range", [big, 0, None, 0], [None] * 5, ": m >= 2^31")
        for observer in (-1, -3, N):
            refused("equity_range", [1, observer, None, 0], [None] * 5, ": observer outside {-2, 0 .. N-1} (a hidden hand needs somebody to be hidden from)")
        refused("equity_rvr", [big, None, 0], [None] * 5, ": m >= 2^31")
        refused("equity_hist", [big, None, 0, 4], [None] * 4, ": m >= 2^31")
        for nbins in (0, 33):
            refused("equity_hist", [1, None, 0, nbins], [None] * 4, ": nbins must be 1 .. PK_EQ_HIST_MAX_BINS (32)")
