"""Operand tables for the solvers' strategy rule and the rule itself in Python integers (TEST INFRASTRUCTURE): include/pokerl_hip.h
"River solver", STRATEGY FROM NON-NEGATIVE INTEGERS.  rule_exact shares nothing with the numpy restatements.  table(kind, nact) is a seeded
list of operand tuples as a caller would hand them over (values below 0 and above the clamp among them); clamp() is what the LOAD paragraph
of "Resuming a solve" does first; check_table() states what a table must contain; pack() lays tuples into state arrays, one tuple per
(row, holding) or per (row, river card, holding), and says where each one went.  No GPU, no kernel."""
import random

ONE = 32768
H = 1326
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TOP = {"river_A": 44, "river_R": 58, "turn_A": 41, "turn_R": 60}      # the clamp of each range: 2^TOP - 1
KINDS = tuple(TOP)


def rule_exact(X):
    """the strategy rule on a list of non-negative Python integers -> a list of probabilities in Q15 summing to ONE"""
    nact, mx = len(X), max(X)
    if mx == 0:
        sig = [ONE // nact] * nact
    else:
        sh = max(0, mx.bit_length() - 31)
        S = sum(x >> sh for x in X)
        sig = [((x >> sh) << 15) // S for x in X]
    sig[0] = ONE - sum(sig[1:])
    return sig


def lim_of(kind):
    return (1 << TOP[kind]) - 1


def clamp(X, kind):
    lim = lim_of(kind)
    return tuple(min(max(int(x), 0), lim) for x in X)


def shift_of(mx):
    return max(0, mx.bit_length() - 31)


def _inverse_pow15(S):
    return pow(1 << 15, -1, S)


def remainder_tuple(rng, nact, sh, want):
    """A seeded search for a tuple whose shifted entry x at some slot a >= 1 has (x << 15) mod S == want(S), S the sum of the shifted entries,
    the largest entry of bit length 31 + sh.  want: "zero", "one" or "last" (S - 1).  -> (tuple, a)"""
    while True:
        rest = [rng.randrange(0, 1 << 29) for _ in range(nact - 2)]
        S = rng.randrange(1 << 30, 1 << 32) | 1                     # odd: 2^15 has an inverse
        if want == "zero":
            S &= ~((1 << 15) - 1)
            x = (S >> 15) * rng.randrange(1, (1 << 14) + 1)         # x 2^15 a multiple of S
        else:
            x = (_inverse_pow15(S) * (1 if want == "one" else S - 1)) % S
        mx = S - x - sum(rest)
        if not (1 << 30) <= mx < (1 << 31) or x > mx or any(c > mx for c in rest) or x == 0:
            continue
        low = lambda: rng.randrange(0, 1 << sh)
        a = rng.randrange(1, nact)
        slots = [s for s in range(nact) if s != a]
        rng.shuffle(slots)
        X = [0] * nact
        X[a] = (x << sh) | low()
        X[slots[0]] = (mx << sh) | low()
        for s, c in zip(slots[1:], rest):
            X[s] = (c << sh) | low()
        assert shift_of(max(X)) == sh and ((X[a] >> sh) << 15) % sum(v >> sh for v in X) == {"zero": 0, "one": 1, "last": S - 1}[want]
        return tuple(X), a


def remainder_shifts(kind):
    top = TOP[kind]
    return (0, 1, 7, top - 31)


def table(kind, nact, seed=0x517A):
    """The operand tuples of one range and action count, raw (before the clamp), in a fixed order."""
    rng = random.Random("%s/%d/%d" % (kind, nact, seed))
    top, lim = TOP[kind], lim_of(kind)
    out = [(0,) * nact, (lim,) * nact, (1,) * nact]
    for k in range(30, top + 1):
        for mx in ((1 << k) - 1, 1 << k, (1 << k) + 1):              # (k = top: the last two lie above the clamp and come down to it)
            sh = shift_of(min(mx, lim))
            out.append((mx,) * nact)                                 # all equal at the largest value
            if nact == 1:
                continue
            for comp in (mx, mx - 1, 0, 1, (1 << sh) - 1, 1 << sh):
                at = rng.randrange(nact)
                X = [comp if nact == 2 else rng.choice((comp, comp, 0, 1, mx - 1, rng.randrange(0, mx + 1), (1 << sh) - 1)) for _ in range(nact)]
                X[(at + 1) % nact] = comp
                X[at] = mx
                out.append(tuple(X))
                if nact == 2:
                    out.append((X[1], X[0]))
    for sh in range(0, top - 30):                                    # all equal at the largest SHIFTED value: S = nact (2^31 - 1)
        out.append(((((1 << 31) - 1) << sh) | ((1 << sh) - 1),) * nact)
    if nact >= 2:
        for sh in remainder_shifts(kind):
            for want in ("zero", "one", "last"):
                out.append(remainder_tuple(rng, nact, sh, want)[0])
        for _ in range(40):                                          # plain seeded tuples of every size
            k = rng.randrange(1, top + 1)
            out.append(tuple(rng.randrange(0, 1 << rng.randrange(1, k + 1)) for _ in range(nact)))
    # the clamps act first: values below 0 and above the clamp, both ends of int64 among them
    wild = (I64_MIN, I64_MAX, -1, lim + 1, lim + 2, 1 << 62, -(1 << 40), lim, 0, 1, 12345, lim - 1)
    for j in range(24):
        X = [rng.choice(wild) for _ in range(nact)]
        X[j % nact] = wild[j % 6]
        out.append(tuple(X))
    assert all(len(X) == nact and all(I64_MIN <= x <= I64_MAX for x in X) for X in out)
    return out


def check_table(kind, nact, tab=None):
    """the conditions a table must meet, on the table itself (AssertionError names the one that is not)"""
    top, lim = TOP[kind], lim_of(kind)
    raw = table(kind, nact) if tab is None else tab
    tab = [clamp(X, kind) for X in raw]
    tops = {max(X) for X in tab}
    for k in range(30, top + 1):
        for mx in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            assert mx > lim or mx in tops, ("the largest entry", k, mx)
    assert {shift_of(max(X)) for X in tab} >= set(range(0, top - 30)), "every shift"
    assert (0,) * nact in tab, "the all-zero tuple"
    assert any(len(set(X)) == 1 and X[0] == lim for X in tab), "all entries at the clamp"
    for sh in range(0, top - 30):
        assert any(len(set(X)) == 1 and shift_of(X[0]) == sh and X[0] >> sh == (1 << 31) - 1 for X in tab), ("S = nact (2^31 - 1)", sh)
    assert any(min(X) < 0 for X in raw) and any(max(X) > lim for X in raw) and any(I64_MIN in X for X in raw) and any(I64_MAX in X for X in raw), "beyond the clamps"
    if nact == 1:
        return len(raw)
    for sh in range(0, top - 30):
        comp = {c for X in tab if shift_of(max(X)) == sh for i, c in enumerate(X) if i != X.index(max(X))}
        mxs = {max(X) for X in tab if shift_of(max(X)) == sh}
        assert any(m in comp for m in mxs) and any(m - 1 in comp for m in mxs) and {0, 1} <= comp, ("companions", sh)
        assert (1 << sh) - 1 in comp and (1 << sh) in comp, ("erased by the shift / kept by it", sh)
    seen = {}
    for X in tab:
        sh = shift_of(max(X))
        S = sum(x >> sh for x in X)
        for x in X[1:]:
            if S and 0 < x >> sh < S:
                r = ((x >> sh) << 15) % S
                for name, v in (("zero", 0), ("one", 1), ("last", S - 1)):
                    if r == v:
                        seen.setdefault(name, set()).add(sh)
    assert all(len(seen.get(name, ())) >= 3 for name in ("zero", "one", "last")), ("remainders 0, 1 and S - 1 at three shifts", seen)
    return len(raw)


# ------------------------------------------------------------------------------------------------ the packer
def pack(slots, tables, m=None):
    """slots: a list of (prefix, nact, holdings) -- prefix the index tuple before [4][1326] (a row, or a row and a river card), holdings the
    indices at which the entry is read; tables: {nact: tuples}.  One tuple per (slot, holding), each nact's table laid along its own slots
    and started again when it ends; m spots (None: as many as the longest table needs).
    -> a list over the spots of {(prefix, h): tuple}, which lay() writes into arrays."""
    cap = {}
    for _, nact, hold in slots:
        cap[nact] = cap.get(nact, 0) + len(hold)
    need = max([-(-len(tables[nact]) // c) for nact, c in cap.items() if c] + [1])
    pos = {nact: 0 for nact in cap}
    spots = []
    for _ in range(need if m is None else m):
        put = {}
        for prefix, nact, hold in slots:
            tab = tables[nact]
            for h in hold:
                put[(prefix, int(h))] = tab[pos[nact] % len(tab)]
                pos[nact] += 1
        spots.append(put)
    return spots


def spots_needed(slots, tables):
    return len(pack(slots, tables))


def covered(spots, tables):
    """whether every tuple of every table was placed"""
    placed = {}
    for put in spots:
        for X in put.values():
            placed.setdefault(len(X), set()).add(X)
    return all(set(tab) <= placed.get(nact, set()) for nact, tab in tables.items())


def lay(spots, shape, fill):
    """int64 [m, *shape, 4, 1326] filled with `fill`, the packed tuples written at their places"""
    import numpy as np
    out = np.full((len(spots),) + tuple(shape) + (4, H), fill, np.int64)
    for i, put in enumerate(spots):
        for (prefix, h), X in put.items():
            for a, x in enumerate(X):
                out[(i,) + prefix + (a, h)] = x
    return out


def river_slots(tree, valid, rows=None):
    """the slots of a river tree's state (or a turn tree's turn level): row d, its node's action count, the valid holdings"""
    return [((row,), tree.num_actions(v), valid) for row, v in enumerate(tree.decision_nodes) if rows is None or row in rows]


def river_level_slots(tree, valid, pool):
    """the slots of a turn tree's river level: one per row and pool card (canonical index), the valid holdings without the card"""
    import rvr_spec as VS
    return [((row, int(c)), tree.num_actions(v), [int(h) for h in valid if VS.PAIR_A[h] != c and VS.PAIR_B[h] != c])
            for row, v in enumerate(tree.river_decision_nodes) for c in pool]


# ------------------------------------------------------------------------------------------------ the calls the tables travel in
SENTINEL = 0x5A5A5A5A5A5A5A5A                # solver_resume_util's: an entry that is not read and must survive a t0 > 0 call
FF = 0xFF


def nine_node_tree():
    """pot + put = 8191, the most the header accepts: check or bet 7190 into 1001, fold or call"""
    from pokerl_amd.solver import river_tree
    return river_tree(1001, 7190, (8.0,), 1)


def corner_turn_tree():
    from pokerl_amd.solver import turn_tree
    return turn_tree(2731, 5460, (1.0,), 1)


def tree_from(spec, pot, turn):
    """a nested (kind, (put0, put1), [children]) -> a RiverTree / TurnTree, nodes numbered breadth first (children after their parent)"""
    from pokerl_amd.solver import RiverTree, TurnTree
    nodes, child = [spec], []
    for kind, put, ch in nodes:                                    # (grows while it is walked)
        child.append([len(nodes) + j for j in range(len(ch))] + [FF] * (4 - len(ch)))
        nodes += ch
    return (TurnTree if turn else RiverTree)([k for k, _, _ in nodes], child, [list(p) for _, p, _ in nodes], pot)


def four_action_turn_tree():
    """A hand-made turn tree with every action count at both levels: a four-action root (check, bet 10, 20 or 40); behind the bet of 10 a
    three-action node (fold, call, raise to 40), behind the bet of 20 fold or call, behind the bet of 40 a forced call; after check and the
    river card the same round again, with a forced check behind the check.  Turn-level rows: 4, 3, 2, 1, 2 actions; river-level: 4, 1, 3, 2, 2, 2."""
    P0, P1, F0, F1, SD, CH = 0, 1, 2, 3, 4, 5
    sd = lambda c: (SD, (c, c), [])
    deal = lambda c: (CH, (c, c), [sd(c)])
    river = (P0, (0, 0), [(P1, (0, 0), [sd(0)]),
                          (P1, (10, 0), [(F1, (10, 0), []), sd(10), (P0, (10, 40), [(F0, (10, 40), []), sd(40)])]),
                          (P1, (20, 0), [(F1, (20, 0), []), sd(20)]),
                          (P1, (40, 0), [(F1, (40, 0), []), sd(40)])])
    root = (P0, (0, 0), [(CH, (0, 0), [river]),
                         (P1, (10, 0), [(F1, (10, 0), []), deal(10), (P0, (10, 40), [(F0, (10, 40), []), deal(40)])]),
                         (P1, (20, 0), [(F1, (20, 0), []), deal(20)]),
                         (P1, (40, 0), [deal(40)])])
    return tree_from(root, 60, True)


def one_spot(street, pool, seed):
    """(board uint8 [street], dead, valid holding indices, the pool's canonical indices) of one seeded spot"""
    import numpy as np
    import rvr_spec as VS
    import solver_resolve_util as RU
    board, _, dead = VS.random_boards(np.random.default_rng(seed), 1, street, pool)
    board = np.ascontiguousarray(board[0, :street])
    valid = np.nonzero(~RU.invalid_holdings(board, street, dead[0]))[0]
    return board, dead[0], valid, RU.pool_of(board, street, dead[0])


def rule_call(street, trees, mode, t0, pool, seed=0x51AA, spots=None):
    """The arguments of ONE resuming call that pushes the tables through the device's rule, every spot on the same seeded board.
    mode "average": iters = 0, the A tables in `average` (turn: and in river_average), regrets zero: `strategy` is the rule of the clamped
    tuple.  mode "regret": iters = 1, the R tables in `regret` (and river_regret), accumulators zero, every weight at the value that makes the
    root reach exactly ONE: the root row's `average` comes back as (t0 + 1) x the rule.  In mode "regret" the spots are as many as the ROOT
    row needs to take its whole table; the other rows take what fits.  spots: at most so many per tree (the tables are then cut short).
    -> dict(board, dead, trees, tree_of, ranges, t0, iters, state (2 or 4 arrays, resume_spec's order), where: per spot {(prefix, h): tuple}
    for the first array that carries tables, river_where: the same for the turn's river level, kind, pool)"""
    import numpy as np
    board, dead, valid, cards = one_spot(street, pool, seed)
    name = ("river_" if street == 5 else "turn_") + ("A" if mode == "average" else "R")
    D = max(len(t.decision_nodes) for t in trees)
    Dr = max(len(t.river_decision_nodes) for t in trees) if street == 4 else 0
    where, rwhere, tree_of = [], [], []
    for k, tree in enumerate(trees):
        slots = river_slots(tree, valid)
        low = river_level_slots(tree, valid, cards) if street == 4 else []
        tabs = {n: table(name, n) for n in {s[1] for s in slots + low}}
        if mode == "regret":
            m = spots_needed(slots[:1], tabs)
        else:
            m = max(spots_needed(slots, tabs), spots_needed(low, tabs) if low else 1)
        m = m if spots is None else min(m, spots)
        if mode == "regret":                                       # (the root row runs through its table on its own)
            where += [{**a, **b} for a, b in zip(pack(slots[:1], tabs, m), pack(slots[1:], tabs, m))]
        else:
            where += pack(slots, tabs, m)
        rwhere += pack(low, tabs, m)
        tree_of += [k] * m
    m = len(where)
    X, zero = lay(where, (D,), SENTINEL), np.zeros((m, D, 4, H), np.int64)
    state = [zero, X] if mode == "average" else [X, zero]
    if street == 4:
        Xr, zr = lay(rwhere, (Dr, 52), SENTINEL), np.zeros((m, Dr, 52, 4, H), np.int64)
        state += [zr, Xr] if mode == "average" else [Xr, zr]
    ranges = np.full((m, 2, H), 2048 if street == 5 else 16384, np.uint16)
    return dict(board=np.tile(board, (m, 1)), dead=np.full(m, dead, np.uint64), trees=list(trees), tree_of=np.array(tree_of, np.uint32), ranges=ranges,
                t0=np.full(m, t0, np.uint32), iters=0 if mode == "average" else 1, state=state, where=where, river_where=rwhere, kind=name, pool=cards)


def rule_wanted(call, out):
    """What the tables say the call must return, in Python integers, against what it did: a list of the first few differences (empty: none).
    mode "average": strategy (and river_strategy) at every packed tuple; mode "regret": the root row's average."""
    bad = []
    t0 = int(call["t0"][0])
    if call["iters"] == 0:
        for key, where in (("strategy", call["where"]), ("river_strategy", call["river_where"])):
            for i, put in enumerate(where):
                for (prefix, h), X in put.items():
                    want = rule_exact(list(clamp(X, call["kind"])))
                    got = [int(v) for v in out[key][(i,) + prefix][:, h]]
                    if got != want + [0] * (4 - len(want)):
                        bad.append((key, i, prefix, h, X, got, want))
    else:
        for i, put in enumerate(call["where"]):
            for (prefix, h), X in put.items():
                if prefix != (0,):
                    continue
                want = [(t0 + 1) * s for s in rule_exact(list(clamp(X, call["kind"])))]
                got = [int(v) for v in out["average"][i, 0, :len(X), h]]
                if got != want:
                    bad.append(("average", i, prefix, h, X, got, want))
    return bad[:6]


def corner_call(street, pool, variant, seed=0x51AB):
    """The bounds corner: the tree whose pot + put is 8191, every weight 65535, t0 = 4093 and 3 iterations, from a state at the clamps.
    variant "top": every entry at RMAX / AMAX; "swing": one action per (row, holding) at RMAX / AMAX and the others 0; "mix": seeded."""
    import numpy as np
    board, dead, valid, cards = one_spot(street, pool, seed)
    tree = nine_node_tree() if street == 5 else corner_turn_tree()
    rmax, amax = (lim_of("river_R"), lim_of("river_A")) if street == 5 else (lim_of("turn_R"), lim_of("turn_A"))
    shapes = [(1, len(tree.decision_nodes), 4, H)] * 2
    if street == 4:
        shapes += [(1, len(tree.river_decision_nodes), 52, 4, H)] * 2
    rng = np.random.default_rng(seed + 1)
    state = []
    for j, shape in enumerate(shapes):
        lim = (rmax, amax)[j % 2]
        if variant == "top":
            a = np.full(shape, lim, np.int64)
        elif variant == "swing":
            a = np.zeros(shape, np.int64)
            pick = rng.integers(0, 2, shape[:-2] + (1, H))           # (every decision node of these trees has two actions)
            np.put_along_axis(a, pick, lim, axis=-2)
        else:
            a = rng.choice(np.array([0, 1, lim, lim - 1, lim >> 1, lim >> 13, 4242], np.int64), shape)
            rnd = rng.integers(0, lim + 1, shape)
            a = np.where(rng.random(shape) < 0.5, rnd, a)
        state.append(a)
    return dict(board=board[None], dead=np.array([dead], np.uint64), trees=[tree], tree_of=None, ranges=np.full((1, 2, H), 65535, np.uint16),
                t0=np.array([4093], np.uint32), iters=3, state=state, pool=cards)


def spec_of(street, call):
    """resume_spec on a call of rule_call / corner_call"""
    import resume_spec as RM
    f = RM.solve_river_batch if street == 5 else RM.solve_turn_batch
    return f(call["board"], call["ranges"], call["trees"], call["tree_of"], call["iters"], dead=call["dead"], t0=call["t0"],
             **dict(zip(RM.STATE_KEYS if street == 5 else RM.TURN_STATE_KEYS, call["state"])))


