"""The river subgame solver (pk_solve_river; the definition: include/pokerl_hip.h "River solver"): heads-up CFR+
over a caller-supplied betting tree, one subgame per workgroup on the device, in integers -- the same call gives the same bytes whatever
the grid.  river_tree builds a tree on the host; solve_river / solve_river_batch / solve_river_d run it.
The turn solver (pk_solve_turn; "Turn solver") is the same one street earlier, on a four-card board with the river
card as a chance node: turn_tree, solve_turn / solve_turn_batch / solve_turn_d, at the end of this module.
A tree per spot (pk_solve_river_trees / pk_solve_turn_trees; "River and turn solvers: a tree per spot"): the batch
and _d functions also take a SEQUENCE of trees with tree_of, the index of each spot's tree; river_trees / turn_trees build both from
per-spot pots and stacks.
Locked nodes (pk_solve_river_locked / pk_solve_turn_locked; "Locked nodes"): every solve function takes lock and
locked (the turn forms also river_lock and river_locked) -- rows of the strategy fixed by the caller, CFR+ on the rest; iters may then be 0.
evaluate_river / evaluate_turn lock every row: the value and the exploitability of a supplied strategy.
Re-solving (pk_solve_river_resolve / pk_solve_turn_resolve; "Re-solving"): every solve function takes reach (the root
reaches in the solver's own units, instead of ranges), at (a node whose reaches, values and best-response values the solution then carries as
node_reach / node_value / node_br; the turn forms also at_card) and, on the river, given (the values at a tree's KIND_GIVEN terminal).
subtree / river_subtree re-root a tree, gadget_tree puts the re-solving gadget on top of one, resolve_river does both kinds of re-solving.
Resuming (pk_solve_river_resume / pk_solve_turn_resume; "Resuming a solve"): every solve function takes state (a
SolverState: the regrets, the average accumulators and the iterations they hold) and keep_state; the solution then carries .state, which the
next call continues from.  solve_river_until / solve_turn_until and their _batch forms run such calls, the state on the device, until the
exploitability is at or under a target.
The pre-flop solver (pk_solve_preflop; "Pre-flop solver") is the river solver with no board and a showdown paid by the
exact matchup table: push_fold_tree / preflop_tree / preflop_trees, solve_preflop / solve_preflop_batch / solve_preflop_d, holding_class."""
import math

import numpy as np

from . import _lib as L
from .judger import _card, dead_mask, equity_status_text, rvr_valid_holdings

ONE = 32768                 # a probability of 1 in the strategy's fixed point (Q15)
MAX_NODES, MAX_ACTIONS, MAX_CHIPS, MAX_ITERS = 64, 4, 8191, 4096
KIND_P0, KIND_P1, KIND_FOLD0, KIND_FOLD1, KIND_SHOWDOWN = 0, 1, 2, 3, 4
KIND_GIVEN = 6              # a terminal whose values the caller supplies (pk_solve_river_resolve only)
REACH_MAX, TURN_REACH_MAX = (1 << 20) - 1, (1 << 17) - 1    # the largest root reach: a 16-bit weight << 4 / << 1 never exceeds it
GIVEN_MAX = (1 << 45) - 1   # the largest |given value|
NO_CHILD = 0xFF
GRID_MAX = 256              # the persistent grid's limit (RS_GRID_MAX): spots beyond it wait for a workgroup to come free


class RiverTree:
    """A betting tree: kind uint8 [n] (0 / 1 = player 0 / 1 to act, 2 / 3 = player 0 / 1 has folded, 4 = showdown), child uint8 [n, 4] (a
    decision node's children packed first, then 0xFF), put uint32 [n, 2] (chips each player has put in since the root) and pot (chips in the
    middle at the root).  decision_nodes: the decision nodes in index order -- row d of a solution's strategy is decision_nodes[d]."""

    def __init__(self, kind, child, put, pot, actions=None):
        self.kind = np.ascontiguousarray(kind, np.uint8)
        self.n = int(self.kind.shape[0])
        self.child = np.ascontiguousarray(child, np.uint8).reshape(self.n, 4)
        self.put = np.ascontiguousarray(put, np.uint32).reshape(self.n, 2)
        self.pot = int(pot)
        self.decision_nodes = [i for i in range(self.n) if self.kind[i] <= KIND_P1]
        self._actions = actions                      # per node: (parent, text) or None

    def num_actions(self, node):
        return int((self.child[node] != NO_CHILD).sum())

    def rows_of(self, player):
        """bool [D]: the rows of a solution's strategy at which `player` (0 or 1) acts -- a `lock` argument that fixes that player's play"""
        return np.array([int(self.kind[v]) == int(player) for v in self.decision_nodes], bool)

    def _cut(self, node):
        """the nodes of the subtree below `node` in index order, and the arguments of the re-rooted tree (pot and every put kept)"""
        node = int(node)
        if not 0 <= node < self.n:
            raise ValueError("no node %d" % node)
        keep = [node]
        for v in keep:                                   # (children have larger indices than their parent: sorted at the end)
            keep += [int(c) for c in self.child[v] if c != NO_CHILD]
        keep.sort()
        new = {v: i for i, v in enumerate(keep)}
        if len(keep) > NO_CHILD:
            raise ValueError("the subtree has more than %d nodes" % NO_CHILD)
        child = np.array([[NO_CHILD if c == NO_CHILD else new[int(c)] for c in self.child[v]] for v in keep], np.uint8).reshape(len(keep), 4)
        actions = None
        if self._actions is not None:
            actions = [None if v == node else (new[self._actions[v][0]], self._actions[v][1]) for v in keep]
        return keep, (self.kind[keep], child, self.put[keep], self.pot, actions)

    def subtree(self, node):
        """(tree, rows): the RiverTree re-rooted at decision node `node` -- its nodes renumbered in index order, pot and every put kept, so
        that its passes are those of this tree below the node -- and rows, the indices [D_sub] of its rows in this tree's strategy."""
        keep, args = self._cut(node)
        if self.kind[int(node)] > KIND_P1:
            raise ValueError("node %d is not a decision node" % int(node))
        rows = np.array([self.decision_nodes.index(v) for v in keep if self.kind[v] <= KIND_P1], np.int64)
        return RiverTree(*args), rows

    def label(self, node):
        """The actions that lead to `node`, such as "0:check 1:bet 50" ("" for the root)."""
        if self._actions is None:
            return "node %d" % node
        parts = []
        while self._actions[node] is not None:
            node, text = self._actions[node]
            parts.append(text)
        return " ".join(reversed(parts))

    def __repr__(self):
        return "RiverTree(n=%d, decisions=%d, pot=%d)" % (self.n, len(self.decision_nodes), self.pot)


class _Builder:
    """The node lists of a tree under construction and the betting rule of one street (river_tree's docstring)."""

    def __init__(self, pot, stack, limit):
        self.pot, self.stack, self.limit = pot, stack, limit
        self.kind, self.child, self.put, self.actions = [], [], [], []

    def new(self, k, p0, p1, parent, text):
        self.kind.append(k); self.child.append([NO_CHILD] * 4); self.put.append([p0, p1]); self.actions.append(None if parent is None else (parent, text))
        if len(self.kind) > self.limit:
            raise ValueError("the tree has more than %d nodes: fewer bet sizes or raises" % self.limit)
        return len(self.kind) - 1

    def sizes(self, p, puts, room, bet_fractions):
        to_call = max(puts) - puts[p]
        after = self.pot + puts[0] + puts[1] + to_call
        left = self.stack - puts[p] - to_call
        out = []
        for f in bet_fractions:
            amount = min(max(1, int(math.floor(f * after))), left)
            if amount > 0 and amount not in out:
                out.append(amount)
        return out[:room]

    def betting_round(self, root, bet_fractions, max_raises, end, limp=None):
        """One street from the decision node `root` (player 0 to act, nothing to call); end(p0, p1, parent, text) makes the node a call
        or a check behind leads to.  limp (preflop_tree: the root faces the big blind): True -- the root's call does not end the street,
        the other player may check behind or raise; False -- the root has no call; None -- a call at the root ends it like any other."""
        new, put = self.new, self.put
        pending = [root]
        state = {root: (0, False, 0)}                    # node -> (actor, a check has been made, raises so far)
        while pending:                                   # breadth first: every child index is above its parent's
            n = pending.pop(0)
            p, checked, raises = state[n]
            puts = put[n]
            facing = max(puts) - puts[p]
            kids = []
            if facing:
                pf = list(puts)
                kids.append(new(KIND_FOLD0 + p, pf[0], pf[1], n, "%d:fold" % p))
                pc = list(puts); pc[p] = max(puts)
                if n == root and limp is not None:
                    if limp:
                        c = new(KIND_P0 + (1 - p), pc[0], pc[1], n, "%d:call" % p)
                        state[c] = (1 - p, True, raises); pending.append(c); kids.append(c)
                else:
                    kids.append(end(pc[0], pc[1], n, "%d:call" % p))
                for amount in (self.sizes(p, puts, 2, bet_fractions) if raises < max_raises else []):
                    pr = list(puts); pr[p] = max(puts) + amount
                    c = new(KIND_P0 + (1 - p), pr[0], pr[1], n, "%d:raise %d" % (p, amount))
                    state[c] = (1 - p, True, raises + 1); pending.append(c); kids.append(c)
            else:
                if checked:
                    kids.append(end(puts[0], puts[1], n, "%d:check" % p))
                else:
                    c = new(KIND_P0 + (1 - p), puts[0], puts[1], n, "%d:check" % p)
                    state[c] = (1 - p, True, raises); pending.append(c); kids.append(c)
                for amount in (self.sizes(p, puts, 3, bet_fractions) if raises < max_raises else []):
                    pb = list(puts); pb[p] += amount
                    c = new(KIND_P0 + (1 - p), pb[0], pb[1], n, "%d:bet %d" % (p, amount))
                    state[c] = (1 - p, True, raises + 1); pending.append(c); kids.append(c)
            self.child[n][:len(kids)] = kids


def river_tree(pot, stack, bet_fractions=(0.5, 1.0), max_raises=2):
    """The tree of a river betting round: `pot` chips in the middle, `stack` chips behind each player, player 0 first.
    The rule: a player who faces no bet may check or bet; one who faces a bet may fold, call or raise.  max_raises counts the opening bet
    too: a bet or raise is offered while fewer than max_raises of them have been made and the player has chips left.  The sizes of a bet
    or raise: for each fraction, amount = max(1, floor(fraction * pot after calling)) chips on top of the call, capped at the chips the
    player has left; duplicates are dropped and, with at most four actions a node, only the first sizes that fit are kept (two when
    facing a bet, three otherwise).  A check behind or a call ends at a showdown."""
    pot, stack, max_raises = int(pot), int(stack), int(max_raises)
    if pot < 0 or stack < 0 or max_raises < 0:
        raise ValueError("pot, stack and max_raises must be non-negative")
    b = _Builder(pot, stack, MAX_NODES)
    b.betting_round(b.new(KIND_P0, 0, 0, None, None), bet_fractions, max_raises, lambda p0, p1, n, text: b.new(KIND_SHOWDOWN, p0, p1, n, text))
    return RiverTree(b.kind, b.child, b.put, pot, b.actions)


class RiverSolution:
    """What pk_solve_river returns for one spot or a batch: strategy uint16 [D, 4, 1326] (the average strategy in Q15: 32768 = always;
    unused action slots and invalid holdings 0; a valid holding of weight 0, like any holding that never reached a node, gets the uniform
    row), value and br int64 [2, 1326] (the counterfactual value of every holding under `strategy`, and against it with the holder
    playing a best response; half-chips times the opponent's reach, which starts at weight << 4), status (PK_EQ_* bits).  A batch has a
    leading [m].  A batch solved with a tree per spot has tree = None, trees and tree_of instead, and strategy [m, Dmax, 4, 1326] (Dmax:
    the most decision nodes of any tree passed); solution[i] is an ordinary single solution with tree trees[tree_of[i]] and the strategy
    cut to that tree's own rows (no tree and no row where tree_of[i] names none: status PK_EQ_BAD_TREE)."""

    _UNIT = 16                  # a root reach per unit of range weight

    def __init__(self, tree, ranges, strategy, value, br, status, valid, trees=None, tree_of=None, node=None, reach=None, state=None):
        self.tree, self.ranges, self.strategy, self.value, self.br, self.status, self.valid = tree, ranges, strategy, value, br, status, valid
        self.trees, self.tree_of = trees, tree_of
        self.state = state      # resuming: a SolverState (None unless the call was given state or keep_state)
        # re-solving: the root reaches the call was given (None: ranges), and the outputs at the node `at` (None when not asked for)
        self.reach = reach
        self.node_reach, self.node_value, self.node_br = node if node is not None else (None, None, None)

    def __getitem__(self, i):
        tree, strategy = self.tree, self.strategy[i]
        if self.trees is not None:
            tree = _spot_tree(self.trees, self.tree_of, i)
            strategy = strategy[:len(tree.decision_nodes) if tree is not None else 0]
        state = self.state
        if state is not None:
            state = state[i]
            if self.trees is not None:
                state.regret, state.average = state.regret[:strategy.shape[0]], state.average[:strategy.shape[0]]
        return RiverSolution(tree, _ith(self.ranges, i), strategy, self.value[i], self.br[i], self.status[i], self.valid[i],
                             node=_ith_node(self, i), reach=_ith(self.reach, i), state=state)

    def _weights(self):
        """(w int64 [2, 1326], unit): the weights ev and exploitability reduce by -- the root reaches where the call was given them
        (unit 1), the ranges otherwise (a reach is `unit` times a weight)"""
        return (self.ranges, self._UNIT) if self.reach is None else (self.reach, 1)

    def _pair_weight(self):
        w = self._weights()[0].astype(np.int64) * self.valid
        a = np.array([a for b in range(52) for a in range(b)])
        b = np.array([b for b in range(52) for a in range(b)])
        per_card = np.zeros((2, 52), np.int64)
        for p in (0, 1):
            np.add.at(per_card[p], a, w[p]); np.add.at(per_card[p], b, w[p])
        return (int(w[0].sum()) * int(w[1].sum()) - sum(int(x) * int(y) for x, y in zip(per_card[0], per_card[1]))
                + sum(int(x) * int(y) for x, y in zip(w[0], w[1])))

    def _one(self):
        if np.ndim(self.status) != 0:
            raise ValueError("index the batch first: solution[i].ev")

    @property
    def ev(self):
        """chips per player: sum_h w_p[h] value[p][h] / (32 sum over disjoint pairs of w_0 w_1); Python integers, one division each
        (solved from root reaches: w is the reach and the factor 2)"""
        self._one()
        w, unit = self._weights()
        den = 2 * unit * self._pair_weight()
        return tuple(sum(int(a) * int(v) for a, v in zip(w[p], self.value[p])) / den if den else float("nan") for p in (0, 1))

    @property
    def exploitability(self):
        """sum_p (br_p - value_p) reduced the same way, in chips"""
        self._one()
        w, unit = self._weights()
        den = 2 * unit * self._pair_weight()
        num = sum(int(a) * (int(b) - int(v)) for p in (0, 1) for a, b, v in zip(w[p], self.br[p], self.value[p]))
        return num / den if den else float("nan")

    def probabilities(self, node):
        """float64 [actions, 1326]: the strategy at decision node `node` (a node index of the tree), nan at invalid holdings"""
        self._one()
        row = self.tree.decision_nodes.index(int(node))
        out = self.strategy[row, :self.tree.num_actions(node)].astype(np.float64) / ONE
        out[:, ~self.valid] = np.nan
        return out

    def __repr__(self):
        return "RiverSolution(status=%r)" % (self.status,)


def _ith(a, i):
    return None if a is None else a[i]


def _ith_node(sol, i):
    return None if sol.node_reach is None else (sol.node_reach[i], sol.node_value[i], sol.node_br[i])


def _tree_args(tree):
    return (int(tree.n), L.ptr(tree.kind), L.ptr(tree.child), L.ptr(tree.put), int(tree.pot))


def _spot_tree(trees, tree_of, i):
    k = int(tree_of[int(i)])
    return trees[k] if k < len(trees) else None


class _TreeRows:
    """A sequence of trees as the tree-per-spot calls take it: tree k is row k of n uint32 [K], kind uint8 [K, rows], child uint8
    [K, rows, 4], put uint32 [K, rows, 2] and pot uint32 [K] (rows = 64 for river trees, 128 for turn trees; the entries past n[k] are
    ignored by the library)."""

    def __init__(self, trees, rows):
        self.trees = list(trees)
        K = len(self.trees)
        if not 1 <= K <= L.RS_MAX_TREES:
            raise ValueError("between 1 and %d trees" % L.RS_MAX_TREES)
        if any(t.n > rows for t in self.trees):
            raise ValueError("a tree has more than %d nodes" % rows)
        self.n = np.array([t.n for t in self.trees], np.uint32)
        self.pot = np.array([t.pot for t in self.trees], np.uint32)
        self.kind, self.child, self.put = np.zeros((K, rows), np.uint8), np.full((K, rows, 4), NO_CHILD, np.uint8), np.zeros((K, rows, 2), np.uint32)
        for k, t in enumerate(self.trees):
            self.kind[k, :t.n], self.child[k, :t.n], self.put[k, :t.n] = t.kind, t.child, t.put

    def args(self):
        return (len(self.trees), L.ptr(self.n), L.ptr(self.kind), L.ptr(self.child), L.ptr(self.put), L.ptr(self.pot))


def _tree_of(tree_of, ntrees, m):
    """tree_of as uint32 [m]; None: spot i uses tree i, which needs exactly m trees"""
    if tree_of is None:
        if ntrees != m:
            raise ValueError("tree_of=None needs one tree per spot: %d trees, %d spots" % (ntrees, m))
        return np.arange(m, dtype=np.uint32)
    tree_of = np.asarray(tree_of)
    if tree_of.shape != (m,) or tree_of.dtype.kind not in "iu":
        raise ValueError("tree_of must be an integer array of shape [m]")
    if m and (int(tree_of.min()) < 0 or int(tree_of.max()) > 0xFFFFFFFF):      # (no wrap-around in the cast: such an index names no tree)
        raise ValueError("tree_of must lie in 0 .. 2^32 - 1")
    return np.ascontiguousarray(tree_of, np.uint32)


def _trees_by_chips(pots, stacks, build):
    pots, stacks = np.asarray(pots).reshape(-1), np.asarray(stacks).reshape(-1)
    if pots.shape != stacks.shape:
        raise ValueError("pots and stacks must have the same shape [m]")
    index, trees, tree_of = {}, [], np.zeros(pots.shape[0], np.uint32)
    for i, key in enumerate(zip(pots.tolist(), stacks.tolist())):
        if key not in index:
            index[key] = len(trees)
            trees.append(build(int(key[0]), int(key[1])))
        tree_of[i] = index[key]
    return trees, tree_of


def _lock_rows(lock, m, D, name):
    """lock as uint8 [m, D]: bool / integer [D] (every spot the same) or [m, D]"""
    lock = np.asarray(lock)
    if lock.dtype.kind not in "biu" or lock.shape not in ((D,), (m, D)):
        raise ValueError("%s must be a bool or integer array of shape [%d] or [%d, %d]" % (name, D, m, D))
    return np.ascontiguousarray(np.broadcast_to(lock != 0, (m, D)), np.uint8)


def _locked_rows(locked, m, shape, name, attr):
    """locked as uint16 [m, *shape]: an array of that shape (or of `shape`: every spot the same), or a solution, whose `attr` is taken"""
    if isinstance(locked, (RiverSolution, TurnSolution)):
        locked = getattr(locked, attr)
        if locked is None:
            raise ValueError("the solution passed as %s has no %s" % (name, attr))
    locked = np.asarray(locked)
    if locked.dtype.kind not in "iu" or locked.shape not in (shape, (m,) + shape):
        raise ValueError("%s must be an integer array of shape %r, with or without a leading [%d]" % (name, list(shape), m))
    if locked.size and (int(locked.min()) < 0 or int(locked.max()) > 0xFFFF):
        raise ValueError("%s must lie in 0 .. 65535" % name)
    return np.ascontiguousarray(np.broadcast_to(locked, (m,) + shape), np.uint16)


def _lock_pair(lock, locked, m, D, shape, names, attr):
    if lock is None and locked is None:
        return None, None
    if lock is None or locked is None:
        raise ValueError("%s and %s come together" % names)
    return _lock_rows(lock, m, D, names[0]), _locked_rows(locked, m, (D,) + shape, names[1], attr)


def _resolve_ranges(ranges, reach, m, limit):
    """(ranges uint16 [m, 2, 1326] or None, reach uint32 [m, 2, 1326] or None): one of them must be given; a reach above `limit` is refused"""
    if ranges is None and reach is None:
        raise ValueError("ranges or reach")
    if ranges is not None:
        ranges = np.ascontiguousarray(ranges, np.uint16)
        if ranges.shape != (m, 2, L.EQ_HOLDINGS):
            raise ValueError("ranges must have shape [m, 2, 1326]")
    if reach is not None:
        reach = np.asarray(reach)
        if reach.shape != (m, 2, L.EQ_HOLDINGS) or reach.dtype.kind not in "iu":
            raise ValueError("reach must be an integer array of shape [m, 2, 1326]")
        if reach.size and (int(reach.min()) < 0 or int(reach.max()) > limit):
            raise ValueError("reach must lie in 0 .. %d" % limit)
        reach = np.ascontiguousarray(reach, np.uint32)
    return ranges, reach


def _resolve_at(at, m, name="at"):
    if at is None:
        return None
    at = np.asarray(at)
    if at.dtype.kind not in "iu" or at.shape not in ((), (m,)):
        raise ValueError("%s must be an integer or an integer array of shape [m]" % name)
    if at.size and (int(at.min()) < 0 or int(at.max()) > 255):
        raise ValueError("%s must lie in 0 .. 255" % name)
    return np.ascontiguousarray(np.broadcast_to(at, (m,)), np.uint8)


def _resolve_given(given, m):
    if given is None:
        return None
    given = np.asarray(given)
    if given.shape != (m, 2, L.EQ_HOLDINGS) or given.dtype.kind not in "iu":
        raise ValueError("given must be an integer array of shape [m, 2, 1326]")
    if given.size and (int(given.min()) < -GIVEN_MAX or int(given.max()) > GIVEN_MAX):
        raise ValueError("given must lie within +- (2^45 - 1)")
    return np.ascontiguousarray(given, np.int64)


def _node_outputs(at, m):
    if at is None:
        return None
    return (np.zeros((m, 2, L.EQ_HOLDINGS), np.uint32), np.zeros((m, 2, L.EQ_HOLDINGS), np.int64), np.zeros((m, 2, L.EQ_HOLDINGS), np.int64))


class SolverState:
    """The state of a solve that can be continued: regret and average int64 [D, 4, 1326] (the strategy's shape: the regrets and the average
    accumulators of every edge) and t, the iterations they hold.  A batch has a leading [m] and t uint32 [m]; state[i] is spot i's.
    river_regret / river_average are the turn solver's river-level arrays (None: the river solver has none).  An entry the solver does not
    use -- an action slot past the node's, an invalid holding, a row past the spot's tree, a locked row -- is 0 after a solve from nothing
    and keeps what it held through a continued one."""

    def __init__(self, regret, average, t, river_regret=None, river_average=None):
        self.regret, self.average, self.t, self.river_regret, self.river_average = regret, average, t, river_regret, river_average

    def __getitem__(self, i):
        return SolverState(self.regret[i], self.average[i], self.t[i], _ith(self.river_regret, i), _ith(self.river_average, i))

    @property
    def nbytes(self):
        return sum(a.nbytes for a in (self.regret, self.average, self.river_regret, self.river_average) if a is not None)

    def __repr__(self):
        return "SolverState(t=%r)" % (self.t,)


def solver_state_bytes(tree_or_trees, m=1):
    """The bytes of the state of m spots: two int64 arrays of the strategy's shape, 42 432 bytes per decision row each (the rows of the
    largest tree passed) -- and for TurnTrees two of river_strategy's, 2 206 464 bytes per river-level row each."""
    trees = [tree_or_trees] if isinstance(tree_or_trees, RiverTree) else list(tree_or_trees)
    rows = max(len(t.decision_nodes) for t in trees) + 52 * max(len(getattr(t, "river_decision_nodes", ())) for t in trees)
    return 2 * int(m) * rows * 4 * L.EQ_HOLDINGS * 8


_STATE_NAMES = ("regret", "average", "river_regret", "river_average")


def _state_arrays(state, keep_state, m, D, Dr=None):
    """(t0 uint32 [m], regret, average int64 [m, D, 4, 1326]) -- with Dr (the turn solver) also river_regret, river_average int64
    [m, Dr, 52, 4, 1326] -- copies, which the call then works in; None where no state is wanted.  state: a SolverState, or the arrays
    (regret, average, t) -- (regret, average, river_regret, river_average, t) -- of one spot or of m."""
    shapes = [(D, 4, L.EQ_HOLDINGS)] * 2 + ([] if Dr is None else [(Dr, 52, 4, L.EQ_HOLDINGS)] * 2)
    if state is None:
        if not keep_state:
            return None
        return (np.zeros(m, np.uint32),) + tuple(np.zeros((m,) + sh, np.int64) for sh in shapes)
    if isinstance(state, SolverState):
        state = tuple(getattr(state, k) for k in _STATE_NAMES[:len(shapes)]) + (state.t,)
    if len(state) != len(shapes) + 1 or any(a is None for a in state):
        raise ValueError("state is a SolverState of this solver or (%s, t)" % ", ".join(_STATE_NAMES[:len(shapes)]))
    out = []
    for a, name, shape in zip(state, _STATE_NAMES, shapes):
        a = np.asarray(a)
        if a.dtype.kind not in "iu" or a.shape not in (shape, (m,) + shape):
            raise ValueError("state.%s must be an integer array of shape %r, with or without a leading [%d]" % (name, list(shape), m))
        out.append(np.array(np.broadcast_to(a, (m,) + shape), np.int64, order="C"))
    t = np.asarray(state[-1])
    if t.dtype.kind not in "iu" or t.shape not in ((), (m,)) or (t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF)):
        raise ValueError("state.t must be a non-negative integer or an integer array of shape [%d]" % m)
    return (np.array(np.broadcast_to(t, (m,)), np.uint32),) + tuple(out)


def _new_state(st, iters, status):
    """the SolverState after a call that worked in st's arrays: t = t0 + iters at the solved spots, t0 at the refused ones (whose state the
    library has not touched)"""
    return SolverState(st[1], st[2], np.where(status == 0, st[0] + np.uint32(iters), st[0]).astype(np.uint32), *st[3:])


def gadget_tree(tree, opponent):
    """The re-solving gadget on top of `tree` (Burch, Johanson, Bowling 2014) -> a RiverTree of tree.n + 2 nodes: node 0 is a decision node
    of `opponent` with the children [1, 2], node 1 the KIND_GIVEN terminal ("terminate": the opponent takes the value it was promised),
    node 2 the old root ("follow"); the old nodes are shifted by 2, pot and every put kept.  Row 0 of a solution's strategy is the gadget's,
    rows 1 .. are `tree`'s."""
    opponent = int(opponent)
    if opponent not in (0, 1):
        raise ValueError("opponent must be 0 or 1")
    if tree.n + 2 > MAX_NODES:
        raise ValueError("the gadget tree has more than %d nodes" % MAX_NODES)
    kind = np.concatenate([np.array([opponent, KIND_GIVEN], np.uint8), tree.kind])
    child = np.where(tree.child == NO_CHILD, NO_CHILD, tree.child.astype(np.int64) + 2)
    child = np.concatenate([np.array([[1, 2, NO_CHILD, NO_CHILD], [NO_CHILD] * 4], np.int64), child]).astype(np.uint8)
    put = np.concatenate([tree.put[:1], tree.put[:1], tree.put])
    actions = [None, (0, "%d:terminate" % opponent), (0, "%d:follow" % opponent)]
    actions += [None if a is None else (a[0] + 2, a[1]) for a in (tree._actions or [None] * tree.n)][1:]
    if tree._actions is None:
        actions = None
    return RiverTree(kind, child, put, tree.pot, actions)


def river_trees(pots, stacks, bet_fractions=(0.5, 1.0), max_raises=2):
    """(trees, tree_of) for spots of per-spot chips: pots and stacks are integer arrays [m]; one river_tree per DISTINCT (pot, stack)
    pair, in the order the pairs first appear, and tree_of uint32 [m] with the index of each spot's tree -- what solve_river_batch takes."""
    return _trees_by_chips(pots, stacks, lambda pot, stack: river_tree(pot, stack, bet_fractions, max_raises))


def solve_river_batch(board, ranges, tree, iters, dead=None, device=0, tree_of=None, lock=None, locked=None, reach=None, given=None, at=None,
                      state=None, keep_state=False):
    """pk_solve_river on host arrays: board uint8 [m, 5] Card.value, ranges uint16 [m, 2, 1326] over holding_index, one tree for the call,
    dead uint64 [m] masks over canonical card indices (None: none) -> RiverSolution with a leading [m].  A bad spot is reported through
    its status with all-zero outputs; the others are unaffected.
    tree may also be a SEQUENCE of trees (pk_solve_river_trees): spot i is solved with tree[tree_of[i]], tree_of an integer array [m]
    (None: spot i uses tree i, which needs m trees); every output of spot i is what the call with that one tree gives for it.
    lock, locked (pk_solve_river_locked): lock is a bool / integer [D] (every spot the same) or [m, D], nonzero = that row of the strategy
    is LOCKED to the strategy rule applied to locked -- an integer array of the strategy's shape (any non-negative weights up to 65535; a
    row of an earlier solution is reproduced unchanged) or a RiverSolution, whose strategy is taken.  CFR+ runs on the other rows; iters
    may be 0 (every free row: the uniform row).  br ignores the locks, so exploitability is that of the profile as played.
    reach, given, at (pk_solve_river_resolve): reach integers [m, 2, 1326] up to 2^20 - 1, the root reaches in the solver's own units
    (ranges may then be None; ranges << 4 is the same call); given integers [m, 2, 1326] within +- (2^45 - 1), the values at a tree's
    KIND_GIVEN terminal; at an integer or integers [m], the node whose reaches, values and best-response values the solution carries as
    node_reach, node_value, node_br.  A value outside those bounds is a ValueError here (the library's device forms clamp).
    state, keep_state (pk_solve_river_resume): state is a SolverState -- the .state of an earlier solution -- or (regret, average, t); the
    call runs iterations t + 1 .. t + iters from it (its arrays are copied, not changed) and the solution carries the new one as .state.
    keep_state=True without state starts from nothing and returns the state; iters may be 0.  t + iters > 4096 is status PK_EQ_BAD_ITER."""
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 5:
        raise ValueError("board must have shape [m, 5]")
    m = board.shape[0]
    resume = state is not None or keep_state
    resolve = resume or reach is not None or given is not None or at is not None
    ranges, reach = _resolve_ranges(ranges, reach, m, REACH_MAX)
    given, at = _resolve_given(given, m), _resolve_at(at, m)
    node = _node_outputs(at, m)
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError("dead must have shape [m]")
    value, br = np.zeros((m, 2, L.EQ_HOLDINGS), np.int64), np.zeros((m, 2, L.EQ_HOLDINGS), np.int64)
    status = np.zeros(m, np.uint8)
    if resolve or lock is not None or locked is not None:
        one = isinstance(tree, RiverTree)
        if one and tree_of is not None:
            raise ValueError("tree_of needs a sequence of trees")
        rows = _TreeRows([tree] if one else tree, MAX_NODES)
        D = max(len(t.decision_nodes) for t in rows.trees)
        trees, tree, tree_of = (None, tree, None) if one else (rows.trees, None, _tree_of(tree_of, len(rows.trees), m))
        lock, locked = _lock_pair(lock, locked, m, D, (4, L.EQ_HOLDINGS), ("lock", "locked"), "strategy")
        strategy = np.zeros((m, D, 4, L.EQ_HOLDINGS), np.uint16)
        if resume:
            nr, nv, nb = node or (None, None, None)
            st = _state_arrays(state, keep_state, m, D)
            L.check(L.lib().pk_solve_river_resume(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters),
                                                  L.ptr(lock), L.ptr(locked), L.ptr(reach), L.ptr(given), L.ptr(at), L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]),
                                                  L.ptr(strategy), L.ptr(value), L.ptr(br), L.ptr(nr), L.ptr(nv), L.ptr(nb), L.ptr(status)))
            state = _new_state(st, iters, status)
        elif resolve:
            nr, nv, nb = node or (None, None, None)
            L.check(L.lib().pk_solve_river_resolve(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters),
                                                   L.ptr(lock), L.ptr(locked), L.ptr(reach), L.ptr(given), L.ptr(at), L.ptr(strategy), L.ptr(value),
                                                   L.ptr(br), L.ptr(nr), L.ptr(nv), L.ptr(nb), L.ptr(status)))
        else:
            L.check(L.lib().pk_solve_river_locked(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters),
                                                  L.ptr(lock), L.ptr(locked), L.ptr(strategy), L.ptr(value), L.ptr(br), L.ptr(status)))
    elif isinstance(tree, RiverTree):
        if tree_of is not None:
            raise ValueError("tree_of needs a sequence of trees")
        strategy = np.zeros((m, len(tree.decision_nodes), 4, L.EQ_HOLDINGS), np.uint16)
        L.check(L.lib().pk_solve_river(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *_tree_args(tree), int(iters), L.ptr(strategy),
                                       L.ptr(value), L.ptr(br), L.ptr(status)))
        trees = None
    else:
        rows = _TreeRows(tree, MAX_NODES)
        trees, tree, tree_of = rows.trees, None, _tree_of(tree_of, len(rows.trees), m)
        strategy = np.zeros((m, max(len(t.decision_nodes) for t in trees), 4, L.EQ_HOLDINGS), np.uint16)
        L.check(L.lib().pk_solve_river_trees(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters),
                                             L.ptr(strategy), L.ptr(value), L.ptr(br), L.ptr(status)))
    valid = rvr_valid_holdings(board, np.full(m, 5, np.uint8), dead) & (status == 0)[:, None]
    return RiverSolution(tree, ranges, strategy, value, br, status, valid, trees, tree_of, node=node, reach=reach, state=state)


def solve_river_d(m, board_d, ranges_d, tree, iters, dead_d=None, strategy_d=None, value_d=None, br_d=None, status_d=None, device=0, stream=None,
                  tree_of=None, lock=None, locked=None, reach=None, given=None, at=None, node_reach_d=None, node_value_d=None, node_br_d=None,
                  t0_d=None, regret_d=None, average_d=None):
    """pk_solve_river_d: the same on device-resident buffers (device pointers as ints / c_void_p; the tree stays a host RiverTree; dead_d and
    the outputs may be None), asynchronous on `stream`.  With a SEQUENCE of trees (pk_solve_river_trees_d) tree_of is the DEVICE pointer of
    uint32 [m] and strategy_d holds [m, Dmax, 4, 1326], Dmax the most decision nodes of any tree passed; the trees are packed and queued
    for upload before the call returns.  lock, locked (pk_solve_river_locked_d): DEVICE pointers of uint8 [m, Dmax] and uint16
    [m, Dmax, 4, 1326]; with one RiverTree Dmax is its own D.  reach, given, at and node_reach_d, node_value_d, node_br_d
    (pk_solve_river_resolve_d): DEVICE pointers of uint32 / int64 [m, 2, 1326] and uint8 [m]; ranges_d may then be None.  t0_d, regret_d,
    average_d (pk_solve_river_resume_d): DEVICE pointers of uint32 [m] (None: all 0) and int64 [m, Dmax, 4, 1326], the state, worked in place."""
    if any(x is not None for x in (t0_d, regret_d, average_d)):
        one = isinstance(tree, RiverTree)
        if one == (tree_of is not None):
            raise ValueError("tree_of, the device pointer of uint32 [m], comes with a sequence of trees and only with one")
        L.check(L.lib().pk_solve_river_resume_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows([tree] if one else tree, MAX_NODES).args(),
                                                tree_of, int(iters), lock, locked, reach, given, at, t0_d, regret_d, average_d, strategy_d, value_d, br_d,
                                                node_reach_d, node_value_d, node_br_d, status_d, stream))
        return
    if any(x is not None for x in (reach, given, at, node_reach_d, node_value_d, node_br_d)):
        one = isinstance(tree, RiverTree)
        if one == (tree_of is not None):
            raise ValueError("tree_of, the device pointer of uint32 [m], comes with a sequence of trees and only with one")
        L.check(L.lib().pk_solve_river_resolve_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows([tree] if one else tree, MAX_NODES).args(),
                                                 tree_of, int(iters), lock, locked, reach, given, at, strategy_d, value_d, br_d, node_reach_d,
                                                 node_value_d, node_br_d, status_d, stream))
        return
    if lock is not None or locked is not None:
        one = isinstance(tree, RiverTree)
        if one == (tree_of is not None):
            raise ValueError("tree_of, the device pointer of uint32 [m], comes with a sequence of trees and only with one")
        L.check(L.lib().pk_solve_river_locked_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows([tree] if one else tree, MAX_NODES).args(),
                                                tree_of, int(iters), lock, locked, strategy_d, value_d, br_d, status_d, stream))
        return
    if not isinstance(tree, RiverTree):
        if tree_of is None:
            raise ValueError("a sequence of trees needs tree_of, the device pointer of uint32 [m]")
        L.check(L.lib().pk_solve_river_trees_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows(tree, MAX_NODES).args(), tree_of, int(iters),
                                               strategy_d, value_d, br_d, status_d, stream))
        return
    if tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    L.check(L.lib().pk_solve_river_d(int(device), int(m), board_d, dead_d, ranges_d, *_tree_args(tree), int(iters), strategy_d, value_d, br_d,
                                     status_d, stream))


def _one_spot(a):
    return None if a is None else np.asarray(a)[None]


def solve_river(board, ranges, tree, iters, dead=(), device=0, lock=None, locked=None, reach=None, given=None, at=None, state=None, keep_state=False):
    """One subgame.  board: the five board cards (Card-likes / 'RS' strings / Card.value ints); ranges: [2, 1326] integers 0 .. 65535 over
    holding_index, player 0 (first to act) then player 1; dead: cards known to be out of play.  Raises ValueError for an invalid spot.
    A reach starts at weight << 4 and every split rounds down, so ranges of small integers (1, 2, ...) lose weight on the way down the
    tree: scale a range so that its largest weight uses the sixteen bits.  lock bool [D], locked [D, 4, 1326] or a RiverSolution: as
    solve_river_batch takes them; so are reach [2, 1326] (ranges may then be None), given [2, 1326], at (a node index), state and keep_state."""
    board = list(board)
    if len(board) != 5:
        raise ValueError("five board cards")
    b = np.array([[_card(c) for c in board]], np.uint8)
    d = np.array([dead if isinstance(dead, (int, np.integer)) else dead_mask(dead)], np.uint64)
    r = solve_river_batch(b, _one_spot(ranges), tree, iters, d, device=device, lock=lock, locked=locked, reach=_one_spot(reach), given=_one_spot(given),
                          at=at, state=state, keep_state=keep_state)[0]
    if state is not None and r.status == L.EQ_BAD_ITER:
        raise ValueError("the state's iterations and iters together exceed %d" % MAX_ITERS)
    if r.status:
        raise ValueError("invalid spot: " + equity_status_text(r.status))
    return r


def solve_river_until_batch(board, ranges, tree, target, step=64, max_iters=MAX_ITERS, dead=None, device=0, tree_of=None, lock=None, locked=None,
                            reach=None, given=None):
    """Solve until every solved spot's exploitability is at or under `target` chips, or max_iters iterations have run: calls of `step`
    iterations each (the last one shorter where max_iters is no multiple), every spot the same number, the state in DEVICE memory from the
    first call to the last (solver_state_bytes(tree, m) of it).  The arguments are solve_river_batch's.  -> the last call's RiverSolution
    with .iters (the iterations run), .trace (float64 [calls, m]: the exploitability of every spot after each call, nan for a refused
    spot) and .state on the host.  By identity (ii) of the definition the solution is the one solve_river_batch gives with .iters iterations."""
    from . import hipmem
    step, max_iters = int(step), int(max_iters)
    if step < 1 or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError("step >= 1 and max_iters in 1 .. %d" % MAX_ITERS)
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 5:
        raise ValueError("board must have shape [m, 5]")
    m = board.shape[0]
    ranges, reach = _resolve_ranges(ranges, reach, m, REACH_MAX)
    given = _resolve_given(given, m)
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError("dead must have shape [m]")
    one = isinstance(tree, RiverTree)
    if one and tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    trees = [tree] if one else list(tree)
    D = max(len(t.decision_nodes) for t in trees)
    tree_of = None if one else _tree_of(tree_of, len(trees), m)
    lock, locked = _lock_pair(lock, locked, m, D, (4, L.EQ_HOLDINGS), ("lock", "locked"), "strategy")
    rows, pair = m * D * 4 * L.EQ_HOLDINGS, m * 2 * L.EQ_HOLDINGS
    bufs = []

    def dev(a=None, nbytes=0):
        if a is None and not nbytes:
            return None
        b = hipmem.DeviceBuffer(a.nbytes if a is not None else nbytes, device)
        bufs.append(b)
        return b.upload(a) if a is not None else b
    ptr = lambda b: None if b is None else b.ptr
    try:
        ins = [dev(a) for a in (board, dead, ranges, tree_of, lock, locked, reach, given)]
        t0 = np.zeros(m, np.uint32)
        t0_d, regret_d, average_d = dev(t0), dev(nbytes=rows * 8), dev(nbytes=rows * 8)
        strategy_d, value_d, br_d, status_d = dev(nbytes=rows * 2), dev(nbytes=pair * 8), dev(nbytes=pair * 8), dev(nbytes=m)
        trace, done = [], 0
        while True:
            it = min(step, max_iters - done)
            t0_d.upload(t0)
            solve_river_d(m, ptr(ins[0]), ptr(ins[2]), tree, it, dead_d=ptr(ins[1]), strategy_d=strategy_d.ptr, value_d=value_d.ptr, br_d=br_d.ptr,
                          status_d=status_d.ptr, device=device, tree_of=ptr(ins[3]), lock=ptr(ins[4]), locked=ptr(ins[5]), reach=ptr(ins[6]),
                          given=ptr(ins[7]), t0_d=t0_d.ptr, regret_d=regret_d.ptr, average_d=average_d.ptr)
            value, br = (b.download(np.int64, pair).reshape(m, 2, L.EQ_HOLDINGS) for b in (value_d, br_d))
            status = status_d.download(np.uint8, m)
            valid = rvr_valid_holdings(board, np.full(m, 5, np.uint8), dead) & (status == 0)[:, None]
            sol = RiverSolution(tree if one else None, ranges, None, value, br, status, valid, None if one else trees, tree_of, reach=reach)
            done += it
            t0 += np.uint32(it)
            trace.append([RiverSolution(None, _ith(ranges, i), None, value[i], br[i], status[i], valid[i], reach=_ith(reach, i)).exploitability
                          if status[i] == 0 else float("nan") for i in range(m)])
            if done >= max_iters or all(not e > target for e in trace[-1]):
                break
        sol.strategy = strategy_d.download(np.uint16, rows).reshape(m, D, 4, L.EQ_HOLDINGS)
        regret, average = (b.download(np.int64, rows).reshape(m, D, 4, L.EQ_HOLDINGS) for b in (regret_d, average_d))
        sol.state = SolverState(regret, average, np.where(status == 0, done, 0).astype(np.uint32))
        sol.iters, sol.trace = done, np.array(trace, np.float64).reshape(len(trace), m)
        return sol
    finally:
        for b in bufs:
            b.free()


def solve_river_until(board, ranges, tree, target, step=64, max_iters=MAX_ITERS, dead=(), device=0, lock=None, locked=None, reach=None, given=None):
    """One subgame solved to a target: solve_river's arguments, solve_river_until_batch's rule -> its RiverSolution (.iters, .trace float64
    [calls], .state).  Raises ValueError for an invalid spot."""
    board = list(board)
    if len(board) != 5:
        raise ValueError("five board cards")
    b = np.array([[_card(c) for c in board]], np.uint8)
    d = np.array([dead if isinstance(dead, (int, np.integer)) else dead_mask(dead)], np.uint64)
    full = solve_river_until_batch(b, _one_spot(ranges), tree, target, step, max_iters, d, device=device, lock=lock, locked=locked, reach=_one_spot(reach),
                                   given=_one_spot(given))
    r = full[0]
    if r.status:
        raise ValueError("invalid spot: " + equity_status_text(r.status))
    r.iters, r.trace = full.iters, full.trace[:, 0]
    return r


def evaluate_river_batch(board, ranges, tree, strategy, dead=None, device=0, tree_of=None):
    """The values and best responses of a SUPPLIED strategy: solve_river_batch with every row locked to `strategy` and no iteration.
    -> an ordinary RiverSolution (solution[i].ev, .exploitability)."""
    trees = [tree] if isinstance(tree, RiverTree) else list(tree)
    return solve_river_batch(board, ranges, tree, 0, dead, device=device, tree_of=tree_of,
                             lock=np.ones(max(len(t.decision_nodes) for t in trees), bool), locked=strategy)


def evaluate_river(board, ranges, tree, strategy, dead=(), device=0):
    """One subgame: the value of `strategy` (integers [D, 4, 1326] or a RiverSolution) and how exploitable it is."""
    return solve_river(board, ranges, tree, 0, dead, device=device, lock=np.ones(len(tree.decision_nodes), bool), locked=strategy)


def resolve_river(board, tree, reach, iters, hero, opponent_values=None, dead=(), device=0):
    """Re-solve the river subgame `tree` for player `hero` from the reaches [2, 1326] at its root -- node_reach of the solve that led here.
    Without opponent_values: UNSAFE re-solving, an ordinary solve from those reaches.  With opponent_values (integers [1326]: the
    opponent's counterfactual values at the root, such as node_br[1 - hero] of that solve): SAFE re-solving through gadget_tree -- the
    opponent chooses per holding between the value it was promised and playing on, and enters with the same reach for every holding (the
    largest entry of its row of `reach`), as the gadget prescribes.  -> a RiverSolution on `tree`: the gadget's row is cut off the
    strategy; value and br are those at the gadget's root."""
    hero = int(hero)
    if hero not in (0, 1):
        raise ValueError("hero must be 0 or 1")
    reach = np.array(reach, np.int64).reshape(2, L.EQ_HOLDINGS)
    if opponent_values is None:
        return solve_river(board, None, tree, iters, dead, device=device, reach=reach)
    given = np.zeros((2, L.EQ_HOLDINGS), np.int64)
    given[1 - hero] = np.asarray(opponent_values).reshape(L.EQ_HOLDINGS)
    reach[1 - hero] = int(reach[1 - hero].max())
    r = solve_river(board, None, gadget_tree(tree, 1 - hero), iters, dead, device=device, reach=reach, given=given)
    return RiverSolution(tree, None, r.strategy[1:], r.value, r.br, r.status, r.valid, reach=r.reach)


# ------------------------------------------------------------------------------------------------ the turn solver
TURN_MAX_NODES = 128
KIND_CHANCE = 5


class TurnTree(RiverTree):
    """A betting tree on a four-card board: RiverTree's arrays, with kind 5 = chance (the river card is dealt; one child).  Nodes not
    below a chance node are turn-level, the others river-level.  decision_nodes: the TURN-LEVEL decision nodes in index order (row d of a
    solution's strategy); river_decision_nodes: the river-level ones (row d of river_strategy)."""

    def __init__(self, kind, child, put, pot, actions=None):
        super().__init__(kind, child, put, pot, actions)
        self.river_level = np.zeros(self.n, bool)
        for v in range(self.n):
            for c in self.child[v]:
                if c != NO_CHILD and c < self.n:
                    self.river_level[c] = self.river_level[v] or self.kind[v] == KIND_CHANCE
        decisions = self.decision_nodes
        self.decision_nodes = [v for v in decisions if not self.river_level[v]]
        self.river_decision_nodes = [v for v in decisions if self.river_level[v]]

    def subtree(self, node):
        """(tree, rows, river_rows): the TurnTree re-rooted at the turn-level decision node `node` (pot and every put kept), and the indices
        of its turn-level and river-level rows in this tree's strategy and river_strategy."""
        node = int(node)
        keep, args = self._cut(node)
        if self.river_level[node] or self.kind[node] > KIND_P1:
            raise ValueError("node %d is not a turn-level decision node" % node)
        rows = np.array([self.decision_nodes.index(v) for v in keep if v in self.decision_nodes], np.int64)
        river_rows = np.array([self.river_decision_nodes.index(v) for v in keep if v in self.river_decision_nodes], np.int64)
        return TurnTree(*args), rows, river_rows

    def river_subtree(self, node):
        """(tree, rows): the RiverTree below the river-level decision node `node` (pot and every put kept) -- what the river solver takes
        on the five-card board -- and the indices of its rows in this tree's river_strategy."""
        node = int(node)
        keep, args = self._cut(node)
        if not self.river_level[node] or self.kind[node] > KIND_P1:
            raise ValueError("node %d is not a river-level decision node" % node)
        rows = np.array([self.river_decision_nodes.index(v) for v in keep if self.kind[v] <= KIND_P1], np.int64)
        return RiverTree(*args), rows

    def rows_of(self, player):
        """(bool [D_t], bool [D_r]): the turn-level and the river-level rows at which `player` acts -- lock and river_lock for that player"""
        return (np.array([int(self.kind[v]) == int(player) for v in self.decision_nodes], bool),
                np.array([int(self.kind[v]) == int(player) for v in self.river_decision_nodes], bool))

    def __repr__(self):
        return "TurnTree(n=%d, turn decisions=%d, river decisions=%d, pot=%d)" % (self.n, len(self.decision_nodes), len(self.river_decision_nodes), self.pot)


def turn_tree(pot, stack, bet_fractions=(0.5, 1.0), max_raises=2, river_bet_fractions=None, river_max_raises=None):
    """The tree of a turn and a river betting round: `pot` chips in the middle, `stack` chips behind each player, player 0 first on both
    streets.  river_tree's betting rule on each street (river_bet_fractions / river_max_raises: None = the turn's).  Every turn line that
    ends in a call or in check-check leads to a chance node and from there to a river round on the chips left -- or straight to a
    showdown if nothing is left.  At most 128 nodes (ValueError)."""
    pot, stack, max_raises = int(pot), int(stack), int(max_raises)
    river_bet_fractions = bet_fractions if river_bet_fractions is None else river_bet_fractions
    river_max_raises = max_raises if river_max_raises is None else int(river_max_raises)
    if pot < 0 or stack < 0 or max_raises < 0 or river_max_raises < 0:
        raise ValueError("pot, stack and max_raises must be non-negative")
    b = _Builder(pot, stack, TURN_MAX_NODES)
    chances = []

    def deal(p0, p1, n, text):
        chances.append(b.new(KIND_CHANCE, p0, p1, n, text))
        return chances[-1]

    b.betting_round(b.new(KIND_P0, 0, 0, None, None), bet_fractions, max_raises, deal)
    for c in chances:
        p0, p1 = b.put[c]
        if p0 >= stack:
            b.child[c][0] = b.new(KIND_SHOWDOWN, p0, p1, c, "deal")
        else:
            b.child[c][0] = b.new(KIND_P0, p0, p1, c, "deal")
            b.betting_round(b.child[c][0], river_bet_fractions, river_max_raises, lambda q0, q1, n, text: b.new(KIND_SHOWDOWN, q0, q1, n, text))
    return TurnTree(b.kind, b.child, b.put, pot, b.actions)


class TurnSolution:
    """What pk_solve_turn returns for one spot or a batch: strategy uint16 [D_t, 4, 1326], river_strategy uint16 [D_r, 52, 4, 1326] (None
    unless asked for; indexed by the river card's canonical index, 0 for cards outside the pool and holdings with the card), value and br
    int64 [2, 1326] (half-chips times the opponent's reach, which starts at weight << 1, times the P - 4 river cards), status, and pool
    (P).  A batch has a leading [m].  A batch solved with a tree per spot has tree = None, trees and tree_of instead, and the strategies
    have the rows of the largest tree passed; solution[i] is an ordinary single solution with tree trees[tree_of[i]] and both strategies
    cut to that tree's own rows."""

    _UNIT = 2                   # a root reach per unit of range weight

    def __init__(self, tree, ranges, strategy, river_strategy, value, br, status, valid, pool, trees=None, tree_of=None, node=None, reach=None, state=None):
        self.state = state      # resuming: a SolverState (None unless the call was given state or keep_state)
        self.tree, self.ranges, self.strategy, self.river_strategy = tree, ranges, strategy, river_strategy
        self.value, self.br, self.status, self.valid, self.pool = value, br, status, valid, pool
        self.trees, self.tree_of = trees, tree_of
        self.reach = reach
        self.node_reach, self.node_value, self.node_br = node if node is not None else (None, None, None)

    def __getitem__(self, i):
        tree, strategy, rstrat = self.tree, self.strategy[i], None if self.river_strategy is None else self.river_strategy[i]
        if self.trees is not None:
            tree = _spot_tree(self.trees, self.tree_of, i)
            strategy = strategy[:len(tree.decision_nodes) if tree is not None else 0]
            if rstrat is not None:
                rstrat = rstrat[:len(tree.river_decision_nodes) if tree is not None else 0]
        state = self.state
        if state is not None:
            state = state[i]
            if self.trees is not None:
                nt, nr = (len(tree.decision_nodes), len(tree.river_decision_nodes)) if tree is not None else (0, 0)
                state.regret, state.average = state.regret[:nt], state.average[:nt]
                state.river_regret, state.river_average = state.river_regret[:nr], state.river_average[:nr]
        return TurnSolution(tree, _ith(self.ranges, i), strategy, rstrat, self.value[i], self.br[i], self.status[i], self.valid[i], self.pool[i],
                            node=_ith_node(self, i), reach=_ith(self.reach, i), state=state)

    _weights = RiverSolution._weights
    _pair_weight = RiverSolution._pair_weight
    _one = RiverSolution._one

    @property
    def ev(self):
        """chips per player: sum_h w_p[h] value[p][h] / (4 (P - 4) sum over disjoint pairs of w_0 w_1); Python integers, one division each"""
        self._one()
        w, unit = self._weights()
        den = 2 * unit * (int(self.pool) - 4) * self._pair_weight()
        return tuple(sum(int(a) * int(v) for a, v in zip(w[p], self.value[p])) / den if den else float("nan") for p in (0, 1))

    @property
    def exploitability(self):
        """sum_p (br_p - value_p) reduced the same way, in chips"""
        self._one()
        w, unit = self._weights()
        den = 2 * unit * (int(self.pool) - 4) * self._pair_weight()
        num = sum(int(a) * (int(b) - int(v)) for p in (0, 1) for a, b, v in zip(w[p], self.br[p], self.value[p]))
        return num / den if den else float("nan")

    def probabilities(self, node, river_card=None):
        """float64 [actions, 1326]: the strategy at decision node `node` (a node index of the tree) -- of a river-level node under
        river_card (a Card-like, 'RS' string or Card.value); nan at invalid holdings and at holdings with the river card"""
        self._one()
        node = int(node)
        nact = self.tree.num_actions(node)
        valid = self.valid
        if node in self.tree.decision_nodes:
            out = self.strategy[self.tree.decision_nodes.index(node), :nact].astype(np.float64) / ONE
        else:
            if self.river_strategy is None:
                raise ValueError("solve with river_strategy=True")
            if river_card is None:
                raise ValueError("a river-level node needs river_card")
            c = int(_card(river_card))
            k = (c & 15) * 4 + (c >> 4)
            out = self.river_strategy[self.tree.river_decision_nodes.index(node), k, :nact].astype(np.float64) / ONE
            a = np.array([a for b in range(52) for a in range(b)])
            b = np.array([b for b in range(52) for a in range(b)])
            valid = valid & (a != k) & (b != k)
        out[:, ~valid] = np.nan
        return out

    def __repr__(self):
        return "TurnSolution(status=%r)" % (self.status,)


def turn_trees(pots, stacks, bet_fractions=(0.5, 1.0), max_raises=2, river_bet_fractions=None, river_max_raises=None):
    """(trees, tree_of) for spots of per-spot chips, as river_trees: one turn_tree per distinct (pot, stack) pair."""
    return _trees_by_chips(pots, stacks, lambda pot, stack: turn_tree(pot, stack, bet_fractions, max_raises, river_bet_fractions, river_max_raises))


def _turn_levels(tree):
    nr = int(np.count_nonzero(tree.river_level))
    return tree.n - nr, nr


def turn_grid(tree, m=None):
    """The number of workgroups a solve of `tree` uses (for m spots; None: for any m that large): min(m, 256, 4 GiB / the work space of
    one workgroup).  No output depends on it.  A sequence of trees: the grid of a tree-per-spot call, whose workgroups are sized for the
    most turn-level and the most river-level nodes of any tree."""
    if not isinstance(tree, RiverTree):
        levels = [_turn_levels(t) for t in tree]
        nt, nr = max(a for a, _ in levels), max(b for _, b in levels)
        return int(L.lib().pk_turn_grid(GRID_MAX if m is None else int(m), nt, nr))
    nt, nr = _turn_levels(tree)
    return int(L.lib().pk_turn_grid(GRID_MAX if m is None else int(m), nt, nr))


def solve_turn_batch(board, ranges, tree, iters, dead=None, river_strategy=False, device=0, tree_of=None, lock=None, locked=None, river_lock=None,
                     river_locked=None, reach=None, at=None, at_card=None, state=None, keep_state=False):
    """pk_solve_turn on host arrays: board uint8 [m, 4] Card.value, ranges uint16 [m, 2, 1326] over holding_index, one TurnTree for the
    call, dead uint64 [m] masks over canonical card indices (None: none) -> TurnSolution with a leading [m].  river_strategy=True also
    returns the river-level strategies (551 616 bytes per river-level decision node and spot).
    tree may also be a SEQUENCE of TurnTrees with tree_of (pk_solve_turn_trees), as solve_river_batch takes them.
    lock, locked (turn-level rows) and river_lock, river_locked (river-level rows, each for all river cards at once; river_locked of
    river_strategy's shape): pk_solve_turn_locked, as solve_river_batch takes them.  A TurnSolution as locked also serves as river_locked
    where that is None and river_lock is given.  iters may then be 0.
    reach, at, at_card (pk_solve_turn_resolve): as solve_river_batch takes reach (up to 2^17 - 1; ranges << 1 is the same call) and at;
    at_card, Card.value integers [m] or one, names the river card under which a river-level node is reported.
    state, keep_state (pk_solve_turn_resume): as solve_river_batch takes them; the state also holds river_regret and river_average, of
    river_strategy's shape (solver_state_bytes(tree, m) in all: 4.4 MB per river-level row, spot and array)."""
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 4:
        raise ValueError("board must have shape [m, 4]")
    m = board.shape[0]
    resume = state is not None or keep_state
    resolve = resume or reach is not None or at is not None or at_card is not None
    ranges, reach = _resolve_ranges(ranges, reach, m, TURN_REACH_MAX)
    at, at_card = _resolve_at(at, m), _resolve_at(at_card, m, "at_card")
    node = _node_outputs(at, m)
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError("dead must have shape [m]")
    rows = None if isinstance(tree, RiverTree) else _TreeRows(tree, TURN_MAX_NODES)
    if rows is None and tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    trees = None if rows is None else rows.trees
    Dt = max(len(t.decision_nodes) for t in (trees or [tree]))
    Dr = max(len(t.river_decision_nodes) for t in (trees or [tree]))
    strategy = np.zeros((m, Dt, 4, L.EQ_HOLDINGS), np.uint16)
    rstrat = np.zeros((m, Dr, 52, 4, L.EQ_HOLDINGS), np.uint16) if river_strategy else None
    value, br = np.zeros((m, 2, L.EQ_HOLDINGS), np.int64), np.zeros((m, 2, L.EQ_HOLDINGS), np.int64)
    status = np.zeros(m, np.uint8)
    if resolve or any(x is not None for x in (lock, locked, river_lock, river_locked)):
        if river_locked is None and river_lock is not None and isinstance(locked, TurnSolution):
            river_locked = locked
        lrows = rows or _TreeRows([tree], TURN_MAX_NODES)
        if rows is not None:
            tree, tree_of = None, _tree_of(tree_of, len(trees), m)
        lock, locked = _lock_pair(lock, locked, m, Dt, (4, L.EQ_HOLDINGS), ("lock", "locked"), "strategy")
        river_lock, river_locked = _lock_pair(river_lock, river_locked, m, Dr, (52, 4, L.EQ_HOLDINGS), ("river_lock", "river_locked"), "river_strategy")
        if resume:
            nr, nv, nb = node or (None, None, None)
            st = _state_arrays(state, keep_state, m, Dt, Dr)
            L.check(L.lib().pk_solve_turn_resume(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *lrows.args(), L.ptr(tree_of), int(iters),
                                                 L.ptr(lock), L.ptr(locked), L.ptr(river_lock), L.ptr(river_locked), L.ptr(reach), L.ptr(at),
                                                 L.ptr(at_card), L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]), L.ptr(st[3]), L.ptr(st[4]), L.ptr(strategy),
                                                 L.ptr(rstrat), L.ptr(value), L.ptr(br), L.ptr(nr), L.ptr(nv), L.ptr(nb), L.ptr(status)))
            state = _new_state(st, iters, status)
        elif resolve:
            nr, nv, nb = node or (None, None, None)
            L.check(L.lib().pk_solve_turn_resolve(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *lrows.args(), L.ptr(tree_of), int(iters),
                                                  L.ptr(lock), L.ptr(locked), L.ptr(river_lock), L.ptr(river_locked), L.ptr(reach), L.ptr(at),
                                                  L.ptr(at_card), L.ptr(strategy), L.ptr(rstrat), L.ptr(value), L.ptr(br), L.ptr(nr), L.ptr(nv),
                                                  L.ptr(nb), L.ptr(status)))
        else:
            L.check(L.lib().pk_solve_turn_locked(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *lrows.args(), L.ptr(tree_of),
                                                 int(iters),
                                                 L.ptr(lock), L.ptr(locked), L.ptr(river_lock), L.ptr(river_locked), L.ptr(strategy), L.ptr(rstrat),
                                                 L.ptr(value), L.ptr(br), L.ptr(status)))
    elif rows is None:
        L.check(L.lib().pk_solve_turn(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *_tree_args(tree), int(iters), L.ptr(strategy),
                                      L.ptr(rstrat), L.ptr(value), L.ptr(br), L.ptr(status)))
    else:
        tree, tree_of = None, _tree_of(tree_of, len(trees), m)
        L.check(L.lib().pk_solve_turn_trees(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters),
                                            L.ptr(strategy), L.ptr(rstrat), L.ptr(value), L.ptr(br), L.ptr(status)))
    board5 = np.concatenate([board, np.zeros((m, 1), np.uint8)], axis=1)
    valid = rvr_valid_holdings(board5, np.full(m, 4, np.uint8), dead) & (status == 0)[:, None]
    pool = np.where(status == 0, valid.sum(axis=1), 0)
    pool = np.array([int(round((1 + math.sqrt(1 + 8 * int(x))) / 2)) if x else 0 for x in pool])      # C(P, 2) valid holdings -> P
    return TurnSolution(tree, ranges, strategy, rstrat, value, br, status, valid, pool, trees, tree_of, node=node, reach=reach, state=state)


def solve_turn_d(m, board_d, ranges_d, tree, iters, dead_d=None, strategy_d=None, river_strategy_d=None, value_d=None, br_d=None, status_d=None,
                 device=0, stream=None, tree_of=None, lock=None, locked=None, river_lock=None, river_locked=None, reach=None, at=None, at_card=None,
                 node_reach_d=None, node_value_d=None, node_br_d=None, t0_d=None, regret_d=None, average_d=None, river_regret_d=None, river_average_d=None):
    """pk_solve_turn_d: the same on device-resident buffers (device pointers as ints / c_void_p; the tree stays a host TurnTree; dead_d and
    the outputs may be None), asynchronous on `stream`.  With a SEQUENCE of trees (pk_solve_turn_trees_d) tree_of is the DEVICE pointer of
    uint32 [m], as solve_river_d takes it; the strategies have the rows of the largest tree passed.  lock, locked, river_lock,
    river_locked (pk_solve_turn_locked_d): DEVICE pointers, as solve_river_d takes them.  reach, at, at_card and node_reach_d,
    node_value_d, node_br_d (pk_solve_turn_resolve_d): DEVICE pointers, as solve_river_d takes them; ranges_d may then be None.  t0_d,
    regret_d, average_d, river_regret_d, river_average_d (pk_solve_turn_resume_d): DEVICE pointers, the state, worked in place."""
    if any(x is not None for x in (t0_d, regret_d, average_d, river_regret_d, river_average_d)):
        one = isinstance(tree, RiverTree)
        if one == (tree_of is not None):
            raise ValueError("tree_of, the device pointer of uint32 [m], comes with a sequence of trees and only with one")
        L.check(L.lib().pk_solve_turn_resume_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows([tree] if one else tree, TURN_MAX_NODES).args(),
                                               tree_of, int(iters), lock, locked, river_lock, river_locked, reach, at, at_card, t0_d, regret_d, average_d,
                                               river_regret_d, river_average_d, strategy_d, river_strategy_d, value_d, br_d, node_reach_d, node_value_d,
                                               node_br_d, status_d, stream))
        return
    if any(x is not None for x in (reach, at, at_card, node_reach_d, node_value_d, node_br_d)):
        one = isinstance(tree, RiverTree)
        if one == (tree_of is not None):
            raise ValueError("tree_of, the device pointer of uint32 [m], comes with a sequence of trees and only with one")
        L.check(L.lib().pk_solve_turn_resolve_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows([tree] if one else tree, TURN_MAX_NODES).args(),
                                                tree_of, int(iters), lock, locked, river_lock, river_locked, reach, at, at_card, strategy_d,
                                                river_strategy_d, value_d, br_d, node_reach_d, node_value_d, node_br_d, status_d, stream))
        return
    if any(x is not None for x in (lock, locked, river_lock, river_locked)):
        one = isinstance(tree, RiverTree)
        if one == (tree_of is not None):
            raise ValueError("tree_of, the device pointer of uint32 [m], comes with a sequence of trees and only with one")
        L.check(L.lib().pk_solve_turn_locked_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows([tree] if one else tree, TURN_MAX_NODES).args(),
                                               tree_of, int(iters), lock, locked, river_lock, river_locked, strategy_d, river_strategy_d, value_d, br_d,
                                               status_d, stream))
        return
    if not isinstance(tree, RiverTree):
        if tree_of is None:
            raise ValueError("a sequence of trees needs tree_of, the device pointer of uint32 [m]")
        L.check(L.lib().pk_solve_turn_trees_d(int(device), int(m), board_d, dead_d, ranges_d, *_TreeRows(tree, TURN_MAX_NODES).args(), tree_of, int(iters),
                                              strategy_d, river_strategy_d, value_d, br_d, status_d, stream))
        return
    if tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    L.check(L.lib().pk_solve_turn_d(int(device), int(m), board_d, dead_d, ranges_d, *_tree_args(tree), int(iters), strategy_d, river_strategy_d,
                                    value_d, br_d, status_d, stream))


def solve_turn(board, ranges, tree, iters, dead=(), river_strategy=False, device=0, lock=None, locked=None, river_lock=None, river_locked=None,
               reach=None, at=None, at_card=None, state=None, keep_state=False):
    """One subgame.  board: the four board cards; ranges: [2, 1326] integers 0 .. 65535 over holding_index, player 0 (first to act on
    both streets) then player 1; dead: cards known to be out of play.  Raises ValueError for an invalid spot.  A reach starts at
    weight << 1 and every split rounds down: scale a range so that its largest weight uses the sixteen bits.  reach [2, 1326] (ranges may
    then be None), at (a node index) and at_card (a Card-like, 'RS' string or Card.value): as solve_turn_batch takes them."""
    board = list(board)
    if len(board) != 4:
        raise ValueError("four board cards")
    b = np.array([[_card(c) for c in board]], np.uint8)
    d = np.array([dead if isinstance(dead, (int, np.integer)) else dead_mask(dead)], np.uint64)
    r = solve_turn_batch(b, _one_spot(ranges), tree, iters, d, river_strategy=river_strategy, device=device, lock=lock, locked=locked,
                         river_lock=river_lock, river_locked=river_locked, reach=_one_spot(reach), at=at,
                         at_card=None if at_card is None else int(_card(at_card)), state=state, keep_state=keep_state)[0]
    if state is not None and r.status == L.EQ_BAD_ITER:
        raise ValueError("the state's iterations and iters together exceed %d" % MAX_ITERS)
    if r.status:
        raise ValueError("invalid spot: " + equity_status_text(r.status))
    return r


def solve_turn_until_batch(board, ranges, tree, target, step=64, max_iters=MAX_ITERS, dead=None, river_strategy=False, device=0, tree_of=None, lock=None,
                           locked=None, river_lock=None, river_locked=None, reach=None):
    """solve_river_until_batch for the turn solver: solve_turn_batch's arguments, calls of `step` iterations with the state in DEVICE memory
    (solver_state_bytes(tree, m) of it: 4.4 MB per river-level row, spot and array) until every solved spot's exploitability is at or
    under `target` chips or max_iters iterations have run -> the last call's TurnSolution with .iters, .trace float64 [calls, m] and .state
    on the host.  river_strategy=True: the river-level strategies too, from the last call."""
    from . import hipmem
    step, max_iters = int(step), int(max_iters)
    if step < 1 or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError("step >= 1 and max_iters in 1 .. %d" % MAX_ITERS)
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 4:
        raise ValueError("board must have shape [m, 4]")
    m = board.shape[0]
    ranges, reach = _resolve_ranges(ranges, reach, m, TURN_REACH_MAX)
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError("dead must have shape [m]")
    one = isinstance(tree, RiverTree)
    if one and tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    trees = [tree] if one else list(tree)
    Dt, Dr = max(len(t.decision_nodes) for t in trees), max(len(t.river_decision_nodes) for t in trees)
    tree_of = None if one else _tree_of(tree_of, len(trees), m)
    if river_locked is None and river_lock is not None and isinstance(locked, TurnSolution):
        river_locked = locked
    lock, locked = _lock_pair(lock, locked, m, Dt, (4, L.EQ_HOLDINGS), ("lock", "locked"), "strategy")
    river_lock, river_locked = _lock_pair(river_lock, river_locked, m, Dr, (52, 4, L.EQ_HOLDINGS), ("river_lock", "river_locked"), "river_strategy")
    trows, rrows, pair = m * Dt * 4 * L.EQ_HOLDINGS, m * Dr * 52 * 4 * L.EQ_HOLDINGS, m * 2 * L.EQ_HOLDINGS
    bufs = []

    def dev(a=None, nbytes=0):
        if a is None and not nbytes:
            return None
        b = hipmem.DeviceBuffer(a.nbytes if a is not None else max(nbytes, 8), device)
        bufs.append(b)
        return b.upload(a) if a is not None else b
    ptr = lambda b: None if b is None else b.ptr
    try:
        ins = [dev(a) for a in (board, dead, ranges, tree_of, lock, locked, river_lock, river_locked, reach)]
        t0 = np.zeros(m, np.uint32)
        t0_d = dev(t0)
        state_d = [dev(nbytes=max(trows, 1) * 8), dev(nbytes=max(trows, 1) * 8), dev(nbytes=max(rrows, 1) * 8), dev(nbytes=max(rrows, 1) * 8)]
        strategy_d, rstrat_d = dev(nbytes=trows * 2), dev(nbytes=rrows * 2) if river_strategy else None
        value_d, br_d, status_d = dev(nbytes=pair * 8), dev(nbytes=pair * 8), dev(nbytes=m)
        board5 = np.concatenate([board, np.zeros((m, 1), np.uint8)], axis=1)
        trace, done = [], 0
        while True:
            it = min(step, max_iters - done)
            t0_d.upload(t0)
            last = done + it >= max_iters
            solve_turn_d(m, ptr(ins[0]), ptr(ins[2]), tree, it, dead_d=ptr(ins[1]), strategy_d=strategy_d.ptr, river_strategy_d=ptr(rstrat_d), value_d=value_d.ptr,
                         br_d=br_d.ptr, status_d=status_d.ptr, device=device, tree_of=ptr(ins[3]), lock=ptr(ins[4]), locked=ptr(ins[5]), river_lock=ptr(ins[6]),
                         river_locked=ptr(ins[7]), reach=ptr(ins[8]), t0_d=t0_d.ptr, regret_d=state_d[0].ptr, average_d=state_d[1].ptr,
                         river_regret_d=state_d[2].ptr, river_average_d=state_d[3].ptr)
            value, br = (b.download(np.int64, pair).reshape(m, 2, L.EQ_HOLDINGS) for b in (value_d, br_d))
            status = status_d.download(np.uint8, m)
            valid = rvr_valid_holdings(board5, np.full(m, 4, np.uint8), dead) & (status == 0)[:, None]
            pool = np.array([int(round((1 + math.sqrt(1 + 8 * int(x))) / 2)) if x else 0 for x in np.where(status == 0, valid.sum(axis=1), 0)])
            sol = TurnSolution(tree if one else None, ranges, None, None, value, br, status, valid, pool, None if one else trees, tree_of, reach=reach)
            done += it
            t0 += np.uint32(it)
            trace.append([TurnSolution(None, _ith(ranges, i), None, None, value[i], br[i], status[i], valid[i], pool[i], reach=_ith(reach, i)).exploitability
                          if status[i] == 0 else float("nan") for i in range(m)])
            if last or all(not e > target for e in trace[-1]):
                break
        sol.strategy = strategy_d.download(np.uint16, trows).reshape(m, Dt, 4, L.EQ_HOLDINGS)
        if river_strategy:
            sol.river_strategy = rstrat_d.download(np.uint16, rrows).reshape(m, Dr, 52, 4, L.EQ_HOLDINGS)
        regret, average = (b.download(np.int64, trows).reshape(m, Dt, 4, L.EQ_HOLDINGS) for b in state_d[:2])
        rregret, raverage = (b.download(np.int64, rrows).reshape(m, Dr, 52, 4, L.EQ_HOLDINGS) for b in state_d[2:])
        sol.state = SolverState(regret, average, np.where(status == 0, done, 0).astype(np.uint32), rregret, raverage)
        sol.iters, sol.trace = done, np.array(trace, np.float64).reshape(len(trace), m)
        return sol
    finally:
        for b in bufs:
            b.free()


def solve_turn_until(board, ranges, tree, target, step=64, max_iters=MAX_ITERS, dead=(), river_strategy=False, device=0, lock=None, locked=None,
                     river_lock=None, river_locked=None, reach=None):
    """One subgame solved to a target: solve_turn's arguments, solve_turn_until_batch's rule -> its TurnSolution (.iters, .trace float64
    [calls], .state).  Raises ValueError for an invalid spot."""
    board = list(board)
    if len(board) != 4:
        raise ValueError("four board cards")
    b = np.array([[_card(c) for c in board]], np.uint8)
    d = np.array([dead if isinstance(dead, (int, np.integer)) else dead_mask(dead)], np.uint64)
    full = solve_turn_until_batch(b, _one_spot(ranges), tree, target, step, max_iters, d, river_strategy=river_strategy, device=device, lock=lock, locked=locked,
                                  river_lock=river_lock, river_locked=river_locked, reach=_one_spot(reach))
    r = full[0]
    if r.status:
        raise ValueError("invalid spot: " + equity_status_text(r.status))
    r.iters, r.trace = full.iters, full.trace[:, 0]
    return r


def evaluate_turn_batch(board, ranges, tree, strategy, river_strategy, dead=None, device=0, tree_of=None, return_river_strategy=False):
    """The values and best responses of a SUPPLIED strategy pair: solve_turn_batch with every turn-level and river-level row locked and no
    iteration -> an ordinary TurnSolution (solution[i].ev, .exploitability)."""
    trees = [tree] if isinstance(tree, RiverTree) else list(tree)
    return solve_turn_batch(board, ranges, tree, 0, dead, river_strategy=return_river_strategy, device=device, tree_of=tree_of,
                            lock=np.ones(max(len(t.decision_nodes) for t in trees), bool), locked=strategy,
                            river_lock=np.ones(max(len(t.river_decision_nodes) for t in trees), bool), river_locked=river_strategy)


def evaluate_turn(board, ranges, tree, strategy, river_strategy, dead=(), device=0):
    """One subgame: the value of (strategy, river_strategy) -- integer arrays or TurnSolutions -- and how exploitable it is."""
    return solve_turn(board, ranges, tree, 0, dead, device=device, lock=np.ones(len(tree.decision_nodes), bool), locked=strategy,
                      river_lock=np.ones(len(tree.river_decision_nodes), bool), river_locked=river_strategy)


# ---------------------------------------------------------------------------------------------------------------- the pre-flop solver
def _blinds(stack, sb, bb, ante):
    stack, sb, bb, ante = int(stack), int(sb), int(bb), int(ante)
    if not 0 < sb <= bb <= stack or ante < 0:
        raise ValueError("0 < sb <= bb <= stack and ante >= 0")
    return stack, sb, bb, ante


def push_fold_tree(stack, sb=1, bb=2, ante=0):
    """The push / fold game as a RiverTree of five nodes: player 0 (the small blind, first to act heads-up) folds or jams; facing the jam,
    player 1 folds or calls, and a call is a showdown.  stack: the effective stack in chips BEFORE the blinds (after the ante), so a jam
    puts `stack` in.  put[root] = (sb, bb), pot = 2 * ante.  Nodes: 0 the root, 1 "0:fold", 2 "0:jam" (player 1 to act), 3 "1:fold",
    4 "1:call" (the showdown).  The showdown is paid by the exact all-in equity: there is no post-flop betting (solve_preflop)."""
    stack, sb, bb, ante = _blinds(stack, sb, bb, ante)
    kind = [KIND_P0, KIND_FOLD0, KIND_P1, KIND_FOLD1, KIND_SHOWDOWN]
    F = NO_CHILD
    child = [[1, 2, F, F], [F] * 4, [3, 4, F, F], [F] * 4, [F] * 4]
    put = [[sb, bb], [sb, bb], [stack, bb], [stack, bb], [stack, stack]]
    actions = [None, (0, "0:fold"), (0, "0:jam"), (2, "1:fold"), (2, "1:call")]
    return RiverTree(kind, child, put, 2 * ante, actions)


def preflop_tree(stack, sb=1, bb=2, ante=0, bet_fractions=(1.0,), max_raises=3, limp=True):
    """A pre-flop betting round as a RiverTree: river_tree's rule, started with the big blind as an outstanding bet.  put[root] = (sb, bb),
    pot = 2 * ante; player 0 (the small blind) may fold, call (limp; not offered with limp=False) or raise; after a limp player 1 may
    check, which is a showdown, or raise; from there on everything is river_tree's: fold, call (a showdown) or raise, sizes = max(1,
    floor(fraction * pot after calling)) on top of the call.  The blind does not count among max_raises.  Amounts are capped at `stack`,
    the effective stack in chips before the blinds (after the ante).  At most 64 nodes and four actions a node (ValueError beyond).
    Every showdown is paid by the exact all-in equity, whatever the puts: there is no post-flop betting (solve_preflop)."""
    stack, sb, bb, ante = _blinds(stack, sb, bb, ante)
    max_raises = int(max_raises)
    if max_raises < 0:
        raise ValueError("max_raises must be non-negative")
    b = _Builder(2 * ante, stack, MAX_NODES)
    b.betting_round(b.new(KIND_P0, sb, bb, None, None), bet_fractions, max_raises, lambda p0, p1, n, text: b.new(KIND_SHOWDOWN, p0, p1, n, text),
                    limp=bool(limp))
    return RiverTree(b.kind, b.child, b.put, 2 * ante, b.actions)


def preflop_trees(stacks, sb=1, bb=2, ante=0, bet_fractions=(1.0,), max_raises=3, limp=True, push_fold=False):
    """(trees, tree_of) for spots of per-spot stacks: stacks is an integer array [m]; one preflop_tree (push_fold=True: push_fold_tree) per
    DISTINCT stack, in the order the stacks first appear, and tree_of uint32 [m] -- what solve_preflop_batch takes."""
    stacks = np.asarray(stacks).reshape(-1)
    index, trees, tree_of = {}, [], np.zeros(stacks.shape[0], np.uint32)
    for i, key in enumerate(stacks.tolist()):
        if key not in index:
            index[key] = len(trees)
            trees.append(push_fold_tree(key, sb, bb, ante) if push_fold else preflop_tree(key, sb, bb, ante, bet_fractions, max_raises, limp))
        tree_of[i] = index[key]
    return trees, tree_of


_PAIR_A = np.array([a for b in range(52) for a in range(b)])
_PAIR_B = np.array([b for b in range(52) for a in range(b)])


def holding_class(h):
    """The class 0 .. 168 of holding index h (an integer or an integer array): the cell 13 * row + column of the 13 x 13 chart over
    ace-high rank indices 0 (deuce) .. 12 (ace).  A pair of rank r is cell (r, r); a suited holding of ranks hi > lo is (hi, lo); an
    off-suit one is (lo, hi).  6 holdings a pair class, 4 a suited one, 12 an off-suit one."""
    h = np.asarray(h)
    a, b = _PAIR_A[h], _PAIR_B[h]
    ra, rb = (a // 4 + 12) % 13, (b // 4 + 12) % 13          # (canonical index = 4 * rank0 + suit, and rank0 0 is the ace)
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    suited = (a % 4 == b % 4) & (lo != hi)
    out = np.where(suited, 13 * hi + lo, 13 * lo + hi)
    return int(out) if out.ndim == 0 else out


class PreflopSolution(RiverSolution):
    """What pk_solve_preflop returns for one spot or a batch: RiverSolution's fields and properties (strategy uint16 [D, 4, 1326], value and
    br int64 [2, 1326], status, ev, exploitability, probabilities, solution[i]) for a spot without a board: every holding is valid."""

    def __getitem__(self, i):
        r = RiverSolution.__getitem__(self, i)
        return PreflopSolution(r.tree, r.ranges, r.strategy, r.value, r.br, r.status, r.valid)

    def by_class(self, node):
        """float64 [actions, 13, 13]: the action probabilities at decision node `node` averaged over the holdings of each class
        (holding_class: cell [row, column]), weighted by the ACTOR's range weight; nan where the class has no weight.  A chart for the eye:
        the counts behind the solution are NOT suit-symmetric (the evaluator's suit quirks are carried by the matchup table: DESIGN.md
        section 3.10), so the holdings of one class need not play alike, and the solver does not make them."""
        self._one()
        p = self.probabilities(node)
        w = np.asarray(self.ranges, np.float64)[int(self.tree.kind[int(node)])] * self.valid
        cls = holding_class(np.arange(L.EQ_HOLDINGS))
        den = np.bincount(cls, w, 169)
        out = np.full((p.shape[0], 169), np.nan)
        for a in range(p.shape[0]):
            num = np.bincount(cls, np.where(w > 0, w * np.nan_to_num(p[a]), 0.0), 169)
            out[a] = np.divide(num, den, out=out[a], where=den > 0)
        return out.reshape(-1, 13, 13)

    def __repr__(self):
        return "PreflopSolution(status=%r)" % (self.status,)


def _preflop_ranges(ranges, m=None):
    ranges = np.ascontiguousarray(ranges, np.uint16)
    if ranges.ndim != 3 or ranges.shape[1:] != (2, L.EQ_HOLDINGS) or (m is not None and ranges.shape[0] != m):
        raise ValueError("ranges must have shape [m, 2, 1326]")
    return ranges


def solve_preflop_batch(ranges, tree, iters, tree_of=None, device=0):
    """pk_solve_preflop on host arrays: ranges uint16 [m, 2, 1326] over holding_index (player 0, the small blind and first to act, then
    player 1), one tree for the call or a SEQUENCE of trees with tree_of, an integer array [m] (None: spot i uses tree i, which needs m
    trees) -> PreflopSolution with a leading [m].  A spot whose tree_of names no tree has status PK_EQ_BAD_TREE and all-zero outputs.
    Showdowns are paid by the exact all-in equity of the two holdings (the resident matchup table, built on the first call): the game has
    no post-flop betting."""
    ranges = _preflop_ranges(ranges)
    m = ranges.shape[0]
    one = isinstance(tree, RiverTree)
    if one and tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    rows = _TreeRows([tree] if one else tree, MAX_NODES)
    trees, tree, tree_of = (None, tree, None) if one else (rows.trees, None, _tree_of(tree_of, len(rows.trees), m))
    D = max(len(t.decision_nodes) for t in rows.trees)
    strategy = np.zeros((m, D, 4, L.EQ_HOLDINGS), np.uint16)
    value, br = np.zeros((m, 2, L.EQ_HOLDINGS), np.int64), np.zeros((m, 2, L.EQ_HOLDINGS), np.int64)
    status = np.zeros(m, np.uint8)
    L.check(L.lib().pk_solve_preflop(int(device), m, L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters), L.ptr(strategy), L.ptr(value), L.ptr(br),
                                     L.ptr(status)))
    valid = np.ones((m, L.EQ_HOLDINGS), bool) & (status == 0)[:, None]
    return PreflopSolution(tree, ranges, strategy, value, br, status, valid, trees, tree_of)


def solve_preflop_d(m, ranges_d, tree, iters, tree_of=None, strategy_d=None, value_d=None, br_d=None, status_d=None, device=0, stream=None):
    """pk_solve_preflop_d: the same on device-resident buffers (device pointers as ints / c_void_p; the trees stay host RiverTrees; the
    outputs except status_d may be None), asynchronous on `stream`.  With a SEQUENCE of trees tree_of is the DEVICE pointer of uint32 [m]
    (None: every spot uses tree 0) and strategy_d holds [m, Dmax, 4, 1326], Dmax the most decision nodes of any tree passed."""
    one = isinstance(tree, RiverTree)
    if one and tree_of is not None:
        raise ValueError("tree_of needs a sequence of trees")
    L.check(L.lib().pk_solve_preflop_d(int(device), int(m), ranges_d, *_TreeRows([tree] if one else tree, MAX_NODES).args(), tree_of, int(iters),
                                       strategy_d, value_d, br_d, status_d, stream))


def solve_preflop(ranges, tree, iters, device=0):
    """One pre-flop spot.  ranges: [2, 1326] integers 0 .. 65535 over holding_index, player 0 (the small blind, first to act) then player 1;
    tree: push_fold_tree / preflop_tree, or any RiverTree of kinds 0 .. 4.  A reach starts at weight << 4 and every split rounds down:
    scale a range so that its largest weight uses the sixteen bits."""
    r = solve_preflop_batch(_preflop_ranges(np.asarray(ranges)[None], 1), tree, iters, device=device)[0]
    if r.status:
        raise ValueError("invalid spot: " + equity_status_text(r.status))
    return r
