"""The river subgame solver (pk_solve_river; the definition: include/pokerl_hip.h "River solver"): heads-up CFR+
over a caller-supplied betting tree, one subgame per workgroup on the device, in integers -- the same call gives the same bytes whatever
the grid.  river_tree builds a tree on the host; solve_river / solve_river_batch / solve_river_d run it."""
import math

import numpy as np

from . import _lib as L
from .judger import _card, dead_mask, equity_status_text, rvr_valid_holdings

ONE = 32768                 # a probability of 1 in the strategy's fixed point (Q15)
MAX_NODES, MAX_ACTIONS, MAX_CHIPS, MAX_ITERS = 64, 4, 8191, 4096
KIND_P0, KIND_P1, KIND_FOLD0, KIND_FOLD1, KIND_SHOWDOWN = 0, 1, 2, 3, 4
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
    kind, child, put, actions = [], [], [], []

    def new(k, p0, p1, parent, text):
        kind.append(k); child.append([NO_CHILD] * 4); put.append([p0, p1]); actions.append(None if parent is None else (parent, text))
        if len(kind) > MAX_NODES:
            raise ValueError("the tree has more than %d nodes: fewer bet sizes or raises" % MAX_NODES)
        return len(kind) - 1

    def sizes(p, puts, room):
        to_call = max(puts) - puts[p]
        after = pot + puts[0] + puts[1] + to_call
        left = stack - puts[p] - to_call
        out = []
        for f in bet_fractions:
            amount = min(max(1, int(math.floor(f * after))), left)
            if amount > 0 and amount not in out:
                out.append(amount)
        return out[:room]

    pending = [new(KIND_P0, 0, 0, None, None)]
    state = {0: (0, False, 0)}                       # node -> (actor, a check has been made, raises so far)
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
            kids.append(new(KIND_SHOWDOWN, pc[0], pc[1], n, "%d:call" % p))
            for amount in (sizes(p, puts, 2) if raises < max_raises else []):
                pr = list(puts); pr[p] = max(puts) + amount
                c = new(KIND_P0 + (1 - p), pr[0], pr[1], n, "%d:raise %d" % (p, amount))
                state[c] = (1 - p, True, raises + 1); pending.append(c); kids.append(c)
        else:
            if checked:
                kids.append(new(KIND_SHOWDOWN, puts[0], puts[1], n, "%d:check" % p))
            else:
                c = new(KIND_P0 + (1 - p), puts[0], puts[1], n, "%d:check" % p)
                state[c] = (1 - p, True, raises); pending.append(c); kids.append(c)
            for amount in (sizes(p, puts, 3) if raises < max_raises else []):
                pb = list(puts); pb[p] += amount
                c = new(KIND_P0 + (1 - p), pb[0], pb[1], n, "%d:bet %d" % (p, amount))
                state[c] = (1 - p, True, raises + 1); pending.append(c); kids.append(c)
        child[n][:len(kids)] = kids
    return RiverTree(kind, child, put, pot, actions)


class RiverSolution:
    """What pk_solve_river returns for one spot or a batch: strategy uint16 [D, 4, 1326] (the average strategy in Q15: 32768 = always;
    unused action slots and invalid holdings 0; a valid holding of weight 0, like any holding that never reached a node, gets the uniform
    row), value and br int64 [2, 1326] (the counterfactual value of every holding under `strategy`, and against it with the holder
    playing a best response; half-chips times the opponent's reach, which starts at weight << 4), status (PK_EQ_* bits).  A batch has a
    leading [m]."""

    def __init__(self, tree, ranges, strategy, value, br, status, valid):
        self.tree, self.ranges, self.strategy, self.value, self.br, self.status, self.valid = tree, ranges, strategy, value, br, status, valid

    def __getitem__(self, i):
        return RiverSolution(self.tree, self.ranges[i], self.strategy[i], self.value[i], self.br[i], self.status[i], self.valid[i])

    def _pair_weight(self):
        w = self.ranges.astype(np.int64) * self.valid
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
        """chips per player: sum_h w_p[h] value[p][h] / (32 sum over disjoint pairs of w_0 w_1); Python integers, one division each"""
        self._one()
        den = 32 * self._pair_weight()
        return tuple(sum(int(w) * int(v) for w, v in zip(self.ranges[p], self.value[p])) / den if den else float("nan") for p in (0, 1))

    @property
    def exploitability(self):
        """sum_p (br_p - value_p) reduced the same way, in chips"""
        self._one()
        den = 32 * self._pair_weight()
        num = sum(int(w) * (int(b) - int(v)) for p in (0, 1) for w, b, v in zip(self.ranges[p], self.br[p], self.value[p]))
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


def _tree_args(tree):
    return (int(tree.n), L.ptr(tree.kind), L.ptr(tree.child), L.ptr(tree.put), int(tree.pot))


def solve_river_batch(board, ranges, tree, iters, dead=None, device=0):
    """pk_solve_river on host arrays: board uint8 [m, 5] Card.value, ranges uint16 [m, 2, 1326] over holding_index, one tree for the call,
    dead uint64 [m] masks over canonical card indices (None: none) -> RiverSolution with a leading [m].  A bad spot is reported through
    its status with all-zero outputs; the others are unaffected."""
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 5:
        raise ValueError("board must have shape [m, 5]")
    m = board.shape[0]
    ranges = np.ascontiguousarray(ranges, np.uint16)
    if ranges.shape != (m, 2, L.EQ_HOLDINGS):
        raise ValueError("ranges must have shape [m, 2, 1326]")
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError("dead must have shape [m]")
    D = len(tree.decision_nodes)
    strategy = np.zeros((m, D, 4, L.EQ_HOLDINGS), np.uint16)
    value, br = np.zeros((m, 2, L.EQ_HOLDINGS), np.int64), np.zeros((m, 2, L.EQ_HOLDINGS), np.int64)
    status = np.zeros(m, np.uint8)
    L.check(L.lib().pk_solve_river(int(device), m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *_tree_args(tree), int(iters), L.ptr(strategy),
                                   L.ptr(value), L.ptr(br), L.ptr(status)))
    valid = rvr_valid_holdings(board, np.full(m, 5, np.uint8), dead) & (status == 0)[:, None]
    return RiverSolution(tree, ranges, strategy, value, br, status, valid)


def solve_river_d(m, board_d, ranges_d, tree, iters, dead_d=None, strategy_d=None, value_d=None, br_d=None, status_d=None, device=0, stream=None):
    """pk_solve_river_d: the same on device-resident buffers (device pointers as ints / c_void_p; the tree stays a host RiverTree; dead_d and
    the outputs may be None), asynchronous on `stream`."""
    L.check(L.lib().pk_solve_river_d(int(device), int(m), board_d, dead_d, ranges_d, *_tree_args(tree), int(iters), strategy_d, value_d, br_d,
                                     status_d, stream))


def solve_river(board, ranges, tree, iters, dead=(), device=0):
    """One subgame.  board: the five board cards (Card-likes / 'RS' strings / Card.value ints); ranges: [2, 1326] integers 0 .. 65535 over
    holding_index, player 0 (first to act) then player 1; dead: cards known to be out of play.  Raises ValueError for an invalid spot.
    A reach starts at weight << 4 and every split rounds down, so ranges of small integers (1, 2, ...) lose weight on the way down the
    tree: scale a range so that its largest weight uses the sixteen bits."""
    board = list(board)
    if len(board) != 5:
        raise ValueError("five board cards")
    b = np.array([[_card(c) for c in board]], np.uint8)
    d = np.array([dead if isinstance(dead, (int, np.integer)) else dead_mask(dead)], np.uint64)
    r = solve_river_batch(b, np.asarray(ranges)[None], tree, iters, d, device=device)[0]
    if r.status:
        raise ValueError("invalid spot: " + equity_status_text(r.status))
    return r
