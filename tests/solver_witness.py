"""A witness that cannot wrap (TEST INFRASTRUCTURE): the iterations and final passes of one river or turn spot of a resuming call in PYTHON
INTEGERS, written from include/pokerl_hip.h ("River solver", "Turn solver", "Resuming a solve") as a recursive walk.  It shares no
arithmetic with river_solver_spec.tree_pass / resolve_spec.river_pass / turn_solver_spec.tree_pass, which run in numpy int64 and would wrap
exactly where a kernel does.  What it takes from the restatements is structure only: the beats / ties / loses matrices of
river_solver_spec.pairwise (through turn_solver_spec.Spot on the turn) and the order of the holdings.  The sums over the opponent's
holdings at a terminal are formed in int64, but only after the sum of the reaches has been checked, in Python integers, to be below the
bound the header states; everything after that -- the chips, the chance node's sum, sigma u, regrets, accumulators, the rule -- is Python
integers.  While it runs it records the largest value of every quantity the header's BOUNDS paragraphs bound; check_bounds() holds them
against the figures stated THERE.  One spot, ranges only (no reach, lock, given or at)."""
import math

import numpy as np

import river_solver_spec as RS
import turn_solver_spec as TS

ONE = 32768
H = 1326
P0, P1, FOLD0, FOLD1, SHOWDOWN, CHANCE = 0, 1, 2, 3, 4, 5
CLAMP = {5: ((1 << 58) - 1, (1 << 44) - 1), 4: ((1 << 60) - 1, (1 << 41) - 1)}     # RMAX, AMAX of "Resuming a solve": LOAD
# The header's own figures, as exclusive upper bounds.  River: "River solver" BOUNDS and "Resuming a solve" BOUNDS (river); turn: "Turn
# solver" BOUNDS and "Resuming a solve" BOUNDS (turn).  A regret and an accumulator are held against the RESUMED bound (a start at the clamp).
BOUNDS = {5: {"reach": 2 ** 20, "reach_sum": 2 ** 31, "terminal_u": 2 ** 45, "u": 2 ** 45, "sigma_u": 2 ** 60, "regret_step": 2 ** 46, "regret": 2 ** 59,
              "average": 2 ** 45, "numerator": 2 ** 46, "divisor": 2 ** 33},
          4: {"reach": 2 ** 17, "reach_sum": 1128 * 2 ** 17, "terminal_u": 2 * 8191 * 1128 * 2 ** 17 + 1, "chance_u": 2 ** 46.7, "u": 2 ** 46.7,
              "sigma_u": 2 ** 61.7, "regret_step": 2 ** 47.7, "regret": 2 ** 60.3, "average": 2 ** 42, "numerator": 2 ** 46, "divisor": 2 ** 33}}


class Record(dict):
    def see(self, key, values):
        v = max(values, default=0)
        if v > self.get(key, 0):
            self[key] = v

    def bits(self):
        """{quantity: log2 of (the largest value + 1)}, to two places: 'below 2^x'"""
        return {k: round(math.log2(v + 1), 2) for k, v in sorted(self.items())}


def check_bounds(street, rec):
    """every recorded quantity below the header's figure for it; every figure of the header recorded"""
    want = BOUNDS[street]
    assert set(rec) == set(want), (sorted(rec), sorted(want))
    for k, v in rec.items():
        assert v < want[k], (k, v, math.log2(v + 1), math.log2(want[k]))


def rule(X, rec):
    """STRATEGY FROM NON-NEGATIVE INTEGERS on one holding's entries"""
    nact, mx = len(X), max(X)
    if mx == 0:
        sig = [ONE // nact] * nact
    else:
        sh = max(0, mx.bit_length() - 31)
        Xp = [x >> sh for x in X]
        S = sum(Xp)
        rec.see("numerator", [x << 15 for x in Xp])
        rec.see("divisor", [S])
        sig = [(x << 15) // S for x in Xp]
    sig[0] = ONE - sum(sig[1:])
    return sig


def rule_rows(X, rec):
    """X[a][h] -> sigma[a][h]"""
    cols = [rule([X[a][h] for a in range(len(X))], rec) for h in range(len(X[0]))]
    return [[c[a] for c in cols] for a in range(len(X))]


class Witness:
    """One spot.  Holdings are numbered as the restatements number them (pool order); set(j) is the list of those without river card j
    (turn), or all of them (river, j = None)."""

    def __init__(self, street, board, dead, tree):
        self.street, self.rec = street, Record()
        self.T = TS.as_tree(tree) if street == 4 else RS.as_tree(tree)
        T = self.T
        self.river_level = T.river if street == 4 else [True] * T.n
        if street == 5:
            status, gone = RS.check_spot([int(c) for c in board], int(dead))
            assert not status
            self.hidx, beats, ties, loses = RS.pairwise([int(c) for c in board], gone)
            self.cards = [None]
            self.sets = {None: list(range(len(self.hidx)))}
            self.M = {None: (beats, ties, loses)}
            self.K = 1
        else:
            status, gone = TS.check_spot([int(c) for c in board], int(dead))
            assert not status
            sp = TS.spot_of([int(c) for c in board], gone)
            self.hidx, self.disjoint, self.K = sp.hidx, sp.disjoint, sp.P - 4
            self.cards = [k for k, _, _ in sp.river]
            self.sets = {k: [int(i) for i in idx] for k, idx, _ in sp.river}
            self.sets[None] = list(range(len(sp.hidx)))
            self.M = {k: sp.matrices(res) for k, _, res in sp.river}
        self.n = len(self.hidx)
        self.limits = BOUNDS[street]

    # -------------------------------------------------------------------------------------------- one pass
    def sums(self, mats, rq):
        """the opponent's reach summed over what each holding beats, ties and loses to -> three lists of Python integers"""
        total = sum(rq)                                              # Python integers
        self.rec.see("reach_sum", [total])
        assert total < self.limits["reach_sum"] and all(0 <= x < self.limits["reach"] for x in rq), "a terminal sum would leave what int64 is trusted with"
        v = np.array(rq, np.int64)
        return [[int(x) for x in (m @ v)] for m in mats]

    def terminal(self, n, r, j, best):
        T, k, rec = self.T, self.T.kind[n], self.rec
        u = []
        for p in (0, 1):
            rq = r[1 - p]
            if k == SHOWDOWN:
                W, Ti, L = self.sums(self.M[j], rq)
                c = T.put[n][0]
                u.append([2 * (T.pot + c) * w + T.pot * t - 2 * c * l for w, t, l in zip(W, Ti, L)])
            else:
                f = k - FOLD0
                if self.river_level[n]:
                    b, t, l = self.M[j]
                    S, scale = self.sums([b + t + l], rq)[0], 1
                else:
                    S, scale = self.sums([self.disjoint], rq)[0], self.K
                chips = -2 * T.put[n][f] if p == f else 2 * (T.pot + T.put[n][f])
                u.append([chips * scale * s for s in S])
            # (a turn-level fold is in the chance node's units, x (P - 4): the header bounds it with the chance node)
            if best is None or best == p:                            # (in p's best-response pass everything of q is ignored)
                rec.see("terminal_u" if self.river_level[n] else "chance_u", [abs(x) for x in u[p]])
        return u

    def walk(self, n, r, j, sigma, best, seen):
        """-> [u_0, u_1] at node n for reaches r = [r_0, r_1] over the holdings of set(j); seen[(n, j)] = (r, u) for the updates"""
        T, k, rec = self.T, self.T.kind[n], self.rec
        rec.see("reach", r[0] + r[1])
        if k == CHANCE:
            u = [[0] * self.n, [0] * self.n]
            for c in self.cards:
                idx = self.sets[c]
                uc = self.walk(T.child[n][0], [[r[p][i] for i in idx] for p in (0, 1)], c, sigma, best, seen)
                for p in (0, 1):
                    for i, x in zip(idx, uc[p]):
                        u[p][i] += x
            rec.see("chance_u", [abs(x) for x in (u[0] + u[1] if best is None else u[best])])
        elif k > 1:
            u = self.terminal(n, r, j, best)
        else:
            p, ch = k, T.child[n]
            sig = sigma[n][j] if self.street == 4 and self.river_level[n] else sigma[n]
            below = []
            for a, c in enumerate(ch):
                rc = [r[0], r[1]]
                if best != p:
                    rc[p] = [(x * s) >> 15 for x, s in zip(r[p], sig[a])]
                below.append(self.walk(c, rc, j, sigma, best, seen))
            u = [None, None]
            if best == p:
                u[p] = [max(col) for col in zip(*[b[p] for b in below])]
            else:
                tot = [sum(s * x for s, x in zip(ss, xs)) for ss, xs in zip(zip(*sig), zip(*[b[p] for b in below]))]
                if best is None:                                     # (in p's best-response pass q's values are ignored: they count p's reach twice)
                    rec.see("sigma_u", [abs(x) for x in tot])
                u[p] = [x // ONE for x in tot]                       # (Python's // floors, as the definition does)
            u[1 - p] = [sum(col) for col in zip(*[b[1 - p] for b in below])]
        rec.see("u", [abs(x) for x in (u[0] + u[1] if best is None else u[best])])     # (a best-response pass of p: everything of q is ignored)
        seen[(n, j)] = (r, u)
        return u

    def levels(self, d):
        return self.cards if self.street == 4 and self.river_level[d] else [None]

    def strategies(self, X):
        out = {}
        for d in self.T.decisions:
            if self.street == 4 and self.river_level[d]:
                out[d] = {j: rule_rows(X[d][j], self.rec) for j in self.cards}
            else:
                out[d] = rule_rows(X[d][None], self.rec)
        return out

    # -------------------------------------------------------------------------------------------- a call
    def where(self, d):
        """(index of the state array pair, row) of decision node d"""
        T = self.T
        if self.street == 4 and self.river_level[d]:
            return 1, T.river_decisions.index(d)
        return 0, (T.turn_decisions if self.street == 4 else T.decisions).index(d)

    def run(self, ranges, t0, iters, state):
        """state: the call's arrays (regret, average[, river_regret, river_average]), one spot's -> dict of the call's outputs and state"""
        T, rec = self.T, self.rec
        rmax, amax = CLAMP[self.street]
        shift = 4 if self.street == 5 else 1
        w = np.asarray(ranges).reshape(2, H)
        root = [[int(w[p][h]) << shift for h in self.hidx] for p in (0, 1)]
        state = [np.array(x, np.int64) for x in state]
        R, A = {}, {}
        for d in T.decisions:
            lvl, row = self.where(d)
            R[d], A[d] = {}, {}
            for j in self.levels(d):
                hs = [int(self.hidx[i]) for i in self.sets[j]]
                at = (row,) if j is None else (row, j)
                nact = len(T.child[d])
                if t0 > 0:
                    R[d][j] = [[min(max(int(state[2 * lvl][at + (a, h)]), 0), rmax) for h in hs] for a in range(nact)]
                    A[d][j] = [[min(max(int(state[2 * lvl + 1][at + (a, h)]), 0), amax) for h in hs] for a in range(nact)]
                else:
                    R[d][j], A[d][j] = [[0] * len(hs) for _ in range(nact)], [[0] * len(hs) for _ in range(nact)]
        for t in range(t0 + 1, t0 + iters + 1):
            seen = {}
            self.walk(0, root, None, self.strategies(R), None, seen)
            for d in T.decisions:
                p = T.kind[d]
                for j in self.levels(d):
                    ud = seen[(d, j)][1][p]
                    for a, c in enumerate(T.child[d]):
                        rc, uc = seen[(c, j)][0][p], seen[(c, j)][1][p]
                        rec.see("regret_step", [abs(x - y) for x, y in zip(uc, ud)])
                        R[d][j][a] = [max(0, x + y - z) for x, y, z in zip(R[d][j][a], uc, ud)]
                        A[d][j][a] = [x + t * y for x, y in zip(A[d][j][a], rc)]
                        rec.see("regret", R[d][j][a])
                        rec.see("average", A[d][j][a])
        if t0 == 0:
            for x in state:
                x[:] = 0
        sigma = self.strategies(A)
        out = dict(value=np.zeros((2, H), np.int64), br=np.zeros((2, H), np.int64), strategy=np.zeros(state[0].shape, np.uint16))
        if self.street == 4:
            out["river_strategy"] = np.zeros(state[2].shape, np.uint16)
        for d in T.decisions:
            lvl, row = self.where(d)
            for j in self.levels(d):
                hs = [int(self.hidx[i]) for i in self.sets[j]]
                at = (row,) if j is None else (row, j)
                sig = sigma[d] if j is None else sigma[d][j]
                for a in range(len(T.child[d])):
                    for i, h in enumerate(hs):
                        state[2 * lvl][at + (a, h)] = R[d][j][a][i]              # (numpy refuses a Python integer outside int64)
                        state[2 * lvl + 1][at + (a, h)] = A[d][j][a][i]
                        out["river_strategy" if lvl else "strategy"][at + (a, h)] = sig[a][i]
        u = self.walk(0, root, None, sigma, None, {})
        for p in (0, 1):
            ub = self.walk(0, root, None, sigma, p, {})
            out["value"][p, self.hidx] = u[p]
            out["br"][p, self.hidx] = ub[p]
        out.update(zip(("regret", "average", "river_regret", "river_average"), state))
        if self.street == 5:
            rec.pop("chance_u", None)
        return out


def run_call(street, call):
    """the witness on a one-spot call of solver_rule_cases.corner_call / rule_call -> (outputs with a leading [1], the record)"""
    assert len(call["board"]) == 1
    w = Witness(street, call["board"][0], call["dead"][0], call["trees"][0])
    out = w.run(call["ranges"][0], int(call["t0"][0]), int(call["iters"]), [x[0] for x in call["state"]])
    return {k: v[None] for k, v in out.items()}, w.rec
