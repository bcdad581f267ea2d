"""The pre-flop solver's bounds, witnessed (TEST INFRASTRUCTURE): the definition of include/pokerl_hip.h "Pre-flop solver" walked in PYTHON
INTEGERS, which cannot wrap, on tables of one weight g per disjoint pair -- G = 2 win + tie = g on every pair that shares no card: all-win
(g = 2 B), all-tie (g = B), all-lose (g = 0), the extremes of what a table can hold.  On such a table E(h) = g S(h), and S(h) is the total minus
the sums of the holding's two cards plus its own entry, all in Python integers; the product (pot + 2c) E is formed EXACTLY (it passes 2^64) and
floored once.  The walk records the largest E, product, |u|, |sum sigma u|, regret step, regret and accumulator it meets.  It shares no code
with tests/preflop_solver_spec.py; the test asserts that the two agree in every output, which they can only do if no int64 of the restatement
wrapped, and that every recorded value is inside the header's bound."""
import math

HOLDINGS = 1326
ONE = 32768
BOARDS = 1712304
CARDS = [(a, b) for b in range(52) for a in range(b)]
BOUNDS = {"E": 52, "product": 66, "u": 45, "sigma_u": 60, "step": 46, "regret": 58, "average": 44}     # each value stays below 2^x


def below(x):
    """x as "below 2^this" (0 for 0)"""
    return math.log2(x + 1) if x else 0.0


def rule(X):
    """the strategy rule on a list of non-negative Python integers"""
    nact, mx = len(X), max(X)
    if mx == 0:
        sig = [0] + [ONE // nact] * (nact - 1)
    else:
        sh = max(0, mx.bit_length() - 31)
        Xp = [x >> sh for x in X]
        S = sum(Xp)
        sig = [0] + [(x << 15) // S for x in Xp[1:]]
    sig[0] = ONE - sum(sig[1:])
    return sig


def disjoint_sums(r):
    """S[h]: the sum of r over the holdings that share no card with h"""
    per_card = [0] * 52
    for (a, b), x in zip(CARDS, r):
        per_card[a] += x
        per_card[b] += x
    total = sum(r)
    return [total - per_card[a] - per_card[b] + x for (a, b), x in zip(CARDS, r)]


def walk(kind, child, put, pot, g, weights, R, A, t0, iters):
    """kind [n], child [n] lists of children, put [n][2], pot; g: the weight of a disjoint pair; weights [2][1326]; R, A {decision node:
    [nact][1326]} Python integers (changed in place), the iterations t0 + 1 .. t0 + iters.  -> (strategy {node: [nact][1326]}, value [2][1326],
    br [2][1326], record)."""
    n = len(kind)
    decisions = [v for v in range(n) if kind[v] <= 1]
    rec = dict.fromkeys(BOUNDS, 0)

    def see(key, x):
        if abs(x) > rec[key]:
            rec[key] = abs(x)

    def one_pass(sigma, best=None):
        r = [{0: [w << 4 for w in weights[0]]}, {0: [w << 4 for w in weights[1]]}]
        u = [{}, {}]
        for v in range(n):
            k = kind[v]
            if k <= 1:
                for a, c in enumerate(child[v]):
                    r[k][c] = list(r[k][v]) if best == k else [(x * s) >> 15 for x, s in zip(r[k][v], sigma[v][a])]
                    r[1 - k][c] = r[1 - k][v]
            elif k == 4:
                c = put[v][0]
                for p in (0, 1):
                    S = disjoint_sums(r[1 - p][v])
                    out = []
                    for s in S:
                        E = g * s
                        product = (pot + 2 * c) * E
                        see("E", E), see("product", product)
                        out.append(product // BOARDS - 2 * c * s)
                        see("u", out[-1])
                    u[p][v] = out
            else:
                f = k - 2
                for p in (0, 1):
                    S = disjoint_sums(r[1 - p][v])
                    u[p][v] = [(-2 * put[v][f] if p == f else 2 * (pot + put[v][f])) * s for s in S]
                    see("u", max(abs(x) for x in u[p][v]))
        for v in reversed(range(n)):
            k = kind[v]
            if k > 1:
                continue
            ch = child[v]
            if best == k:
                u[k][v] = [max(u[k][c][h] for c in ch) for h in range(HOLDINGS)]
            else:
                acc = [sum(sigma[v][a][h] * u[k][c][h] for a, c in enumerate(ch)) for h in range(HOLDINGS)]
                see("sigma_u", max(abs(x) for x in acc))
                u[k][v] = [x >> 15 for x in acc]                     # (Python's >> floors, as the definition does)
            u[1 - k][v] = [sum(u[1 - k][c][h] for c in ch) for h in range(HOLDINGS)]
            see("u", max(abs(x) for x in u[k][v])), see("u", max(abs(x) for x in u[1 - k][v]))
        return r, u

    def rule_at(X):
        cols = [rule([X[a][h] for a in range(len(X))]) for h in range(HOLDINGS)]
        return [[cols[h][a] for h in range(HOLDINGS)] for a in range(len(X))]

    for t in range(t0 + 1, t0 + iters + 1):
        sigma = {d: rule_at(R[d]) for d in decisions}
        r, u = one_pass(sigma)
        for d in decisions:
            p = kind[d]
            for a, c in enumerate(child[d]):
                for h in range(HOLDINGS):
                    step = u[p][c][h] - u[p][d][h]
                    see("step", step)
                    R[d][a][h] = max(0, R[d][a][h] + step)
                    A[d][a][h] += t * r[p][c][h]
                see("regret", max(R[d][a])), see("average", max(A[d][a]))
    sigma = {d: rule_at(A[d]) for d in decisions}
    _, u = one_pass(sigma)
    value = [u[0][0], u[1][0]]
    br = [one_pass(sigma, best=p)[1][p][0] for p in (0, 1)]
    return sigma, value, br, rec
