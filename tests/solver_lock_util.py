"""What the locked-solver tests share (TEST INFRASTRUCTURE): random ranges and lock arrays, the slots the definition says are NOT READ, and
byte-for-byte comparison of a device solution with a dict of the restatement (tests/solver_lock_spec.py).  Nothing here comes from a kernel."""
import numpy as np

H = 1326


def random_ranges(rng, m):
    w = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def random_weights(rng, shape):
    """uint16 weights with zeros and 65535s among them"""
    w = rng.integers(0, 65536, shape).astype(np.uint16)
    u = rng.random(shape)
    w[u < 0.1] = 0
    w[u > 0.97] = 65535
    return w


def rows_where(tree, pattern, river=False):
    """bool [D] of one tree and level.  pattern: "none", "all", "p0", "p1", or a list of rows"""
    nodes = tree.river_decision_nodes if river else tree.decision_nodes
    out = np.zeros(len(nodes), bool)
    if pattern == "all":
        out[:] = True
    elif pattern in ("p0", "p1"):
        out[:] = [int(tree.kind[v]) == int(pattern[1]) for v in nodes]
    elif pattern != "none":
        out[[r for r in pattern if r < len(nodes)]] = True
    return out


def lock_of(trees, tree_of, patterns, river=False):
    """uint8 [m, Dmax] for a call; a spot whose tree_of names no tree: zeros"""
    D = max(len(t.river_decision_nodes if river else t.decision_nodes) for t in trees)
    out = np.zeros((len(patterns), D), np.uint8)
    for i, pat in enumerate(patterns):
        if int(tree_of[i]) < len(trees):
            r = rows_where(trees[int(tree_of[i])], pat, river)
            out[i, :len(r)] = r
    return out


def poison_unread(lock, locked, trees, tree_of, valid, river=False, pool=None):
    """(lock, locked) copies with 0xFF / 0xFFFF wherever the definition says the call does not read: action slots >= nact, invalid holdings,
    rows whose flag is 0, rows at or past the spot's own D (their flags too), every array of a refused spot (valid[i] all False) and, at the
    river level, cards outside the pool and holdings that contain the river card (pool[i]: the canonical indices of the pool's cards)."""
    lock, locked = lock.copy(), locked.copy()
    A = np.array([a for b in range(52) for a in range(b)])
    B = np.array([b for b in range(52) for a in range(b)])
    for i in range(lock.shape[0]):
        if int(tree_of[i]) >= len(trees) or not valid[i].any():
            lock[i], locked[i] = 0xFF, 0xFFFF
            continue
        t = trees[int(tree_of[i])]
        nodes = t.river_decision_nodes if river else t.decision_nodes
        lock[i, len(nodes):], locked[i, len(nodes):] = 0xFF, 0xFFFF
        locked[i][..., ~valid[i]] = 0xFFFF
        for r, v in enumerate(nodes):
            if not lock[i, r]:
                locked[i, r] = 0xFFFF
            locked[i, r][..., t.num_actions(v):, :] = 0xFFFF
        if river:
            for k in range(52):
                if k not in pool[i]:
                    locked[i, :, k] = 0xFFFF
                else:
                    locked[i, :, k][..., (A == k) | (B == k)] = 0xFFFF
    return lock, locked


def assert_equal(got, want, where, keys):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def same_bytes(a, b, keys, where=""):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or np.asarray(x).tobytes() == np.asarray(y).tobytes()), (where, k)
