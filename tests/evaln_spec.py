"""The one definition of the partial-hand digests in tests/golden/evaln_digest.json (numpy only): which hands, in which order, and
how their results are folded.  tests/golden/make_evaln_digest.py (the imported reference), tests/test_oracle_golden.py (the CPU
oracle) and tests/test_hip_evaln.py (the device) all go through this module.

Hands of k DISTINCT cards, k = 0 .. 6: the C(52, k) subsets of the canonical deck indices 0 .. 51 in itertools.combinations
order; the card value of index c is ((c % 4) << 4) | (c // 4) (cards.py:77).  Hand i (its position within k) yields the word
    v_i = len(kickers) << 24 | HandRanking << 20 | get_kickers_value(kickers)
and  digest = sum_i mix64(v_i ^ (i * 0x9E3779B97F4A7C15)) mod 2^64  (mix64 = the splitmix64 finaliser): the definition of
eval7_digest.json with len(kickers) added.  per_first_card[a] is the same sum over the hands whose lowest index is a (the one
empty hand of k = 0 has no first card: its per_first_card is all zero and `digest` is its own term).

Hands that REPEAT cards (`multiset`): every ordered pair (52^2) and ordered triple (52^3) of deck indices, index order
i = (a * 52 + b) * 52 + c, and for k = 4 .. 7 a generated set of GEN_HANDS hands each -- see gen_hands."""
import functools
import math

import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
CARD_VALUES = np.array([((c % 4) << 4) | (c // 4) for c in range(52)], np.uint8)
PAD = 0xFF                       # what unused slots hold in the plain layout
DISTINCT_K = range(0, 7)
GEN_K = range(4, 8)
GEN_HANDS = 200000
GEN_WINDOW = 6                   # ranks per hand's window
GEN_SEED = 0xD1B54A32D192ED03    # stream of size k starts at state k * GEN_SEED


def mix64(z):
    z = np.array(z, np.uint64)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def count_of_first(k, a):
    return math.comb(51 - a, k - 1) if k >= 1 else 0


def offset_of_first(k, a):
    """Position within k of the first hand whose lowest index is a."""
    return sum(count_of_first(k, x) for x in range(a))


@functools.lru_cache(maxsize=2)
def all_subsets(r):
    """uint8 [C(52, r), r] (read-only): every r-subset of 0..51, ascending inside a subset, combinations order."""
    cols = [np.arange(52 - r + 1, dtype=np.uint8)] if r else []
    for level in range(1, r):
        last = cols[-1].astype(np.int64)
        cnt = (52 - (r - level)) - last            # the next index runs over last+1 .. 51-(r-1-level)
        start = np.cumsum(cnt) - cnt
        rep = np.repeat(np.arange(len(last)), cnt)
        cols = [c[rep] for c in cols]
        cols.append((last[rep] + 1 + (np.arange(int(cnt.sum())) - start[rep])).astype(np.uint8))
    out = np.stack(cols, axis=1) if r else np.zeros((1, 0), np.uint8)
    out.setflags(write=False)
    return out


def subsets_of_first(k, a):
    """uint8 [C(51-a, k-1), k]: the k-subsets of 0..51 with lowest index a, combinations order: a, then the (k-1)-subsets whose lowest
    index is above a -- a tail of all_subsets(k-1).  (Never the list of all k-subsets: at k = 6 one first card is 2.35 M hands.)"""
    assert k >= 1
    rest = all_subsets(k - 1)
    rest = rest[len(rest) - count_of_first(k, a):]
    return np.concatenate([np.full((len(rest), 1), a, np.uint8), rest], axis=1)


def pad7(vals, fill=PAD):
    """uint8 [m, k] card values -> [m, 7] with the unused slots = fill."""
    m, k = vals.shape
    out = np.full((m, 7), fill, np.uint8)
    out[:, :k] = vals
    return out


def hands_of_first(k, a):
    """(cards uint8 [m, 7] in the plain layout, position of its first hand within k)."""
    return pad7(CARD_VALUES[subsets_of_first(k, a)]), offset_of_first(k, a)


def value_words(rank, kick, nkick):
    return (np.asarray(nkick, np.uint64) << np.uint64(24)) | (np.asarray(rank, np.uint64) << np.uint64(20)) | np.asarray(kick, np.uint64)


class Acc:
    """Folds value words into digest / category_counts[11] / nkick_counts[6]."""

    def __init__(self):
        self.hands, self.digest = 0, 0
        self.category = np.zeros(11, np.int64)
        self.nkick = np.zeros(6, np.int64)

    def add(self, v, start):
        """v: value words of the hands at positions start .. start+len(v)-1; returns their share of the digest."""
        v = np.asarray(v, np.uint64)
        idx = np.arange(len(v), dtype=np.uint64) + np.uint64(start)
        with np.errstate(over="ignore"):
            part = int(np.sum(mix64(v ^ (idx * GOLD)), dtype=np.uint64))
        self.digest = (self.digest + part) % (1 << 64)
        self.hands += len(v)
        self.category += np.bincount(((v >> np.uint64(20)) & np.uint64(15)).astype(np.int64), minlength=11)
        self.nkick += np.bincount((v >> np.uint64(24)).astype(np.int64), minlength=6)
        return part

    def record(self):
        return dict(hands=self.hands, digest="%016x" % self.digest, category_counts=self.category.tolist(),
                    nkick_counts=self.nkick.tolist())


def digest_distinct(k, evaluate):
    """The JSON record of size k from evaluate(cards [m, 7], ncards [m]) -> (rank, kick, nkick)."""
    acc = Acc()
    per_first = [0] * 52
    if k == 0:
        acc.add(value_words(*evaluate(np.full((1, 7), PAD, np.uint8), np.zeros(1, np.uint8))), 0)
    else:
        for a in range(52):
            cards, start = hands_of_first(k, a)
            if len(cards):
                per_first[a] = acc.add(value_words(*evaluate(cards, np.full(len(cards), k, np.uint8))), start)
    out = acc.record()
    out["per_first_card"] = ["%016x" % x for x in per_first]
    return out


# ---------------------------------------------------------------------------------------------- hands that repeat cards
def ordered_tuples(k):
    """uint8 [52^k, 7]: every ordered k-tuple of cards (repeats included), the last slot fastest."""
    i = np.arange(52 ** k)
    cols = [(i // 52 ** (k - 1 - j)) % 52 for j in range(k)]
    return pad7(CARD_VALUES[np.stack(cols, axis=1)])


def gen_hands(k, count=GEN_HANDS):
    """uint8 [count, 7]: hand i of size k from outputs 2i, 2i+1 of the splitmix64 stream whose state starts at k * GEN_SEED
    (output j = mix64(state0 + (j + 1) * GOLD)) -- integer arithmetic only, no library generator.
    z0 picks a window of GEN_WINDOW consecutive ranks (rank0 base .. base+5 mod 13, so windows wrap through the ace on both
    sides) and two suits; byte j of z1 picks slot j's rank inside the window and which of the two suits.  Twelve possible cards
    for up to seven slots: repeats, trips holding a repeat, flushes made of repeated cards and near-straight-flushes are
    common.  Half of the hands (bit 26 of z0) also copy slot p onto slot q != p, so that hands with a repeat are the majority at
    every size (at k = 4 twelve cards alone give 43 %)."""
    assert 2 <= k <= 7
    with np.errstate(over="ignore"):
        j = np.arange(count, dtype=np.uint64) * np.uint64(2)
        state0 = np.uint64((k * GEN_SEED) % (1 << 64))
        z0 = mix64(state0 + (j + np.uint64(1)) * GOLD)
        z1 = mix64(state0 + (j + np.uint64(2)) * GOLD)

    def bits(z, lo, n):
        return ((z >> np.uint64(lo)) & np.uint64((1 << n) - 1)).astype(np.int64)

    base = bits(z0, 0, 16) % 13
    s0 = bits(z0, 16, 2)
    s1 = (s0 + 1 + bits(z0, 18, 8) % 3) & 3
    force = bits(z0, 26, 1) == 1
    p = bits(z0, 27, 8) % k
    q = (p + 1 + bits(z0, 35, 8) % (k - 1)) % k
    vals = np.zeros((count, k), np.int64)
    for s in range(k):
        b = bits(z1, 8 * s, 8)
        rank0 = (base + (b & 0x3f) % GEN_WINDOW) % 13
        suit = np.where(b >> 7, s1, s0)
        vals[:, s] = (suit << 4) | rank0
    rows = np.nonzero(force)[0]
    vals[rows, q[rows]] = vals[rows, p[rows]]
    return pad7(vals.astype(np.uint8))


def repeat_share(cards, k):
    s = np.sort(cards[:, :k], axis=1)
    return float((s[:, 1:] == s[:, :-1]).any(axis=1).mean())


MULTISET_NAMES = ["pairs", "triples"] + ["gen%d" % k for k in GEN_K]   # the JSON's `multiset` section, in its order


def multiset_set(name):
    """(k, cards [m, 7]) of one set."""
    if name in ("pairs", "triples"):
        k = 2 if name == "pairs" else 3
        return k, ordered_tuples(k)
    k = int(name[3:])
    return k, gen_hands(k)


def multiset_sets():
    """[(name, k, cards [m, 7])]"""
    return [(name,) + multiset_set(name) for name in MULTISET_NAMES]


def digest_multiset(name, k, cards, evaluate):
    acc = Acc()
    acc.add(value_words(*evaluate(cards, np.full(len(cards), k, np.uint8))), 0)
    out = acc.record()
    out["ncards"] = k
    out["repeat_share"] = round(repeat_share(cards, k), 6)
    return out


# ---------------------------------------------------------------------------------------------- the second layout of a chunk
def scrambled(cards, k):
    """Layout (b) of a chunk of k-card hands: the used bytes of hand i rotated left by i mod k, the unused slots filled with REAL
    card bytes -- slot k a copy of the hand's first used card (where k >= 1), the others cards that depend on i -- which an
    evaluator must ignore.  Results equal those of `cards` for distinct cards (the reference's result does not depend on the
    order of distinct cards: tests/test_oracle_golden.py checks that on every hand of up to five cards)."""
    m = len(cards)
    out = np.empty((m, 7), np.uint8)
    for r in range(k):                             # the hands with i mod k == r
        out[r::k, :k] = np.roll(cards[r::k, :k], -r, axis=1)
    i = np.arange(m)
    for s in range(k, 7):
        out[:, s] = CARD_VALUES[(i * 7 + s * 11) % 52]
    if 1 <= k < 7:
        out[:, k] = out[:, 0]
    return out
