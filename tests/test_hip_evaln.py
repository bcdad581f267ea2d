"""pk_eval_hands(_d) on hands of 0 .. 6 cards and pk_compare_rankings up to 32 hands, on the GPU, against the imported reference
(tests/golden/evaln_digest.json: every hand of 0 .. 6 distinct cards and the hands that repeat cards; the definition is
tests/evaln_spec.py) and, where a test needs single hands, against the CPU oracle, which tests/test_oracle_golden.py pins to the
same digests.  Exact equality everywhere.  Three device paths are under test (k_eval_hands_tab): the LDS-table path for 3 .. 7
distinct cards, eval_small for 0 .. 2 cards, the literal scan for repeated cards and bytes that are no card."""
import ctypes as C
import math

import numpy as np
import pytest

import evaln_spec as S
import golden_util as GU

pytestmark = pytest.mark.gpu

CANARY = 0xEE
NONE = 10        # HandRanking.NONE
FLUSH = 4        # HandRanking.FLUSH (lower = stronger)


@pytest.fixture(scope="module")
def O():
    from oracle import loader
    loader.lib()
    return loader


@pytest.fixture(scope="module")
def gold():
    return GU.load_json("evaln_digest")


class Device:
    """eval_hands_d on grow-only device buffers; the card bytes start `off` bytes into their allocation, every buffer has canary
    bytes around its payload, and the outputs' canaries are checked after each call (a write outside rank[m] / kick[m] / nkick[m])."""
    PAD = 8

    def __init__(self):
        import pokerl_amd
        assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
        from pokerl_amd import judger
        self.judger = judger
        self.hip = C.CDLL("libamdhip64.so")
        self.buf = {}

    def _get(self, name, nbytes):
        from pokerl_amd.hipmem import DeviceBuffer
        b = self.buf.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self.buf[name] = DeviceBuffer(nbytes + nbytes // 4)
        return b

    def _wrapped(self, name, payload, off):
        raw = np.concatenate([np.full(off, CANARY, np.uint8), payload.reshape(-1).view(np.uint8), np.full(2 * self.PAD - off, CANARY, np.uint8)])
        return self._get(name, raw.nbytes).upload(raw)

    def eval(self, cards, ncards, off):
        m = len(cards)
        P = self.PAD
        d_c = self._wrapped("cards", np.ascontiguousarray(cards, np.uint8), off)
        d_n = None if ncards is None else self._wrapped("ncards", np.ascontiguousarray(ncards, np.uint8), 0)
        outs = [("rank", np.uint8), ("kick", np.uint32), ("nkick", np.uint8)]
        d_o = [self._wrapped(name, np.full(m, CANARY * 0x01010101 if dt == np.uint32 else CANARY, dt), P) for name, dt in outs]
        at = lambda b, o: C.c_void_p(b.ptr.value + o)
        self.judger.eval_hands_d(at(d_c, off), None if d_n is None else d_n.ptr, m, at(d_o[0], P), at(d_o[1], P), at(d_o[2], P))
        assert self.hip.hipDeviceSynchronize() == 0
        got = []
        for (name, dt), b in zip(outs, d_o):
            raw = b.download(np.uint8, m * np.dtype(dt).itemsize + 2 * P)
            assert (raw[:P] == CANARY).all() and (raw[-P:] == CANARY).all(), "bytes around %s[m] were written (m = %d)" % (name, m)
            got.append(raw[P:-P].view(dt).copy())
        return tuple(got)

    def close(self):
        for b in self.buf.values():
            b.free()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def unaligned_host(cards):
    """The same [m, 7] bytes at offset 1 of a host allocation."""
    raw = np.full(cards.size + 16, CANARY, np.uint8)
    view = raw[1:1 + cards.size].reshape(cards.shape)
    view[...] = cards
    return view


def four_runs(dev, cards, k):
    """A chunk of k-card hands in both layouts through both forms: [(label, cards as given to the call, (rank, kick, nkick))].
    Layout (a): ascending cards, unused slots 0xFF, aligned base.  Layout (b): evaln_spec.scrambled (rotated, real cards -- one of them
    the hand's own -- in the unused slots), the bytes starting at offset 1 of their allocation."""
    nc = np.full(len(cards), k, np.uint8)
    b = unaligned_host(S.scrambled(cards, k))
    return [("host form, plain layout", cards, dev.judger.eval_hands(cards, nc)),
            ("device form, plain layout", cards, dev.eval(cards, nc, 0)),
            ("host form, scrambled layout", b, dev.judger.eval_hands(b, nc)),
            ("device form, scrambled layout at byte offset 1", b, dev.eval(b, nc, 1))], nc


def explain(O, cards, nc, got, where):
    """The first hand on which `got` differs from the oracle, with its cards."""
    want = O.eval_hands(np.ascontiguousarray(cards), nc)
    bad = np.nonzero((want[0] != got[0]) | (want[1] != got[1]) | (want[2] != got[2]))[0]
    if not len(bad):
        return "%s: the device equals the oracle on all %d hands, and both differ from the reference's digest" % (where, len(cards))
    i = int(bad[0])
    n = int(nc[i])
    return "%s: %d of %d hands differ from the oracle; first: hand %d, cards %s (slots beyond %d: %s): oracle (rank %d, kickers %#x, %d of them), device (%d, %#x, %d)" % (
        where, len(bad), len(cards), i, " ".join("%02x" % c for c in cards[i, :n]), n, " ".join("%02x" % c for c in cards[i, n:]),
        want[0][i], want[1][i], want[2][i], got[0][i], got[1][i], got[2][i])


def check_runs(O, runs, nc, start, want_part, acc, where):
    """The first run's share of the digest (its hands are at positions start ..) equals want_part; the other runs equal the first."""
    label0, cards0, first = runs[0]
    part = acc.add(S.value_words(*first), start)
    if part != want_part:
        pytest.fail(explain(O, cards0, nc, first, "%s, %s" % (where, label0)))
    for label, cards, got in runs[1:]:
        if not all(np.array_equal(a, b) for a, b in zip(first, got)):
            pytest.fail(explain(O, cards, nc, got, "%s, %s" % (where, label)))


@pytest.mark.parametrize("k", list(S.DISTINCT_K))
def test_evaln_exhaustive_digest(dev, O, gold, k):
    """EVERY hand of k distinct cards (k = 6: 20 358 520), one first card per chunk, through judger.eval_hands and eval_hands_d in two
    layouts each: per-first-card digests, category counts, len(kickers) counts and the digest of the imported reference."""
    g = gold["distinct"][str(k)]
    acc = S.Acc()
    if k == 0:
        cards = np.full((1, 7), S.PAD, np.uint8)
        runs, nc = four_runs(dev, cards, 0)
        check_runs(O, runs, nc, 0, int(g["digest"], 16), acc, "k=0")
    for a in range(52 if k else 0):
        cards, start = S.hands_of_first(k, a)
        if not len(cards):
            assert int(g["per_first_card"][a], 16) == 0
            continue
        runs, nc = four_runs(dev, cards, k)
        check_runs(O, runs, nc, start, int(g["per_first_card"][a], 16), acc, "k=%d, first card index %d" % (k, a))
    got = acc.record()
    assert got["hands"] == g["hands"] == math.comb(52, k)
    assert got["category_counts"] == g["category_counts"]
    assert got["nkick_counts"] == g["nkick_counts"]
    assert got["digest"] == g["digest"]


@pytest.mark.parametrize("name", S.MULTISET_NAMES)
def test_evaln_multiset_digest(dev, O, gold, name):
    """Hands that repeat cards (every ordered pair and triple; the generated 4 .. 7-card hands over twelve cards) against the reference's
    digests, same forms and layouts.  The scrambled layout returns the same there too: the CPU twin of this test checks it on the oracle."""
    g = gold["multiset"][name]
    k, cards = S.multiset_set(name)
    assert len(cards) == g["hands"] and k == g["ncards"]
    runs, nc = four_runs(dev, cards, k)
    acc = S.Acc()
    check_runs(O, runs, nc, 0, int(g["digest"], 16), acc, name)
    got = acc.record()
    assert got["category_counts"] == g["category_counts"] and got["nkick_counts"] == g["nkick_counts"] and got["digest"] == g["digest"]
    if k == 7:   # ncards == NULL: the kernel's seven-card instantiation
        seven = dev.eval(cards, None, 1)
        if not all(np.array_equal(a, b) for a, b in zip(runs[0][2], seven)):
            pytest.fail(explain(O, cards, nc, seven, name + ", device form without ncards"))


def test_evaln_mixed_waves(dev, O):
    """One batch in which every wavefront holds lanes for the table, for eval_small and for the scan (which a wave enters only if one of
    its lanes needs it): every 5- and 6-card hand that is a flush or better (chosen by the oracle; a few hundred thousand), 0-, 1- and
    2-card hands, hands that repeat a card and plain hands, interleaved by a fixed stride permutation.  m is above 2048 x 512, so that
    the kernel's grid-stride loop and its prefetch of the next hand wrap, and no multiple of 512.  Element-wise against the oracle."""
    parts, ncs, kinds = [], [], []     # kinds: 0 table, 1 eval_small, 2 scan

    def add(cards, k, kind):
        parts.append(cards); ncs.append(np.full(len(cards), k, np.uint8)); kinds.append(np.full(len(cards), kind, np.uint8))

    for k in (5, 6):
        strong = []
        for a in range(52):
            cards, _ = S.hands_of_first(k, a)
            if len(cards):
                rank, _, _ = O.eval_hands(cards, np.full(len(cards), k, np.uint8))
                strong.append(cards[rank <= FLUSH])
        add(np.concatenate(strong), k, 0)
    assert len(parts[0]) == 40 + 624 + 3744 + 5108 and len(parts[1]) == 1732 + 14664 + 165984 + 205568   # straight flush, poker, full, flush
    for k in (3, 4):                                        # plain hands
        add(np.concatenate([S.hands_of_first(k, a)[0] for a in range(52 - k + 1)]), k, 0)
    seven = S.gen_hands(7, 60000)
    s7 = np.sort(seven, axis=1)
    add(seven[(s7[:, 1:] != s7[:, :-1]).all(axis=1)], 7, 0)
    pairs, triples = S.ordered_tuples(2), S.ordered_tuples(3)
    for rep in range(40):                                   # 0-, 1- and 2-card hands, real cards in their unused slots
        add(S.scrambled(pairs, 2), 2, 1)
        add(S.scrambled(pairs[rep::3], 1), 1, 1)
        add(S.scrambled(pairs[rep::5], 0), 0, 1)
    for k in (3, 4, 5, 6, 7):                               # a repeated card: the scan
        g = triples if k == 3 else S.gen_hands(k, 80000)
        s = np.sort(g[:, :k], axis=1)
        add(g[(s[:, 1:] == s[:, :-1]).any(axis=1)], k, 2)
    cards, nc, kind = np.concatenate(parts), np.concatenate(ncs), np.concatenate(kinds)
    m = len(cards)
    if m % 512 == 0:
        m -= 1
    assert m > 2048 * 512 + 64 and m % 512
    stride = int(m * 0.381966) | 1
    while math.gcd(stride, m) != 1:
        stride += 2
    perm = (np.arange(m, dtype=np.int64) * stride) % m
    cards, nc, kind = np.ascontiguousarray(cards[perm]), nc[perm], kind[perm]
    waves = kind[:m // 64 * 64].reshape(-1, 64)
    for c in range(3):
        assert (waves == c).any(axis=1).all(), "a wavefront without a lane of kind %d" % c
    want = O.eval_hands(cards, nc)
    for m2 in (m, 100001):
        for label, got in [("host form", dev.judger.eval_hands(cards[:m2], nc[:m2])),
                           ("device form at byte offset 1", dev.eval(unaligned_host(cards[:m2]), nc[:m2], 1))]:
            if not all(np.array_equal(a[:m2], b) for a, b in zip(want, got)):
                pytest.fail(explain(O, cards[:m2], nc[:m2], got, "mixed batch of %d hands, %s" % (m2, label)))


NONCARD_BASES = [[0x01, 0x02, 0x03, 0x04, 0x1c, 0x2b, 0x35], [0x3c, 0x2c, 0x1c, 0x0b, 0x1b, 0x2a, 0x00], [0x10, 0x1c, 0x1b, 0x1a, 0x19, 0x25, 0x36],
                 [0x00, 0x11, 0x22, 0x33, 0x04, 0x1c, 0x2b]]   # the last: A 2 3 4 5 and two more, where a rank above the ace takes the wheel away


def test_eval_hands_bytes_that_are_no_card(dev, O):
    """A byte that is no card (suit > 3 or rank nibble 13 .. 15) reads as suit = bits 4 .. 5, rank nibble as it is, and a hand that holds a
    rank above the ace (nibble 14, 15) never scores the plain five-high straight: the reading include/pokerl_hip.h states at pk_eval_hands
    and the oracle restates as orc_eval_hands_bytes (confirmed on the CPU build: tools/host_sim noncard).  Apart from that exception it is
    the oracle's result on (byte & 0x3F); the hands chosen here meet the exception.  EVERY byte value 0x00 .. 0xFF in EVERY used position
    of a 3-, a 5- and a 7-card hand, for four base hands (4 x 256 x 15 hands)."""
    rows, ns = [], []
    for base in NONCARD_BASES:
        for n in (3, 5, 7):
            for pos in range(n):
                h = np.tile(np.array(base, np.uint8), (256, 1))
                h[:, pos] = np.arange(256)
                rows.append(h); ns.append(np.full(256, n, np.uint8))
    cards, nc = np.concatenate(rows), np.concatenate(ns)
    assert len(cards) == 4 * 256 * 15
    want = O.eval_hands(cards, nc, any_bytes=True)
    plain = O.eval_hands(cards & 0x3F, nc)
    differs = (want[0] != plain[0]) | (want[1] != plain[1]) | (want[2] != plain[2])
    above_ace = ((cards & 0x0F) >= 14).any(axis=1)        # (7-card rows only can differ: unused slots hold base cards)
    assert differs.any() and not (differs & ~above_ace).any() and (plain[0][differs] == 5).all() and (plain[1][differs] == 4).all()
    runs = [("host form", cards, nc, dev.judger.eval_hands(cards, nc))]
    for off in (0, 1):
        runs.append(("device form at byte offset %d" % off, cards, nc, dev.eval(cards, nc, off)))
    seven = nc == 7
    c7, w7 = np.ascontiguousarray(cards[seven]), tuple(w[seven] for w in want)
    runs.append(("device form without ncards", c7, nc[seven], dev.eval(c7, None, 1)))
    for label, c, n, got in runs:
        w = w7 if len(c) == len(c7) else want
        if not all(np.array_equal(a, b) for a, b in zip(w, got)):
            bad = int(np.nonzero((w[0] != got[0]) | (w[1] != got[1]) | (w[2] != got[2]))[0][0])
            pytest.fail("bytes that are no card, %s: hand %s (%d cards): documented reading (rank %d, kickers %#x, %d of them), device (%d, %#x, %d)" % (
                label, " ".join("%02x" % x for x in c[bad]), n[bad], w[0][bad], w[1][bad], w[2][bad], got[0][bad], got[1][bad], got[2][bad]))


def line_148_lists(rank, kick):
    """Which lists hold the pattern that makes judger.py:148 visible: k1 the kicker of the first hand of the best rank (0, the initial
    best_kicker, where every hand is NONE), then a later hand of that rank with k2 > k1, then a still later one with k1 < k3 < k2 -- it
    wins under the reference's rule although k2 beats it."""
    best = rank.min(axis=1, keepdims=True)
    isbest = rank == best
    first = isbest.argmax(axis=1)
    none = best[:, 0] == NONE
    k1 = np.where(none, 0, kick[np.arange(len(kick)), first]).astype(np.int64)[:, None]
    pos = np.arange(rank.shape[1])[None, :]
    later = isbest & ((pos > first[:, None]) | none[:, None]) & (kick > k1)
    above = np.where(later, kick.astype(np.int64), -1)
    seen = np.maximum.accumulate(above, axis=1)
    prev = np.concatenate([np.full((len(kick), 1), -1, np.int64), seen[:, :-1]], axis=1)
    return (later & (kick < prev)).any(axis=1)


@pytest.mark.parametrize("n", range(1, 33))
def test_compare_rankings_up_to_32_hands(dev, O, n):
    """pk_compare_rankings for every list length it accepts against orc_compare_rankings: 4 096 lists per n with ranks from three values
    plus NONE and kickers from three values, so ties are the rule.  Independent draws alone put the line-148 pattern (line_148_lists) in
    under 1 list in 27 at n = 3 -- it needs the kickers (low, high, middle) in that order on three hands of the best rank -- so every
    second list has it planted at three drawn positions; at least 1 000 lists per n >= 3 must hold it."""
    M = 4096
    rng = np.random.default_rng(1480 + n)
    RV = np.array([2, 5, 8, NONE], np.uint8)
    KV = np.array([0x00432, 0x0D0C5, 0xDCBA9], np.uint32)
    rank = RV[rng.integers(0, 4, (M, n))]
    kick = KV[rng.integers(0, 3, (M, n))]
    if n >= 3:
        for i in range(0, M, 2):
            a, b, c = np.sort(rng.choice(n, 3, replace=False))
            head = rank[i, :a]
            head[head == RV[0]] = RV[1]                # no hand of the best rank before a
            rank[i, [a, b, c]] = RV[0]
            kick[i, [a, b, c]] = KV[[0, 2, 1]]
        assert int(line_148_lists(rank, kick).sum()) >= 1000
    want = np.stack([O.compare_rankings(rank[i], kick[i]) for i in range(M)])
    got = dev.judger.compare_rankings_batch(rank, kick)
    bad = np.nonzero((want != got).any(axis=1))[0]
    assert not len(bad), "n=%d: %d lists differ; first: ranks %s kickers %s oracle %s device %s" % (
        n, len(bad), rank[bad[0]].tolist(), [hex(x) for x in kick[bad[0]]], want[bad[0]].tolist(), got[bad[0]].tolist())
