"""pokerl.judger on the device: eval_hand / compare_rankings / compare_hands (reference pokerl/judger.py:7-189),
batched through the C ABI.  Cards are Card.value bytes (or 'RS' strings / Card-likes via cards.card_value)."""
import numpy as np

from . import _lib as L
from .cards import card_value
from .enums import HandRanking


def _unpack(kick, nk):
    return [int((kick >> (4 * (nk - 1 - i))) & 0xf) for i in range(nk)]


def get_kickers_value(kickers) -> int:
    """judger.py:101-109: kickers packed big-endian in nibbles."""
    v = 0
    for k in kickers:
        v = (v << 4) | int(k)
    return v


def eval_hands(cards, ncards=None, device=0):
    """cards: uint8 [M,7] Card.value (slots >= ncards ignored), ncards: [M] in 0..7 or None (=7).
    Returns (rank uint8[M], kickers_value uint32[M], num_kickers uint8[M])."""
    cards = np.ascontiguousarray(cards, np.uint8)
    if cards.ndim != 2 or cards.shape[1] != 7:
        raise ValueError('cards must have shape [M, 7]')
    m = cards.shape[0]
    nc = None if ncards is None else np.ascontiguousarray(ncards, np.uint8)
    rank = np.zeros(m, np.uint8)
    kick = np.zeros(m, np.uint32)
    nk = np.zeros(m, np.uint8)
    L.check(L.lib().pk_eval_hands(int(device), L.ptr(cards), L.ptr(nc), m, L.ptr(rank), L.ptr(kick), L.ptr(nk)))
    return rank, kick, nk


def eval_hands_d(cards_d, ncards_d, m, rank_d, kick_d, nkick_d=None, device=0, stream=None):
    """pk_eval_hands_d: the same op on device-resident buffers (device pointers as ints / c_void_p), asynchronous on
    `stream` -- e.g. the rank feature of examples/q_learning.py:29-33 for a learner that lives on the GPU."""
    L.check(L.lib().pk_eval_hands_d(int(device), cards_d, ncards_d, int(m), rank_d, kick_d, nkick_d, stream))


def eval_hand(hand, device=0):
    """judger.eval_hand(hand) -> (HandRanking, [kickers]) for one hand of 0..7 cards (judger.py:7-99)."""
    vals = [card_value(c) for c in hand]
    if len(vals) > 7:
        raise ValueError('at most seven cards')
    row = np.zeros((1, 7), np.uint8)
    row[0, :len(vals)] = vals
    rank, kick, nk = eval_hands(row, np.array([len(vals)], np.uint8), device)
    return int(rank[0]), _unpack(int(kick[0]), int(nk[0]))


def compare_rankings_batch(rank, kick, device=0):
    """rank uint8 [M,n], kick uint32 [M,n] -> onehot uint8 [M,n] (judger.py:111-158, incl. its line-148 behaviour)."""
    rank = np.ascontiguousarray(rank, np.uint8)
    kick = np.ascontiguousarray(kick, np.uint32)
    if rank.ndim != 2 or rank.shape != kick.shape:
        raise ValueError('rank and kick must both have shape [M, n]')
    m, n = rank.shape
    onehot = np.zeros((m, n), np.uint8)
    L.check(L.lib().pk_compare_rankings(int(device), L.ptr(rank), L.ptr(kick), n, m, L.ptr(onehot)))
    return onehot


def compare_rankings(rankings, device=0):
    """judger.compare_rankings(rankings) -> (onehot list, winners list); rankings = [(rank, [kickers]), ...]."""
    rank = np.array([[r for r, _ in rankings]], np.uint8)
    kick = np.array([[get_kickers_value(k) for _, k in rankings]], np.uint32)
    onehot = compare_rankings_batch(rank, kick, device)[0]
    return [int(x) for x in onehot], [i for i, x in enumerate(onehot) if x]


def compare_hands(hands, device=0):
    """judger.compare_hands(hands) -> (onehot, winners, rankings) (judger.py:160-189)."""
    rankings = [eval_hand(h, device) for h in hands]
    return compare_rankings(rankings, device) + (rankings,)


def eval7_prefix(a, b, fast=True, device=0):
    """Values rank<<20|kick of all 7-card hands whose two lowest canonical indices are (a, b) (exhaustive checks).
    fast=True / 1: the distinct-card evaluator used by the showdown kernels; False / 0: the general evaluator; 3: what
    pk_eval_hands applies (fast path for 3..7 distinct cards);
    2: the table-driven distinct-card evaluator of the streaming kernel (eval7_stream)."""
    import ctypes as C
    import math
    n = math.comb(51 - b, 5)
    out = np.zeros(max(n, 1), np.uint32)
    cnt = C.c_size_t(0)
    L.check(L.lib().pk_eval7_prefix(int(device), int(a), int(b), int(fast), L.ptr(out), C.byref(cnt)))
    return out[:cnt.value]


NONE_RANKING = (HandRanking.NONE, [])


def eval7_stream(hands_d, m, out_d, distinct=True, device=0):
    """pk_eval7_d: m 7-card hands resident in HBM (one per 64-bit word, card i = byte i) -> rank<<20|kickers words."""
    L.check(L.lib().pk_eval7_d(int(device), hands_d, int(m), out_d, int(bool(distinct))))


def make_hands(hands_d, m, seed=0x706F6B65726C, device=0):
    """pk_make_hands_d: synthetic distinct 7-card hands (first 7 cards of the RNG-spec deck of table_id = i)."""
    L.check(L.lib().pk_make_hands_d(int(device), int(seed), int(m), hands_d))


def time_eval7_stream(hands_d, m, out_d, distinct=True, reps=5, device=0):
    import ctypes as C
    ms = C.c_double(0.0)
    L.check(L.lib().pk_time_eval7_d(int(device), hands_d, int(m), out_d, int(bool(distinct)), int(reps), C.byref(ms)))
    return ms.value


# ---------------------------------------------------------------------------------------------- showdown equity
# "If the cards still to come were dealt now, how often does each seat win?" -- every board enumerated on the device (pk_equity; the
# definition: include/pokerl_hip.h "Showdown equity").  Winners are the reference's compare_rankings, line 148 included.
UNKNOWN_CARD = 0xFF
_EQ_STATUS = [(L.EQ_BAD_CARD, 'a byte that is no card (or an unknown card in the board or at a live seat)'), (L.EQ_DUP_CARD, 'a card twice'),
              (L.EQ_NO_LIVE, 'no live seat'), (L.EQ_BAD_NBOARD, 'more than five board cards'),
              (L.EQ_IN_FLIGHT, "the table's step is in flight"), (L.EQ_BAD_TABLE, 'table index out of range'),
              (L.EQ_PREFLOP, 'fewer than three board cards (range equity is post-flop only)'),
              (L.EQ_SMALL_POOL, 'too few cards left for the board to come and one holding')]


def equity_status_text(status):
    return '; '.join(t for bit, t in _EQ_STATUS if int(status) & bit) or 'ok'


class Equity:
    """Counts of one spot or of a batch ([N] or [m, N] arrays; `boards`, `status` scalars or [m]): win = boards a seat wins alone, tie = boards
    it wins with others, share = sum of 720720 / (number of winners) over the boards it wins.  `equity` = share / (720720 * boards) in float64
    (0 where a spot was refused: status != 0)."""

    def __init__(self, win, tie, share, boards, status):
        self.win, self.tie, self.share, self.boards, self.status = win, tie, share, boards, status

    @property
    def equity(self):
        b = np.asarray(self.boards, np.float64)[..., None] * float(L.EQ_SHARE_UNIT)
        return np.divide(np.asarray(self.share, np.float64), b, out=np.zeros(np.shape(self.share), np.float64), where=b > 0)

    def __getitem__(self, i):
        return Equity(self.win[i], self.tie[i], self.share[i], self.boards[i], self.status[i])

    def __repr__(self):
        return 'Equity(boards=%r, status=%r, win=%r, tie=%r, equity=%r)' % (self.boards, self.status, self.win, self.tie, self.equity)


def showdown_equity_batch(holes, board, nboard, live, device=0):
    """pk_equity on host arrays: holes uint8 [m, N, 2] Card.value (0xFF = unknown, at seats that are not live only), board uint8 [m, 5] (the
    first nboard[i] used), nboard uint8 [m], live uint16 [m] seat masks -> Equity of [m, N] / [m] arrays.  A bad spot is reported through
    its `status` (PK_EQ_* bits) with all-zero counts; the others are unaffected."""
    holes = np.ascontiguousarray(holes, np.uint8)
    if holes.ndim != 3 or holes.shape[2] != 2 or not (L.MIN_PLAYERS <= holes.shape[1] <= L.MAX_PLAYERS):
        raise ValueError('holes must have shape [m, N, 2] with 2 <= N <= 16')
    m, n = holes.shape[:2]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    live = np.ascontiguousarray(live, np.uint16)
    if board.shape != (m, 5) or nboard.shape != (m,) or live.shape != (m,):
        raise ValueError('board must have shape [m, 5], nboard and live shape [m]')
    win, tie = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32)
    share = np.zeros((m, n), np.uint64)
    boards, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity(int(device), n, m, L.ptr(holes), L.ptr(board), L.ptr(nboard), L.ptr(live), L.ptr(win), L.ptr(tie), L.ptr(share),
                              L.ptr(boards), L.ptr(status)))
    return Equity(win, tie, share, boards, status)


def showdown_equity_d(num_players, m, holes_d, board_d, nboard_d, live_d, win_d=None, tie_d=None, share_d=None, boards_d=None, status_d=None,
                      device=0, stream=None):
    """pk_equity_d: the same on device-resident buffers (device pointers as ints / c_void_p; outputs may be None), asynchronous on `stream`."""
    L.check(L.lib().pk_equity_d(int(device), int(num_players), int(m), holes_d, board_d, nboard_d, live_d, win_d, tie_d, share_d, boards_d,
                                status_d, stream))


def _card(c):
    try:
        return card_value(c)
    except (AssertionError, KeyError, IndexError) as e:
        raise ValueError('not a card: %r' % (c,)) from e


def showdown_equity(hands, board=(), live=None, device=0):
    """One spot.  hands: per seat two cards (Card-likes / 'RS' strings / Card.value ints), or None for a seat whose cards are unknown (it
    cannot be live); board: 0 .. 5 known cards; live: the seats that show down (iterable of seat numbers or a bit mask; default: every seat
    with cards).  Returns an Equity with [N] arrays; raises ValueError for an invalid spot."""
    hands = list(hands)
    n = len(hands)
    if not (L.MIN_PLAYERS <= n <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    board = list(board)
    if len(board) > 5:
        raise ValueError('at most five board cards')
    holes = np.full((1, n, 2), UNKNOWN_CARD, np.uint8)
    for p, h in enumerate(hands):
        if h is None:
            continue
        h = list(h)
        if len(h) != 2:
            raise ValueError('seat %d: two hole cards (or None)' % p)
        holes[0, p] = [_card(c) for c in h]
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    if live is None:
        mask = sum(1 << p for p, h in enumerate(hands) if h is not None)
    elif isinstance(live, (int, np.integer)):
        mask = int(live)
    else:
        mask = 0
        for p in live:
            if not 0 <= int(p) < n:
                raise ValueError('live seat %r out of range' % (p,))
            mask |= 1 << int(p)
    if mask < 0 or mask >> n:
        raise ValueError('live mask names seats >= %d' % n)
    r = showdown_equity_batch(holes, b, np.array([len(board)], np.uint8), np.array([mask], np.uint16), device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- showdown EV in chips
# "If the cards still to come were dealt now, what does each seat expect to be paid?" -- the side pots of Game.end_hand (game.py:494-531)
# over every board (pk_equity_ev; the definition: include/pokerl_hip.h "Showdown EV").  With equal bets this is
# pot * equity - bet; with unequal stacks the pot is paid out in levels and main-pot equity gives the wrong number.
NO_LEVEL = 0xFF
_EV_STATUS = [(bit, t) for bit, t in _EQ_STATUS if bit < L.EQ_BAD_BET] + [(L.EQ_BAD_BET, 'a bet that is negative, NaN or infinite')]


def ev_status_text(status):
    return '; '.join(t for bit, t in _EV_STATUS if int(status) & bit) or 'ok'


class ShowdownEV:
    """Expected payoffs of one spot or of a batch ([N] / [N, N] or [m, N] / [m, N, N] arrays; `boards`, `status` scalars or [m]):
    ev = expected payoff minus what the seat has put in (what Game.end_hand writes to `payoffs`, averaged over the boards), share[i][p] = sum
    of 720720 / (number of winners) over the boards seat p wins pot level i, level_seat[i] / amount[i] = the seat visited at level i (0xFF:
    no such level) and the chips that level pays, bets = the bets of the spot."""

    def __init__(self, ev, share, level_seat, amount, boards, status, bets):
        self.ev, self.share, self.level_seat, self.amount, self.boards, self.status, self.bets = ev, share, level_seat, amount, boards, status, bets

    @property
    def payout(self):
        """ev + bets: what a seat expects to take out of the pot (0 where a spot was refused)."""
        if self.bets is None:
            return None
        ok = np.asarray(self.status)[..., None] == 0
        return np.where(ok, np.asarray(self.ev) + np.asarray(self.bets), 0.0)

    @property
    def levels(self):
        """(seat, amount) pairs of the levels that exist, in visiting order (a batch: one list per spot)."""
        seat, amount = np.asarray(self.level_seat), np.asarray(self.amount)
        if seat.ndim == 1:
            return [(int(s), float(a)) for s, a in zip(seat, amount) if s != NO_LEVEL]
        return [[(int(s), float(a)) for s, a in zip(ss, aa) if s != NO_LEVEL] for ss, aa in zip(seat, amount)]

    def __getitem__(self, i):
        return ShowdownEV(self.ev[i], self.share[i], self.level_seat[i], self.amount[i], self.boards[i], self.status[i],
                          None if self.bets is None else self.bets[i])

    def __repr__(self):
        return 'ShowdownEV(boards=%r, status=%r, ev=%r, levels=%r)' % (self.boards, self.status, self.ev, self.levels)


def showdown_ev_batch(holes, board, nboard, live, bets, device=0):
    """pk_equity_ev on host arrays: the spots of showdown_equity_batch plus bets float64 [m, N] (what each seat has committed, folded seats
    included) -> ShowdownEV of [m, N] / [m, N, N] / [m] arrays.  A bad spot is reported through its `status` (PK_EQ_* bits, PK_EQ_BAD_BET
    among them) with zeros everywhere; the others are unaffected."""
    holes = np.ascontiguousarray(holes, np.uint8)
    if holes.ndim != 3 or holes.shape[2] != 2 or not (L.MIN_PLAYERS <= holes.shape[1] <= L.MAX_PLAYERS):
        raise ValueError('holes must have shape [m, N, 2] with 2 <= N <= 16')
    m, n = holes.shape[:2]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    live = np.ascontiguousarray(live, np.uint16)
    bets = np.ascontiguousarray(bets, np.float64)
    if board.shape != (m, 5) or nboard.shape != (m,) or live.shape != (m,) or bets.shape != (m, n):
        raise ValueError('board must have shape [m, 5], nboard and live shape [m], bets shape [m, N]')
    share = np.zeros((m, n, n), np.uint64)
    level_seat = np.full((m, n), NO_LEVEL, np.uint8)
    amount, ev = np.zeros((m, n), np.float64), np.zeros((m, n), np.float64)
    boards, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_ev(int(device), n, m, L.ptr(holes), L.ptr(board), L.ptr(nboard), L.ptr(live), L.ptr(bets), L.ptr(share),
                                 L.ptr(level_seat), L.ptr(amount), L.ptr(ev), L.ptr(boards), L.ptr(status)))
    return ShowdownEV(ev, share, level_seat, amount, boards, status, bets)


def showdown_ev_d(num_players, m, holes_d, board_d, nboard_d, live_d, bets_d, status_d, share_d=None, level_seat_d=None, amount_d=None, ev_d=None,
                  boards_d=None, device=0, stream=None):
    """pk_equity_ev_d: the same on device-resident buffers (device pointers as ints / c_void_p; every output but status_d may be None),
    asynchronous on `stream`."""
    L.check(L.lib().pk_equity_ev_d(int(device), int(num_players), int(m), holes_d, board_d, nboard_d, live_d, bets_d, share_d, level_seat_d,
                                   amount_d, ev_d, boards_d, status_d, stream))


def showdown_ev(hands, board=(), live=None, bets=None, device=0):
    """One spot: showdown_equity's arguments plus bets, one number per seat (what the seat has committed to the pot; a folded seat's money
    counts).  Returns a ShowdownEV with [N] / [N, N] arrays; raises ValueError for an invalid spot."""
    hands = list(hands)
    n = len(hands)
    if not (L.MIN_PLAYERS <= n <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    if bets is None:
        raise ValueError('bets: one number per seat')
    try:
        b = np.array([float(x) for x in bets], np.float64)
    except TypeError as e:
        raise ValueError('bets: one number per seat') from e
    if b.shape != (n,):
        raise ValueError('bets: one number per seat')
    if not np.all(np.isfinite(b)) or np.any(b < 0):
        raise ValueError('bets must be finite and not negative')
    board = list(board)
    if len(board) > 5:
        raise ValueError('at most five board cards')
    holes = np.full((1, n, 2), UNKNOWN_CARD, np.uint8)
    for p, h in enumerate(hands):
        if h is None:
            continue
        h = list(h)
        if len(h) != 2:
            raise ValueError('seat %d: two hole cards (or None)' % p)
        holes[0, p] = [_card(c) for c in h]
    bd = np.zeros((1, 5), np.uint8)
    bd[0, :len(board)] = [_card(c) for c in board]
    if live is None:
        mask = sum(1 << p for p, h in enumerate(hands) if h is not None)
    elif isinstance(live, (int, np.integer)):
        mask = int(live)
    else:
        mask = 0
        for p in live:
            if not 0 <= int(p) < n:
                raise ValueError('live seat %r out of range' % (p,))
            mask |= 1 << int(p)
    if mask < 0 or mask >> n:
        raise ValueError('live mask names seats >= %d' % n)
    r = showdown_ev_batch(holes, bd, np.array([len(board)], np.uint8), np.array([mask], np.uint16), b[None, :], device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + ev_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- sampled showdown equity
# The same question for a seat that does not know the other hands: hidden cards are DRAWN on the device, `samples` times per spot, on a fixed
# counter-based stream (pk_equity_sampled; the definition: include/pokerl_hip.h "Sampled showdown equity").
DEFAULT_SEED = 0x706F6B65726C


class SampledEquity:
    """Counts of one spot or of a batch over `samples` samples ([N] or [m, N] arrays; `samples`, `status` scalars or [m]): as Equity, with
    samples in place of boards.  `equity` = share / (720720 * samples); `stderr` = the binomial standard error of (win + tie) / samples per
    seat (0 where a spot was refused).  Counts of calls with different nonces add exactly."""

    def __init__(self, win, tie, share, samples, status):
        self.win, self.tie, self.share, self.samples, self.status = win, tie, share, samples, status

    @property
    def equity(self):
        b = np.asarray(self.samples, np.float64)[..., None] * float(L.EQ_SHARE_UNIT)
        return np.divide(np.asarray(self.share, np.float64), b, out=np.zeros(np.shape(self.share), np.float64), where=b > 0)

    @property
    def stderr(self):
        s = np.broadcast_to(np.asarray(self.samples, np.float64)[..., None], np.shape(self.win))
        p = np.divide(np.asarray(self.win, np.float64) + np.asarray(self.tie, np.float64), s, out=np.zeros(np.shape(self.win), np.float64), where=s > 0)
        return np.sqrt(np.divide(p * (1.0 - p), s, out=np.zeros(np.shape(self.win), np.float64), where=s > 0))

    def __getitem__(self, i):
        return SampledEquity(self.win[i], self.tie[i], self.share[i], self.samples[i], self.status[i])

    def __repr__(self):
        return 'SampledEquity(samples=%r, status=%r, win=%r, tie=%r, equity=%r)' % (self.samples, self.status, self.win, self.tie, self.equity)


def check_samples(samples, nonce=0):
    """The (samples, nonce) of a sampled-equity call as ints; ValueError outside 1 .. 2^24 / 0 .. 2^32 - 1 (before any device call)."""
    samples, nonce = int(samples), int(nonce)
    if not 1 <= samples <= L.EQS_SAMPLES_MAX:
        raise ValueError('samples must be 1 .. 2^24 per call (more: further calls with other nonces; the counts add)')
    if not 0 <= nonce <= 0xFFFFFFFF:
        raise ValueError('nonce must fit 32 bits')
    return samples, nonce


def sampled_equity_batch(holes, board, nboard, live, samples=4096, seed=DEFAULT_SEED, nonce=0, ids=None, device=0):
    """pk_equity_sampled on host arrays: as showdown_equity_batch, but a 0xFF hole byte at a live seat is HIDDEN and drawn anew in each of the
    `samples` samples.  ids uint32 [m]: the spots' stream ids (default: the spot index).  Returns a SampledEquity of [m, N] / [m] arrays."""
    holes = np.ascontiguousarray(holes, np.uint8)
    if holes.ndim != 3 or holes.shape[2] != 2 or not (L.MIN_PLAYERS <= holes.shape[1] <= L.MAX_PLAYERS):
        raise ValueError('holes must have shape [m, N, 2] with 2 <= N <= 16')
    m, n = holes.shape[:2]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    live = np.ascontiguousarray(live, np.uint16)
    if board.shape != (m, 5) or nboard.shape != (m,) or live.shape != (m,):
        raise ValueError('board must have shape [m, 5], nboard and live shape [m]')
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.uint32)
        if ids.shape != (m,):
            raise ValueError('ids must have shape [m]')
    samples, nonce = check_samples(samples, nonce)
    if m * ((samples + 63) // 64) > 0xFFFFFFFF:
        raise ValueError('m * ceil(samples / 64) must fit 32 bits: split the batch')
    win, tie = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32)
    share = np.zeros((m, n), np.uint64)
    count, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_sampled(int(device), n, m, L.ptr(holes), L.ptr(board), L.ptr(nboard), L.ptr(live), L.ptr(ids), samples,
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, nonce, L.ptr(win), L.ptr(tie), L.ptr(share), L.ptr(count), L.ptr(status)))
    return SampledEquity(win, tie, share, count, status)


def sampled_equity_d(num_players, m, holes_d, board_d, nboard_d, live_d, samples, ids_d=None, seed=DEFAULT_SEED, nonce=0, win_d=None, tie_d=None,
                     share_d=None, samples_d=None, status_d=None, device=0, stream=None):
    """pk_equity_sampled_d: the same on device-resident buffers (device pointers as ints / c_void_p; ids_d and the outputs may be None),
    asynchronous on `stream`."""
    samples, nonce = check_samples(samples, nonce)
    if not (L.MIN_PLAYERS <= int(num_players) <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    L.check(L.lib().pk_equity_sampled_d(int(device), int(num_players), int(m), holes_d, board_d, nboard_d, live_d, ids_d, samples,
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, nonce, win_d, tie_d, share_d, samples_d, status_d, stream))


def sampled_equity(hands, board=(), live=None, samples=4096, seed=DEFAULT_SEED, nonce=0, device=0):
    """One spot.  hands: per seat two cards (Card-likes / 'RS' strings / Card.value ints), either of which may be None = hidden, or None for
    a seat with both cards hidden; board: 0 .. 5 known cards; live: the seats that show down (iterable of seat numbers or a bit mask; default:
    EVERY seat -- a hidden hand is drawn).  Returns a SampledEquity with [N] arrays; raises ValueError for an invalid spot."""
    hands = list(hands)
    n = len(hands)
    if not (L.MIN_PLAYERS <= n <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    board = list(board)
    if len(board) > 5:
        raise ValueError('at most five board cards')
    holes = np.full((1, n, 2), UNKNOWN_CARD, np.uint8)
    for p, h in enumerate(hands):
        if h is None:
            continue
        h = list(h)
        if len(h) != 2:
            raise ValueError('seat %d: two hole cards (each a card or None), or None' % p)
        holes[0, p] = [UNKNOWN_CARD if c is None else _card(c) for c in h]
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    if live is None:
        mask = (1 << n) - 1
    elif isinstance(live, (int, np.integer)):
        mask = int(live)
    else:
        mask = 0
        for p in live:
            if not 0 <= int(p) < n:
                raise ValueError('live seat %r out of range' % (p,))
            mask |= 1 << int(p)
    if mask < 0 or mask >> n:
        raise ValueError('live mask names seats >= %d' % n)
    r = sampled_equity_batch(holes, b, np.array([len(board)], np.uint8), np.array([mask], np.uint16), samples, seed, nonce, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- ranged sampled equity
# Sampled equity where every hidden seat draws its HOLDING from a weighted range -- any seat count, any street (pk_equity_ranged; the
# definition: include/pokerl_hip.h "Ranged sampled equity").  Attempts whose holdings collide are rejected, so the
# counts are over the ACCEPTED attempts.
class RangedEquity:
    """Counts of one spot or of a batch over the accepted attempts ([N] or [m, N] arrays; `accepted`, `status` scalars or [m]; `samples` =
    the attempts asked for).  `equity` = share / (720720 * accepted), nan where nothing was accepted; `acceptance` = accepted / samples.
    Counts of calls with different nonces add exactly, `accepted` included."""

    def __init__(self, win, tie, share, accepted, status, samples):
        self.win, self.tie, self.share, self.accepted, self.status, self.samples = win, tie, share, accepted, status, samples

    @property
    def equity(self):
        b = np.asarray(self.accepted, np.float64)[..., None] * float(L.EQ_SHARE_UNIT)
        return np.divide(np.asarray(self.share, np.float64), b, out=np.full(np.shape(self.share), np.nan, np.float64), where=b > 0)

    @property
    def acceptance(self):
        return np.asarray(self.accepted, np.float64) / float(self.samples)

    def __getitem__(self, i):
        return RangedEquity(self.win[i], self.tie[i], self.share[i], self.accepted[i], self.status[i], self.samples)

    def __repr__(self):
        return 'RangedEquity(accepted=%r of %r, status=%r, win=%r, tie=%r, equity=%r)' % (self.accepted, self.samples, self.status, self.win,
                                                                                          self.tie, self.equity)


def check_ranges(ranges, range_of, n, m, shared_ok=True):
    """(weights uint16 [R, 1326] or None, R, range_of uint16 or None, per_spot) of a ranged-equity call; ValueError for a wrong shape or more
    than 16 rows -- before any device call.  ranges: None, one [1326] vector or [R, 1326]; range_of: None (every hidden seat uniform; with
    ONE row: every seat that row), [n] for every spot, or [m, n].  shared_ok False: an [n] vector is repeated to [m, n].  An entry that
    names no row is not refused here: where its seat is hidden the SPOT reports EQ_BAD_CARD."""
    w, r = None, 0
    if ranges is not None:
        w = np.ascontiguousarray(ranges, np.uint16)
        if w.ndim == 1:
            w = w.reshape(1, -1)
        if w.ndim != 2 or w.shape[1] != L.EQ_HOLDINGS:
            raise ValueError('ranges must have shape [1326] or [R, 1326]')
        r = w.shape[0]
        if r > L.EQW_MAX_RANGES:
            raise ValueError('at most %d ranges per call' % L.EQW_MAX_RANGES)
        if r == 0:
            w = None
    if range_of is None:
        ro = np.zeros(n, np.int64) if r == 1 else None
    else:
        ro = np.asarray(range_of)
        if ro.shape not in ((n,), (m, n)):
            raise ValueError('range_of must have shape [N] or [m, N]')
        if ((ro < 0) | (ro > 0xFFFF)).any():
            raise ValueError('range_of entries must fit 16 bits')
    per_spot = False
    if ro is not None:
        if ro.shape == (m, n) and (ro.ndim == 2):
            per_spot = True
        elif not shared_ok:
            ro, per_spot = np.broadcast_to(ro, (m, n)), True
        ro = np.ascontiguousarray(ro, np.uint16)
    return w, r, ro, per_spot


def ranged_equity_batch(holes, board, nboard, live, ranges=None, range_of=None, samples=4096, seed=DEFAULT_SEED, nonce=0, ids=None, device=0):
    """pk_equity_ranged on host arrays: as sampled_equity_batch, but a live seat hides both cards or none, and a hidden seat p draws its
    holding from row range_of[i, p] of `ranges` (uint16 [1326] or [R, 1326]; 0xFFFF or range_of None: uniform; an [N] vector serves every
    spot).  Returns a RangedEquity of [m, N] / [m] arrays."""
    holes = np.ascontiguousarray(holes, np.uint8)
    if holes.ndim != 3 or holes.shape[2] != 2 or not (L.MIN_PLAYERS <= holes.shape[1] <= L.MAX_PLAYERS):
        raise ValueError('holes must have shape [m, N, 2] with 2 <= N <= 16')
    m, n = holes.shape[:2]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    live = np.ascontiguousarray(live, np.uint16)
    if board.shape != (m, 5) or nboard.shape != (m,) or live.shape != (m,):
        raise ValueError('board must have shape [m, 5], nboard and live shape [m]')
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.uint32)
        if ids.shape != (m,):
            raise ValueError('ids must have shape [m]')
    samples, nonce = check_samples(samples, nonce)
    if m * ((samples + 63) // 64) > 0xFFFFFFFF:
        raise ValueError('m * ceil(samples / 64) must fit 32 bits: split the batch')
    w, r, ro, _ = check_ranges(ranges, range_of, n, m, shared_ok=False)
    win, tie = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32)
    share = np.zeros((m, n), np.uint64)
    count, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_ranged(int(device), n, m, L.ptr(holes), L.ptr(board), L.ptr(nboard), L.ptr(live), L.ptr(ids), samples,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, nonce, L.ptr(w), r, L.ptr(ro), L.ptr(win), L.ptr(tie), L.ptr(share),
                                     L.ptr(count), L.ptr(status)))
    return RangedEquity(win, tie, share, count, status, samples)


def ranged_equity_d(num_players, m, holes_d, board_d, nboard_d, live_d, samples, weights_d=None, num_ranges=0, range_of_d=None, ids_d=None,
                    seed=DEFAULT_SEED, nonce=0, win_d=None, tie_d=None, share_d=None, accepted_d=None, status_d=None, device=0, stream=None):
    """pk_equity_ranged_d: the same on device-resident buffers (device pointers as ints / c_void_p; weights_d uint16 [num_ranges, 1326],
    range_of_d uint16 [m, N]; ids_d, range_of_d and the outputs may be None), asynchronous on `stream`."""
    samples, nonce = check_samples(samples, nonce)
    if not (L.MIN_PLAYERS <= int(num_players) <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    if not 0 <= int(num_ranges) <= L.EQW_MAX_RANGES:
        raise ValueError('at most %d ranges per call' % L.EQW_MAX_RANGES)
    L.check(L.lib().pk_equity_ranged_d(int(device), int(num_players), int(m), holes_d, board_d, nboard_d, live_d, ids_d, samples,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, nonce, weights_d, int(num_ranges), range_of_d, win_d, tie_d, share_d,
                                       accepted_d, status_d, stream))


def ranged_equity(hands, board=(), live=None, ranges=None, range_of=None, samples=4096, seed=DEFAULT_SEED, nonce=0, device=0):
    """One spot.  hands: per seat two cards (Card-likes / 'RS' strings / Card.value ints) or None = hidden: that seat draws its holding from
    row range_of[seat] of `ranges`; board: 0 .. 5 known cards; live: the seats that show down (iterable of seat numbers or a bit mask;
    default: EVERY seat).  Returns a RangedEquity with [N] arrays; raises ValueError for an invalid spot."""
    hands = list(hands)
    n = len(hands)
    if not (L.MIN_PLAYERS <= n <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    board = list(board)
    if len(board) > 5:
        raise ValueError('at most five board cards')
    holes = np.full((1, n, 2), UNKNOWN_CARD, np.uint8)
    for p, h in enumerate(hands):
        if h is None:
            continue
        h = list(h)
        if len(h) != 2 or any(c is None for c in h):
            raise ValueError('seat %d: two hole cards, or None for a hidden hand' % p)
        holes[0, p] = [_card(c) for c in h]
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    if live is None:
        mask = (1 << n) - 1
    elif isinstance(live, (int, np.integer)):
        mask = int(live)
    else:
        mask = 0
        for p in live:
            if not 0 <= int(p) < n:
                raise ValueError('live seat %r out of range' % (p,))
            mask |= 1 << int(p)
    if mask < 0 or mask >> n:
        raise ValueError('live mask names seats >= %d' % n)
    r = ranged_equity_batch(holes, b, np.array([len(board)], np.uint8), np.array([mask], np.uint16), ranges, range_of, samples, seed, nonce,
                            device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- ranged showdown EV
# Showdown EV in chips where every hidden seat draws its holding from a weighted range: the side pots of showdown_ev over the attempts of
# ranged_equity (pk_ev_ranged; the definition: include/pokerl_hip.h "Ranged showdown EV").  "With what I believe
# about their hands, what am I paid in chips if I call?"
def ranged_ev_status_text(status):
    return ev_status_text(status)           # (the same bits: PK_EQ_BAD_BET in the place of PK_EQ_PREFLOP)


def ranged_ev_formula(amount, share, accepted, bets):
    """ev [N] of one spot by the stated formula in binary64: acc = +0.0; for i ascending: acc = acc + (amount[i] * float(share[i][p])) /
    (720720.0 * float(accepted)); ev[p] = acc - bets[p].  accepted == 0: all +0.0."""
    n = len(bets)
    ev = np.zeros(n, np.float64)
    if int(accepted) == 0:
        return ev
    den = np.float64(L.EQ_SHARE_UNIT) * np.float64(int(accepted))
    for p in range(n):
        acc = np.float64(0.0)
        for i in range(n):
            acc = acc + (np.float64(amount[i]) * np.float64(int(share[i][p]))) / den
        ev[p] = acc - np.float64(bets[p])
    return ev


class RangedEV:
    """Expected payoffs of one spot or of a batch over the ACCEPTED attempts ([N] / [N, N] or [m, N] / [m, N, N] arrays; `accepted`, `status`
    scalars or [m]; `samples` = the attempts asked for): ev, share, level_seat, amount as ShowdownEV with `accepted` in the place of `boards`.
    accepted == 0 with status 0 (a range with no weight left): ev is all +0.0 and is no estimate."""

    def __init__(self, ev, share, level_seat, amount, accepted, status, bets, samples):
        self.ev, self.share, self.level_seat, self.amount, self.accepted, self.status, self.bets, self.samples = (
            ev, share, level_seat, amount, accepted, status, bets, samples)

    @property
    def payout(self):
        """ev + bets: what a seat expects to take out of the pot (0 where a spot was refused or nothing was accepted)."""
        if self.bets is None:
            return None
        ok = ((np.asarray(self.status) == 0) & (np.asarray(self.accepted) > 0))[..., None]
        return np.where(ok, np.asarray(self.ev) + np.asarray(self.bets), 0.0)

    @property
    def levels(self):
        """(seat, amount) pairs of the levels that exist, in visiting order (a batch: one list per spot)."""
        seat, amount = np.asarray(self.level_seat), np.asarray(self.amount)
        if seat.ndim == 1:
            return [(int(s), float(a)) for s, a in zip(seat, amount) if s != NO_LEVEL]
        return [[(int(s), float(a)) for s, a in zip(ss, aa) if s != NO_LEVEL] for ss, aa in zip(seat, amount)]

    @property
    def acceptance(self):
        return np.asarray(self.accepted, np.float64) / float(self.samples)

    def __getitem__(self, i):
        return RangedEV(self.ev[i], self.share[i], self.level_seat[i], self.amount[i], self.accepted[i], self.status[i],
                        None if self.bets is None else self.bets[i], self.samples)

    def merged(self, other):
        """The result of both calls together: two results of the SAME spots drawn with different nonces.  share and accepted add exactly; ev
        is re-formed on the host by the formula on the sums."""
        if self.bets is None or other.bets is None:
            raise ValueError('merged needs the bets of both results')
        a, b = (np.asarray(x.level_seat) for x in (self, other))
        if a.shape != b.shape or not np.array_equal(a, b) or not np.array_equal(np.asarray(self.status), np.asarray(other.status)) or \
                not np.array_equal(np.asarray(self.amount, np.float64).view(np.uint64), np.asarray(other.amount, np.float64).view(np.uint64)):
            raise ValueError('merged: the two results are not of the same spots')
        share = np.asarray(self.share, np.uint64) + np.asarray(other.share, np.uint64)
        acc = np.asarray(self.accepted, np.uint64) + np.asarray(other.accepted, np.uint64)
        bets = np.asarray(self.bets, np.float64)
        if a.ndim == 1:
            ev = ranged_ev_formula(self.amount, share, acc, bets)
        else:
            ev = np.array([ranged_ev_formula(self.amount[i], share[i], acc[i], bets[i]) for i in range(a.shape[0])], np.float64).reshape(a.shape)
        return RangedEV(ev, share, self.level_seat, self.amount, acc, self.status, self.bets, self.samples + other.samples)

    def __repr__(self):
        return 'RangedEV(accepted=%r of %r, status=%r, ev=%r, levels=%r)' % (self.accepted, self.samples, self.status, self.ev, self.levels)


def ranged_ev_batch(holes, board, nboard, live, bets, ranges=None, range_of=None, samples=1024, seed=DEFAULT_SEED, nonce=0, ids=None, device=0):
    """pk_ev_ranged on host arrays: the spots, ranges and stream of ranged_equity_batch plus bets float64 [m, N] (what each seat has committed,
    folded seats included) -> RangedEV of [m, N] / [m, N, N] / [m] arrays.  A bad spot is reported through its `status` (PK_EQ_* bits,
    PK_EQ_BAD_BET among them) with zeros everywhere; the others are unaffected."""
    holes = np.ascontiguousarray(holes, np.uint8)
    if holes.ndim != 3 or holes.shape[2] != 2 or not (L.MIN_PLAYERS <= holes.shape[1] <= L.MAX_PLAYERS):
        raise ValueError('holes must have shape [m, N, 2] with 2 <= N <= 16')
    m, n = holes.shape[:2]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    live = np.ascontiguousarray(live, np.uint16)
    if bets is None:
        raise ValueError('bets: float64 [m, N]')
    bets = np.ascontiguousarray(bets, np.float64)
    if board.shape != (m, 5) or nboard.shape != (m,) or live.shape != (m,) or bets.shape != (m, n):
        raise ValueError('board must have shape [m, 5], nboard and live shape [m], bets shape [m, N]')
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.uint32)
        if ids.shape != (m,):
            raise ValueError('ids must have shape [m]')
    samples, nonce = check_samples(samples, nonce)
    groups = (n - 1 + (3 if n <= 8 else 2) - 1) // (3 if n <= 8 else 2)
    if m * ((samples + 63) // 64) * groups > 0xFFFFFFFF:
        raise ValueError('m * ceil(samples / 64) * (groups of levels) must fit 32 bits: split the batch')
    w, r, ro, _ = check_ranges(ranges, range_of, n, m, shared_ok=False)
    share = np.zeros((m, n, n), np.uint64)
    level_seat = np.full((m, n), NO_LEVEL, np.uint8)
    amount, ev = np.zeros((m, n), np.float64), np.zeros((m, n), np.float64)
    count, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_ev_ranged(int(device), n, m, L.ptr(holes), L.ptr(board), L.ptr(nboard), L.ptr(live), L.ptr(bets), L.ptr(ids), samples,
                                 int(seed) & 0xFFFFFFFFFFFFFFFF, nonce, L.ptr(w), r, L.ptr(ro), L.ptr(share), L.ptr(level_seat), L.ptr(amount),
                                 L.ptr(ev), L.ptr(count), L.ptr(status)))
    return RangedEV(ev, share, level_seat, amount, count, status, bets, samples)


def ranged_ev_d(num_players, m, holes_d, board_d, nboard_d, live_d, bets_d, samples, status_d, weights_d=None, num_ranges=0, range_of_d=None,
                ids_d=None, seed=DEFAULT_SEED, nonce=0, share_d=None, level_seat_d=None, amount_d=None, ev_d=None, accepted_d=None, device=0,
                stream=None):
    """pk_ev_ranged_d: the same on device-resident buffers (device pointers as ints / c_void_p; bets_d float64 [m, N], weights_d uint16
    [num_ranges, 1326], range_of_d uint16 [m, N]; ids_d, range_of_d and every output but status_d may be None), asynchronous on `stream`."""
    samples, nonce = check_samples(samples, nonce)
    if not (L.MIN_PLAYERS <= int(num_players) <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    if not 0 <= int(num_ranges) <= L.EQW_MAX_RANGES:
        raise ValueError('at most %d ranges per call' % L.EQW_MAX_RANGES)
    if bets_d is None or status_d is None:
        raise ValueError('bets_d and status_d are required')
    L.check(L.lib().pk_ev_ranged_d(int(device), int(num_players), int(m), holes_d, board_d, nboard_d, live_d, bets_d, ids_d, samples,
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, nonce, weights_d, int(num_ranges), range_of_d, share_d, level_seat_d, amount_d,
                                   ev_d, accepted_d, status_d, stream))


def ranged_ev(hands, board=None, live=None, bets=None, ranges=None, range_of=None, samples=1024, seed=DEFAULT_SEED, nonce=0, device=0):
    """One spot: ranged_equity's arguments (hands: per seat two cards or None = hidden, drawn from row range_of[seat] of `ranges`) plus bets,
    one number per seat (what the seat has committed to the pot; a folded seat's money counts).  Returns a RangedEV with [N] / [N, N] arrays;
    raises ValueError for an invalid spot."""
    hands = list(hands)
    n = len(hands)
    if not (L.MIN_PLAYERS <= n <= L.MAX_PLAYERS):
        raise ValueError('between 2 and 16 seats')
    if bets is None:
        raise ValueError('bets: one number per seat')
    try:
        bt = np.array([float(x) for x in bets], np.float64)
    except TypeError as e:
        raise ValueError('bets: one number per seat') from e
    if bt.shape != (n,):
        raise ValueError('bets: one number per seat')
    if not np.all(np.isfinite(bt)) or np.any(bt < 0):
        raise ValueError('bets must be finite and not negative')
    board = [] if board is None else list(board)
    if len(board) > 5:
        raise ValueError('at most five board cards')
    holes = np.full((1, n, 2), UNKNOWN_CARD, np.uint8)
    for p, h in enumerate(hands):
        if h is None:
            continue
        h = list(h)
        if len(h) != 2 or any(c is None for c in h):
            raise ValueError('seat %d: two hole cards, or None for a hidden hand' % p)
        holes[0, p] = [_card(c) for c in h]
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    if live is None:
        mask = (1 << n) - 1
    elif isinstance(live, (int, np.integer)):
        mask = int(live)
    else:
        mask = 0
        for p in live:
            if not 0 <= int(p) < n:
                raise ValueError('live seat %r out of range' % (p,))
            mask |= 1 << int(p)
    if mask < 0 or mask >> n:
        raise ValueError('live mask names seats >= %d' % n)
    r = ranged_ev_batch(holes, b, np.array([len(board)], np.uint8), np.array([mask], np.uint16), bt[None, :], ranges, range_of, samples, seed,
                        nonce, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + ranged_ev_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- range equity
# Exact hand strength against ONE hidden hand, post-flop: the hero's win / tie counts against every holding the opponent can have, and their
# sum under a range of weights (pk_equity_range; the definition: include/pokerl_hip.h "Range equity").
_CANON = [((k % 4) << 4) | (k // 4) for k in range(52)]                # canonical index k = rank0 * 4 + suit -> Card.value (cards.py:77)
HOLDINGS = np.array([[_CANON[a], _CANON[b]] for b in range(52) for a in range(b)], np.uint8)   # [1326][2]: holding h = b (b - 1) / 2 + a
HOLDINGS.setflags(write=False)


def _canon_index(c):
    v = _card(c)
    return (v & 15) * 4 + (v >> 4)


def holding_index(c0, c1):
    """The index 0 .. 1325 of the holding {c0, c1} (Card-likes / 'RS' strings / Card.value ints; either order): h = b (b - 1) / 2 + a over
    the canonical indices a < b.  HOLDINGS[h] names its two cards."""
    a, b = sorted((_canon_index(c0), _canon_index(c1)))
    if a == b:
        raise ValueError('a holding is two different cards')
    return b * (b - 1) // 2 + a


def dead_mask(cards):
    """The `dead` word of a range-equity spot: bit k = the card of canonical index k is out of play."""
    mask = 0
    for c in cards:
        mask |= 1 << _canon_index(c)
    return mask


class RangeEquity:
    """Counts of one spot or of a batch against every holding of ONE hidden hand ([1326] or [m, 1326] arrays win / tie, or None where only
    the aggregates were asked for; `boards`, `status` scalars or [m]; agg [3] or [m, 3]): win / tie = boards the hero wins alone / splits
    against that holding, of `boards` completions each; agg = (sum w win, sum w tie, boards * sum of w over the valid holdings).
    `valid` = the holdings both of whose cards are in the pool; `equity` = (win + tie / 2) / boards per holding; `strength` =
    (agg[0] + agg[1] / 2) / agg[2] in float64 (0 where a spot was refused or the range is empty)."""

    def __init__(self, win, tie, boards, status, agg, valid=None):
        self.win, self.tie, self.boards, self.status, self.agg, self.valid = win, tie, boards, status, agg, valid

    @property
    def equity(self):
        if self.win is None:
            raise ValueError('the per-holding counts were not asked for (per_holding=False)')
        b = np.asarray(self.boards, np.float64)[..., None]
        num = np.asarray(self.win, np.float64) + 0.5 * np.asarray(self.tie, np.float64)
        return np.divide(num, b, out=np.zeros(np.shape(self.win), np.float64), where=b > 0)

    @property
    def strength(self):
        a = np.asarray(self.agg, np.float64)
        num, den = a[..., 0] + 0.5 * a[..., 1], a[..., 2]
        return np.divide(num, den, out=np.zeros(np.shape(den), np.float64), where=den > 0)[()]

    def __getitem__(self, i):
        return RangeEquity(None if self.win is None else self.win[i], None if self.tie is None else self.tie[i], self.boards[i], self.status[i],
                           self.agg[i], None if self.valid is None else self.valid[i])

    def __repr__(self):
        return 'RangeEquity(boards=%r, status=%r, strength=%r)' % (self.boards, self.status, self.strength)


def range_weights(weights, m):
    """(array or None, weights_per_spot) of a range-equity call: None = every weight 1, uint16 [1326] = one range for every spot, [m, 1326] =
    one per spot; ValueError for another shape or a weight outside 0 .. 65535 (before any device call)."""
    if weights is None:
        return None, 0
    w = np.asarray(weights)
    if w.dtype.kind not in 'iub' or w.shape not in ((L.EQ_HOLDINGS,), (m, L.EQ_HOLDINGS)):
        raise ValueError('weights must be integers of shape [1326] or [m, 1326]')
    if w.size and (w.min() < 0 or w.max() > 0xFFFF):
        raise ValueError('weights must fit 16 bits')
    return np.ascontiguousarray(w, np.uint16), int(w.ndim == 2)


def valid_holdings(hero, board, nboard, dead=None):
    """bool [m, 1326]: the holdings both of whose cards are in the pool of each spot (host arithmetic on the inputs; refused spots are not
    looked at here -- mask with status == 0)."""
    hero, board = np.asarray(hero, np.uint8), np.asarray(board, np.uint8)
    m = hero.shape[0]
    canon = lambda v: (v.astype(np.int64) & 15) * 4 + (v.astype(np.int64) >> 4)
    out = np.zeros((m, 52), bool)
    rows = np.arange(m)
    for v in (hero[:, 0], hero[:, 1]):
        out[rows, np.clip(canon(v), 0, 51)] = True
    nb = np.minimum(np.asarray(nboard, np.int64), 5)
    for j in range(5):
        sel = nb > j
        out[rows[sel], np.clip(canon(board[sel, j]), 0, 51)] = True
    if dead is not None:
        out |= ((np.asarray(dead, np.uint64)[:, None] >> np.arange(52, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    a = np.array([a for b in range(52) for a in range(b)])
    b = np.array([b for b in range(52) for a in range(b)])
    return ~out[:, a] & ~out[:, b]


def range_equity_batch(hero, board, nboard, dead=None, weights=None, per_holding=True, device=0):
    """pk_equity_range on host arrays: hero uint8 [m, 2] Card.value, board uint8 [m, 5] (the first nboard[i] = 3, 4 or 5 used), nboard uint8
    [m], dead uint64 [m] masks over canonical card indices (None: none), weights None / uint16 [1326] / [m, 1326] -> RangeEquity.  A bad
    spot is reported through its `status` (PK_EQ_* bits) with all-zero outputs; the others are unaffected."""
    hero = np.ascontiguousarray(hero, np.uint8)
    if hero.ndim != 2 or hero.shape[1] != 2:
        raise ValueError('hero must have shape [m, 2]')
    m = hero.shape[0]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    if board.shape != (m, 5) or nboard.shape != (m,):
        raise ValueError('board must have shape [m, 5], nboard shape [m]')
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError('dead must have shape [m]')
    w, per_spot = range_weights(weights, m)
    win = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
    tie = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
    agg, boards, status = np.zeros((m, 3), np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_range(int(device), m, L.ptr(hero), L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(w), per_spot, L.ptr(agg),
                                    L.ptr(win), L.ptr(tie), L.ptr(boards), L.ptr(status)))
    valid = valid_holdings(hero, board, nboard, dead) & (status == 0)[:, None]
    return RangeEquity(win, tie, boards, status, agg, valid)


def range_equity_d(m, hero_d, board_d, nboard_d, dead_d=None, weights_d=None, weights_per_spot=False, agg_d=None, win_d=None, tie_d=None,
                   boards_d=None, status_d=None, device=0, stream=None):
    """pk_equity_range_d: the same on device-resident buffers (device pointers as ints / c_void_p; dead_d, weights_d and the outputs may be
    None), asynchronous on `stream`."""
    L.check(L.lib().pk_equity_range_d(int(device), int(m), hero_d, board_d, nboard_d, dead_d, weights_d, int(bool(weights_per_spot)), agg_d,
                                      win_d, tie_d, boards_d, status_d, stream))


def range_equity(hero, board, dead=(), weights=None, device=0):
    """One spot.  hero: two cards (Card-likes / 'RS' strings / Card.value ints); board: 3 .. 5 known cards; dead: cards known to be out of
    play; weights: None or [1326] integers 0 .. 65535 over holding_index.  Returns a RangeEquity with [1326] arrays and the scalar
    `strength`; raises ValueError for an invalid spot."""
    hero, board = list(hero), list(board)
    if len(hero) != 2:
        raise ValueError('the hero holds two cards')
    if not 3 <= len(board) <= 5:
        raise ValueError('three to five board cards (range equity is post-flop only)')
    h = np.array([[_card(c) for c in hero]], np.uint8)
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    d = np.array([dead_mask(dead)], np.uint64)
    if weights is not None and np.ndim(weights) != 1:
        raise ValueError('weights must have shape [1326]')
    r = range_equity_batch(h, b, np.array([len(board)], np.uint8), d, weights, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- range vs range
# The same three numbers for EVERY holding the hero can have on a public board, against a weighted opponent range: the terminal-node
# evaluation of a solver (pk_equity_rvr; the definition: include/pokerl_hip.h "Range vs range").
class RangeVsRange:
    """Sums of one spot or of a batch ([1326] or [m, 1326] uint64 arrays; `boards`, `status` scalars or [m]): for hero holding h, win / tie =
    the weight of (villain holding, completion) pairs the hero wins alone / splits, tot = the weight of all of them; `valid` = the holdings
    both of whose cards are in the pool.  `strength` = (win + tie / 2) / tot per holding in float64 (nan where tot = 0);
    `against(hero_weights)` = the one range-against-range number."""

    def __init__(self, win, tie, tot, boards, status, valid=None):
        self.win, self.tie, self.tot, self.boards, self.status, self.valid = win, tie, tot, boards, status, valid

    @property
    def strength(self):
        num = np.asarray(self.win, np.float64) + 0.5 * np.asarray(self.tie, np.float64)
        den = np.asarray(self.tot, np.float64)
        return np.divide(num, den, out=np.full(np.shape(den), np.nan, np.float64), where=den > 0)

    def against(self, hero_weights=None):
        """sum u[h] (win[h] + tie[h] / 2) / sum u[h] tot[h] over the hero's range u ([1326] integers; None = ones): the sums in Python
        integers, the quotient in float64 (nan where the denominator is 0).  One spot -> float, a batch -> [m] float64."""
        u = [1] * L.EQ_HOLDINGS if hero_weights is None else [int(x) for x in np.asarray(hero_weights).reshape(-1)]
        if len(u) != L.EQ_HOLDINGS or min(u) < 0:
            raise ValueError('hero_weights must be 1326 non-negative integers')

        def one(win, tie, tot):
            num2 = sum(x * (2 * int(w) + int(t)) for x, w, t in zip(u, win, tie))
            den = sum(x * int(t) for x, t in zip(u, tot))
            return num2 / (2 * den) if den else float('nan')
        if np.ndim(self.win) == 1:
            return one(self.win, self.tie, self.tot)
        return np.array([one(w, t, d) for w, t, d in zip(self.win, self.tie, self.tot)], np.float64)

    def __getitem__(self, i):
        return RangeVsRange(self.win[i], self.tie[i], self.tot[i], self.boards[i], self.status[i], None if self.valid is None else self.valid[i])

    def __repr__(self):
        return 'RangeVsRange(boards=%r, status=%r)' % (self.boards, self.status)


def range_vs_range_batch(board, nboard, dead=None, weights=None, device=0):
    """pk_equity_rvr on host arrays: board uint8 [m, 5] Card.value (the first nboard[i] = 3, 4 or 5 used), nboard uint8 [m], dead uint64 [m]
    masks over canonical card indices (None: none), weights None / uint16 [1326] / [m, 1326] (the opponent's range) -> RangeVsRange.  A bad
    spot is reported through its `status` (PK_EQ_* bits) with all-zero outputs; the others are unaffected."""
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 5:
        raise ValueError('board must have shape [m, 5]')
    m = board.shape[0]
    nboard = np.ascontiguousarray(nboard, np.uint8)
    if nboard.shape != (m,):
        raise ValueError('nboard must have shape [m]')
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError('dead must have shape [m]')
    w, per_spot = range_weights(weights, m)
    win, tie, tot = (np.zeros((m, L.EQ_HOLDINGS), np.uint64) for _ in range(3))
    boards, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_rvr(int(device), m, L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(w), per_spot, L.ptr(win), L.ptr(tie),
                                  L.ptr(tot), L.ptr(boards), L.ptr(status)))
    return RangeVsRange(win, tie, tot, boards, status, rvr_valid_holdings(board, nboard, dead) & (status == 0)[:, None])


def rvr_valid_holdings(board, nboard, dead=None):
    """bool [m, 1326]: the holdings both of whose cards are in the pool of each range-vs-range spot (valid_holdings without a hero)."""
    board = np.asarray(board, np.uint8)
    m = board.shape[0]
    canon = lambda v: (v.astype(np.int64) & 15) * 4 + (v.astype(np.int64) >> 4)
    out = np.zeros((m, 52), bool)
    rows = np.arange(m)
    nb = np.minimum(np.asarray(nboard, np.int64), 5)
    for j in range(5):
        sel = nb > j
        out[rows[sel], np.clip(canon(board[sel, j]), 0, 51)] = True
    if dead is not None:
        out |= ((np.asarray(dead, np.uint64)[:, None] >> np.arange(52, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    a = np.array([a for b in range(52) for a in range(b)])
    b = np.array([b for b in range(52) for a in range(b)])
    return ~out[:, a] & ~out[:, b]


def range_vs_range_d(m, board_d, nboard_d, dead_d=None, weights_d=None, weights_per_spot=False, win_d=None, tie_d=None, tot_d=None,
                     boards_d=None, status_d=None, device=0, stream=None):
    """pk_equity_rvr_d: the same on device-resident buffers (device pointers as ints / c_void_p; dead_d, weights_d and the outputs may be
    None; win / tie / tot are uint64 [m, 1326]), asynchronous on `stream`."""
    L.check(L.lib().pk_equity_rvr_d(int(device), int(m), board_d, nboard_d, dead_d, weights_d, int(bool(weights_per_spot)), win_d, tie_d,
                                    tot_d, boards_d, status_d, stream))


def range_vs_range(board, dead=(), weights=None, device=0):
    """One spot.  board: 3 .. 5 known cards (Card-likes / 'RS' strings / Card.value ints); dead: cards known to be out of play; weights:
    None or [1326] integers 0 .. 65535 over holding_index, the opponent's range.  Returns a RangeVsRange with [1326] arrays; raises
    ValueError for an invalid spot."""
    board = list(board)
    if not 3 <= len(board) <= 5:
        raise ValueError('invalid spot: ' + equity_status_text(L.EQ_PREFLOP) if len(board) < 3 else 'three to five board cards')
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    d = np.array([dead_mask(dead)], np.uint64)
    if weights is not None and np.ndim(weights) != 1:
        raise ValueError('weights must have shape [1326]')
    r = range_vs_range_batch(b, np.array([len(board)], np.uint8), d, weights, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- pre-flop matchups
# The pre-flop forms of the two families above: every ordered pair of holdings over every five-card board, counted once per device and kept
# resident (pk_preflop_*; the definition: include/pokerl_hip.h "Pre-flop matchups").
class PreflopMatchups:
    """The matchup table: uint32 [1326, 1326] win / tie over judger.holding_index -- win[h, o] = boards (of `boards` = 1 712 304) on which h
    wins alone against o, tie[h, o] = boards both win; 0 where the two share a card.  `equity` = (win + tie / 2) / boards in float64, nan
    where the pair shares a card.  The evaluator's suit quirks are in it: it is not invariant under a renaming of suits."""
    boards = L.PREFLOP_BOARDS

    def __init__(self, win, tie):
        self.win, self.tie = win, tie

    @property
    def shared(self):
        """bool [1326, 1326]: the two holdings share a card (the diagonal included)."""
        a, b = HOLDINGS[:, 0].astype(np.int64), HOLDINGS[:, 1].astype(np.int64)
        m = (np.uint64(1) << a.astype(np.uint64)) | (np.uint64(1) << b.astype(np.uint64))     # (Card.value < 64: one bit per card)
        return (m[:, None] & m[None, :]) != 0

    @property
    def equity(self):
        e = (self.win.astype(np.float64) + 0.5 * self.tie.astype(np.float64)) / float(self.boards)
        e[self.shared] = np.nan
        return e

    def __repr__(self):
        return 'PreflopMatchups(boards=%d)' % self.boards


def preflop_counts(first, n, win=None, tie=None, device=0):
    """pk_preflop_count: the partial counts over the boards of rank first .. first + n - 1 (itertools.combinations(range(52), 5) order over
    the canonical card indices) as uint32 [1326, 1326] (win, tie).  With win / tie given (C-contiguous uint32 [1326, 1326]) the counts are
    ADDED to them in place; otherwise fresh arrays are returned.  Counts over disjoint ranges add exactly."""
    first, n = int(first), int(n)
    if first < 0 or n < 0 or first + n > L.PREFLOP_ALL_BOARDS:
        raise ValueError('the board range must lie in 0 .. %d' % L.PREFLOP_ALL_BOARDS)
    if (win is None) != (tie is None):
        raise ValueError('give both win and tie, or neither')
    accumulate = win is not None
    if accumulate:
        for a in (win, tie):
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.shape == (L.EQ_HOLDINGS, L.EQ_HOLDINGS) and a.flags.c_contiguous):
                raise ValueError('win / tie must be C-contiguous uint32 [1326, 1326] arrays')
    else:
        win, tie = np.zeros((L.EQ_HOLDINGS, L.EQ_HOLDINGS), np.uint32), np.zeros((L.EQ_HOLDINGS, L.EQ_HOLDINGS), np.uint32)
    L.check(L.lib().pk_preflop_count(int(device), first, n, int(accumulate), L.ptr(win), L.ptr(tie)))
    return win, tie


def preflop_counts_d(first, n, win_d, tie_d, accumulate=False, device=0, stream=None):
    """pk_preflop_count_d: the same into device buffers (uint32 [1326, 1326]; either may be None), asynchronous on `stream`."""
    L.check(L.lib().pk_preflop_count_d(int(device), int(first), int(n), int(bool(accumulate)), win_d, tie_d, stream))


def preflop_matchups(device=0):
    """The matchup table of `device` as a PreflopMatchups (pk_preflop_matchups): built on the device on first use -- every holding ranked
    once per board, every pair compared on every board -- and resident from then on; a later call only copies it."""
    win, tie = np.empty((L.EQ_HOLDINGS, L.EQ_HOLDINGS), np.uint32), np.empty((L.EQ_HOLDINGS, L.EQ_HOLDINGS), np.uint32)
    L.check(L.lib().pk_preflop_matchups(int(device), L.ptr(win), L.ptr(tie)))
    return PreflopMatchups(win, tie)


def preflop_matchups_d(win_d, tie_d, device=0, stream=None):
    """pk_preflop_matchups_d: the table into device buffers (uint32 [1326, 1326]; either may be None), asynchronous on `stream`."""
    L.check(L.lib().pk_preflop_matchups_d(int(device), win_d, tie_d, stream))


def preflop_valid_holdings(hero):
    """bool [m, 1326]: the holdings that share no card with each spot's hero (host arithmetic; mask with status == 0)."""
    hero = np.asarray(hero, np.uint8)
    return (HOLDINGS[None, :, :, None] != hero[:, None, None, :]).all(axis=(2, 3))


def preflop_equity_batch(hero, weights=None, per_holding=True, device=0):
    """pk_equity_preflop on host arrays: hero uint8 [m, 2] Card.value, weights None / uint16 [1326] / [m, 1326] -> RangeEquity (boards =
    1 712 304): the hero's starting hand against ONE hidden hand, no board.  A bad spot is reported through its `status` (PK_EQ_BAD_CARD /
    PK_EQ_DUP_CARD) with all-zero outputs; the others are unaffected."""
    hero = np.ascontiguousarray(hero, np.uint8)
    if hero.ndim != 2 or hero.shape[1] != 2:
        raise ValueError('hero must have shape [m, 2]')
    m = hero.shape[0]
    w, per_spot = range_weights(weights, m)
    win = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
    tie = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
    agg, boards, status = np.zeros((m, 3), np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_preflop(int(device), m, L.ptr(hero), L.ptr(w), per_spot, L.ptr(agg), L.ptr(win), L.ptr(tie), L.ptr(boards),
                                      L.ptr(status)))
    return RangeEquity(win, tie, boards, status, agg, preflop_valid_holdings(hero) & (status == 0)[:, None])


def preflop_equity_d(m, hero_d, weights_d=None, weights_per_spot=False, agg_d=None, win_d=None, tie_d=None, boards_d=None, status_d=None,
                     device=0, stream=None):
    """pk_equity_preflop_d: the same on device-resident buffers (device pointers as ints / c_void_p; weights_d and the outputs may be
    None), asynchronous on `stream`."""
    L.check(L.lib().pk_equity_preflop_d(int(device), int(m), hero_d, weights_d, int(bool(weights_per_spot)), agg_d, win_d, tie_d, boards_d,
                                        status_d, stream))


def preflop_equity(hero, weights=None, device=0):
    """One starting hand.  hero: two cards (Card-likes / 'RS' strings / Card.value ints); weights: None or [1326] integers 0 .. 65535 over
    holding_index.  Returns a RangeEquity with [1326] arrays and the scalar `strength`; raises ValueError for an invalid spot."""
    hero = list(hero)
    if len(hero) != 2:
        raise ValueError('the hero holds two cards')
    if weights is not None and np.ndim(weights) != 1:
        raise ValueError('weights must have shape [1326]')
    r = preflop_equity_batch(np.array([[_card(c) for c in hero]], np.uint8), weights, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


def preflop_range_vs_range_batch(weights, device=0):
    """pk_equity_rvr_preflop on host arrays: weights uint16 [m, 1326], one opponent range per spot -> RangeVsRange with uint64 [m, 1326]
    win / tie / tot (boards = 1 712 304, status 0, every holding valid): every starting hand against each range, no board."""
    w = np.asarray(weights)
    if w.dtype.kind not in 'iub' or w.ndim != 2 or w.shape[1] != L.EQ_HOLDINGS:
        raise ValueError('weights must be integers of shape [m, 1326]')
    if w.size and (w.min() < 0 or w.max() > 0xFFFF):
        raise ValueError('weights must fit 16 bits')
    w = np.ascontiguousarray(w, np.uint16)
    m = w.shape[0]
    win, tie, tot = (np.zeros((m, L.EQ_HOLDINGS), np.uint64) for _ in range(3))
    L.check(L.lib().pk_equity_rvr_preflop(int(device), m, L.ptr(w), L.ptr(win), L.ptr(tie), L.ptr(tot)))
    return RangeVsRange(win, tie, tot, np.full(m, L.PREFLOP_BOARDS, np.uint32), np.zeros(m, np.uint8), np.ones((m, L.EQ_HOLDINGS), bool))


def preflop_range_vs_range_d(m, weights_d=None, win_d=None, tie_d=None, tot_d=None, device=0, stream=None):
    """pk_equity_rvr_preflop_d: the same on device-resident buffers (weights_d uint16 [m, 1326] or None = ones; win / tie / tot uint64
    [m, 1326], any may be None), asynchronous on `stream`."""
    L.check(L.lib().pk_equity_rvr_preflop_d(int(device), int(m), weights_d, win_d, tie_d, tot_d, stream))


def preflop_range_vs_range(weights=None, device=0):
    """One opponent range (None: uniform; or [1326] integers 0 .. 65535 over holding_index) -> a RangeVsRange with [1326] arrays: the
    pre-flop strength of every starting hand against it (`.strength`, `.against(hero_weights)`)."""
    if weights is None:
        weights = np.ones(L.EQ_HOLDINGS, np.uint16)
    if np.ndim(weights) != 1:
        raise ValueError('weights must have shape [1326]')
    return preflop_range_vs_range_batch(np.asarray(weights)[None, :], device=device)[0]


# ---------------------------------------------------------------------------------------------- strength histograms
# For EVERY holding the hero can have on a public board: how its river strength against a weighted opponent range is distributed over the
# completions of the board (pk_equity_hist; the definition: include/pokerl_hip.h "Strength histograms").
def check_bins(bins):
    """bins as an int 1 .. PK_EQ_HIST_MAX_BINS; ValueError otherwise (before any device call)."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= L.EQ_HIST_MAX_BINS:
        raise ValueError('bins must be an integer 1 .. %d' % L.EQ_HIST_MAX_BINS)
    return int(bins)


class StrengthHistogram:
    """Counts of one spot or of a batch: hist uint16 [1326, bins] or [m, 1326, bins] -- completions of the board on which holding h's river
    strength (below + equal / 2) / den falls into each of `bins` equal parts of [0, 1] --, void uint16 [1326] or [m, 1326] -- completions on
    which the opponent's range has no weight left --, `completions` = C(P - 2, k) and `status` scalars or [m]; `valid` = the holdings both
    of whose cards are in the pool.  For a valid h: hist[h].sum() + void[h] == completions.  `pdf` = hist / hist.sum(-1) in float64 (nan
    where nothing was counted), `cdf` its running sum."""

    def __init__(self, hist, void, completions, status, valid=None):
        self.hist, self.void, self.completions, self.status, self.valid = hist, void, completions, status, valid

    @property
    def bins(self):
        return np.shape(self.hist)[-1]

    @property
    def pdf(self):
        h = np.asarray(self.hist, np.float64)
        n = h.sum(axis=-1, keepdims=True)
        return np.divide(h, n, out=np.full(h.shape, np.nan, np.float64), where=n > 0)

    @property
    def cdf(self):
        return np.cumsum(self.pdf, axis=-1)

    def __getitem__(self, i):
        return StrengthHistogram(self.hist[i], self.void[i], self.completions[i], self.status[i], None if self.valid is None else self.valid[i])

    def cluster(self, k, iters=20, seed=DEFAULT_SEED, nonce=0, init=None, device=0):
        """cluster_histograms over every row of `hist`: labels come back in the shape of `hist` without its last axis ([1326] or [m, 1326]),
        PK_CL_NONE (0xFFFF) at the invalid holdings and refused spots, whose rows are empty."""
        return cluster_histograms(self.hist, k, iters=iters, seed=seed, nonce=nonce, init=init, device=device)

    def __repr__(self):
        return 'StrengthHistogram(bins=%r, completions=%r, status=%r)' % (self.bins, self.completions, self.status)


def histogram_emd(a, b):
    """The 1-D earth mover's distance of two strength histograms in BIN units: the L1 distance of their CDFs, sum over bins of |cdf_a -
    cdf_b|.  a, b: count or probability arrays [..., bins] (each normalised by its own sum; broadcast against each other), float64 out;
    nan where either has no mass.  Divide by bins for units of strength."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim < 1 or b.ndim < 1 or a.shape[-1] != b.shape[-1]:
        raise ValueError('histograms must have the same number of bins')

    def cdf(x):
        n = x.sum(axis=-1, keepdims=True)
        return np.cumsum(np.divide(x, n, out=np.full(x.shape, np.nan, np.float64), where=n > 0), axis=-1)
    return np.abs(cdf(a) - cdf(b)).sum(axis=-1)


def strength_histogram_batch(board, nboard, dead=None, weights=None, bins=10, device=0):
    """pk_equity_hist on host arrays: board uint8 [m, 5] Card.value (the first nboard[i] = 3, 4 or 5 used), nboard uint8 [m], dead uint64 [m]
    masks over canonical card indices (None: none), weights None / uint16 [1326] / [m, 1326] (the opponent's range), bins 1 .. 32 ->
    StrengthHistogram.  A bad spot is reported through its `status` (PK_EQ_* bits) with all-zero outputs; the others are unaffected."""
    bins = check_bins(bins)
    board = np.ascontiguousarray(board, np.uint8)
    if board.ndim != 2 or board.shape[1] != 5:
        raise ValueError('board must have shape [m, 5]')
    m = board.shape[0]
    nboard = np.ascontiguousarray(nboard, np.uint8)
    if nboard.shape != (m,):
        raise ValueError('nboard must have shape [m]')
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError('dead must have shape [m]')
    w, per_spot = range_weights(weights, m)
    hist, void = np.zeros((m, L.EQ_HOLDINGS, bins), np.uint16), np.zeros((m, L.EQ_HOLDINGS), np.uint16)
    completions, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_hist(int(device), m, L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(w), per_spot, bins, L.ptr(hist), L.ptr(void),
                                   L.ptr(completions), L.ptr(status)))
    return StrengthHistogram(hist, void, completions, status, rvr_valid_holdings(board, nboard, dead) & (status == 0)[:, None])


def strength_histogram_d(m, board_d, nboard_d, dead_d=None, weights_d=None, weights_per_spot=False, bins=10, hist_d=None, void_d=None,
                         completions_d=None, status_d=None, device=0, stream=None):
    """pk_equity_hist_d: the same on device-resident buffers (device pointers as ints / c_void_p; dead_d, weights_d and the outputs may be
    None; hist is uint16 [m, 1326, bins], void uint16 [m, 1326]), asynchronous on `stream`."""
    L.check(L.lib().pk_equity_hist_d(int(device), int(m), board_d, nboard_d, dead_d, weights_d, int(bool(weights_per_spot)), check_bins(bins),
                                     hist_d, void_d, completions_d, status_d, stream))


def strength_histogram(board, dead=(), weights=None, bins=10, device=0):
    """One spot.  board: 3 .. 5 known cards (Card-likes / 'RS' strings / Card.value ints); dead: cards known to be out of play; weights:
    None or [1326] integers 0 .. 65535 over holding_index, the opponent's range; bins 1 .. 32.  Returns a StrengthHistogram with
    [1326, bins] / [1326] arrays; raises ValueError for an invalid spot."""
    bins = check_bins(bins)
    board = list(board)
    if not 3 <= len(board) <= 5:
        raise ValueError('invalid spot: ' + equity_status_text(L.EQ_PREFLOP) if len(board) < 3 else 'three to five board cards')
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    d = np.array([dead_mask(dead)], np.uint64)
    if weights is not None and np.ndim(weights) != 1:
        raise ValueError('weights must have shape [1326]')
    r = strength_histogram_batch(b, np.array([len(board)], np.uint8), d, weights, bins, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- hero strength histogram
# The strength histogram of ONE holding -- row holding_index(hero) of the histograms above at the cost of one range-equity spot -- and,
# with centroids, its bucket in the same call (pk_equity_hist_hero; the definition: include/pokerl_hip.h "Hero strength histogram",
# DESIGN.md section 3.9).
class HeroHistogram:
    """Counts of one spot or of a batch: hist uint16 [bins] or [m, bins] -- completions of the board on which the hero's river strength
    (below + equal / 2) / den falls into each of `bins` equal parts of [0, 1] --, void -- completions on which the opponent's range has no
    weight left --, `completions` = C(P, k) and `status`, scalars or [m]: hist.sum(-1) + void == completions.  `pdf` = hist / hist.sum(-1) in
    float64 (nan where nothing was counted), `cdf` its running sum.  With centroids: `label` uint16 (PK_CL_NONE = 0xFFFF for an empty row),
    `dist` uint32 and `emd` = dist / 65535, the earth mover's distance to the bucket's centroid in bins; None without."""

    def __init__(self, hist, void, completions, status, label=None, dist=None):
        self.hist, self.void, self.completions, self.status, self.label, self.dist = hist, void, completions, status, label, dist

    @property
    def bins(self):
        return np.shape(self.hist)[-1]

    @property
    def pdf(self):
        h = np.asarray(self.hist, np.float64)
        n = h.sum(axis=-1, keepdims=True)
        return np.divide(h, n, out=np.full(h.shape, np.nan, np.float64), where=n > 0)

    @property
    def cdf(self):
        return np.cumsum(self.pdf, axis=-1)

    @property
    def emd(self):
        return None if self.dist is None else np.asarray(self.dist, np.float64) / 65535.0

    def __getitem__(self, i):
        return HeroHistogram(self.hist[i], self.void[i], self.completions[i], self.status[i], None if self.label is None else self.label[i],
                             None if self.dist is None else self.dist[i])

    def __repr__(self):
        return 'HeroHistogram(bins=%r, completions=%r, status=%r, label=%r)' % (self.bins, self.completions, self.status, self.label)


def hero_bucket_args(bins, centroids, m):
    """(bins, centroids or None, K, label or None, dist or None) of a hero-histogram call; ValueError before any device call."""
    bins = check_bins(bins)
    if centroids is None:
        return bins, None, 0, None, None
    cen = _cl_centroids(centroids, bins)
    return bins, cen, cen.shape[0], np.zeros(m, np.uint16), np.zeros(m, np.uint32)


def hero_histogram_batch(hero, board, nboard, dead=None, weights=None, bins=10, centroids=None, device=0):
    """pk_equity_hist_hero on host arrays: hero uint8 [m, 2] Card.value, board uint8 [m, 5] (the first nboard[i] = 3, 4 or 5 used), nboard
    uint8 [m], dead uint64 [m] masks over canonical card indices (None: none), weights None / uint16 [1326] / [m, 1326] (the opponent's
    range), bins 1 .. 32, centroids None or uint16 [k, bins] (cluster_histograms(...).centroids) -> HeroHistogram.  A bad spot is reported
    through its `status` (PK_EQ_* bits) with all-zero outputs and label PK_CL_NONE; the others are unaffected."""
    hero = np.ascontiguousarray(hero, np.uint8)
    if hero.ndim != 2 or hero.shape[1] != 2:
        raise ValueError('hero must have shape [m, 2]')
    m = hero.shape[0]
    board = np.ascontiguousarray(board, np.uint8)
    nboard = np.ascontiguousarray(nboard, np.uint8)
    if board.shape != (m, 5) or nboard.shape != (m,):
        raise ValueError('board must have shape [m, 5], nboard shape [m]')
    if dead is not None:
        dead = np.ascontiguousarray(dead, np.uint64)
        if dead.shape != (m,):
            raise ValueError('dead must have shape [m]')
    w, per_spot = range_weights(weights, m)
    bins, cen, k, label, dist = hero_bucket_args(bins, centroids, m)
    hist, void = np.zeros((m, bins), np.uint16), np.zeros(m, np.uint16)
    completions, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(L.lib().pk_equity_hist_hero(int(device), m, L.ptr(hero), L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(w), per_spot, bins,
                                        L.ptr(hist), L.ptr(void), L.ptr(completions), L.ptr(status), k, L.ptr(cen), L.ptr(label), L.ptr(dist)))
    return HeroHistogram(hist, void, completions, status, label, dist)


def hero_histogram_d(m, hero_d, board_d, nboard_d, dead_d=None, weights_d=None, weights_per_spot=False, bins=10, hist_d=None, void_d=None,
                     completions_d=None, status_d=None, k=0, centroids_d=None, label_d=None, dist_d=None, device=0, stream=None):
    """pk_equity_hist_hero_d: the same on device-resident buffers (device pointers as ints / c_void_p; dead_d, weights_d and the outputs may
    be None; hist is uint16 [m, bins]; k = 0: no bucket stage, else centroids_d uint16 [k, bins] and label_d uint16 [m] / dist_d uint32 [m]),
    asynchronous on `stream`."""
    k = _cl_int('k', k, 0, L.CL_MAX_K)
    if k and centroids_d is None:
        raise ValueError('k > 0 needs centroids_d')
    if not k and (label_d is not None or dist_d is not None):
        raise ValueError('label_d / dist_d need k > 0 and centroids_d')
    L.check(L.lib().pk_equity_hist_hero_d(int(device), int(m), hero_d, board_d, nboard_d, dead_d, weights_d, int(bool(weights_per_spot)),
                                          check_bins(bins), hist_d, void_d, completions_d, status_d, k, centroids_d, label_d, dist_d, stream))


def hero_histogram(hero, board, dead=(), weights=None, bins=10, centroids=None, device=0):
    """One spot.  hero: two cards (Card-likes / 'RS' strings / Card.value ints); board: 3 .. 5 known cards; dead: cards known to be out of
    play; weights: None or [1326] integers 0 .. 65535 over holding_index, the opponent's range; bins 1 .. 32; centroids: None or uint16
    [k, bins].  Returns a HeroHistogram with a [bins] hist and scalars; raises ValueError for an invalid spot."""
    bins = check_bins(bins)
    hero, board = list(hero), list(board)
    if len(hero) != 2:
        raise ValueError('the hero holds two cards')
    if not 3 <= len(board) <= 5:
        raise ValueError('invalid spot: ' + equity_status_text(L.EQ_PREFLOP) if len(board) < 3 else 'three to five board cards')
    h = np.array([[_card(c) for c in hero]], np.uint8)
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = [_card(c) for c in board]
    d = np.array([dead_mask(dead)], np.uint64)
    if weights is not None and np.ndim(weights) != 1:
        raise ValueError('weights must have shape [1326]')
    r = hero_histogram_batch(h, b, np.array([len(board)], np.uint8), d, weights, bins, centroids, device=device)[0]
    if r.status:
        raise ValueError('invalid spot: ' + equity_status_text(r.status))
    return r


# ---------------------------------------------------------------------------------------------- histogram clustering
# Buckets of strength histograms: exact k-means under the earth mover's distance on the device (pk_hist_cluster; the definition:
# include/pokerl_hip.h "Histogram clustering").  Every quantity is an integer.
CL_NONE = L.CL_NONE      # the label of an empty row (an invalid holding, a refused spot)


def _cl_rows(hist):
    """hist [..., bins] counts -> (uint16 [n, bins] C-contiguous, the leading shape); ValueError otherwise (before any device call)."""
    a = np.asarray(hist)
    if a.ndim < 2 or not 1 <= a.shape[-1] <= L.EQ_HIST_MAX_BINS:
        raise ValueError('hist must have shape [..., bins] with bins 1 .. %d' % L.EQ_HIST_MAX_BINS)
    if a.dtype != np.uint16:
        if a.dtype.kind not in 'iu' or (a.size and (a.min() < 0 or a.max() > 65535)):
            raise ValueError('hist must hold integers 0 .. 65535')
    lead = a.shape[:-1]
    flat = np.ascontiguousarray(a.reshape(-1, a.shape[-1]), np.uint16)
    if not 1 <= flat.shape[0] < 2 ** 31:
        raise ValueError('hist must have 1 .. 2^31 - 1 rows')
    return flat, lead


def _cl_int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError('%s must be an integer %d .. %d' % (name, lo, hi))
    return int(v)


def _cl_k(k, flat):
    k = _cl_int('k', k, 1, L.CL_MAX_K)
    live = int(np.count_nonzero(flat.any(axis=1)))
    if k > live:
        raise ValueError('k = %d is larger than the number of non-empty rows (%d)' % (k, live))
    return k


def _cl_centroids(centroids, bins, name='centroids'):
    c = np.asarray(centroids)
    if c.ndim != 2 or c.shape[1] != bins or not 1 <= c.shape[0] <= L.CL_MAX_K:
        raise ValueError('%s must have shape [k, %d] with k 1 .. %d' % (name, bins, L.CL_MAX_K))
    if c.dtype != np.uint16 and (c.dtype.kind not in 'iu' or c.min() < 0 or c.max() > 65535):
        raise ValueError('%s must hold integers 0 .. 65535 (quantised CDFs)' % name)
    return np.ascontiguousarray(c, np.uint16)


class HistogramClusters:
    """The result of cluster_histograms: centroids uint16 [k, bins] (quantised CDFs, 65535 = 1), labels uint16 [...] (PK_CL_NONE = 0xFFFF for an
    empty row) and dist uint32 [...] in the leading shape of the input, inertia uint64 [iterations run + 1] (the last entry belongs to the
    returned labels), changed uint32 [iterations run].  `emd` = dist / 65535, the earth mover's distance to the row's centroid in bins
    (histogram_emd's unit).  assign(hist) labels further rows with the learned centroids."""

    def __init__(self, centroids, labels, dist, inertia, changed, device=0):
        self.centroids, self.labels, self.dist, self.inertia, self.changed, self.device = centroids, labels, dist, inertia, changed, device

    @property
    def k(self):
        return self.centroids.shape[0]

    @property
    def bins(self):
        return self.centroids.shape[1]

    @property
    def emd(self):
        return np.asarray(self.dist, np.float64) / 65535.0

    def assign(self, hist):
        """(labels, dist) of the rows of hist [..., bins] under these centroids."""
        return assign_histograms(hist, self.centroids, device=self.device)

    def __repr__(self):
        return 'HistogramClusters(k=%d, bins=%d, iterations=%d, inertia=%d)' % (self.k, self.bins, len(self.changed), int(self.inertia[-1]))


def seed_histogram_centroids(hist, k, seed=DEFAULT_SEED, nonce=0, device=0):
    """pk_hist_cluster_seed on host arrays: exact k-means++ with linear weights -> centroids uint16 [k, bins]."""
    flat, _ = _cl_rows(hist)
    k = _cl_k(k, flat)
    seed, nonce = _cl_int('seed', seed, 0, 2 ** 64 - 1), _cl_int('nonce', nonce, 0, 2 ** 32 - 1)
    cen = np.zeros((k, flat.shape[1]), np.uint16)
    L.check(L.lib().pk_hist_cluster_seed(int(device), flat.shape[0], flat.shape[1], L.ptr(flat), k, seed, nonce, L.ptr(cen)))
    return cen


def assign_histograms(hist, centroids, device=0):
    """pk_hist_cluster_assign on host arrays -> (labels uint16, dist uint32) in the leading shape of hist: the nearest centroid (the smallest
    index among equals) and the distance to it; PK_CL_NONE and 0 for an empty row.  Any number of rows against any number of centroids."""
    flat, lead = _cl_rows(hist)
    cen = _cl_centroids(centroids, flat.shape[1])
    label, dist = np.zeros(flat.shape[0], np.uint16), np.zeros(flat.shape[0], np.uint32)
    L.check(L.lib().pk_hist_cluster_assign(int(device), flat.shape[0], flat.shape[1], L.ptr(flat), cen.shape[0], L.ptr(cen), L.ptr(label), L.ptr(dist)))
    return label.reshape(lead), dist.reshape(lead)


def cluster_histograms(hist, k, iters=20, seed=DEFAULT_SEED, nonce=0, init=None, device=0):
    """Buckets the rows of hist [..., bins] into k clusters: seeds (seed_histogram_centroids; `init`: a [k, bins] uint16 centroid array to
    start from instead), then ONE pk_hist_cluster call of `iters` iterations: ALL `iters` ARE ALWAYS PAID FOR on the device, also by a run
    that settles early.  An iteration that changes no label is a fixed point -- the iterations after it are no-ops --, so `inertia` and
    `changed` are cut there: the result is that of stopping.  -> HistogramClusters."""
    flat, lead = _cl_rows(hist)
    k = _cl_k(k, flat)
    iters = _cl_int('iters', iters, 1, L.CL_MAX_ITERS)
    if init is None:
        cen = seed_histogram_centroids(flat, k, seed=seed, nonce=nonce, device=device)
    else:
        cen = _cl_centroids(init, flat.shape[1], 'init').copy()
        if cen.shape[0] != k:
            raise ValueError('init must have shape [k, bins]')
    n = flat.shape[0]
    label, dist = np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    inertia, changed = np.zeros(iters + 1, np.uint64), np.zeros(iters, np.uint32)
    L.check(L.lib().pk_hist_cluster(int(device), n, flat.shape[1], L.ptr(flat), k, L.ptr(cen), iters, L.ptr(label), L.ptr(dist), L.ptr(inertia),
                                    L.ptr(changed)))
    still = np.flatnonzero(changed == 0)
    ran = int(still[0]) + 1 if still.size else iters
    return HistogramClusters(cen, label.reshape(lead), dist.reshape(lead), np.concatenate([inertia[:ran], inertia[-1:]]), changed[:ran], device)


def seed_histogram_centroids_d(n, bins, hist_d, k, centroids_d, seed=DEFAULT_SEED, nonce=0, device=0, stream=None):
    """pk_hist_cluster_seed_d: seeding on device-resident buffers (device pointers as ints / c_void_p), asynchronous on `stream`."""
    L.check(L.lib().pk_hist_cluster_seed_d(int(device), int(n), check_bins(bins), hist_d, _cl_int('k', k, 1, L.CL_MAX_K),
                                           _cl_int('seed', seed, 0, 2 ** 64 - 1), _cl_int('nonce', nonce, 0, 2 ** 32 - 1), centroids_d, stream))


def assign_histograms_d(n, bins, hist_d, k, centroids_d, label_d, dist_d=None, device=0, stream=None):
    """pk_hist_cluster_assign_d: hist uint16 [n, bins], centroids uint16 [k, bins] -> label uint16 [n], dist uint32 [n] (None: not wanted)."""
    L.check(L.lib().pk_hist_cluster_assign_d(int(device), int(n), check_bins(bins), hist_d, _cl_int('k', k, 1, L.CL_MAX_K), centroids_d, label_d, dist_d,
                                             stream))


def cluster_histograms_d(n, bins, hist_d, k, centroids_d, iters, label_d, dist_d=None, inertia_d=None, changed_d=None, device=0, stream=None):
    """pk_hist_cluster_d: EXACTLY `iters` iterations from the centroids in centroids_d (in: seeds, out: result) and one final assign;
    inertia uint64 [iters + 1], changed uint32 [iters] (None: not wanted).  Asynchronous on `stream`."""
    L.check(L.lib().pk_hist_cluster_d(int(device), int(n), check_bins(bins), hist_d, _cl_int('k', k, 1, L.CL_MAX_K), centroids_d,
                                      _cl_int('iters', iters, 1, L.CL_MAX_ITERS), label_d, dist_d, inertia_d, changed_d, stream))
