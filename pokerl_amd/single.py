"""`Game` and `PokerGameEnv` with the reference's OWN shapes: one table, scalars and per-seat vectors, `Card` lists and
`StateView` objects -- for code written against pokerl/game.py and pokerl/envs/game_env.py that is moved over unchanged
(examples/random_game.py, a learner's evaluation loop, a debugger session).  Thin views over VecGame / VecPokerGameEnv with
`num_tables = 1`: every value still comes from the HIP kernels, nothing is computed here.  (One table per launch is a
latency-bound way to use a GPU: batch with VecGame when throughput matters.)
"""
import copy

import numpy as np

from .enums import PlayerState
from .envs import VecPokerGameEnv
from .game import VecGame
from .state_view import Card, StateView


class Game:
    """`pokerl.game.Game(**config)` (game.py:242-264): same config keys, attributes, properties and methods."""

    StateView = StateView    # game.py:39: the reference nests the class in Game

    def __init__(self, **config):
        self.logger = config.pop('logger', None)       # accepted and ignored: no result depends on it (game.py:250)
        self._v = VecGame(1, **config)
        self.num_players = self._v.num_players
        self.start_credits = self._v.start_credits
        self.big_blind, self.small_blind = self._v.big_blind, self._v.small_blind

    def close(self):
        self._v.close()

    # ---- copy.deepcopy / pickle (a reference Game is a plain Python object: both work on it): through the table's snapshot
    def __deepcopy__(self, memo):
        """A standalone Game on a handle of its own, holding a copy of this table: it continues bit-identically under the same
        actions (same seed and table id), and stepping it leaves this game untouched.  Also for `env.game`."""
        return _game_of(copy.deepcopy(self._v, memo))

    def __reduce__(self):
        return (_game_of, (self._v,))

    # ---- attributes of game.py:251-264 (read fresh from the device on every access)
    credits = property(lambda self: self._v.credits[0])
    bets = property(lambda self: self._v.bets[0])
    pending_bets = property(lambda self: self._v.pending_bets[0])
    payoffs = property(lambda self: self._v.payoffs[0])
    player_states = property(lambda self: self._v.player_states[0])
    minimum_raise_value = property(lambda self: float(self._v.minimum_raise_value[0]))
    active_player = property(lambda self: int(self._v.active_player[0]))
    turn = property(lambda self: int(self._v.turn[0]))
    hand = property(lambda self: int(self._v.hand[0]))
    dealer_idx = property(lambda self: int(self._v.dealer_idx[0]))
    big_blind_idx = property(lambda self: int(self._v.big_blind_idx[0]))
    small_blind_idx = property(lambda self: int(self._v.small_blind_idx[0]))

    @property
    def deck(self):
        """deck[0 : 5 + 2N] as Card objects -- the part of the deck the game ever reads (game.py:278, :385-395)."""
        return [Card(int(v)) for v in self._v.deck[0]]

    # ---- properties of game.py:266-332
    @property
    def community_cards(self):
        return [] if self.turn == 0 else self.deck[:self.turn + 2]                 # :266-278

    pot = property(lambda self: float(self._v.pot[0]))                            # :281-284
    high_bet = property(lambda self: float(self._v.high_bet[0]))                  # :287-290
    high_bidders = property(lambda self: self.bets == self.high_bet)              # :293-296
    pending_credits = property(lambda self: self.credits - self.pending_bets)     # :299-302
    blind_idx = property(lambda self: [self.big_blind_idx, self.small_blind_idx])  # :305-308
    blind_value = property(lambda self: [self.big_blind, self.small_blind])       # :311-314
    game_over = property(lambda self: bool(self._v.game_over[0]))                 # :317-320
    active_state = property(lambda self: self._v.state_view(0))                   # :323-332

    def get_first_playing(self, idx):                                             # :334-337
        alive = np.roll(self.player_states, -idx) != PlayerState.BROKEN
        return int((idx + np.argmax(alive)) % self.num_players)

    def get_valid_actions(self, player=None):                                     # :339-383
        onehot, gen = self._v.get_valid_actions(player)
        return onehot[0], (int(i) for i in next(gen))

    def get_cards_of(self, player):                                               # :385-389
        i = 5 + player * 2
        return self.deck[i:i + 2]

    def get_hand_for(self, player):                                               # :391-395
        i = 5 + player * 2
        d = self.deck
        return d[:5] + d[i:i + 2]

    def reset(self, **config):                                                    # :397-412
        self._v.reset(**config)

    def equity(self):
        """Showdown equity of the table as it stands (VecGame.equity): a judger.Equity with [N] arrays.  Not in the reference."""
        r = self._v.equity()[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def equity_ev(self):
        """Showdown EV in chips of the table as it stands (VecGame.equity_ev): a judger.ShowdownEV with [N] arrays.  Not in the reference."""
        r = self._v.equity_ev()[0]
        if r.status:
            from .judger import ev_status_text
            raise ValueError('the table cannot be evaluated: ' + ev_status_text(r.status))
        return r

    def equity_sampled(self, observer=None, samples=1024, nonce=0):
        """Sampled showdown equity of the table as `observer` sees it (VecGame.equity_sampled; None = the active seat): a
        judger.SampledEquity with [N] arrays.  Not in the reference."""
        from ._lib import OBSERVER_ACTIVE
        r = self._v.equity_sampled(observer=OBSERVER_ACTIVE if observer is None else observer, samples=samples, nonce=nonce)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def equity_ranged(self, observer=None, ranges=None, range_of=None, samples=1024, nonce=0):
        """Sampled showdown equity of the table as `observer` sees it (None = the active seat) with every other live seat's holding drawn
        from a weighted range (VecGame.equity_ranged): a judger.RangedEquity with [N] arrays.  Not in the reference."""
        from ._lib import OBSERVER_ACTIVE
        r = self._v.equity_ranged(observer=OBSERVER_ACTIVE if observer is None else observer, ranges=ranges, range_of=range_of, samples=samples,
                                  nonce=nonce)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def ev_ranged(self, observer=None, ranges=None, range_of=None, samples=1024, nonce=0):
        """Showdown EV in chips of the table as `observer` sees it (None = the active seat) with every other live seat's holding drawn from
        a weighted range (VecGame.ev_ranged): a judger.RangedEV with [N] / [N, N] arrays.  Not in the reference."""
        from ._lib import OBSERVER_ACTIVE
        r = self._v.ev_ranged(observer=OBSERVER_ACTIVE if observer is None else observer, ranges=ranges, range_of=range_of, samples=samples,
                              nonce=nonce)[0]
        if r.status:
            from .judger import ranged_ev_status_text
            raise ValueError('the table cannot be evaluated: ' + ranged_ev_status_text(r.status))
        return r

    def equity_range(self, observer=None, weights=None):
        """Exact hand strength of `observer` (None = the active seat) against one hidden hand, post-flop (VecGame.equity_range): a
        judger.RangeEquity with [1326] arrays and the scalar `strength`.  Not in the reference."""
        from ._lib import OBSERVER_ACTIVE
        r = self._v.equity_range(observer=OBSERVER_ACTIVE if observer is None else observer, weights=weights, per_holding=True)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def equity_preflop(self, observer=None, weights=None):
        """Exact starting-hand strength of `observer` (None = the active seat) against one hidden hand, the board not read
        (VecGame.equity_preflop): a judger.RangeEquity with [1326] arrays and the scalar `strength`.  Not in the reference."""
        from ._lib import OBSERVER_ACTIVE
        r = self._v.equity_preflop(observer=OBSERVER_ACTIVE if observer is None else observer, weights=weights, per_holding=True)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def equity_rvr(self, weights=None):
        """Range against range on the public board, post-flop (VecGame.equity_rvr): a judger.RangeVsRange with [1326] arrays -- every
        holding the hero can have against the opponent's range `weights`.  Not in the reference."""
        r = self._v.equity_rvr(weights=weights)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def equity_hist(self, weights=None, bins=10):
        """Strength histograms on the public board, post-flop (VecGame.equity_hist): a judger.StrengthHistogram with [1326, bins] hist --
        the distribution of every holding's river strength against the opponent's range `weights`.  Not in the reference."""
        r = self._v.equity_hist(weights=weights, bins=bins)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def equity_hist_hero(self, observer=None, weights=None, bins=10, centroids=None):
        """The strength histogram of `observer`'s hand (None = the active seat), post-flop (VecGame.equity_hist_hero): a
        judger.HeroHistogram with a [bins] hist and, with centroids, its bucket `label` / `dist`.  Not in the reference."""
        from ._lib import OBSERVER_ACTIVE
        r = self._v.equity_hist_hero(observer=OBSERVER_ACTIVE if observer is None else observer, weights=weights, bins=bins, centroids=centroids)[0]
        if r.status:
            from .judger import equity_status_text
            raise ValueError('the table cannot be evaluated: ' + equity_status_text(r.status))
        return r

    def bucket(self, centroids, observer=None, weights=None):
        """The bucket of `observer`'s hand (None = the active seat) under `centroids` uint16 [k, bins], post-flop: an int.  Not in the
        reference."""
        return int(self.equity_hist_hero(observer=observer, weights=weights, bins=int(np.shape(centroids)[-1]), centroids=centroids).label)

    def step(self, action):                                                       # :621-700
        """Returns (game_over, hand_over, turn_over); raises the reference's ValueError / NotImplementedError /
        AssertionError in the reference's situations."""
        if not isinstance(action, (int, np.integer)) or isinstance(action, bool):
            raise NotImplementedError                                             # :646, :700
        over, hand, turn = self._v.step(np.array([action], np.int64))
        return bool(over[0]), bool(hand[0]), bool(turn[0])


def _game_of(vec_game):
    """A Game over an existing one-table VecGame (copy.deepcopy and unpickling)."""
    g = Game.__new__(Game)
    g.logger = None
    g._v = vec_game
    g.num_players = vec_game.num_players
    g.start_credits = vec_game.start_credits
    g.big_blind, g.small_blind = vec_game.big_blind, vec_game.small_blind
    return g


class PokerGameEnv:
    """`pokerl.envs.PokerGameEnv(agents, **game_config)` (envs/game_env.py:6-53) for one table: reset() -> StateView,
    step(action) -> (StateView, reward, done, hand).  agents: in-kernel agents and / or callables, see pokerl_amd.agents."""

    def __init__(self, agents=None, **game_config):
        self._e = VecPokerGameEnv(agents, num_tables=1, **game_config)
        self.agents = self._e.agents                       # [None, *agents], game_env.py:17
        self.player_agent = 0
        self.game = _GameView(self._e.game)

    def reset(self):
        return StateView(self._e.reset()[0], self._e.game.num_players)           # game_env.py:20-29

    def step(self, action):
        if not isinstance(action, (int, np.integer)) or isinstance(action, bool):
            raise NotImplementedError
        obs, reward, done, hand = self._e.step(np.array([action], np.int64))      # game_env.py:31-53
        return StateView(obs[0], self._e.game.num_players), float(reward[0]), bool(done[0]), bool(hand[0])

    def close(self):
        self._e.close()


class _GameView(Game):
    """`env.game` of the single-table env: the Game view over the env's own table."""

    def __init__(self, vec_game):                 # no second handle: shares the env's
        self.logger = None
        self._v = vec_game
        self.num_players = vec_game.num_players
        self.start_credits = vec_game.start_credits
        self.big_blind, self.small_blind = vec_game.big_blind, vec_game.small_blind

    def close(self):
        pass
