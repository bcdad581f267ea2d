"""pokerl_amd -- MI355X-native vectorised No-Limit Hold'em hot path (drop-in for sneppy/pokerl's
Game.step/reset, judger and PokerGameEnv.step over thousands of tables).  HIP kernels behind a ctypes C ABI."""
from .enums import CardRank, CardSuit, HandRanking, PlayerState, PokerMoves, Policy
from .game import VecGame, snapshot_nbytes
from .envs import VecPokerGameEnv, VecPokerGameEnvPool
from .agents import AllInAgent, CallAgent, PokerAgent, RandomAgent
from .judger import (Equity, SampledEquity, compare_hands, compare_rankings, eval_hand, eval_hands, sampled_equity, sampled_equity_batch,
                     showdown_equity, showdown_equity_batch)
from .judger import HOLDINGS, RangeEquity, holding_index, range_equity, range_equity_batch, range_equity_d
from .judger import RangeVsRange, range_vs_range, range_vs_range_batch, range_vs_range_d
from .judger import (PreflopMatchups, preflop_counts, preflop_counts_d, preflop_equity, preflop_equity_batch, preflop_equity_d, preflop_matchups,
                     preflop_matchups_d, preflop_range_vs_range, preflop_range_vs_range_batch, preflop_range_vs_range_d)
from .judger import StrengthHistogram, histogram_emd, strength_histogram, strength_histogram_batch, strength_histogram_d
from .judger import HeroHistogram, hero_histogram, hero_histogram_batch, hero_histogram_d
from .judger import (HistogramClusters, assign_histograms, assign_histograms_d, cluster_histograms, cluster_histograms_d,
                     seed_histogram_centroids, seed_histogram_centroids_d)
from .judger import RangedEquity, ranged_equity, ranged_equity_batch, ranged_equity_d
from .judger import ShowdownEV, showdown_ev, showdown_ev_batch, showdown_ev_d
from .judger import RangedEV, ranged_ev, ranged_ev_batch, ranged_ev_d
from .solver import (RiverSolution, RiverTree, TurnSolution, TurnTree, river_tree, river_trees, solve_river, solve_river_batch, solve_river_d,
                     solve_turn, solve_turn_batch, solve_turn_d, turn_grid, turn_tree, turn_trees, evaluate_river, evaluate_river_batch,
                     evaluate_turn, evaluate_turn_batch, gadget_tree, resolve_river, KIND_GIVEN,
                     SolverState, solver_state_bytes, solve_river_until, solve_river_until_batch, solve_turn_until, solve_turn_until_batch)
from .solver import (PreflopSolution, holding_class, preflop_tree, preflop_trees, push_fold_tree, solve_preflop, solve_preflop_batch,
                     solve_preflop_d)
from .sharding import gather_f64, shard_tables
from .single import Game, PokerGameEnv
from .state_view import Card, StateView, packed_dtype, unpack_obs
from .hipmem import pinned_empty
from ._lib import OBSERVER_ACTIVE, OBSERVER_NONE, PokerlHipError, device_count

__all__ = ['Game', 'PokerGameEnv', 'VecGame', 'VecPokerGameEnv', 'VecPokerGameEnvPool', 'eval_hand', 'eval_hands', 'compare_rankings', 'compare_hands',
           'shard_tables', 'gather_f64', 'Card', 'StateView', 'HandRanking', 'PokerMoves', 'PlayerState', 'CardRank', 'CardSuit', 'Policy',
           'PokerlHipError', 'device_count', 'packed_dtype', 'unpack_obs', 'pinned_empty', 'PokerAgent', 'RandomAgent', 'AllInAgent', 'CallAgent',
           'snapshot_nbytes', 'OBSERVER_NONE', 'OBSERVER_ACTIVE', 'Equity', 'showdown_equity', 'showdown_equity_batch',
           'SampledEquity', 'sampled_equity', 'sampled_equity_batch',
           'HOLDINGS', 'RangeEquity', 'holding_index', 'range_equity', 'range_equity_batch', 'range_equity_d',
           'RangeVsRange', 'range_vs_range', 'range_vs_range_batch', 'range_vs_range_d',
           'StrengthHistogram', 'histogram_emd', 'strength_histogram', 'strength_histogram_batch', 'strength_histogram_d',
           'HeroHistogram', 'hero_histogram', 'hero_histogram_batch', 'hero_histogram_d',
           'HistogramClusters', 'cluster_histograms', 'assign_histograms', 'seed_histogram_centroids', 'cluster_histograms_d',
           'assign_histograms_d', 'seed_histogram_centroids_d',
           'RangedEquity', 'ranged_equity', 'ranged_equity_batch', 'ranged_equity_d',
           'ShowdownEV', 'showdown_ev', 'showdown_ev_batch', 'showdown_ev_d',
           'RangedEV', 'ranged_ev', 'ranged_ev_batch', 'ranged_ev_d',
           'PreflopMatchups', 'preflop_matchups', 'preflop_matchups_d', 'preflop_counts', 'preflop_counts_d',
           'preflop_equity', 'preflop_equity_batch', 'preflop_equity_d',
           'preflop_range_vs_range', 'preflop_range_vs_range_batch', 'preflop_range_vs_range_d',
           'RiverTree', 'RiverSolution', 'river_tree', 'solve_river', 'solve_river_batch', 'solve_river_d',
           'TurnTree', 'TurnSolution', 'turn_tree', 'turn_grid', 'solve_turn', 'solve_turn_batch', 'solve_turn_d', 'river_trees', 'turn_trees',
           'evaluate_river', 'evaluate_river_batch', 'evaluate_turn', 'evaluate_turn_batch', 'gadget_tree', 'resolve_river', 'KIND_GIVEN',
           'SolverState', 'solver_state_bytes', 'solve_river_until', 'solve_river_until_batch', 'solve_turn_until', 'solve_turn_until_batch',
           'PreflopSolution', 'holding_class', 'push_fold_tree', 'preflop_tree', 'preflop_trees', 'solve_preflop', 'solve_preflop_batch', 'solve_preflop_d']
