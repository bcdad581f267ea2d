"""ctypes binding of libpokerl_hip.so (C ABI: include/pokerl_hip.h).  There is NO CPU fallback: if the HIP library is
missing or no MI355X is visible, calls raise."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("POKERL_HIP_LIB") or os.path.join(HERE, "libpokerl_hip.so")  # override: diagnostic builds

PK_OK, PK_E_INVALID_ARG, PK_E_NO_DEVICE, PK_E_HIP, PK_E_OOM, PK_E_TABLE, PK_E_BUSY = 0, -1, -2, -3, -4, -5, -6
TERR_INVALID_ACTION, TERR_NO_WINNER, TERR_HAND_CAP, TERR_ENV_CAP = 1, 2, 4, 8
FLAG_GAME_OVER, FLAG_HAND_OVER, FLAG_TURN_OVER = 1, 2, 4
F_CREDITS, F_BETS, F_PENDING_BETS, F_PAYOFFS = 0, 1, 2, 3
I_ACTIVE_PLAYER, I_TURN, I_DEALER_IDX, I_SMALL_BLIND_IDX, I_BIG_BLIND_IDX, I_HAND = range(6)
TF_POT, TF_HIGH_BET, TF_MIN_RAISE = 0, 1, 2
ACTION_SKIP = -2   # pk_env_step_multi_d: leave an idle table alone (PK_ACTION_SKIP)
POLICY_EXTERNAL = 15
ABI_VERSION = 6
NUM_COUNTERS = 4
MIN_PLAYERS, MAX_PLAYERS = 2, 16
EQ_SHARE_UNIT = 720720   # lcm(1 .. 16): a board's pot share of one of nw winners is EQ_SHARE_UNIT / nw (pk_equity)
EQ_BAD_CARD, EQ_DUP_CARD, EQ_NO_LIVE, EQ_BAD_NBOARD, EQ_IN_FLIGHT, EQ_BAD_TABLE = 1, 2, 4, 8, 16, 32   # PK_EQ_* status bits
OBSERVER_NONE, OBSERVER_ACTIVE = -1, -2   # pk_clone_tables_d: an exact copy / redeal from each source table's active player
EQ_PREFLOP, EQ_SMALL_POOL = 64, 128   # ... of pk_equity_range: nb < 3 / fewer pool cards than the board to come plus one holding
EQ_BAD_BET = 64   # ... of pk_equity_ev: a bet that is negative, NaN or infinite (the value of EQ_PREFLOP, which no EV call reports)
EQ_BAD_ITER = 16   # PK_EQ_BAD_ITER, of the solvers' resuming calls: t0 + iters > 4096 (the value of EQ_IN_FLIGHT, which no spot form reports)
EQ_BAD_TREE = 32   # PK_EQ_BAD_TREE, of the solvers' tree-per-spot calls: tree_of >= ntrees (the value of EQ_BAD_TABLE, which no spot form reports)
RS_MAX_TREES = 65536   # PK_RS_MAX_TREES: trees of one pk_solve_river_trees / pk_solve_turn_trees call at most
EQ_HIST_MAX_BINS = 32   # PK_EQ_HIST_MAX_BINS: the most bins of a strength histogram
EQ_HOLDINGS = 1326   # PK_EQ_HOLDINGS: unordered pairs of the 52 cards, h = b (b - 1) / 2 + a over canonical indices a < b
CL_MAX_K, CL_NONE, CL_MAX_ITERS = 4096, 0xFFFF, 1024   # PK_CL_MAX_K, PK_CL_NONE; iterations of one pk_hist_cluster call at most
PREFLOP_BOARDS, PREFLOP_ALL_BOARDS = 1712304, 2598960   # PK_PREFLOP_BOARDS = C(48, 5): boards of one pre-flop matchup; PK_PREFLOP_ALL_BOARDS = C(52, 5)
EQS_SAMPLES_MAX = 1 << 24   # pk_equity_sampled: samples per call and spot at most
EQW_MAX_RANGES, EQW_UNIFORM = 16, 0xFFFF   # pk_equity_ranged: rows of a call's weight table at most / the range_of entry "every weight 1"

# every symbol include/pokerl_hip.h declares (tests check the library exports each one)
SYMBOLS = ["pk_abi_version", "pk_device_count", "pk_last_error", "pk_create", "pk_destroy", "pk_num_tables",
           "pk_num_players", "pk_reset", "pk_step", "pk_step_d", "pk_get_valid_actions", "pk_get_f64",
           "pk_get_min_raise", "pk_get_player_states", "pk_get_i32", "pk_get_cards", "pk_get_hand_ranks",
           "pk_eval_hands", "pk_compare_rankings", "pk_eval7_prefix", "pk_pick_actions", "pk_rollout",
           "pk_env_reset", "pk_env_step", "pk_get_obs", "pk_sync", "pk_time_rollout", "pk_get_obs_d",
           "pk_get_valid_actions_d", "pk_env_step_d", "pk_env_reset_d", "pk_eval7_d", "pk_make_hands_d", "pk_time_eval7_d",
           "pk_get_serials", "pk_set_serials", "pk_get_table_f64", "pk_get_game_over", "pk_eval_hands_d",
           "pk_pick_actions_d", "pk_flush", "pk_get_owed", "pk_env_step_fused_d", "pk_env_step_async_d", "pk_set_tuning", "pk_get_stream", "pk_set_stream", "pk_wait_event",
           "pk_record_event", "pk_use_own_stream", "pk_set_coalesce", "pk_get_launch_stats", "pk_env_step_multi_d", "pk_env_end_multi_d", "pk_get_f64_d", "pk_set_env_batches", "pk_env_last_range",
           "pk_get_obs_packed", "pk_get_obs_packed_d", "pk_set_env_obs_packed", "pk_host_alloc", "pk_host_free", "pk_check_actions",
           "pk_env_step_begin", "pk_env_step_end", "pk_reset_d", "pk_step_auto_d", "pk_stream_pool_drain", "pk_step_async_d", "pk_set_step_obs", "pk_build_info",
           "pk_snapshot_bytes", "pk_save_tables_d", "pk_load_tables_d", "pk_save_tables", "pk_load_tables", "pk_clone_tables_d",
           "pk_equity_d", "pk_equity", "pk_table_equity_d", "pk_table_equity",
           "pk_equity_sampled_d", "pk_equity_sampled", "pk_table_equity_sampled_d", "pk_table_equity_sampled", "pk_get_wave_shape",
           "pk_equity_range_d", "pk_equity_range", "pk_table_equity_range_d", "pk_table_equity_range",
           "pk_equity_rvr_d", "pk_equity_rvr", "pk_table_equity_rvr_d", "pk_table_equity_rvr",
           "pk_equity_hist_d", "pk_equity_hist", "pk_table_equity_hist_d", "pk_table_equity_hist",
           "pk_equity_hist_hero_d", "pk_equity_hist_hero", "pk_table_equity_hist_hero_d", "pk_table_equity_hist_hero",
           "pk_equity_ranged_d", "pk_equity_ranged", "pk_table_equity_ranged_d", "pk_table_equity_ranged",
           "pk_equity_ev_d", "pk_equity_ev", "pk_table_equity_ev_d", "pk_table_equity_ev",
           "pk_ev_ranged_d", "pk_ev_ranged", "pk_table_ev_ranged_d", "pk_table_ev_ranged",
           "pk_hist_cluster_seed_d", "pk_hist_cluster_assign_d", "pk_hist_cluster_d", "pk_hist_cluster_seed", "pk_hist_cluster_assign", "pk_hist_cluster",
           "pk_preflop_count_d", "pk_preflop_count", "pk_preflop_matchups_d", "pk_preflop_matchups",
           "pk_equity_preflop_d", "pk_equity_preflop", "pk_table_equity_preflop_d", "pk_table_equity_preflop",
           "pk_equity_rvr_preflop_d", "pk_equity_rvr_preflop",
           "pk_solve_river_d", "pk_solve_river", "pk_solve_turn_d", "pk_solve_turn", "pk_turn_grid",
           "pk_solve_river_trees_d", "pk_solve_river_trees", "pk_solve_turn_trees_d", "pk_solve_turn_trees", "pk_rs_trees_rows", "pk_ts_trees_rows",
           "pk_solve_river_locked_d", "pk_solve_river_locked", "pk_solve_turn_locked_d", "pk_solve_turn_locked",
           "pk_solve_river_resolve_d", "pk_solve_river_resolve", "pk_solve_turn_resolve_d", "pk_solve_turn_resolve",
           "pk_solve_river_resume_d", "pk_solve_river_resume", "pk_solve_turn_resume_d", "pk_solve_turn_resume",
           "pk_solve_preflop_d", "pk_solve_preflop"]


class PokerlHipError(RuntimeError):
    code = None     # the library's PK_E_* return code where check() raised it


_lib = None
_vp = C.c_void_p


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PokerlHipError(
            "%s not found: build it with `python -m pokerl_amd.build` (hipcc, gfx950). "
            "pokerl_amd has no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.pk_abi_version.restype = C.c_int
    L.pk_device_count.restype = C.c_int
    L.pk_last_error.restype = C.c_char_p
    L.pk_last_error.argtypes = [_vp]
    L.pk_build_info.restype = C.c_char_p
    L.pk_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _vp, C.c_double, C.c_double, C.c_double,
                            C.c_int, C.c_uint64, C.c_uint32]
    L.pk_destroy.argtypes = [_vp]
    L.pk_num_tables.argtypes = [_vp]
    L.pk_num_players.argtypes = [_vp]
    L.pk_get_wave_shape.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_reset.argtypes = [_vp, _vp, C.c_int]
    L.pk_reset_d.argtypes = [_vp, _vp, C.c_int, C.c_int]
    L.pk_step.argtypes = [_vp, _vp, _vp, _vp]
    L.pk_step_d.argtypes = [_vp, _vp, _vp, _vp]
    L.pk_step_auto_d.argtypes = [_vp, _vp, _vp, _vp]
    L.pk_step_async_d.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]
    L.pk_get_valid_actions.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_f64.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_f64_d.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_min_raise.argtypes = [_vp, _vp]
    L.pk_get_player_states.argtypes = [_vp, _vp]
    L.pk_get_i32.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_cards.argtypes = [_vp, _vp]
    L.pk_get_hand_ranks.argtypes = [_vp, _vp, _vp]
    L.pk_eval_hands.argtypes = [C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp]
    L.pk_compare_rankings.argtypes = [C.c_int, _vp, _vp, C.c_int, C.c_size_t, _vp]
    L.pk_eval7_prefix.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(C.c_size_t)]
    L.pk_pick_actions.argtypes = [_vp, C.c_int, _vp]
    L.pk_rollout.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
    L.pk_env_reset.argtypes = [_vp, _vp, C.c_int]
    L.pk_env_step.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp]
    L.pk_get_obs.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_obs_d.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_valid_actions_d.argtypes = [_vp, C.c_int, _vp]
    L.pk_env_step_d.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp]
    L.pk_env_reset_d.argtypes = [_vp, _vp, C.c_int]
    L.pk_eval7_d.argtypes = [C.c_int, _vp, C.c_size_t, _vp, C.c_int]
    L.pk_make_hands_d.argtypes = [C.c_int, C.c_uint64, C.c_size_t, _vp]
    L.pk_time_eval7_d.argtypes = [C.c_int, _vp, C.c_size_t, _vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.pk_sync.argtypes = [_vp]
    L.pk_get_serials.argtypes = [_vp, _vp, _vp]
    L.pk_set_serials.argtypes = [_vp, _vp, _vp]
    L.pk_get_table_f64.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_game_over.argtypes = [_vp, _vp]
    L.pk_eval_hands_d.argtypes = [C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp]
    L.pk_pick_actions_d.argtypes = [_vp, C.c_int, _vp]
    L.pk_flush.argtypes = [_vp]
    L.pk_env_step_fused_d.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]
    L.pk_env_step_async_d.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    L.pk_env_step_multi_d.argtypes = [_vp, _vp, _vp, C.c_uint64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.pk_env_end_multi_d.argtypes = [_vp]
    L.pk_set_env_batches.argtypes = [_vp, C.c_int]
    L.pk_env_last_range.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_get_obs_packed.argtypes = [_vp, C.c_int, _vp]
    L.pk_get_obs_packed_d.argtypes = [_vp, C.c_int, _vp]
    L.pk_set_env_obs_packed.argtypes = [_vp, _vp]
    L.pk_set_step_obs.argtypes = [_vp, _vp, _vp]
    L.pk_host_alloc.argtypes = [C.POINTER(_vp), C.c_size_t]
    L.pk_host_free.argtypes = [_vp]
    L.pk_check_actions.argtypes = [_vp, _vp, C.POINTER(C.c_int32)]
    L.pk_env_step_begin.argtypes = [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
    L.pk_env_step_end.argtypes = [_vp]
    L.pk_stream_pool_drain.argtypes = [C.c_int]
    L.pk_get_owed.argtypes = [_vp, _vp]
    L.pk_set_tuning.argtypes = [_vp, C.c_int, C.c_int]
    L.pk_get_stream.argtypes = [_vp, C.POINTER(_vp)]
    L.pk_set_stream.argtypes = [_vp, _vp]
    L.pk_use_own_stream.argtypes = [_vp]
    L.pk_set_coalesce.argtypes = [_vp, C.c_int]
    L.pk_get_launch_stats.argtypes = [_vp, _vp, C.c_int]
    L.pk_wait_event.argtypes = [_vp, _vp]
    L.pk_record_event.argtypes = [_vp, _vp]
    L.pk_time_rollout.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _vp]
    L.pk_snapshot_bytes.argtypes = [C.c_int, C.c_size_t]
    for name in ("pk_save_tables_d", "pk_load_tables_d", "pk_save_tables", "pk_load_tables"):
        getattr(L, name).argtypes = [_vp, _vp, C.c_size_t, _vp]
    L.pk_clone_tables_d.argtypes = [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_uint64]
    L.pk_equity_d.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 10
    L.pk_equity.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 9
    L.pk_table_equity_d.argtypes = [_vp, _vp, C.c_size_t] + [_vp] * 5
    L.pk_table_equity.argtypes = [_vp, _vp, C.c_size_t] + [_vp] * 5
    L.pk_equity_ev_d.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 12
    L.pk_equity_ev.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 11
    L.pk_table_equity_ev_d.argtypes = [_vp, _vp, C.c_size_t] + [_vp] * 6
    L.pk_table_equity_ev.argtypes = [_vp, _vp, C.c_size_t] + [_vp] * 6
    L.pk_equity_sampled_d.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_uint32, C.c_uint64, C.c_uint32] + [_vp] * 6
    L.pk_equity_sampled.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_uint32, C.c_uint64, C.c_uint32] + [_vp] * 5
    L.pk_table_equity_sampled_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32] + [_vp] * 5
    L.pk_table_equity_sampled.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32] + [_vp] * 5
    L.pk_equity_ranged_d.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_uint32, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp] + [_vp] * 6
    L.pk_equity_ranged.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_uint32, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp] + [_vp] * 5
    L.pk_table_equity_ranged_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, C.c_int] + [_vp] * 5
    L.pk_table_equity_ranged.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, C.c_int] + [_vp] * 5
    L.pk_ev_ranged_d.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 6 + [C.c_uint32, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp] + [_vp] * 7
    L.pk_ev_ranged.argtypes = [C.c_int, C.c_int, C.c_size_t] + [_vp] * 6 + [C.c_uint32, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp] + [_vp] * 6
    L.pk_table_ev_ranged_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, C.c_int] + [_vp] * 6
    L.pk_table_ev_ranged.argtypes = [_vp, _vp, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, C.c_int] + [_vp] * 6
    L.pk_equity_range_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_int] + [_vp] * 6
    L.pk_equity_range.argtypes = [C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_int] + [_vp] * 5
    L.pk_table_equity_range_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int] + [_vp] * 5
    L.pk_table_equity_range.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int] + [_vp] * 5
    L.pk_equity_rvr_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 4 + [C.c_int] + [_vp] * 6
    L.pk_equity_rvr.argtypes = [C.c_int, C.c_size_t] + [_vp] * 4 + [C.c_int] + [_vp] * 5
    L.pk_table_equity_rvr_d.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_int] + [_vp] * 5
    L.pk_table_equity_rvr.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_int] + [_vp] * 5
    L.pk_equity_hist_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 4 + [C.c_int, C.c_int] + [_vp] * 5
    L.pk_equity_hist.argtypes = [C.c_int, C.c_size_t] + [_vp] * 4 + [C.c_int, C.c_int] + [_vp] * 4
    L.pk_table_equity_hist_d.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_int, C.c_int] + [_vp] * 4
    L.pk_table_equity_hist.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_int, C.c_int] + [_vp] * 4
    L.pk_equity_hist_hero_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_int, C.c_int] + [_vp] * 4 + [C.c_int] + [_vp] * 4
    L.pk_equity_hist_hero.argtypes = [C.c_int, C.c_size_t] + [_vp] * 5 + [C.c_int, C.c_int] + [_vp] * 4 + [C.c_int] + [_vp] * 3
    L.pk_table_equity_hist_hero_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 4 + [C.c_int] + [_vp] * 3
    L.pk_table_equity_hist_hero.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 4 + [C.c_int] + [_vp] * 3
    L.pk_hist_cluster_seed_d.argtypes = [C.c_int, C.c_size_t, C.c_int, _vp, C.c_int, C.c_uint64, C.c_uint32, _vp, _vp]
    L.pk_hist_cluster_seed.argtypes = [C.c_int, C.c_size_t, C.c_int, _vp, C.c_int, C.c_uint64, C.c_uint32, _vp]
    L.pk_hist_cluster_assign_d.argtypes = [C.c_int, C.c_size_t, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]
    L.pk_hist_cluster_assign.argtypes = [C.c_int, C.c_size_t, C.c_int, _vp, C.c_int, _vp, _vp, _vp]
    L.pk_hist_cluster_d.argtypes = [C.c_int, C.c_size_t, C.c_int, _vp, C.c_int, _vp, C.c_int] + [_vp] * 5
    L.pk_hist_cluster.argtypes = [C.c_int, C.c_size_t, C.c_int, _vp, C.c_int, _vp, C.c_int] + [_vp] * 4
    L.pk_preflop_count_d.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, _vp, _vp, _vp]
    L.pk_preflop_count.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, _vp, _vp]
    L.pk_preflop_matchups_d.argtypes = [C.c_int, _vp, _vp, _vp]
    L.pk_preflop_matchups.argtypes = [C.c_int, _vp, _vp]
    L.pk_equity_preflop_d.argtypes = [C.c_int, C.c_size_t, _vp, _vp, C.c_int] + [_vp] * 6
    L.pk_equity_preflop.argtypes = [C.c_int, C.c_size_t, _vp, _vp, C.c_int] + [_vp] * 5
    L.pk_table_equity_preflop_d.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int] + [_vp] * 5
    L.pk_table_equity_preflop.argtypes = [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int] + [_vp] * 5
    L.pk_equity_rvr_preflop_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 5
    L.pk_equity_rvr_preflop.argtypes = [C.c_int, C.c_size_t] + [_vp] * 4
    L.pk_solve_river_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 3 + [C.c_uint32, C.c_uint32] + [_vp] * 5
    L.pk_solve_river.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 3 + [C.c_uint32, C.c_uint32] + [_vp] * 4
    L.pk_solve_turn_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 3 + [C.c_uint32, C.c_uint32] + [_vp] * 6
    L.pk_solve_turn.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 3 + [C.c_uint32, C.c_uint32] + [_vp] * 5
    L.pk_turn_grid.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32]
    L.pk_solve_river_trees_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 5
    L.pk_solve_river_trees.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 4
    L.pk_solve_turn_trees_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 6
    L.pk_solve_turn_trees.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 5
    L.pk_solve_river_locked_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 7
    L.pk_solve_river_locked.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 6
    L.pk_solve_turn_locked_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 10
    L.pk_solve_turn_locked.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 9
    L.pk_solve_river_resolve_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 13
    L.pk_solve_river_resolve.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 12
    L.pk_solve_turn_resolve_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 16
    L.pk_solve_turn_resolve.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 15
    L.pk_solve_river_resume_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 16
    L.pk_solve_river_resume.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 15
    L.pk_solve_turn_resume_d.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 21
    L.pk_solve_turn_resume.argtypes = [C.c_int, C.c_size_t] + [_vp] * 3 + [C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 20
    L.pk_rs_trees_rows.argtypes = [C.c_uint32] + [_vp] * 3
    L.pk_solve_preflop_d.argtypes = [C.c_int, C.c_size_t, _vp, C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 5
    L.pk_solve_preflop.argtypes = [C.c_int, C.c_size_t, _vp, C.c_uint32] + [_vp] * 6 + [C.c_uint32] + [_vp] * 4
    L.pk_ts_trees_rows.argtypes = [C.c_uint32] + [_vp] * 5
    for name in SYMBOLS:
        if name not in ("pk_last_error", "pk_build_info", "pk_snapshot_bytes"):
            getattr(L, name).restype = C.c_int
    L.pk_snapshot_bytes.restype = C.c_size_t
    if L.pk_abi_version() != ABI_VERSION:
        raise PokerlHipError("libpokerl_hip.so ABI version mismatch")
    _lib = L
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def check(rc, handle=None, allow_table_errors=False):
    if rc == PK_OK or (allow_table_errors and rc == PK_E_TABLE):
        return rc
    msg = lib().pk_last_error(handle)
    err = PokerlHipError("libpokerl_hip: error %d: %s" % (rc, msg.decode() if msg else "?"))
    err.code = rc
    raise err


def source_hash():
    """The hash of the kernel sources the loaded library was built from (pk_build_info; pokerl_amd/build.py source_hash)."""
    info = lib().pk_build_info().decode()
    return info.split("src=")[-1]


def device_count():
    return lib().pk_device_count()
