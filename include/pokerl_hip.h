/* pokerl_hip.h -- C ABI of libpokerl_hip.so: the MI355X (gfx950) vectorised No-Limit Hold'em hot path.
 *
 * The reference (sneppy/pokerl) is pure Python and has no plugin/FFI layer; its boundary for this
 * path is the Python object API.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference root).  T = num_tables, N = num_players.
 *
 * Conventions
 *   - every pointer is a HOST pointer owned by the caller unless the name ends in `_d` (device pointer,
 *     caller-owned, on the handle's device);  the library owns all table state behind the opaque handle;
 *   - arrays are table-major: [T][N] for per-seat data, [T] for per-table data;
 *   - return value: PK_OK (0) or a negative PK_E_* code; pk_last_error() gives text; the library never aborts;
 *   - per-table error bits (PK_TERR_*) are reported separately from the call's return code;
 *   - a handle is bound to one device and one HIP stream and is not thread-safe; different handles may be
 *     driven from different threads/processes (one process per GPU is the intended deployment);
 *   - RNG is counter-based per handle: Philox4x32-10 keyed by `seed`, indexed by the GLOBAL table id
 *     (table_id_base + t) and 64-bit per-table serials, so results do not depend on how tables are sharded over
 *     GPUs and a table's streams never repeat;
 *   - `_d` entry points are asynchronous on the handle's stream and take buffers that must be COMPLETE in stream order:
 *     either make the handle run on your stream (pk_set_stream) or order the two streams with events
 *     (pk_wait_event before the call, pk_record_event after it).  pk_sync() waits for everything requested so far.
 *
 * All money arithmetic is IEEE binary64 in the reference's operation order (no FMA contraction), so
 * valid_actions / payoffs / credits / flags / hand ranks are bit-identical to the CPU reference.  Money must be FINITE: the
 * library is built with -fno-honor-nans (np.max / np.minimum as v_max_f64 / v_min_f64), and pk_create refuses inf / NaN stacks
 * and blinds (PK_E_INVALID_ARG) -- an infinite stack would turn into NaN at the first all-in (inf - inf).
 */
#ifndef POKERL_HIP_H
#define POKERL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_ABI_VERSION 6
#define PK_MIN_PLAYERS 2
#define PK_MAX_PLAYERS 16 /* the reference takes any num_players (game.py:246; the deck allows 23).  Up to 16 the numpy routines it
                             calls are restated exactly: np.sum's eight-lane pairwise blocks (one up to 15 seats, two at 16) and
                             np.argsort's stable insertion sort (the pinned numpy sorts up to 17 elements that way); from 18 seats on
                             argsort's order among EQUAL bets -- which decides side pots -- is no longer a rule the reference pins,
                             and a 17th seat does not fit the 16 nibbles of a policy word: DESIGN.md section 8, docs/history.md section 9.  13 ... 16 seats
                             run kernels that keep part of the table in AGPRs at one wave per SIMD (no scratch memory). */
#define PK_MAX_ENV_BATCHES 8 /* pk_set_env_batches */
#define PK_MAX_DEVICES 64 /* the handle-less judger calls keep one scratch arena per device index below this */
#define PK_NUM_MOVES 7 /* pokerl/enums.py:104-114 PokerMoves */

/* return codes */
#define PK_OK 0
#define PK_E_INVALID_ARG (-1)
#define PK_E_NO_DEVICE (-2)
#define PK_E_HIP (-3)
#define PK_E_OOM (-4)
#define PK_E_TABLE (-5) /* at least one table reported a PK_TERR_* bit; call completed for all other tables */
#define PK_E_BUSY (-6)  /* PokerGameEnv steps are in flight (pk_env_step_async_d); nothing was done: drain them first */

/* per-table error bits */
#define PK_TERR_INVALID_ACTION 1 /* Game.step ValueError, pokerl/game.py:649-651: that table is left untouched */
#define PK_TERR_NO_WINNER 2      /* Game.end_hand AssertionError, pokerl/game.py:473: state partially mutated as in the reference */
#define PK_TERR_HAND_CAP 4       /* the reference would (as good as) never return from this Game.step: either every seat's
                                    credits are exactly 0 with no seat ACTIVE after a hand rolled over (each further hand
                                    re-creates that state: detected at once), or more than PK_HAND_CAP hands were rolled
                                    inside ONE step (sane configs roll <= 6; blinds 40x the stacks: 1 315 observed) */
#define PK_HAND_CAP 4096
#define PK_TERR_ENV_CAP 8        /* PokerGameEnv.reset/step auto-played more than PK_ENV_STEP_CAP opponent steps without
                                    reaching seat 0 or the end of the game (the reference's loops, envs/game_env.py:24,
                                    :41, :49, would still be spinning -- e.g. seat 0 broke with the game not over) */
#define PK_ENV_STEP_CAP 8192

/* step flags (bit set) = the tuple Game.step returns, pokerl/game.py:634-641 */
#define PK_FLAG_GAME_OVER 1
#define PK_FLAG_HAND_OVER 2
#define PK_FLAG_TURN_OVER 4

/* in-kernel agents (synthetic workload; RandomAgent semantics of pokerl/agents/random.py:12-16) */
#define PK_POLICY_RANDOM 0 /* uniform over the valid mask */
#define PK_POLICY_ALLIN 1  /* always PokerMoves.ALL_IN */
#define PK_POLICY_CALL 2   /* the calling station: CALL if valid, else CHECK if valid, else ALL_IN (no random draw) */
#define PK_NUM_POLICIES 3
/* One agent per seat, as PokerGameEnv(agents=[...]) has (pokerl/envs/game_env.py:13-18, :25, :43, :51): a 64-bit word with
 * the policy of seat p in nibble p (bits 4p..4p+3).  PK_POLICY_EXTERNAL: the CALLER plays that seat (pk_env_step_multi_d). */
#define PK_POLICY_EXTERNAL 15
#define PK_SEAT_POLICY(word, p) ((int)(((word) >> (4 * (p))) & 15))
#define PK_ACTION_SKIP (-2) /* pk_env_step_multi_d: "no action for this (idle) table" */

/* f64 [T][N] fields of pk_get_f64 = Game attributes, pokerl/game.py:260-264 */
#define PK_F_CREDITS 0
#define PK_F_BETS 1
#define PK_F_PENDING_BETS 2
#define PK_F_PAYOFFS 3

/* int32 [T] fields of pk_get_i32 = Game attributes, pokerl/game.py:251-258 */
#define PK_I_ACTIVE_PLAYER 0
#define PK_I_TURN 1
#define PK_I_DEALER_IDX 2
#define PK_I_SMALL_BLIND_IDX 3
#define PK_I_BIG_BLIND_IDX 4
#define PK_I_HAND 5

/* f64 [T] per-table values of pk_get_table_f64 = Game properties */
#define PK_TF_POT 0       /* Game.pot: np.sum(bets) in numpy's association order, pokerl/game.py:281-284 */
#define PK_TF_HIGH_BET 1  /* Game.high_bet: np.max(pending_bets), pokerl/game.py:287-290 */
#define PK_TF_MIN_RAISE 2 /* Game.minimum_raise_value */

/* rollout counters */
#define PK_C_STEPS 0
#define PK_C_HANDS 1 /* hands played: end_hand() calls that ran to their end, pokerl/game.py:453-539 */
#define PK_C_EVALS 2 /* 7-card eval_hand calls made by showdowns, pokerl/game.py:489 */
#define PK_C_GAMES 3
#define PK_NUM_COUNTERS 4

typedef struct pk_handle pk_handle;

int pk_abi_version(void);
/* "abi=<PK_ABI_VERSION> src=<16 hex digits>": the hash pokerl_amd/build.py takes over the kernel sources and compiler flags this library was built
 * from (comments and white space excluded).  Every profiles/ *_summary.json carries the hash of the library it was measured on; bench.py marks a
 * roofline figure that rests on a summary of OTHER sources `profile_stale`. */
const char *pk_build_info(void);
/* Number of visible HIP devices (0 if none / no driver). */
int pk_device_count(void);
const char *pk_last_error(const pk_handle *h); /* h may be NULL: last create/standalone error of this thread */

/* Game(**config), pokerl/game.py:242-264.  start_credits: N doubles or NULL (then start_credit_scalar is
 * broadcast, the `isinstance(self.start_credits, int)` branch of game.py:408).  `dealer` is kept for API parity;
 * Game.reset() overwrites it (game.py:403).  Tables start un-reset (credits 0), as in the reference. */
int pk_create(pk_handle **out, int device, int num_tables, int num_players, const double *start_credits,
              double start_credit_scalar, double big_blind, double small_blind, int dealer, uint64_t seed,
              uint32_t table_id_base);
int pk_destroy(pk_handle *h);
int pk_num_tables(const pk_handle *h);
int pk_num_players(const pk_handle *h);
/* How pk_create laid the tables out over wavefronts (read-only; fixed for the handle's life).  tables_per_wave: a power of two, 1 .. 64 --
 * small batches are spread over the chip: 64 halved while num_tables <= 1024 * (tables_per_wave / 2), so 1 up to 1 024 tables and 64 only
 * above 32 768 (knob: env PK_TPB); a wave's lanes >= tables_per_wave are dead.  env_tables_per_wave: the same of the PokerGameEnv kernels
 * (env PK_ENV_TPB, a power of two; default tables_per_wave).  Results do not depend on either.  NULL arguments: PK_E_INVALID_ARG. */
int pk_get_wave_shape(pk_handle *h, int *tables_per_wave, int *env_tables_per_wave);

/* Game.reset(dealer=...), pokerl/game.py:397-412, on tables with mask[t] != 0 (mask NULL = all tables). */
int pk_reset(pk_handle *h, const uint8_t *mask, int dealer);
/* Same with a DEVICE mask, asynchronous on the handle's stream: tables with (mask_d[t] & mask_bits) != 0 are reset (mask_d NULL = all
 * tables).  mask_bits picks the bits of a mask byte that count, so that the flags pk_step_d wrote can serve as the mask directly:
 * pk_reset_d(h, flags_d, PK_FLAG_GAME_OVER, 0) is the `if game_over: game.reset()` of a device-resident rollout loop
 * (examples/random_game.py:8-12) without a host round trip; 0xFF = any non-zero byte. */
int pk_reset_d(pk_handle *h, const uint8_t *mask_d, int mask_bits, int dealer);

/* Game.step(action), pokerl/game.py:621-700, one action per table.
 * flags[T] (PK_FLAG_*), terr[T] (PK_TERR_*, may be NULL).  Returns PK_E_TABLE if any terr != 0. */
int pk_step(pk_handle *h, const int32_t *actions, uint8_t *flags, uint8_t *terr);
/* Same, device-resident I/O (inputs already in HBM; asynchronous on the handle's stream). */
int pk_step_d(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d);
/* pk_step_d with the `if game_over: game.reset()` of a rollout loop (examples/random_game.py:8-12) in the SAME launch: a table whose
 * step ends its game (or runs into PK_TERR_HAND_CAP, which the reference would never leave) is Game.reset(dealer = 0) on the spot, exactly
 * as pk_rollout's auto_reset does; flags_d[t] still reports PK_FLAG_GAME_OVER and terr_d[t] the error bits of the step that ended it.
 * Saves the pk_reset_d launch of the loop (a launch costs ~4 us of a ~25 us step at 65 536 tables). */
int pk_step_auto_d(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d);
/* Game.step as a BOUNDED launch, for callers that act on whichever tables are ready (the pk_env_step_async_d idea applied to Game.step).
 * The reference's next_player loop plays whole hands in which nobody can act (pokerl/game.py:607-611), so ONE step can roll through
 * several hands: about one table in 10 000 per step does -- but among 65 536 tables the slowest needs ~4 hands, each ~3 us of serial work,
 * and a synchronous step launch (pk_step_d: ~20 us) lasts as long as that one table.  Here a launch serves at most max_hands end_hand
 * rounds (1: every table's step up to its first hand end): a table whose step has returned gets ready_d[t] = 1 and its flags_d / terr_d
 * written; a table whose step rolls on gets ready_d[t] = 0, its outputs are left untouched and the step stays IN FLIGHT on the device --
 * the next call carries on with it and IGNORES actions_d[t].  An invalid action returns at once (ready, PK_TERR_INVALID_ACTION, table
 * untouched).  auto_reset != 0: as pk_step_auto_d.  Per table the sequence of steps, flags and RNG draws is exactly the synchronous one;
 * only the call that delivers them differs.  max_hands <= 0: run every step to its end (every table ready) -- which also ends the state in
 * which every other entry point that reads or changes tables returns PK_E_BUSY (pk_sync only waits) -- EXCEPT the device-resident readers a
 * caller needs to act on the ready tables: pk_pick_actions_d, pk_get_obs_d, pk_get_obs_packed_d, pk_get_valid_actions_d, pk_get_f64_d (their
 * rows for a table in flight show that table in the middle of its step: ignore them).  auto_reset must not change while
 * steps are in flight (PK_E_INVALID_ARG).  A step that has already rolled 16 hands is carried to its end whatever the budget.
 * A DRAIN (max_hands <= 0) IS A FULL STEP CALL: besides finishing what is in flight it steps every idle (ready) table with actions_d[t], like any other
 * call.  To drain WITHOUT stepping, fill actions_d with an invalid action (-1): those tables come back untouched with PK_TERR_INVALID_ACTION in terr_d[t]
 * (the error byte of a table that was merely passed over -- not an error of the call) -- or pass actions_d == NULL, which only a drain accepts and which
 * means the same "no action for anybody".  Draining with the buffer the previous launch consumed steps the ready tables a second time with stale actions. */
int pk_step_async_d(pk_handle *h, const int32_t *actions_d, uint8_t *flags_d, uint8_t *terr_d, uint8_t *ready_d, int max_hands, int auto_reset);

/* Game.get_valid_actions(player), pokerl/game.py:339-383: out[T][7] one-hot bytes.  player < 0: each table's active
 * player (the reference's `player=None`); 0 <= player < N: that seat on every table. */
int pk_get_valid_actions(pk_handle *h, int player, uint8_t *out);

/* State reads (Game attributes). */
int pk_get_f64(pk_handle *h, int field, double *out /* [T][N] */);
/* The same into a DEVICE buffer, asynchronous on the handle's stream (e.g. the send buffer of an RCCL all-gather of the
 * payoffs: pokerl_amd/sharding.py gather_f64). */
int pk_get_f64_d(pk_handle *h, int field, double *out_d /* [T][N] */);
int pk_get_min_raise(pk_handle *h, double *out /* [T] minimum_raise_value */);
int pk_get_table_f64(pk_handle *h, int field /* PK_TF_* */, double *out /* [T] */);
int pk_get_game_over(pk_handle *h, uint8_t *out /* [T] Game.game_over, pokerl/game.py:317-320 */);
int pk_get_player_states(pk_handle *h, uint8_t *out /* [T][N] PlayerState, pokerl/enums.py:130-136 */);
int pk_get_i32(pk_handle *h, int field, int32_t *out /* [T] */);
/* RNG-spec serials of each table: setup_hand() calls / completed Game.step() calls so far (64-bit; either pointer may be
 * NULL).  pk_set_serials resumes a table's streams at given serials (e.g. restoring a checkpoint); call before pk_reset. */
int pk_get_serials(pk_handle *h, uint64_t *hand_serial, uint64_t *step_serial);
int pk_set_serials(pk_handle *h, const uint64_t *hand_serial, const uint64_t *step_serial);
/* deck[0 : 5+2N] as Card.value bytes ((suit<<4)|rank0, pokerl/cards.py:28-62): community = [0:5], hole(p) = [5+2p : 7+2p]
 * (pokerl/game.py:385-395). out[T][5+2N]. */
int pk_get_cards(pk_handle *h, uint8_t *out);
/* Rankings of the last showdown of each table (pokerl/game.py:488-489): rank[T][N] HandRanking (10 = NONE for
 * seats not shown down), kick[T][N] = judger.get_kickers_value(kickers) (pokerl/judger.py:101-109). */
int pk_get_hand_ranks(pk_handle *h, uint8_t *rank, uint32_t *kick);

/* pokerl.judger.eval_hand (pokerl/judger.py:7-99) on M hands.  cards[M][7] Card.value bytes (unused slots ignored),
 * ncards[M] in 0..7 (NULL = all 7).  rank[M], kick[M] (packed kickers, judger.py:101-109), nkick[M] (may be NULL).
 * The FIRST call per device that needs the evaluator's 32 KB table builds it (unless a handle of up to ten seats exists on the device: pk_create has
 * built it): one hipMalloc, one small kernel and one hipStreamSynchronize -- on the stream the call was given (pk_eval_hands_d) or on the legacy default
 * stream (the host-buffer entry points, which run there anyway).  A one-off host block, not legal inside a stream capture: make one warm-up call
 * (any m >= 1) before capturing or timing.
 * Multiset semantics: duplicate cards are legal, as in the reference's own tests (those hands, hands of fewer than three cards and
 * hands with a byte that is no card -- suit > 3 or rank nibble > 12 -- take the reference's sort-and-scan; 3..7 DISTINCT cards a
 * table-driven evaluator that equals it on every subset of the deck: tools/host_sim `evalntab`, GPU digest fast = 4).
 * Pinned on the device against the imported reference: every hand of 0..7 distinct cards and the hands that repeat cards
 * (tests/test_hip_evaln.py, tests/golden/evaln_digest.json; seven cards: eval7_digest.json).
 * A byte that is no card (the reference refuses to construct one, cards.py:58-59) is READ as suit = bits 4..5 and rank nibble as it
 * is: the result is eval_hand's on (byte & 0x3F) with Card.rank = (value & 0xf) or 13 applied to it -- nibbles 0 and 13 both rank as
 * the ace, 14 and 15 as two ranks above it; bits 6..7 are ignored -- with ONE exception: a hand that holds a rank above the ace
 * (nibble 14 or 15) never scores the plain five-high straight of judger.py:86-88, because the scan looks for that straight's ace at the
 * head of the rank-sorted hand.  The oracle states this reading as orc_eval_hands_bytes; tested for every byte value in every position. */
int pk_eval_hands(int device, const uint8_t *cards, const uint8_t *ncards, size_t m, uint8_t *rank, uint32_t *kick,
                  uint8_t *nkick);
/* Same op on device-resident buffers, asynchronous on `stream` (a hipStream_t; NULL = the default stream): the
 * partial-hand rank feature of examples/q_learning.py:29-33 (2/5/6/7-card hands every step) without a host round trip. */
int pk_eval_hands_d(int device, const uint8_t *cards_d, const uint8_t *ncards_d, size_t m, uint8_t *rank_d, uint32_t *kick_d,
                    uint8_t *nkick_d, void *stream);
/* pokerl.judger.compare_rankings (pokerl/judger.py:111-158) on M lists of n rankings: rank[M][n], kick[M][n] ->
 * onehot[M][n].  Includes the reference's line-148 behaviour. */
int pk_compare_rankings(int device, const uint8_t *rank, const uint32_t *kick, int n, size_t m, uint8_t *onehot);

/* Streaming evaluator on device-resident data: hands_d[m] = one 7-card hand per 64-bit word (card i = byte i, byte 7
 * unused), out_d[m] = HandRanking<<20 | kickers value.  12 algorithmic bytes per evaluation (8 in + 4 out): HBM-bound.
 * distinct != 0: the caller guarantees 7 DISTINCT cards per hand (every in-game hand) and the bitmask evaluator is used;
 * distinct == 0: the general (multiset) evaluator of pk_eval_hands.  Runs on the default stream, synchronous.
 * hands_d must be 8-byte and out_d 4-byte aligned; 16-byte / 8-byte alignment (any allocation base) enables the
 * two-hands-per-lane vector path. */
int pk_eval7_d(int device, const uint64_t *hands_d, size_t m, uint32_t *out_d, int distinct);
/* Synthetic workload for it: hand i = the first 7 cards of the RNG-spec deck of (seed, table_id = i, hand_serial = 0). */
int pk_make_hands_d(int device, uint64_t seed, size_t m, uint64_t *hands_d);
/* `reps` back-to-back passes of pk_eval7_d timed with HIP events: average milliseconds per pass. */
int pk_time_eval7_d(int device, const uint64_t *hands_d, size_t m, uint32_t *out_d, int distinct, int reps, double *ms_per_pass);

/* Exhaustive-check hook for the evaluators: v = HandRanking<<20 | kickers value of every 7-card hand whose two lowest
 * canonical deck indices (pokerl/cards.py:77 order) are (a, b), in lexicographic order; out holds C(51-b, 5) words.
 * fast == 1: the 7-distinct-card evaluator the showdown kernels use; fast == 0: the general one behind pk_eval_hands;
 * fast == 2: the table-driven 7-distinct-card evaluator of pk_eval7_d (cards of hand i rotated by i inside the packed word);
 * fast == 3: the register evaluator that backed pk_eval_hands(_d) up to ABI 4 and still does when the evaluator table cannot be allocated
 * (a bitmask fast path for 3..7 distinct cards, the reference's scan for hands that repeat a card or hold fewer than three);
 * fast == 4: the table path pk_eval_hands(_d) takes (eval_tab_n, cards rotated as for fast == 2). */
int pk_eval7_prefix(int device, int a, int b, int fast, uint32_t *out, size_t *count_out);

/* Actions the in-kernel agent `policy` would take now (one per table) -- lets a host loop reproduce rollouts. */
int pk_pick_actions(pk_handle *h, int policy, int32_t *actions);
int pk_pick_actions_d(pk_handle *h, int policy, int32_t *actions_d);

/* Throughput path: K lockstep Game.step()s per table with in-kernel agents; finished games are reset
 * (Game.reset()) when auto_reset != 0.  fused != 0: ONE launch, table state held in registers for all K steps;
 * fused == 0: K launches, state round-trips HBM every step.  counters[PK_NUM_COUNTERS] are ADDED to (may be NULL).
 * Asynchronous unless counters != NULL.  With counters == NULL a fused call may also DEFER part of its steps: a launch
 * ends when the first lanes of a wave run out of work instead of idling until the slowest table has finished, and the
 * tables remember what they still owe; the next pk_rollout picks that up, and every other entry point (getters,
 * pk_step, pk_reset, pk_sync, pk_record_event, ...) first completes it (pk_flush), so no caller can observe a table
 * that has made fewer than the requested steps.  Results do not depend on how the steps were split over launches. */
/* Kernel choice (internal, bit-identical results either way): for random agents up to six seats and all-in agents up to ten, batches of at most one
 * wave per SIMD (<= 65 536 tables) and launches of >= 16 steps run the variant that ranks the showdown hands with the table-driven evaluator out of
 * each wave's own 32 KB LDS copy of the table (+2 ... 14 %).  That variant takes ALL of a CU's LDS (four 40 KB workgroups): two handles that roll out
 * CONCURRENTLY on one GPU then run one after the other instead of side by side -- env PK_ROLLOUT_TAB=0 switches the variant off for such a process
 * (PK_ROLLOUT_TAB=<n>: minimum steps per launch, default 16). */
int pk_rollout(pk_handle *h, int k_steps, int policy, int auto_reset, int fused, uint64_t *counters);
/* Asynchronous fused pk_rollout calls (counters == NULL, auto_reset != 0) are also COALESCED on the host: while the two
 * most recent launches are still running, a call only adds its steps to a host-side count, which is launched as ONE kernel
 * as soon as a launch slot frees up, when it reaches `max_steps`, or by the flush every observer issues -- so a stream of
 * short calls (20 steps each) runs as launches of up to max_steps steps and pays the fixed cost of a launch once per
 * launch, not per call.  Invisible like deferral: no entry point can observe fewer than the requested steps.
 * max_steps: 0 = every call launches at once; default 1024 (env PK_COALESCE).
 * What it buys depends on the CALLER: a loop that never looks at the tables between calls (bench.py's command: 20-step calls)
 * runs as ~1 000-step launches (30 G env-steps/s at 65 536 x 6); a caller that reads observations or rewards every 20 steps
 * flushes each time and gets the one-launch-per-call rate (21 G: bench.py's extra leg "one launch per call").  Held steps start
 * with the next pk_rollout, flush, getter or pk_wait_event -- not by themselves. */
int pk_set_coalesce(pk_handle *h, int max_steps);
/* Launches of the rollout kernel since the last reset: out[4] = {launches (including the 0-step flushes of deferred
 * work), steps summed over them, min and max steps per launch over the launches with steps}.  reset != 0 clears them. */
int pk_get_launch_stats(pk_handle *h, uint64_t *out, int reset);
/* Diagnostic: the steps each table still owes ON THE DEVICE (out[T]); waits for the launches queued so far but does NOT
 * complete the deferred work (and does not see steps a coalescing host still holds back). */
int pk_get_owed(pk_handle *h, uint32_t *out);
/* Completes deferred rollout steps now (asynchronous on the handle's stream); a no-op when there are none. */
int pk_flush(pk_handle *h);
/* Tuning knobs of the fused rollout (values outside 1..64 leave the knob unchanged): `park` = lanes of a wave waiting at
 * end_hand before the wave runs it (default: per kernel, 28 for random agents, 32 otherwise); `endk` = a deferred launch
 * ends once fewer than this many lanes have work (1 = never defer). */
int pk_set_tuning(pk_handle *h, int park, int endk);

/* PokerGameEnv.reset() / .step(action) (pokerl/envs/game_env.py:20-29, :31-53): seat 0 is the controlled seat,
 * the other seats play `opp_policy` in-kernel.  reward[T] f64, done[T], hand[T] bytes. */
int pk_env_reset(pk_handle *h, const uint8_t *mask, int opp_policy);
int pk_env_step(pk_handle *h, const int32_t *actions, int opp_policy, double *reward, uint8_t *done, uint8_t *hand,
                uint8_t *terr);

/* Dense observation of Game.StateView(active player) (pokerl/game.py:117-131), one row of PK_OBS_DIM(N) doubles
 * per table: [player, turn, minimum_raise_value, valid_actions[7], player_cards[2], community_cards[5] (-1 where
 * not yet visible: game.py:278), credits[N], bets[N], pending_bets[N]]. */
#define PK_OBS_DIM(n) (3 + 7 + 2 + 5 + 3 * (n))
/* player < 0: each table's active player (Game.active_state, game.py:323-332); 0 <= player < N: that SEAT's view on every
 * table.  NOTE the one difference from the reference's constructor: StateView(game, 0) there is the ACTIVE player's view
 * (`player or game.active_player`, game.py:122, treats seat 0 like None); here player == 0 is seat 0 and "the active
 * player" is spelled -1.  The Python mirror (VecGame.observations_of / state_views) maps 0 and None to -1 like the
 * reference. */
int pk_get_obs(pk_handle *h, int player, double *out /* [T][PK_OBS_DIM(N)] */);

/* The same row, compact, for callers that move observations over PCIe or keep millions of them: PK_OBS_PACKED_BYTES(N) bytes
 * per table, 8-byte aligned --
 *   byte 0 player (seat), 1 turn, 2 valid_actions as bits (bit a = PokerMoves a), 3-4 player_cards, 5-9 community_cards
 *   (Card.value bytes; 0xFF where the f64 row has -1), 10-15 zero;
 *   then (3N+1) f64: minimum_raise_value, credits[N], bets[N], pending_bets[N] -- the money stays binary64, bit for bit.
 * 168 bytes against 280 at six seats.  pokerl_amd.state_view.PACKED_DTYPE(N) is the numpy structured dtype of a row. */
#define PK_OBS_PACKED_BYTES(n) (16 + 8 * (3 * (n) + 1))
int pk_get_obs_packed(pk_handle *h, int player, uint8_t *out /* [T][PK_OBS_PACKED_BYTES(N)] */);

/* Pinned host memory for the host-pointer entry points: a getter / pk_step / pk_env_step* whose buffers were allocated here
 * copies at PCIe line rate and (pk_env_step_begin) without blocking; any other host memory works too, through the HIP
 * runtime's staged copies (about half the rate).  Wraps hipHostMalloc / hipHostFree. */
int pk_host_alloc(void **out, size_t bytes);
int pk_host_free(void *p);

/* Game.step's precondition for a whole batch, nothing mutated (pokerl/game.py:648-651: `if action not in valid_actions:
 * raise ValueError`): *first_bad = the lowest table index whose action is not valid for its active player, or -1. */
int pk_check_actions(pk_handle *h, const int32_t *actions, int32_t *first_bad);

/* Device-resident variants for a learner that lives on the same GPU (no host round trip; asynchronous on the handle's
 * stream -- see "Stream control" below for ordering against your own stream): out_d / actions_d / ... are DEVICE pointers. */
int pk_get_obs_d(pk_handle *h, int player, double *out_d /* [T][PK_OBS_DIM(N)] */);
int pk_get_valid_actions_d(pk_handle *h, int player, uint8_t *out_d /* [T][7] one-hot */);
int pk_env_step_d(pk_handle *h, const int32_t *actions_d, int opp_policy, double *reward_d, uint8_t *done_d,
                  uint8_t *hand_d, uint8_t *terr_d);
int pk_env_reset_d(pk_handle *h, const uint8_t *mask_d /* NULL = all */, int opp_policy);
/* PokerGameEnv.step with the rest of a learner's loop fused into the same launch (each option removes a launch per env
 * step): actions_d == NULL lets the in-kernel agent `seat0_policy` play seat 0; auto_reset != 0 applies
 * PokerGameEnv.reset() (pokerl/envs/game_env.py:20-29) on the spot to every table whose step returned done (or ran into
 * PK_TERR_HAND_CAP / PK_TERR_ENV_CAP) -- reward / done / hand / terr still describe the step that ended the episode, and
 * terr also carries the error bits of that reset, should its loop (game_env.py:24-27) run into one;
 * obs_d != NULL receives the dense StateView row of the player to act (PK_OBS_DIM(N) doubles per table). */
int pk_env_step_fused_d(pk_handle *h, const int32_t *actions_d, int seat0_policy, int opp_policy, int auto_reset,
                        double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d, double *obs_d);

/* The compact row (PK_OBS_PACKED_BYTES) from the PokerGameEnv kernels: once a device buffer is set here, every
 * pk_env_step_fused_d / _async_d / _multi_d call writes the packed row of each table it delivers into it (beside the f64 row
 * if obs_d is given too), from registers.  NULL switches it off.  8-byte aligned, [T][PK_OBS_PACKED_BYTES(N)]. */
/* Exactly those three write it (pk_env_step_d, pk_env_step / _begin and pk_env_reset_d do not: after a reset the rows are those of the last
 * step -- refresh them with pk_get_obs_packed_d).  The handle keeps the RAW pointer: call pk_set_env_obs_packed(h, NULL) before freeing the
 * buffer.  PK_E_BUSY while env steps are in flight. */
int pk_set_env_obs_packed(pk_handle *h, uint8_t *obs_packed_d);
int pk_get_obs_packed_d(pk_handle *h, int player, uint8_t *out_d);

/* The observation from the Game.step kernels themselves (pokerl/game.py:323-332: `game.active_state`, the StateView of the player to act,
 * is what a learner that drives Game.step reads right after every step; pokerl/game.py:117-131).  Once a buffer is set here, every
 * pk_step_d / pk_step_auto_d / pk_step_async_d launch (pk_step too: it runs pk_step_d) writes, for each table whose step RETURNED in that
 * launch, the row of the player to act -- from the registers the step left, in the same launch -- into
 *   obs_d         [T][PK_OBS_DIM(N)] f64, the row of pk_get_obs_d(h, -1, ...), and / or
 *   obs_packed_d  [T][PK_OBS_PACKED_BYTES(N)], the row of pk_get_obs_packed_d(h, -1, ...);
 * either may be NULL (both NULL: off, the default).  A table whose action was refused (PK_TERR_INVALID_ACTION) gets the row of its untouched
 * table; a table pk_step_auto_d reset on the spot gets the first row of its new game; a table whose step is still in flight after a bounded
 * launch (ready_d[t] == 0) keeps the row it had.  Saves the k_obs launch per step and the second pass over the 285 B/table the step kernel has
 * just stored.  8-byte aligned buffers; the handle keeps the RAW pointers: call pk_set_step_obs(h, NULL, NULL) before freeing them.  Rows are NOT
 * written by pk_reset / pk_reset_d / pk_rollout (refresh with pk_get_obs(_packed)_d after those).  PK_E_BUSY while steps are in flight. */
int pk_set_step_obs(pk_handle *h, double *obs_d, uint8_t *obs_packed_d);

/* pk_env_step through host buffers in two halves, for callers that want the copies off their critical path:
 * pk_env_step_begin uploads actions[T], launches PokerGameEnv.step (auto_reset != 0: finished episodes are reset on the spot,
 * as in pk_env_step_fused_d) and queues the device-to-host copies of reward / done / hand / terr and, where not NULL, of the
 * f64 observation rows (obs) and / or the packed ones (obs_packed); pk_env_step_end waits for them.  With buffers from
 * pk_host_alloc nothing in `begin` blocks and the copies run at PCIe line rate, so the caller's own work -- or the step of
 * ANOTHER handle -- overlaps with them.  Per-table errors are in terr[] after `end` (which does not scan them).  The handle
 * must not be used between the two calls -- every entry point that reads or changes tables, a second pk_env_step_begin included, returns
 * PK_E_BUSY until pk_env_step_end (pk_sync only waits); pk_env_step_end without a begin is PK_E_INVALID_ARG -- and EVERY buffer --
 * actions[] included, which a pinned upload reads when the copy engine gets to it, not when `begin` returns -- must stay valid and
 * untouched until `end` has returned.  Invalid actions are NOT an error of either call: such a table is left untouched and terr[t] says
 * PK_TERR_INVALID_ACTION -- read terr[] after `end`. */
int pk_env_step_begin(pk_handle *h, const int32_t *actions, int opp_policy, int auto_reset, double *reward, uint8_t *done,
                      uint8_t *hand, uint8_t *terr, double *obs, uint8_t *obs_packed);
int pk_env_step_end(pk_handle *h);

/* The same as a BOUNDED launch for learners that act on whichever tables are ready (asynchronous vector environment).
 * One PokerGameEnv.step of a whole batch lasts as long as its slowest table: a seat 0 that goes broke during an
 * opponent's step waits for the end of the game (game_env.py:49-52), ~150 Game.steps against a mean of 6.  Here a launch
 * runs at most max_passes betting passes (each busy table executes about one Game.step per pass); a table whose
 * env.step (and, with auto_reset, the reset after it) has returned by then gets ready_d[t] = 1 and its reward / done /
 * hand / terr / obs row written; the others get ready_d[t] = 0, their outputs are left untouched and their step stays IN
 * FLIGHT on the device: the next call carries on with it and IGNORES actions_d[t].  A table with an invalid action
 * returns at once (ready, PK_TERR_INVALID_ACTION, untouched).  Per table the sequence of steps, outputs and RNG draws is
 * exactly that of pk_env_step_fused_d; only the call that delivers them differs.  max_passes <= 0: run every step to its
 * end (every table ready).  While steps may be in flight (after any call with max_passes > 0) all other entry points
 * that read or change tables return PK_E_BUSY (pk_sync only waits); a call with max_passes <= 0 ends that state.
 * Use auto_reset != 0 with bounded launches: pk_env_reset_d is one of the entry points that are busy meanwhile, so a
 * finished episode could only be reset after a drain.  Steps in flight keep their agents: while that state lasts every
 * call must pass the same seat-0 source (actions_d NULL or not, seat0_policy), opp_policy and auto_reset as the call that
 * started it, else PK_E_INVALID_ARG (nothing done).
 * How long a table can stay in flight: a Game.step that rolls hand after hand is carried to its end inside one launch once it has rolled
 * 16 hands; an env.step whose loops never reach seat 0 (seat 0 broke with the game not over: the reference would spin forever, here
 * PK_ENV_STEP_CAP = 8 192 opponent steps end it with PK_TERR_ENV_CAP) makes about max_passes Game.steps per launch, i.e. is delivered
 * after ~8 192 / max_passes launches -- slow, never stuck; the other tables are not held up by it. */
int pk_env_step_async_d(pk_handle *h, const int32_t *actions_d, int seat0_policy, int opp_policy, int auto_reset,
                        int max_passes, double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d,
                        double *obs_d, uint8_t *ready_d);

/* Sub-batches of pk_env_step_async_d inside ONE handle.  A bounded launch ends with a tail (its last waves run alone) and
 * the launches of one handle are serialised on its stream, so one handle of 524 288 tables delivers 2.99 G env.step/s where
 * the same handle in three sub-batches delivers 3.56 G (profiles/r03_env_inner_sweep.txt).  pk_set_env_batches(h, B) splits
 * the handle's tables into B contiguous ranges (whole waves each; fewer than B for a small batch: right after the call pk_env_last_range reports range 0, [0, tables per range)),
 * each with an internal stream.  From then on a call with max_passes > 0
 *   - LAUNCHES one range (round robin), reading actions_d only inside it, and
 *   - DELIVERS the range launched longest ago: the call WAITS ON THE HOST for that launch (made B - 1 calls ago, so done or
 *     nearly so; ABI 3 queued a device-side wait on the handle's stream instead, whose barrier packet could stall another range's
 *     hardware queue -- docs/history.md section 5), and pk_env_last_range reports [begin, end): ready_d / reward_d / ... / obs_d are
 *     COMPLETE inside that range when the call returns (and untouched outside).  The launch itself is ordered after the work the
 *     caller queued on the handle's stream (an event pair) unless that stream is idle, in which case nothing needs ordering.
 *     fresh != 0: that range has not been launched yet since pk_set_env_batches / the last drain -- nothing was written, every
 *     table of it awaits its first action (its observation is the one pk_env_reset_d / pk_get_obs_d left).
 * The range delivered by one call is the range the next call launches, so a learner acts on [begin, end) between two
 * calls.  max_passes <= 0 drains every range and delivers [0, T).  Per table nothing changes: the sequence of steps, outputs
 * and RNG draws is that of the synchronous call.  Call it while no env step is in flight (PK_E_BUSY otherwise).
 * Use B <= 3 (524 288 tables: 3.40 / 3.65 / 1.5 G env.step/s at B = 2 / 3 / 4): the internal streams are created with the highest
 * stream priority -- their own set of hardware queues, apart from the caller's stream, the legacy default stream and whatever else
 * the process created -- and a fourth one shares a queue with another range.
 * Ranges of >= 131 072 tables are the ones that pay (smaller batches: several handles, each on its own stream). */
int pk_set_env_batches(pk_handle *h, int batches);
int pk_env_last_range(pk_handle *h, int *begin, int *end, int *fresh);

/* PokerGameEnv with ONE AGENT PER SEAT, some of them played by the CALLER (self-play, league opponents, a learner's
 * earlier checkpoints): pokerl/envs/game_env.py:13-18 takes a list of agent callables and calls
 * self.agents[active_player](state) wherever an opponent is to act (:25, :43, :51).  seat_policies holds the agent of seat p
 * in nibble p: an in-kernel policy, or PK_POLICY_EXTERNAL.  The call is pk_env_step_async_d with two more outcomes per table:
 *   ready_d[t] = 1  PokerGameEnv.step (or .reset) has returned: reward / done / hand / terr / obs row written; the next
 *                   call reads actions_d[t] as seat 0's action (ignored if seat 0's nibble is an in-kernel policy);
 *   ready_d[t] = 2  an EXTERNAL opponent seat is to act inside the env call, which stays in flight: who_d[t] = that
 *                   seat, the obs row is ITS StateView, terr_d[t] = 0; the next call reads actions_d[t] as ITS action.  An
 *                   invalid one is refused: ready 2 again, terr_d[t] = PK_TERR_INVALID_ACTION, table untouched;
 *   ready_d[t] = 0  the pass budget ran out first (only with max_passes > 0); supply nothing;
 *   ready_d[t] = 3  the table was idle and actions_d[t] was PK_ACTION_SKIP: left alone, no output written (how a caller
 *                   that serves the yielded tables keeps the tables that have already returned out of further launches).
 *                   PK_ACTION_SKIP is honoured WHATEVER seat 0's agent is: also with an in-kernel policy in nibble 0 (where
 *                   actions_d[t] is otherwise ignored for idle tables) a -2 parks the table -- write 0 there, not stale data.
 * who_d[t] is always the seat to act next.  reset_d (may be NULL): reset_d[t] != 0 starts PokerGameEnv.reset()
 * (game_env.py:20-29) on table t instead of a step -- delivered like a step, with reward 0, done 0, hand 0 -- dropping
 * whatever that table had in flight.  max_passes <= 0: run until every table has returned or yielded.
 * Per table the Game.steps, their order and every RNG draw are those of the reference's loop with the same agents; external
 * seats whose caller plays an in-kernel policy's rule reproduce that policy's trajectory bit for bit (tested).
 * While tables may be in flight all other entry points that read or change tables return PK_E_BUSY (as after
 * pk_env_step_async_d); with an external seat that state lasts until pk_env_end_multi_d, which drains and ABANDONS the env
 * calls still waiting for an external action (their tables stay where they are, between two Game.steps); call it after a
 * drain (max_passes <= 0) so that no delivered step is lost.  seat_policies and auto_reset must not change meanwhile. */
int pk_env_step_multi_d(pk_handle *h, const int32_t *actions_d, const uint8_t *reset_d, uint64_t seat_policies, int auto_reset,
                        int max_passes, double *reward_d, uint8_t *done_d, uint8_t *hand_d, uint8_t *terr_d, double *obs_d,
                        uint8_t *who_d, uint8_t *ready_d);
int pk_env_end_multi_d(pk_handle *h);

/* Stream control (no torch types: `stream` is a hipStream_t, `event` a hipEvent_t, passed as void*).  A handle creates
 * its own NON-BLOCKING stream (no implicit ordering with the legacy default stream).  pk_set_stream makes it run on the
 * caller's stream instead, which orders every `_d` call after the work already queued there.  stream == NULL IS a
 * stream: the legacy default stream -- what `torch.cuda.current_stream().cuda_stream` (0) denotes unless the caller
 * entered a torch.cuda.Stream -- so the documented pattern g.set_stream(torch.cuda.current_stream().cuda_stream) orders
 * the handle with torch in every case (ABI 2 silently went back to the handle's own stream for 0: a data race).  A
 * stream of another device is refused (PK_E_INVALID_ARG).  pk_use_own_stream goes back to the handle's own stream.
 * Or keep two streams and order them with events:
 * pk_wait_event = the handle's stream waits for `event` (record it on your stream after producing actions_d),
 * pk_record_event = records `event` on the handle's stream (wait for it on your stream before reading obs_d); deferred
 * rollout steps are completed first, and the launches pk_env_step_async_d made on the handle's internal sub-batch streams
 * (pk_set_env_batches) are waited for, so the event covers everything requested so far. */
int pk_get_stream(pk_handle *h, void **stream_out);
int pk_set_stream(pk_handle *h, void *stream);
int pk_use_own_stream(pk_handle *h);
int pk_wait_event(pk_handle *h, void *event);
int pk_record_event(pk_handle *h, void *event);
/* Completes deferred rollout steps and waits until everything requested so far has finished. */
int pk_sync(pk_handle *h);

/* ---- Snapshots: save, restore and clone tables (copy.deepcopy / pickle of a Game, checkpoints, search over copies).
 *
 * A snapshot is a position-independent byte blob of m table RECORDS.  It holds no pointers: it can be written to disk or moved to another
 * device or process running the same library build.  Layout (pk_snapshot_bytes(N, m) bytes):
 *   header, 256 bytes: u32 magic "PKSN", u32 format version (1), u32 N, u32 0, u64 m, f64 start_credits[16] (seats >= N: 0),
 *                      f64 big_blind, f64 small_blind, zero padding;
 *   records, FIELD-MAJOR: each field an array [rows][m] that starts 256-byte aligned (offset of the next = previous + round_up(bytes, 256)):
 *     credits, bets, pending_bets, payoffs  f64 [N][m]     min_raise  f64 [m]     seat_states  u64 [m]     hand_serial, step_serial  u64 [m]
 *     cursors  u32 [m]     hand  i32 [m]     cards  u32 [ceil((5+2N)/4)][m]     show  u32 [N][m]     valid, terr  u8 [m]
 *   (the fields of the handle's own table state, table-major along m: one lane per table reads and writes coalesced words on both sides).
 * A record is everything a caller can observe of a table or that decides its future.  Not in a record: the deferred-launch and in-flight
 * bookkeeping (zero for an idle table; a load or clone writes zeros there), counters, the seed key and the table id.
 * FUTURE RANDOMNESS BELONGS TO THE DESTINATION: its seed key and its table id table_id_base + t.  A record carries the table's serials, so
 *   - a table restored into the same slot of the same handle, or of a handle with the same seed and table_id_base, continues bit-identically;
 *   - a table cloned into another slot continues its CURRENT hand identically under the same actions; its next decks and random-agent draws
 *     are those of the new table id.
 * Every entry point below completes deferred rollout work first, returns PK_E_BUSY while steps of pk_step_async_d / pk_env_step_async_d /
 * pk_env_step_begin are in flight (on either handle of a clone; nothing written), treats m == 0 as a no-op and is ordered on the handle's
 * stream.  `tables` / `tables_d` (int32 [m], NULL = tables 0 .. m-1) name the tables.  Refused with PK_E_INVALID_ARG, the reason in
 * pk_last_error and NOTHING written: a table index out of range; a destination named twice (sources may repeat); handles on different
 * devices; N or the money configuration (start credits, blinds) differing between blob / source and destination; a bad magic or version; a
 * load whose m differs from the blob's; an observer outside {-2, -1, 0 .. N-1}.  A call that takes an index array, and every load, checks on
 * the device and reads one refusal word back before it writes (the call waits for its stream up to there).
 * Blobs in device memory must be 8-byte aligned. */
#define PK_OBSERVER_NONE (-1)   /* clone: an exact copy */
#define PK_OBSERVER_ACTIVE (-2) /* clone: redeal from the point of view of each source table's active player */
/* Bytes of a blob of m records at N seats; 0 for N outside [PK_MIN_PLAYERS, PK_MAX_PLAYERS].  Needs no device. */
size_t pk_snapshot_bytes(int num_players, size_t m);
/* Save m tables into blob_d (device memory, asynchronous without an index array). */
int pk_save_tables_d(pk_handle *h, const int32_t *tables_d, size_t m, void *blob_d);
/* Restore m records of blob_d into the named tables.  Every record is checked on the device BEFORE any write, and the whole call is
 * refused if one fails -- a blob from this library always passes; a corrupted one must never make a later kernel index out of bounds:
 * cursor nibbles (active, dealer, sb, bb) < N, turn <= 4 (a finished game may stay at 4, game.py:561-564), in-flight bits 20..31 zero; the
 * four 16-bit seat masks use bits < N only and are pairwise disjoint; every card byte a Card.value and the 5+2N cards distinct -- or,
 * for a table never dealt (created, not reset yet), all 5+2N bytes zero at turn 0; all money finite; valid < 128.  A clone copies the
 * zero deck of a never-dealt table as it is (there is nothing hidden to redeal). */
int pk_load_tables_d(pk_handle *h, const int32_t *tables_d, size_t m, const void *blob_d);
/* The same through host memory (tables and blob), synchronous. */
int pk_save_tables(pk_handle *h, const int32_t *tables, size_t m, void *blob);
int pk_load_tables(pk_handle *h, const int32_t *tables, size_t m, const void *blob);
/* Table src_tables_d[i] of `src` -> table dst_tables_d[i] of `dst`, on dst's stream (after src's queued work; src's later work waits for
 * the clone's reads).  dst == src and overlapping index sets are allowed: the result is that of all reads before any write.
 * observer PK_OBSERVER_NONE: an exact copy.  observer = a seat p (0 .. N-1), or PK_OBSERVER_ACTIVE (p = each source table's active
 * player): a REDEAL of the cards p cannot see, so that a search over the copies does not know the future board or the opponents' cards.
 * p sees the board deck[0:nb] (nb = 0 at turn 0, else min(turn + 2, 5): game.py:266-278) and its hole cards deck[5+2p : 7+2p]; they stay.
 * The hidden slots -- board nb..4, then the two hole cards of every other seat in ascending seat order, folded and broken seats included --
 * are refilled by a uniform draw without replacement from the P = 52 - nb - 2 cards p has not seen (the deck's RNG spec with its own
 * stream): Philox4x32-10 with the DESTINATION's key, counter (dst table id, nonce lo, 'RDL0' + b, nonce hi), 64-bit words
 * X[2b] = w0 | w1 << 32, X[2b+1] = w2 | w3 << 32, chained bounded draws c_i = (x * (P - i)) >> 64 (x = X[i / 9] when i % 9 == 0, then
 * x = low 64 bits of the product), card i = the c_i-th not yet drawn unseen card in canonical order (value[k] = ((k%4)<<4) | (k/4)).
 * Money, cursors, serials, show, valid and terr are copied unchanged.  Both handles need the same N and money configuration. */
int pk_clone_tables_d(pk_handle *dst, const int32_t *dst_tables_d, pk_handle *src, const int32_t *src_tables_d, size_t m, int observer,
                      uint64_t nonce);
/* ---- Showdown equity: "if the cards still to come were dealt now, how often does each seat win?" -- every board enumerated on the device,
 * exact integer counts.
 *
 * A SPOT is N seats (the num_players of the call, 2 .. 16), two hole-card bytes per seat (Card.value; 0xFF = unknown / not dealt, allowed only
 * at a seat that is not live), nb = 0 .. 5 known board cards and a 16-bit live mask (bit p: seat p takes part in the showdown; bits >= N are
 * ignored).  Dead cards = the nb board cards and every hole card that is not 0xFF, live or not.  Pool = the 52 cards minus the dead ones,
 * P of them; boards = all C(P, 5 - nb) completions.  On each board v[p] = eval_hand(board + hole[p]) for a live seat and eval_hand([]) =
 * (NONE, []) for the others -- the list Game.end_hand builds (game.py:488-490) -- and the winners are compare_rankings(v) (judger.py:111-158
 * INCLUDING its line-148 behaviour: who takes the main pot as the reference judges it, which is not always who wins at poker).
 * This is the FIRST comparison end_hand makes -- main-pot equity.  It is an all-in EV only while every live seat has bet the same; with
 * unequal stacks the pot is paid out in levels: "Showdown EV" below (pk_equity_ev) gives the expected payoff in chips.
 * Per spot and seat, nw = the number of winners of a board:
 *   win[p]   u32  boards on which p is the only winner          tie[p]  u32  boards on which p wins and nw > 1
 *   share[p] u64  sum over the boards p wins of PK_EQ_SHARE_UNIT / nw  (720720 = lcm(1 .. 16): exact; sum over p = 720720 * boards)
 *   boards   u32  C(P, 5 - nb)                                    status  u8   PK_EQ_* bits, 0 = evaluated
 * equity[p] = share[p] / (720720 * boards).  A spot with a non-zero status gets all-zero counts and boards = 0; it never fails the call or
 * disturbs another spot.  Any of win / tie / share / boards / status may be NULL (not wanted).  m == 0 is a no-op; m < 2^31, and
 * a call whose worst-case task count (every spot pre-flop: 33 per spot in the explicit form from 256 spots on) does not fit 32 bits -- about
 * 130 M spots -- is refused with PK_E_INVALID_ARG: split the batch.  device < PK_MAX_DEVICES.
 * STREAMS: the device form runs on the stream it is given, asynchronously (its work space is a grow-only buffer the library keeps per
 * stream, for the 8 most recently used streams of a device); the host forms are synchronous -- the handle-less one on a pooled non-blocking stream, the table one on the handle's stream.
 * None of them touches the legacy default stream unless the caller passes it (stream == NULL) explicitly.
 * TABLE FORM: spot i is table tables[i] of the handle (NULL: table i; indices may repeat): board = deck[0:nb] with nb = 0 at turn 0, else
 * min(turn + 2, 5); hole cards = deck[5+2p : 7+2p] of EVERY seat (all 2N are dead, folded and broken seats included); live = the seats that are
 * ACTIVE, CALLED or ALL_IN.  The future board cards the deck already holds are unknown: they are in the pool.  It reads the handle's state and
 * writes nothing to it, completes deferred rollout work first like the getters, and runs on the handle's stream.  A table created but never
 * reset has an all-zero deck and reports PK_EQ_DUP_CARD. */
#define PK_EQ_SHARE_UNIT 720720u
#define PK_EQ_BAD_CARD 1u    /* a byte that is no card; 0xFF in the board or at a live seat */
#define PK_EQ_DUP_CARD 2u    /* a card twice */
#define PK_EQ_NO_LIVE 4u     /* no live seat */
#define PK_EQ_BAD_NBOARD 8u  /* nb > 5 */
#define PK_EQ_IN_FLIGHT 16u  /* table form: the table's step is in flight (the asynchronous Game.step entry point) */
#define PK_EQ_BAD_TABLE 32u  /* table form: the table index is out of range (nothing is read) */
/* holes_d u8 [m][N][2], board_d u8 [m][5] (the first nboard_d[i] used), nboard_d u8 [m], live_d u16 [m]; outputs [m][N] / [m]. */
int pk_equity_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                const uint16_t *live_d, uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *boards_d, uint8_t *status_d, void *stream);
int pk_equity(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
              uint32_t *win, uint32_t *tie, uint64_t *share, uint32_t *boards, uint8_t *status);
int pk_table_equity_d(pk_handle *h, const int32_t *tables_d, size_t m, uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *boards_d,
                      uint8_t *status_d);
int pk_table_equity(pk_handle *h, const int32_t *tables, size_t m, uint32_t *win, uint32_t *tie, uint64_t *share, uint32_t *boards,
                    uint8_t *status);
/* ---- Sampled showdown equity: the same question for a seat that does NOT know the other hands -- the hidden cards are drawn, S samples per
 * spot, on the device; the counts are exact integers and bit-identical to a restatement of this definition.
 *
 * A SPOT is as above with one difference: a 0xFF hole byte at a LIVE seat is legal and means HIDDEN (each byte on its own: a seat may show one
 * card).  Dead cards = the nb board cards and every hole byte that is a card, live or not; a 0xFF at a seat that is not live is "not known" as
 * above (that card is simply in the pool).  Pool = the 52 cards minus the dead ones, P of them, in canonical order value[k] = ((k%4)<<4) | (k/4).
 * Hidden slots, in this order: board positions nb .. 4, then the hidden hole bytes by ascending seat, byte 0 before byte 1 -- D of them
 * (D <= 37 <= P always).  STATUS: the PK_EQ_* bits above; PK_EQ_BAD_CARD is "a byte that is no card, or 0xFF in the board".  A spot with a
 * non-zero status gets all-zero counts and samples = 0 and disturbs nothing else.
 * SAMPLE s (0 .. S-1) of a spot with stream id `id` (u32) is the redeal's draw (pk_clone_tables_d) on its own stream: Philox4x32-10 under
 * `key`, counter (id, s, 'EQS0' + b, nonce) with 'EQS0' = 0x45515330 and block b = 0, 1, 2; 64-bit words X[2b] = w0 | w1 << 32,
 * X[2b+1] = w2 | w3 << 32; chained bounded draws c_i = (x * (P - i)) >> 64 (x = X[i / 9] when i % 9 == 0, then x = the low 64 bits of the
 * product); hidden slot i receives the c_i-th not yet drawn pool card.  Then v[p] = eval_hand(board + hole[p]) for a live seat and (NONE, [])
 * for the others, and the winners are compare_rankings(v), exactly as above.  Outputs per spot and seat over the S samples: win, tie (u32),
 * share (u64, units of 720720 / nw); per spot samples (u32: S, or 0 where status != 0) and status (u8).  Any output may be NULL; m == 0 is a
 * no-op.  S = 1 .. 2^24 per call, nonce any u32; a spot's counts depend on (spot, key, nonce, id, S) only -- not on the batch it travels in --
 * and COUNTS OF CALLS WITH DIFFERENT NONCES ADD EXACTLY: that is the way to more samples (and to a running estimate).
 * Refused with PK_E_INVALID_ARG (pk_last_error names the function): N outside 2 .. 16, samples 0 or > 2^24, m * ceil(samples / 64) not
 * fitting 32 bits, an observer outside {-2, -1, 0 .. N-1}.
 * EXPLICIT FORM: key = (seed lo, seed hi) as pk_create's seed; id = ids[i] where the optional ids array (u32 [m]) is given, else i.
 * TABLE FORM: the handle's key, id = table_id_base + table index (independent of sharding); nb, board and live seats as pk_table_equity.
 * observer = a seat p (0 .. N-1) or PK_OBSERVER_ACTIVE (each table's active seat): p's two hole cards are known; every other seat's are
 * hidden if the seat is live and, if it is not, NOT dead (p never saw a folded hand: those cards are in the pool).  PK_OBSERVER_NONE: all 2N
 * hole cards known and dead as in pk_table_equity, only the board is sampled.  Like pk_table_equity the call completes deferred rollout work,
 * reads only, runs on the handle's stream, and reports PK_EQ_IN_FLIGHT / PK_EQ_BAD_TABLE / PK_EQ_DUP_CARD (a table never dealt) per table.
 * STREAMS and work space: as pk_equity (the device form asynchronous on the stream it is given, the host forms synchronous).
 * The EXACT post-flop answer against one hidden opponent, per holding and under a range, is pk_equity_range below. */
int pk_equity_sampled_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                        const uint16_t *live_d, const uint32_t *ids_d /* NULL: i */, uint32_t samples, uint64_t seed, uint32_t nonce,
                        uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *samples_d, uint8_t *status_d, void *stream);
int pk_equity_sampled(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard,
                      const uint16_t *live, const uint32_t *ids /* NULL: i */, uint32_t samples, uint64_t seed, uint32_t nonce, uint32_t *win,
                      uint32_t *tie, uint64_t *share, uint32_t *samples_out, uint8_t *status);
int pk_table_equity_sampled_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, uint32_t samples, uint32_t nonce,
                              uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *samples_d, uint8_t *status_d);
int pk_table_equity_sampled(pk_handle *h, const int32_t *tables, size_t m, int observer, uint32_t samples, uint32_t nonce, uint32_t *win,
                            uint32_t *tie, uint64_t *share, uint32_t *samples_out, uint8_t *status);
/* ---- Ranged sampled equity: sampled showdown equity where every hidden seat draws its HOLDING from a weighted range -- any seat count, any
 * street.  Everything not stated here is "Sampled showdown equity" above.
 *
 * A SPOT is as there, except that a live seat shows both hole cards or hides both (0xFF 0xFF): a live seat with exactly one 0xFF is refused
 * with PK_EQ_BAD_CARD (a weighted draw of half a holding is not defined).  Dead cards = the nb board cards and every hole byte that is a card,
 * live or not; a 0xFF at a seat that is not live is in the pool; P = 52 - dead.  Hidden seats in ascending seat order, j = 0 .. H-1; always
 * P - 2H >= 15 >= 5 - nb.
 * RANGES: per call one table weights u16 [R][1326], 0 <= R <= PK_EQW_MAX_RANGES, over the holding index h = b (b - 1) / 2 + a of range equity
 * below.  Per spot, range_of u16 [N] names each seat's row (the explicit form: [m][N]); PK_EQW_UNIFORM (0xFFFF) = every weight 1; range_of == NULL = every hidden seat uniform.  An
 * entry is read only where the seat is hidden; there a value >= R other than 0xFFFF gives the spot PK_EQ_BAD_CARD (the u8 status word has no
 * bit left: a row that does not exist is reported as a bad input byte).  cum_r[h] = sum of w_r[0 .. h] (u32), T_r = cum_r[1325] < 2^27; the
 * uniform row has cum[h] = h + 1, T = 1326.
 * ATTEMPT s (0 .. S-1) of a spot with stream id `id`: Philox4x32-10 under `key`, counter (id, s, 'EQW0' + b, nonce) with 'EQW0' = 0x45515730,
 * blocks b = 0 .. ceil((H + 1) / 2) - 1, words X[2b] = w0 | w1 << 32, X[2b+1] = w2 | w3 << 32.
 *   1. hidden seat j draws u_j = (X[j] * T_j) >> 64; its holding h_j = the number of h with cum[h] <= u_j.
 *   2. the attempt is REJECTED if some T_j = 0, a drawn holding contains a dead card, or two drawn holdings share a card.  The accepted joint
 *      law is proportional to the product of w_j[h_j] over holdings disjoint from each other and from the dead cards.
 *   3. an accepted attempt draws the 5 - nb board cards from the P' = P - 2H pool cards left, canonical order, by the chained rule from the ONE
 *      word x = X[H]: c_i = (x * (P' - i)) >> 64, x = the low 64 bits; slot nb + i receives the c_i-th card not yet drawn.
 *   4. v[p] = eval_hand(board + hole[p]) for a live seat, (NONE, []) otherwise; winners = compare_rankings(v) as in "Showdown equity".
 * OUTPUTS over the ACCEPTED attempts: win, tie u32 [m][N], share u64 [m][N] (units of 720720 / nw), per spot accepted u32 and status u8.
 * equity = share / (720720 * accepted), formed by the caller (nan at accepted = 0).  A range with no weight left is NOT an error: status 0,
 * accepted 0.  A non-zero status gives zeros and disturbs no neighbour.  S = 1 .. 2^24, m * ceil(S / 64) must fit 32 bits, counts of calls
 * with different nonces add exactly (accepted included), a spot's counts depend on (spot, ranges, key, nonce, id, S) only.
 * Refused with PK_E_INVALID_ARG: what pk_equity_sampled refuses, num_ranges > PK_EQW_MAX_RANGES, num_ranges > 0 with weights NULL, and in the
 * table form observer PK_OBSERVER_NONE (nothing would be hidden).
 * TABLE FORM: the spot is exactly pk_table_equity_sampled's for a seat or PK_OBSERVER_ACTIVE (folded seats are not dead and not read);
 * range_of is u16 [N] by seat for all tables (range_per_table = 0) or [m][N] (1); the observer's own entry is ignored.  Key, id, deferred
 * rollout work, read-only, the handle's stream, PK_EQ_IN_FLIGHT / PK_EQ_BAD_TABLE / PK_EQ_DUP_CARD: as pk_table_equity_sampled.
 * STREAMS and work space: as pk_equity_sampled; the work space also holds the u32 [R][1326] cumulative sums. */
#define PK_EQW_MAX_RANGES 16
#define PK_EQW_UNIFORM 0xFFFFu
int pk_equity_ranged_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                       const uint16_t *live_d, const uint32_t *ids_d /* NULL: i */, uint32_t samples, uint64_t seed, uint32_t nonce,
                       const uint16_t *weights_d /*[R][1326]*/, uint32_t num_ranges, const uint16_t *range_of_d /*[m][N], NULL: uniform*/,
                       uint32_t *win_d, uint32_t *tie_d, uint64_t *share_d, uint32_t *accepted_d, uint8_t *status_d, void *stream);
int pk_equity_ranged(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard,
                     const uint16_t *live, const uint32_t *ids /* NULL: i */, uint32_t samples, uint64_t seed, uint32_t nonce,
                     const uint16_t *weights, uint32_t num_ranges, const uint16_t *range_of, uint32_t *win, uint32_t *tie, uint64_t *share,
                     uint32_t *accepted, uint8_t *status);
int pk_table_equity_ranged_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, uint32_t samples, uint32_t nonce,
                             const uint16_t *weights_d, uint32_t num_ranges, const uint16_t *range_of_d, int range_per_table, uint32_t *win_d,
                             uint32_t *tie_d, uint64_t *share_d, uint32_t *accepted_d, uint8_t *status_d);
int pk_table_equity_ranged(pk_handle *h, const int32_t *tables, size_t m, int observer, uint32_t samples, uint32_t nonce,
                           const uint16_t *weights, uint32_t num_ranges, const uint16_t *range_of, int range_per_table, uint32_t *win,
                           uint32_t *tie, uint64_t *share, uint32_t *accepted, uint8_t *status);
/* ---- Range equity: exact hand strength against ONE hidden hand -- the hero's result against every holding the hidden opponent can have, per
 * holding and reduced by a range of weights.  POST-FLOP ONLY: pre-flop a hidden hand is 2 * 10^9 boards per spot and
 * the pre-flop hero-versus-holding table is a constant nobody needs recomputed; such a spot reports PK_EQ_PREFLOP.
 *
 * A SPOT is hero u8[2] (Card.value bytes), board u8[5] with nb = 3, 4 or 5 known cards, and dead u64: bit k = the card of canonical index
 * k = rank0 * 4 + suit is known to be out of play (a shown folded hand, say; 0 = none).  Dead cards = hero + board[0:nb] + `dead`; pool = the
 * other cards, P of them, in canonical order value[k] = ((k%4)<<4) | (k/4).
 * A HOLDING is an unordered pair of cards with canonical indices a < b; its index is h = b (b - 1) / 2 + a, 0 .. 1325 (PK_EQ_HOLDINGS),
 * fixed and independent of the spot.  It is VALID when both cards are in the pool.
 * COUNTS: for a valid holding every completion of the board from the pool minus the holding is enumerated -- boards = C(P - 2, 5 - nb) of
 * them, the same for every valid holding of a spot; on each, v = [eval_hand(board + hero), eval_hand(board + holding)] and the winners are
 * compare_rankings(v) as above (the hero is index 0).  win[h] u32 = boards the hero wins alone, tie[h] u32 = boards both win; losses are
 * boards - win - tie, the hero's share is 720720 * win + 360360 * tie (not stored).  Invalid holdings get zeros.
 * RANGE: weights u16 [1326] is optional -- one vector for every spot of the call (weights_per_spot = 0) or one per spot ([m][1326],
 * weights_per_spot = 1); NULL = every weight 1.  agg u64 [3] per spot = sum w[h] win[h], sum w[h] tie[h], boards * sum over the valid h of
 * w[h]; hand strength = (agg[0] + agg[1] / 2) / agg[2], formed by the caller in binary64 (the largest aggregate, 65 535 * 990 * 1 081, fits
 * 64 bits with room).
 * STATUS (u8; a non-zero status gives all-zero outputs and boards = 0, never fails the call, and disturbs no neighbour): PK_EQ_BAD_CARD a
 * byte that is no card, 0xFF anywhere, or a `dead` bit >= 52; PK_EQ_DUP_CARD a card twice among hero and board, or a hero / board card that is
 * also in `dead`; PK_EQ_BAD_NBOARD nb > 5; PK_EQ_PREFLOP nb < 3; PK_EQ_SMALL_POOL P < (5 - nb) + 2 (nb <= 5); the table form also
 * PK_EQ_IN_FLIGHT, PK_EQ_BAD_TABLE and PK_EQ_DUP_CARD for a table never dealt, as pk_table_equity.
 * Any output may be NULL (not wanted); m == 0 is a no-op; m < 2^31; device < PK_MAX_DEVICES.
 * TABLE FORM: observer = a seat p (0 .. N-1) or PK_OBSERVER_ACTIVE (each table's active seat); PK_OBSERVER_NONE is refused with
 * PK_E_INVALID_ARG.  Spot = p's two hole cards plus the board so far (nb as pk_table_equity); dead = 0: p has seen no folded hand, and the
 * board cards the deck already holds for later streets are in the pool.  The question is the same at any seat count -- "against ONE hidden
 * hand" -- and does not look at who is live.  Like the other table forms it completes deferred rollout work, reads only, and runs on the
 * handle's stream.
 * STREAMS and work space: as pk_equity (the device form asynchronous on the stream it is given, the host forms synchronous). */
#define PK_EQ_HOLDINGS 1326
#define PK_EQ_PREFLOP 64u      /* range equity: nb < 3 (out of scope: see above) */
#define PK_EQ_SMALL_POOL 128u  /* range equity: fewer pool cards than the board to come plus one holding */
int pk_equity_range_d(int device, size_t m, const uint8_t *hero_d /*[m][2]*/, const uint8_t *board_d /*[m][5]*/, const uint8_t *nboard_d,
                      const uint64_t *dead_d /*NULL: none*/, const uint16_t *weights_d /*NULL: 1*/, int weights_per_spot,
                      uint64_t *agg_d /*[m][3]*/, uint32_t *win_d /*[m][1326]*/, uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d,
                      void *stream);
int pk_equity_range(int device, size_t m, const uint8_t *hero, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead,
                    const uint16_t *weights, int weights_per_spot, uint64_t *agg, uint32_t *win, uint32_t *tie, uint32_t *boards,
                    uint8_t *status);
int pk_table_equity_range_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, const uint16_t *weights_d, int weights_per_spot,
                            uint64_t *agg_d, uint32_t *win_d, uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d);
int pk_table_equity_range(pk_handle *h, const int32_t *tables, size_t m, int observer, const uint16_t *weights, int weights_per_spot,
                          uint64_t *agg, uint32_t *win, uint32_t *tie, uint32_t *boards, uint8_t *status);
/* ---- Range vs range: the exact result of EVERY holding the hero can have on a public board against a weighted opponent range -- the
 * terminal-node evaluation of a solver.  POST-FLOP ONLY, as range equity.
 *
 * A SPOT is board u8[5] with nb = 3, 4 or 5 known cards and dead u64 (bit k = the card of canonical index k is out of play); there is NO hero.
 * Dead cards = board[0:nb] + `dead`; the pool is the other P cards in canonical order, as above; k = 5 - nb.  A holding (the fixed index
 * h = b (b - 1) / 2 + a above) is VALID when both its cards are in the pool.
 * WEIGHTS: weights u16 [1326] is the opponent's range -- one vector for the call (weights_per_spot = 0) or one per spot ([m][1326]); NULL = all 1.
 * OUTPUTS, three u64 per spot and hero holding h ([m][1326] each; invalid holdings get zeros): take every valid villain holding h' that
 * shares no card with h and every one of the C(P - 4, k) completions of the board from the pool minus h and h'; on each,
 * winners = compare_rankings([eval_hand(board + h), eval_hand(board + h')]) exactly as above, the hero at index 0.  Then
 *   win[h] = sum of w[h'] * (boards the hero wins alone)      tie[h] = sum of w[h'] * (boards both win)
 *   tot[h] = C(P - 4, k) * (sum of w[h'] over the valid h' that share no card with h)
 * and per spot boards u32 = C(P - 4, k), status u8.  Strength[h] = (win + tie / 2) / tot is formed by the caller in binary64 (nan where
 * tot = 0).  The largest value is 65 535 * 1 081 * 990 ~ 7.0e10: u64 holds it; one completion's partial sum, at most 65 535 * 1 081, fits u32.
 * IDENTITY: row h of a spot is the agg[3] that pk_equity_range returns for hero = h with the same board, `dead` and weights.
 * STATUS: the PK_EQ_* bits of range equity, except that there is no hero to be a bad or duplicate card, and PK_EQ_SMALL_POOL is P < k + 4
 * (the pool must hold the board to come and TWO holdings).  A non-zero status gives all-zero outputs and boards = 0, never fails the call and
 * disturbs no neighbour.
 * Any output may be NULL; asking for boards / status alone runs only the preparation kernel.  m == 0 is a no-op; m < 2^31;
 * device < PK_MAX_DEVICES.
 * TABLE FORM: board = the table's board so far (nb as pk_table_equity), dead = 0; no hole card is read and there is no observer.  It
 * completes deferred rollout work, reads only, runs on the handle's stream, and reports PK_EQ_IN_FLIGHT / PK_EQ_BAD_TABLE; a table at turn
 * 0, one never dealt included, is PK_EQ_PREFLOP.
 * STREAMS and work space: as pk_equity_range. */
int pk_equity_rvr_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint8_t *nboard_d, const uint64_t *dead_d /*NULL: none*/,
                    const uint16_t *weights_d /*NULL: 1*/, int weights_per_spot, uint64_t *win_d /*[m][1326]*/, uint64_t *tie_d, uint64_t *tot_d,
                    uint32_t *boards_d, uint8_t *status_d, void *stream);
int pk_equity_rvr(int device, size_t m, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead, const uint16_t *weights,
                  int weights_per_spot, uint64_t *win, uint64_t *tie, uint64_t *tot, uint32_t *boards, uint8_t *status);
int pk_table_equity_rvr_d(pk_handle *h, const int32_t *tables_d, size_t m, const uint16_t *weights_d, int weights_per_spot, uint64_t *win_d,
                          uint64_t *tie_d, uint64_t *tot_d, uint32_t *boards_d, uint8_t *status_d);
int pk_table_equity_rvr(pk_handle *h, const int32_t *tables, size_t m, const uint16_t *weights, int weights_per_spot, uint64_t *win, uint64_t *tie,
                        uint64_t *tot, uint32_t *boards, uint8_t *status);
/* ---- Strength histograms: for EVERY holding the hero can have on a public board, how its RIVER strength against a weighted opponent range
 * is distributed over the completions of the board -- the input of distribution-aware card abstraction and a "hand potential" feature
 * (DESIGN.md section 3.5).  POST-FLOP ONLY, as range equity.
 *
 * SPOT, WEIGHTS, STATUS, TABLE FORM, STREAMS and work space are exactly those of range vs range above: board u8[5] with nb = 3, 4 or 5 known
 * cards, dead u64, no hero; weights u16 [1326] shared or per spot, NULL = all 1; a holding is VALID when both its cards are in the pool of
 * P cards; k = 5 - nb; the PK_EQ_* bits with PK_EQ_SMALL_POOL = P < k + 4.  The same spot gets the same status from both families.
 * NBINS: one per call, 1 .. PK_EQ_HIST_MAX_BINS; anything else is PK_E_INVALID_ARG before any launch.
 * PER valid hero holding h and per completion c -- one of the C(P - 2, k) sets of k cards from the pool minus h: let V(h, c) be the valid
 * holdings that share no card with h or c (never empty: P >= k + 4).  On board + c every h' in V has
 * winners = compare_rankings([eval_hand(board + c + h), eval_hand(board + c + h')]) exactly as above, the hero at index 0, and
 *   below = sum of w[h'] where the hero wins alone     equal = sum of w[h'] where both win     den = sum of w[h'] over V.
 * If den = 0 (the range has no weight left after card removal) void[h] += 1; otherwise, in integers,
 *   bin = min(nbins - 1, floor(nbins * (2 below + equal) / (2 den)))     hist[h][bin] += 1
 * so strength exactly j / nbins lands in bin j and strength 1 in the last bin.  Every product fits 32 bits:
 * 32 * 2 * 65 535 * C(45, 2) = 4 152 297 600 < 2^32 (990 = the most villain holdings that can be live at once).
 * OUTPUTS: hist u16 [m][1326][nbins], void u16 [m][1326] (the largest count is C(47, 2) = 1 081), completions u32 [m] = C(P - 2, k) -- the
 * completions ONE holding meets, NOT the `boards` = C(P - 4, k) of range vs range, which counts per pair of holdings -- and status u8 [m].
 * Invalid holdings and refused spots are all zeros (completions = 0); every entry is written, the caller clears nothing.
 * INVARIANT: for a valid h, sum over b of hist[h][b] + void[h] = completions.
 * IDENTITY: for a completion c, the river spot (board + c, the same dead, the same weights) has the same pool minus c, and row h of its
 * pk_equity_rvr is (win, tie, tot) = (below, equal, den) for every h that shares no card with c: a spot's histogram is the sum over its
 * completions of the one-hot bins of those river rows.  At nb = 5 there is one completion: a single count of 1 per valid holding.
 * Any output may be NULL; asking for completions / status alone runs only the one-lane-per-spot kernels.  m == 0 is a no-op; m < 2^31;
 * device < PK_MAX_DEVICES. */
#define PK_EQ_HIST_MAX_BINS 32
int pk_equity_hist_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint8_t *nboard_d, const uint64_t *dead_d /*NULL: none*/,
                     const uint16_t *weights_d /*NULL: 1*/, int weights_per_spot, int nbins, uint16_t *hist_d /*[m][1326][nbins]*/,
                     uint16_t *void_d /*[m][1326]*/, uint32_t *completions_d, uint8_t *status_d, void *stream);
int pk_equity_hist(int device, size_t m, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead, const uint16_t *weights,
                   int weights_per_spot, int nbins, uint16_t *hist, uint16_t *void_, uint32_t *completions, uint8_t *status);
int pk_table_equity_hist_d(pk_handle *h, const int32_t *tables_d, size_t m, const uint16_t *weights_d, int weights_per_spot, int nbins,
                           uint16_t *hist_d, uint16_t *void_d, uint32_t *completions_d, uint8_t *status_d);
int pk_table_equity_hist(pk_handle *h, const int32_t *tables, size_t m, const uint16_t *weights, int weights_per_spot, int nbins, uint16_t *hist,
                         uint16_t *void_, uint32_t *completions, uint8_t *status);
/* ---- Hero strength histogram: the strength histogram of ONE seat's holding, and optionally its bucket -- "which bucket is the hand of the
 * seat to act in, on each of my tables?" (DESIGN.md section 3.9).  It is row h of "Strength histograms" above for the one holding that is
 * wanted, at the cost of one "Range equity" spot.  POST-FLOP ONLY, as range equity.
 *
 * SPOT, WEIGHTS, STATUS, TABLE FORM, STREAMS: exactly those of "Range equity" above: hero u8[2], board u8[5] with nb = 3, 4 or 5 known cards,
 * dead u64; dead cards = hero + board[0:nb] + `dead`, the pool is the other P cards in canonical order, k = 5 - nb; weights u16 [1326] shared
 * or per spot (weights_per_spot), NULL = all 1; PK_EQ_PREFLOP for nb < 3 and PK_EQ_SMALL_POOL for P < k + 2, so the same spot gets the same
 * status from pk_equity_range and from this family.
 * NBINS: one per call, 1 .. PK_EQ_HIST_MAX_BINS; anything else is PK_E_INVALID_ARG before any launch.
 * PER completion c of the board -- one of the C(P, k) sets of k cards from the pool: let V(c) be the valid holdings (both cards in the pool)
 * that share no card with c.  On board + c every h' in V has winners = compare_rankings([eval_hand(board + c + hero),
 * eval_hand(board + c + h')]) exactly as above, the hero at index 0, and
 *   below = sum of w[h'] where the hero wins alone     equal = sum of w[h'] where both win     den = sum of w[h'] over V.
 * If den = 0, void += 1; otherwise, in integers, bin = min(nbins - 1, floor(nbins * (2 below + equal) / (2 den))) and hist[bin] += 1: the
 * rule of "Strength histograms" word for word; every product fits 32 bits by its bound, and below, equal, den <= 65 535 * 990 fit u32.
 * OUTPUTS (any may be NULL; every entry is written, the caller clears nothing): hist u16 [m][nbins], void u16 [m], completions u32 [m] =
 * C(P, k), status u8 [m].  A refused spot is all zeros.
 * INVARIANT: sum over b of hist[b] + void = completions.
 * IDENTITY: the outputs equal row h = holding index of the hero of pk_equity_hist on the same board, the same `dead` (WITHOUT the hero's
 * cards) and the same weights; that form's completions = C(P' - 2, k) with P' = P + 2 is the same number, and its PK_EQ_SMALL_POOL rule
 * P' < k + 4 the same inequality.
 * BUCKET STAGE (optional, in the same call): K = 0 is none; else K 1 .. PK_CL_MAX_K and centroids u16 [K][nbins] give label u16 [m] and
 * dist u32 [m], each exactly what pk_hist_cluster_assign returns for the m rows hist[m][nbins] of this call against those centroids (the
 * quantised CDF, the L1 distance and the smallest-index rule of "Histogram clustering" below).  An empty row -- a refused spot, pre-flop, or
 * every completion void -- gives PK_CL_NONE and distance 0.  label or dist may be asked for with hist NULL: the rows then live in the work
 * space.  K > 0 with NULL centroids is PK_E_INVALID_ARG, and so is K = 0 with a non-NULL label or dist, and K outside 0 .. PK_CL_MAX_K.
 * m == 0 is a no-op; m < 2^31; device < PK_MAX_DEVICES.  Asking for completions / status alone runs only the one-lane-per-spot kernels.
 * TABLE FORM: as pk_table_equity_range: observer = a seat or PK_OBSERVER_ACTIVE (PK_OBSERVER_NONE is refused); spot = that seat's hole cards
 * plus the board so far, dead = 0; reports PK_EQ_IN_FLIGHT, PK_EQ_BAD_TABLE, and PK_EQ_PREFLOP at turn 0; completes deferred rollout work,
 * reads only, runs on the handle's stream.
 * NOT HERE: pre-flop, the per-completion raw terms as an output, the bucket inside the step kernels' observation rows, multiway hidden hands. */
int pk_equity_hist_hero_d(int device, size_t m, const uint8_t *hero_d /*[m][2]*/, const uint8_t *board_d /*[m][5]*/, const uint8_t *nboard_d,
                          const uint64_t *dead_d /*NULL: none*/, const uint16_t *weights_d /*NULL: 1*/, int weights_per_spot, int nbins,
                          uint16_t *hist_d /*[m][nbins]*/, uint16_t *void_d /*[m]*/, uint32_t *completions_d, uint8_t *status_d, int K /*0: no bucket*/,
                          const uint16_t *centroids_d /*[K][nbins]*/, uint16_t *label_d /*[m]*/, uint32_t *dist_d /*[m]*/, void *stream);
int pk_equity_hist_hero(int device, size_t m, const uint8_t *hero, const uint8_t *board, const uint8_t *nboard, const uint64_t *dead,
                        const uint16_t *weights, int weights_per_spot, int nbins, uint16_t *hist, uint16_t *void_, uint32_t *completions,
                        uint8_t *status, int K, const uint16_t *centroids, uint16_t *label, uint32_t *dist);
int pk_table_equity_hist_hero_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, const uint16_t *weights_d, int weights_per_spot,
                                int nbins, uint16_t *hist_d, uint16_t *void_d, uint32_t *completions_d, uint8_t *status_d, int K,
                                const uint16_t *centroids_d, uint16_t *label_d, uint32_t *dist_d);
int pk_table_equity_hist_hero(pk_handle *h, const int32_t *tables, size_t m, int observer, const uint16_t *weights, int weights_per_spot, int nbins,
                              uint16_t *hist, uint16_t *void_, uint32_t *completions, uint8_t *status, int K, const uint16_t *centroids,
                              uint16_t *label, uint32_t *dist);
/* ---- Showdown EV: "if the cards still to come were dealt now, what does each seat expect to be paid, in chips?" -- the side pots of
 * Game.end_hand (game.py:494-531) enumerated over every board on the device, exact.  pk_equity above answers only the
 * first comparison of end_hand (who wins when every live seat is compared); with unequal stacks the pot is paid out in LEVELS, each judged
 * after the lower bettors' hands have been taken out of the comparison.
 *
 * A SPOT is a "Showdown equity" spot plus bets f64 [N]: what each seat has committed to the pot this hand -- seats that are not live
 * included (a folded seat's money is in the pot).  Dead cards, pool, boards and v[p] per board are exactly those of "Showdown equity".
 * LEVELS depend on bets and live only, never on the board:
 *     order = [p for p in stable_argsort(bets) if live[p]];  work = copy(bets);  remain = set(order)
 *     for i, s in enumerate(order):
 *         if all(work <= 0): break
 *         if len(remain) == 1:  level i: seat s, amount = np.sum(work), LAST;  break                  (the "last stand", game.py:500-505)
 *         mb = clip(work, 0, work[s]);  level i: seat s, amount = np.sum(mb), remain as it is now
 *         remain.remove(s);  work -= mb
 * (np.sum in numpy's association order).  A level that is not reached does not exist: level_seat 0xFF, amount 0.
 * PER BOARD and level i that is not LAST: W_i = compare_rankings(v with every seat outside remain_i set to (NONE, [])), line 148 as it is
 * -- W_i is NOT W_0 restricted to remain_i: the first hand of the best rank class fixes best_kicker, so taking that hand out changes
 * who wins among the rest.
 *   share      u64 [m][N][N]  level-major: share[i][p] = sum of 720720 / |W_i| over the boards with p in W_i; 0 for a level whose amount is 0 or
 *                             that does not exist; for the LAST level 720720 * boards at the level's seat, 0 elsewhere
 *   level_seat u8  [m][N]     the seat visited at level i (0xFF: no such level)        amount  f64 [m][N]
 *   boards     u32 [m]        status  u8 [m]  (the PK_EQ_* bits of "Showdown equity" plus PK_EQ_BAD_BET)
 *   ev         f64 [m][N]     acc = +0.0;  for i ascending: acc = acc + (amount[i] * (double)share[i][p]) / (720720.0 * (double)boards);
 *                             ev[p] = acc - bets[p] -- every operation rounded on its own, nothing fused: bit-identical to that formula
 *                             evaluated in binary64 anywhere.  On a complete board with money of integer value every product is exact and
 *                             ev equals the payoffs Game.end_hand writes, bit for bit.
 * A spot with a non-zero status gets zeros everywhere, boards = 0 and level_seat = 0xFF; it disturbs nothing else.  Any output except
 * `status` may be NULL.  m, device, STREAMS and work space: as pk_equity (the work space also holds the levels, and the share counters
 * when share is NULL); the task bound counts ceil((N - 1) / L) groups of levels per spot (L = 3 up to eight seats, 2 beyond).
 * TABLE FORM: cards, nb and live seats as pk_table_equity (an ACTIVE seat counts as one that shows down: "nobody bets further");
 * bets = bets + pending_bets per seat, one binary64 addition each -- the commit end_hand makes (game.py:457).  Completes deferred rollout
 * work, reads only, runs on the handle's stream; PK_EQ_IN_FLIGHT / PK_EQ_BAD_TABLE / PK_EQ_DUP_CARD per table as pk_table_equity. */
#define PK_EQ_BAD_BET 64u    /* showdown EV: a bet that is negative, NaN or infinite (the value of PK_EQ_PREFLOP, which no EV call reports) */
/* holes_d, board_d, nboard_d, live_d as pk_equity_d; bets_d f64 [m][N]. */
int pk_equity_ev_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                   const uint16_t *live_d, const double *bets_d, uint64_t *share_d, uint8_t *level_seat_d, double *amount_d, double *ev_d,
                   uint32_t *boards_d, uint8_t *status_d, void *stream);
int pk_equity_ev(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
                 const double *bets, uint64_t *share, uint8_t *level_seat, double *amount, double *ev, uint32_t *boards, uint8_t *status);
int pk_table_equity_ev_d(pk_handle *h, const int32_t *tables_d, size_t m, uint64_t *share_d, uint8_t *level_seat_d, double *amount_d, double *ev_d,
                         uint32_t *boards_d, uint8_t *status_d);
int pk_table_equity_ev(pk_handle *h, const int32_t *tables, size_t m, uint64_t *share, uint8_t *level_seat, double *amount, double *ev,
                       uint32_t *boards, uint8_t *status);
/* ---- Ranged showdown EV: "with what I believe about their hands, what am I paid in chips if I call?" -- the side pots of "Showdown EV"
 * over attempts in which every hidden seat draws its holding from a weighted range, as in "Ranged sampled equity" (DESIGN.md section 3.11).
 * Everything not stated here is "Ranged sampled equity" for cards, ranges, attempts and streams, and "Showdown EV" for bets, levels and ev.
 *
 * A SPOT is a "Ranged sampled equity" spot (a live seat shows both hole cards or hides both; weights u16 [R][1326], R <= PK_EQW_MAX_RANGES,
 * range_of u16 per seat) plus bets f64 [N]: what each seat has put into the pot this hand, seats that are not live included.
 * STATUS: the bits of "Ranged sampled equity" plus PK_EQ_BAD_BET (64, free in that family) for a bet that is negative, NaN or infinite, read
 * from its bits (-0.0 is a zero, and is read as +0.0).  A refused spot gets zeros everywhere, level_seat = 0xFF, accepted = 0, and disturbs no neighbour.
 * LEVELS: exactly the loop of "Showdown EV", on bets and live only: the same level_seat u8 [m][N] and amount f64 [m][N].
 * ATTEMPT s of a spot is the attempt of "Ranged sampled equity", verbatim: stream 'EQW0' with the same key, id, nonce and S, the holdings by
 * cumulative search, rejection, the board from word X[H].  For the same arguments the set of accepted attempts, their cards and `accepted`
 * equal those of pk_equity_ranged.
 * PER ACCEPTED ATTEMPT: v[p] = eval_hand(board + hole[p]) for live seats; for every level i that is not LAST and whose amount is > 0:
 * W_i = compare_rankings(v with every seat outside remain_i set to (NONE, [])), share[i][p] += 720720 / |W_i| for p in W_i.  The LAST level
 * gets 720720 * accepted at its seat.  A level with amount 0, or that does not exist, stays 0.
 *   share      u64 [m][N][N]  level-major          level_seat u8 [m][N]     amount f64 [m][N]
 *   accepted   u32 [m]                             status     u8 [m]
 *   ev         f64 [m][N]     acc = +0.0;  for i ascending: acc = acc + (amount[i] * (double)share[i][p]) / (720720.0 * (double)accepted);
 *                             ev[p] = acc - bets[p] -- every operation rounded on its own.  With accepted == 0 the ev row is +0.0: status 0,
 *                             no estimate, the caller reads `accepted`.
 * `status` may not be NULL; every other output may.  S = 1 .. 2^24; m * ceil(S / 64) * G must fit 32 bits, G = ceil((N - 1) / L) groups of
 * levels (L = 3 up to eight seats, 2 beyond): otherwise PK_E_INVALID_ARG.  num_ranges > PK_EQW_MAX_RANGES, or > 0 with weights NULL:
 * PK_E_INVALID_ARG before any launch.  share and accepted of calls with different nonces add exactly; ev of the sum is the formula applied to
 * the summed counts (formed by the caller).
 * TABLE FORM: observer is a seat or PK_OBSERVER_ACTIVE (PK_OBSERVER_NONE: PK_E_INVALID_ARG); cards and live seats are exactly
 * pk_table_equity_ranged's spot for that observer (folded seats are not dead and not read); bets = bets + pending_bets per seat, one binary64
 * addition each, as pk_table_equity_ev; range_of u16 [N], or [m][N] with range_per_table.  Completes deferred rollout work, reads only, runs on
 * the handle's stream; PK_EQ_IN_FLIGHT / PK_EQ_BAD_TABLE / PK_EQ_DUP_CARD per table; PK_EQ_BAD_BET can be met through the negative-credit
 * quirk of "Showdown EV".  STREAMS and work space: as pk_equity_ranged; the work space also holds the levels, the bets, the amounts, and
 * share / accepted when they are NULL. */
int pk_ev_ranged_d(int device, int num_players, size_t m, const uint8_t *holes_d, const uint8_t *board_d, const uint8_t *nboard_d,
                   const uint16_t *live_d, const double *bets_d /*[m][N]*/, const uint32_t *ids_d /* NULL: i */, uint32_t samples, uint64_t seed,
                   uint32_t nonce, const uint16_t *weights_d /*[R][1326]*/, uint32_t num_ranges, const uint16_t *range_of_d /*[m][N], NULL: uniform*/,
                   uint64_t *share_d, uint8_t *level_seat_d, double *amount_d, double *ev_d, uint32_t *accepted_d, uint8_t *status_d, void *stream);
int pk_ev_ranged(int device, int num_players, size_t m, const uint8_t *holes, const uint8_t *board, const uint8_t *nboard, const uint16_t *live,
                 const double *bets, const uint32_t *ids /* NULL: i */, uint32_t samples, uint64_t seed, uint32_t nonce, const uint16_t *weights,
                 uint32_t num_ranges, const uint16_t *range_of, uint64_t *share, uint8_t *level_seat, double *amount, double *ev, uint32_t *accepted,
                 uint8_t *status);
int pk_table_ev_ranged_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, uint32_t samples, uint32_t nonce, const uint16_t *weights_d,
                         uint32_t num_ranges, const uint16_t *range_of_d, int range_per_table, uint64_t *share_d, uint8_t *level_seat_d,
                         double *amount_d, double *ev_d, uint32_t *accepted_d, uint8_t *status_d);
int pk_table_ev_ranged(pk_handle *h, const int32_t *tables, size_t m, int observer, uint32_t samples, uint32_t nonce, const uint16_t *weights,
                       uint32_t num_ranges, const uint16_t *range_of, int range_per_table, uint64_t *share, uint8_t *level_seat, double *amount,
                       double *ev, uint32_t *accepted, uint8_t *status);
/* ---- Histogram clustering: bucket strength histograms on the device -- exact k-means under the earth mover's distance (DESIGN.md section
 * 3.8).  Everything is an integer; the device equals the numpy restatement tests/hist_cluster_spec.py bit for bit.
 *
 * POINTS: hist u16 [n][nbins], any rows -- for example an [m][1326][nbins] output of pk_equity_hist_d viewed flat; nbins 1 ..
 * PK_EQ_HIST_MAX_BINS, n 1 .. 2^31 - 1.  The mass of row i is m_i = sum over b of hist[i][b]; a row with m_i = 0 is EMPTY (invalid holdings
 * and refused spots are exactly these rows): label PK_CL_NONE, distance 0, it takes part in nothing.
 * QUANTISED CDF: q[i][b] = floor(65535 * (hist[i][0] + ... + hist[i][b]) / m_i) as u16 (a 64-bit division, once per row and bin);
 * q[i][nbins - 1] = 65535 always.
 * DISTANCE: d(i, c) = sum over b of |q[i][b] - C[c][b]|, a u32 of at most 32 * 65535; d / 65535 is the earth mover's distance in bin units
 * (histogram_emd's unit).  Against a centroid that is another row's q: |d / 65535 - histogram_emd| < nbins / 65535.
 * CENTROIDS: C u16 [K][nbins], K 1 .. PK_CL_MAX_K.
 * ASSIGN: label[i] = the SMALLEST c among those that minimise d(i, c); dist[i] = that d.
 * UPDATE: n_c = rows with label c, S_c[b] = sum of q[i][b] over them (u64); C[c][b] = floor((S_c[b] + floor(n_c / 2)) / n_c); a cluster with
 * n_c = 0 keeps its centroid.
 * ONE ITERATION t = assign, then update from those labels; inertia[t] = sum of dist, changed[t] = labels that differ from the iteration
 * before (the first iteration counts every non-empty row).  pk_hist_cluster runs EXACTLY `iters` iterations (1 .. 1024) and then one final
 * assign -- inertia[iters] is its sum --, so the returned labels belong to the returned centroids.  changed = 0 is a fixed point: later
 * iterations change nothing.  Inertia is NOT monotone (the mean does not minimise L1, and the centroids are rounded).
 * SEEDING (k-means++ with LINEAR weights, exact): rounds j = 0 .. K - 1.  Round 0: w_i = 1 for a non-empty row, 0 for an empty one; later
 * rounds: w_i = the smallest d(i, .) to the centroids chosen so far.  W = sum of w_i (fits u64 for every legal n);  r = (x * W) >> 64 with
 * x = w0 | w1 << 32 of the Philox4x32-10 block with key (seed & 0xffffffff, seed >> 32) -- as pk_create -- and counter (j, 0, 'CLS0' =
 * 0x434C5330, nonce); the chosen row is the smallest i whose inclusive prefix sum of w exceeds r, and its q becomes C[j].  W = 0 (every
 * non-empty row coincides with a centroid): the lowest-index non-empty row.
 * ERRORS, PK_E_INVALID_ARG before any launch: nbins, K, iters or n out of range, a NULL array that is needed; for seeding and clustering,
 * whose centroids come from rows, also K > n, and in their host forms K larger than the number of non-empty rows (they see the rows).
 * ASSIGN takes any n >= 1 with any K: one histogram against 4 096 centroids is its ordinary use.  The _d forms of seeding and clustering
 * run asynchronously and cannot see the rows: THE CALLER MUST GUARANTEE AT LEAST ONE NON-EMPTY ROW.  With fewer non-empty rows than K the
 * W = 0 rule repeats a row; with none pk_hist_cluster_seed_d still returns PK_OK and leaves centroids_d UNWRITTEN -- pk_hist_cluster_d
 * would then iterate on whatever that buffer held.
 * label u16 [n], dist u32 [n] (NULL: not wanted), inertia u64 [iters + 1], changed u32 [iters] (either NULL: not wanted).  The _d forms run
 * asynchronously on `stream`; work space (q, the packed centroids, the seeding's distances and partial sums, the update's sums and counts)
 * is the grow-only per-(device, stream) buffer of pk_equity_d.  The host forms are synchronous on a pooled stream.  Launches: seeding 1 + 2 K,
 * assign 3, clustering 2 + 3 iters + 1.  NOT HERE: per-row multiplicities, squared distances, k-medians, a table form. */
#define PK_CL_MAX_K 4096
#define PK_CL_NONE 0xFFFFu
int pk_hist_cluster_seed_d(int device, size_t n, int nbins, const uint16_t *hist_d, int K, uint64_t seed, uint32_t nonce,
                           uint16_t *centroids_d /*[K][nbins]*/, void *stream);
int pk_hist_cluster_assign_d(int device, size_t n, int nbins, const uint16_t *hist_d, int K, const uint16_t *centroids_d, uint16_t *label_d,
                             uint32_t *dist_d /*NULL ok*/, void *stream);
int pk_hist_cluster_d(int device, size_t n, int nbins, const uint16_t *hist_d, int K, uint16_t *centroids_d /*in: seeds, out: result*/, int iters,
                      uint16_t *label_d, uint32_t *dist_d, uint64_t *inertia_d /*[iters+1], last = final assign*/, uint32_t *changed_d /*[iters]*/,
                      void *stream);
int pk_hist_cluster_seed(int device, size_t n, int nbins, const uint16_t *hist, int K, uint64_t seed, uint32_t nonce, uint16_t *centroids);
int pk_hist_cluster_assign(int device, size_t n, int nbins, const uint16_t *hist, int K, const uint16_t *centroids, uint16_t *label,
                           uint32_t *dist);
int pk_hist_cluster(int device, size_t n, int nbins, const uint16_t *hist, int K, uint16_t *centroids, int iters, uint16_t *label,
                    uint32_t *dist, uint64_t *inertia, uint32_t *changed);
/* ---- Pre-flop matchups: the exact result of every ordered pair of holdings over every five-card board, counted on the device, and the
 * pre-flop forms of range equity and range vs range that read it.  Every other hidden-hand family refuses nb < 3
 * (PK_EQ_PREFLOP) and keeps doing so; these entry points are the pre-flop capability.
 *
 * Cards by canonical index k = rank0 * 4 + suit, value[k] = ((k%4)<<4) | (k/4); holdings h = b (b - 1) / 2 + a over a < b, 0 .. 1325, as
 * above.  The two-seat result is decided by the ORDER KEY of section 3.4 (larger key wins, equal keys tie): exactly the winners of
 * compare_rankings([eval_hand(board + h), eval_hand(board + o)]).  BOARDS are the 5-subsets of the canonical indices 0 .. 51 in
 * lexicographic order (itertools.combinations(range(52), 5)); a board's rank r runs over 0 .. 2 598 959 (PK_PREFLOP_ALL_BOARDS).
 * PARTIAL COUNTS over the board range [first, first + n), for every ordered pair (h, o) of holdings that share no card:
 *   win[h][o] = boards b of the range with b disjoint from h and o on which h wins alone,   tie[h][o] = such boards on which both win;
 * pairs that share a card, the diagonal included, get 0.  Both are u32 [1326][1326]; either may be NULL.  accumulate != 0 ADDS the counts to
 * what the arrays hold; otherwise the arrays are overwritten, zeros included (no memset is needed).  Counts over disjoint ranges add exactly.
 * first + n > PK_PREFLOP_ALL_BOARDS is PK_E_INVALID_ARG; n = 0 writes nothing.  The evaluator's suit quirks are carried by the keys: no
 * suit symmetry is assumed anywhere, and the table is NOT invariant under a renaming of suits.
 * THE MATCHUP TABLE is the partial count over all boards.  For disjoint (h, o): win[h][o] + tie[h][o] + win[o][h] = 1 712 304
 * (PK_PREFLOP_BOARDS = C(48, 5)); tie[h][o] = tie[o][h]; (win[h][o], tie[h][o]) are win[0], tie[0] of pk_equity on the two-seat spot [h, o],
 * nb = 0, live = 3, bit for bit.  It is built once per device on first use, on the stream of the call that needs it (as the evaluator
 * table is), and stays resident: 2 x 7.03 MB (the build's own key work space, 92 MB at the default chunk, is freed when the table stands).
 * pk_preflop_matchups copies it out (either output may be NULL).  A call of the two families below that asks for boards / status alone
 * neither reads nor builds it.
 * PRE-FLOP RANGE EQUITY is range equity with nb = 0, dead = 0.  A spot is hero u8[2]; per spot win / tie u32 [1326] = row
 * holding_index(hero) of the table, agg u64 [3] = sum w[o] win[o], sum w[o] tie[o], boards * sum of w[o] over the o that share no card with
 * the hero, boards u32 = 1 712 304 (0 when refused), status u8: PK_EQ_BAD_CARD a byte that is no card (0xFF too), PK_EQ_DUP_CARD the same
 * card twice; the table form also PK_EQ_IN_FLIGHT, PK_EQ_BAD_TABLE and PK_EQ_DUP_CARD for a table never dealt.  A non-zero status gives
 * all-zero outputs, never fails the call and disturbs no neighbour.  Weights as range equity (u16 [1326] shared or [m][1326], NULL = ones);
 * the largest aggregate, 65 535 * 1 225 * 1 712 304 ~ 1.4e14, fits u64.  TABLE FORM: observer = a seat or PK_OBSERVER_ACTIVE
 * (PK_OBSERVER_NONE is refused); the spot is the observer's two hole cards AT WHATEVER TURN THE TABLE RESTS -- the board is not read: the
 * starting-hand strength, a feature that stays meaningful later in the hand.
 * PRE-FLOP RANGE VS RANGE: a spot is one weight row u16 [1326] (weights NULL: every row all ones); per spot and hero holding h, u64 [m][1326]:
 *   win[h] = sum w[o] M.win[h][o],   tie[h] = sum w[o] M.tie[h][o],   tot[h] = 1 712 304 * (sum of w[o] over the o that share no card with h).
 * Row h equals the agg of pre-flop range equity for hero = h with the same weights.  There is no table form (no board, no observer).
 * Any output may be NULL; a call with no spot writes nothing; m < 2^31; device < PK_MAX_DEVICES.  STREAMS and work space: as pk_equity; the
 * count pass's work space (the keys of one chunk of boards, PK_PFM_CHUNK = 1 .. 65 536 boards, default 16 384) is a grow-only piece of
 * it; no launch ranks more boards than one chunk. */
#define PK_PREFLOP_BOARDS 1712304u
#define PK_PREFLOP_ALL_BOARDS 2598960u
int pk_preflop_count_d(int device, uint32_t first, uint32_t n, int accumulate, uint32_t *win_d /*[1326][1326]*/, uint32_t *tie_d, void *stream);
int pk_preflop_count(int device, uint32_t first, uint32_t n, int accumulate, uint32_t *win, uint32_t *tie);
int pk_preflop_matchups_d(int device, uint32_t *win_d /*[1326][1326]*/, uint32_t *tie_d, void *stream);
int pk_preflop_matchups(int device, uint32_t *win, uint32_t *tie);
int pk_equity_preflop_d(int device, size_t m, const uint8_t *hero_d /*[m][2]*/, const uint16_t *weights_d /*NULL: 1*/, int weights_per_spot,
                        uint64_t *agg_d /*[m][3]*/, uint32_t *win_d /*[m][1326]*/, uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d,
                        void *stream);
int pk_equity_preflop(int device, size_t m, const uint8_t *hero, const uint16_t *weights, int weights_per_spot, uint64_t *agg, uint32_t *win,
                      uint32_t *tie, uint32_t *boards, uint8_t *status);
int pk_table_equity_preflop_d(pk_handle *h, const int32_t *tables_d, size_t m, int observer, const uint16_t *weights_d, int weights_per_spot,
                              uint64_t *agg_d, uint32_t *win_d, uint32_t *tie_d, uint32_t *boards_d, uint8_t *status_d);
int pk_table_equity_preflop(pk_handle *h, const int32_t *tables, size_t m, int observer, const uint16_t *weights, int weights_per_spot,
                            uint64_t *agg, uint32_t *win, uint32_t *tie, uint32_t *boards, uint8_t *status);
int pk_equity_rvr_preflop_d(int device, size_t m, const uint16_t *weights_d /*[m][1326]; NULL: 1*/, uint64_t *win_d /*[m][1326]*/, uint64_t *tie_d,
                            uint64_t *tot_d, void *stream);
int pk_equity_rvr_preflop(int device, size_t m, const uint16_t *weights, uint64_t *win, uint64_t *tie, uint64_t *tot);

/* ---- River solver: heads-up CFR+ over a caller's betting tree on a complete board, exact integers (the numpy
 * restatement: tests/river_solver_spec.py).  No result depends on the order of a sum, so the output is the same bytes whatever the grid.
 * PLAYERS AND RANGES: two players, five board cards, an optional `dead` mask as in range vs range.  Player 0 acts first.  ranges u16
 * [m][2][1326] over the holding index.  A holding with a board or dead card is INVALID: its weight is ignored and every output at it is 0.
 * P = pool cards <= 47.
 * TREE: one per call, shared by the m spots, in HOST memory in every form (it travels with the launch).  n nodes, 1 <= n <= 64; kind u8 [n]:
 * 0 / 1 = player 0 / 1 to act, 2 / 3 = player 0 / 1 has folded, 4 = showdown; child u8 [n][4]: a decision node's 1 .. 4 children packed
 * first, then 0xFF; put u32 [n][2]: chips each player has put in since the subgame's root; pot u32: chips in the middle at the root.
 * D = number of decision nodes; the d-th decision node in index order is row d of `strategy`.  Refused with PK_E_INVALID_ARG before any
 * device is looked at: the root is not a decision node; a child index <= its parent or >= n; a non-root node without exactly one parent; a
 * terminal with a child; a decision node without one; a showdown with put[0] != put[1]; pot + max put > 8191; iters outside 1 .. 4096; a NULL
 * pointer where one is required (board, ranges, kind, child, put, status).
 * UNITS: ONE = 32768 (Q15).  Root reach r_p[0][h] = w_p[h] << 4 for valid h, else 0.  Utilities are in half-chips x opponent reach.
 * q = 1 - p throughout.
 * STRATEGY FROM NON-NEGATIVE INTEGERS X[a] (the regrets, and at the end the average accumulators) at a node with nact actions: mx = max X;
 * if mx = 0, sigma_a = ONE / nact (floor) for a >= 1; otherwise sh = max(0, bitlen(mx) - 31), X' = X >> sh, S = sum X', sigma_a =
 * (X'_a << 15) / S (floor) for a >= 1; in both cases sigma_0 = ONE - sum_{a >= 1} sigma_a.
 * ONE TREE PASS WITH STRATEGIES sigma.  DOWN, in index order, at a decision node n of actor p: r_p[c_a][h] = (r_p[n][h] sigma[n][a][h])
 * >> 15, and r_q is copied.  TERMINALS: sums over the valid h' that share no card with h; `compare` is the two-seat decision of range vs
 * range.  S_q(h) = sum r_q[n][h']; W_q(h), T_q(h), L_q(h) = the same sum over the h' that h beats, ties, loses to.  Fold by f:
 * u_f[h] = -2 put[f] S_q(h) and u_{1-f}[h] = 2 (pot + put[f]) S_q(h).  Showdown, c = put[0]: u_p[h] = 2 (pot + c) W_q(h) + pot T_q(h)
 * - 2 c L_q(h).  UP, in reverse index order, at a decision node of actor p: u_p[n][h] = floor(sum_a sigma[n][a][h] u_p[c_a][h] / 32768),
 * the sum first and the floor once; u_q[n][h] = sum_a u_q[c_a][h].
 * ITERATIONS t = 1 .. iters, both players updated from the same pass (simultaneous CFR+): sigma from the regrets R (which start at 0), one
 * pass, then at every decision node n of actor p, action a, valid h: R[n][a][h] = max(0, R[n][a][h] + u_p[c_a][h] - u_p[n][h]) and
 * A[n][a][h] += t r_p[c_a][h].
 * OUTPUTS, each optional except status: strategy u16 [m][D][4][1326] = the strategy rule applied to A (unused action slots and invalid holdings 0; a
 * valid holding of weight 0, like any holding whose accumulators are all 0, gets the uniform row); value i64 [m][2][1326] = u_p[root] of one
 * pass in which every node plays `strategy`; br i64 [m][2][1326] = for each p, u_p[root] of a pass with `strategy` in which p's reach is
 * copied unchanged at p's own nodes, u_p[n][h] = max_a u_p[c_a][h] there, and everything of q is ignored; status u8 [m]: PK_EQ_BAD_CARD
 * (a `dead` bit >= 52 too), PK_EQ_DUP_CARD, PK_EQ_SMALL_POOL for P < 4.  A refused spot gives all-zero outputs and disturbs no neighbour;
 * a call with no spot writes nothing.
 * BOUNDS: reaches < 2^20 and their sums < 2^31; |u| < 2^45, so |sigma u| < 2^60; |R| < 2^58 after 4096 iterations; A < 2^44.  Everything
 * fits int64_t.  STREAMS and work space: as pk_equity; the work space is the descriptors plus a slice per RESIDENT workgroup (at most 256):
 * 47 872 bytes per tree node.  There is no table form: a tree carries absolute chips. */
#define PK_RS_MAX_NODES 64
#define PK_RS_MAX_ITERS 4096
#define PK_RS_MAX_CHIPS 8191u
#define PK_RS_ONE 32768u
int pk_solve_river_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                     const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t n, const uint8_t *kind /*[n], host*/, const uint8_t *child /*[n][4], host*/,
                     const uint32_t *put /*[n][2], host*/, uint32_t pot, uint32_t iters, uint16_t *strategy_d /*[m][D][4][1326]*/,
                     int64_t *value_d /*[m][2][1326]*/, int64_t *br_d, uint8_t *status_d, void *stream);
int pk_solve_river(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t n, const uint8_t *kind,
                   const uint8_t *child, const uint32_t *put, uint32_t pot, uint32_t iters, uint16_t *strategy, int64_t *value, int64_t *br,
                   uint8_t *status);

/* ---- Turn solver: heads-up CFR+ on a FOUR-card board through the river card, exact integers (the numpy
 * restatement: tests/turn_solver_spec.py).  The river solver's definition holds wherever nothing is said here; no result depends on the
 * order of a sum, so the output is the same bytes whatever the grid.
 * SPOT: board u8 [m][4], optional dead u64 [m], ranges u16 [m][2][1326].  P = 52 - 4 - |dead| pool cards <= 48: at most 1128 valid
 * holdings.  status: PK_EQ_BAD_CARD, PK_EQ_DUP_CARD, PK_EQ_SMALL_POOL for P < 5 (two disjoint holdings and one river card).
 * TREE: as the river solver's, n <= 128, plus kind 5 = CHANCE (the river card is dealt): exactly one child, put[0] == put[1] at it, no
 * chance node below a chance node.  Nodes not below a chance node are TURN-LEVEL, the others RIVER-LEVEL.  A showdown must be river-level
 * (an all-in call on the turn is a chance node whose child is a showdown); folds may be at either level.  D_t / D_r = the number of
 * turn-level / river-level decision nodes, each counted in index order.  Refused as the river solver's trees are, and: n outside 1 .. 128;
 * a node kind outside 0 .. 5; a chance node without exactly one child; a chance node below a chance node; a turn-level showdown; a chance
 * node with put[0] != put[1].
 * UNITS: ONE = 32768.  Root reach r_p[0][h] = w_p[h] << 1 (NOT << 4: see BOUNDS).  At a chance node, for each river card c of the pool, the
 * child gets r_p[h] at the holdings without c and 0 at the others, for both players; everything below it under c is the river solver's
 * pass on the board + c.  On the way up u_p[chance][h] = sum over c not in h of u_p[child under c][h]: a plain sum, never an average.  Two
 * disjoint holdings always leave exactly P - 4 river cards, so every utility is in half-chips x opponent reach x (P - 4), and a TURN-LEVEL
 * fold by f is scaled to agree: u_f[h] = -2 put[f] (P - 4) S_q(h), u_{1-f}[h] = 2 (pot + put[f]) (P - 4) S_q(h).
 * ITERATIONS: the river solver's rule, regret and accumulator updates; a river-level decision node has its R and A PER RIVER CARD.  A
 * best-response pass of p takes the maximum per river card below the chance node, then sums.
 * OUTPUTS, each optional except status: strategy u16 [m][D_t][4][1326]; river_strategy u16 [m][D_r][52][4][1326], indexed by the river
 * card's canonical index, 0 for cards outside the pool and for holdings with the card (551 616 bytes per river-level decision node and
 * spot); value, br i64 [m][2][1326]; status u8 [m].  A refused spot gives all-zero outputs and disturbs no neighbour; a call with no spot
 * writes nothing.
 * BOUNDS: a reach < 2^17 (65535 << 1); a sum of reaches < 1128 * 2^17 < 2^27.2; a terminal's |u| <= 2 * 8191 * that < 2^41.2; at the
 * chance node, 44 river cards: |u| < 2^46.7; |sum sigma u| < 2^61.7 (x ONE; the sigma of a node sum to ONE, so the sum is no larger than
 * ONE times the largest |u|); a regret grows by at most 2 max|u| < 2^47.7 an iteration, so |R| < 2^59.7 after 4096; A <= sum t * reach <
 * 2^23 * 2^17 = 2^40 < 2^41.  Everything fits int64_t; with << 4 the sigma u sum would not.  The packed prefix sums keep both players'
 * sums of reaches below 2^32 each.
 * STREAMS and work space: as pk_equity; the work space is the descriptors plus a slice per RESIDENT workgroup, sized for P = 48 whatever the
 * spots: 423 936 bytes of per-card tables, 50 688 bytes per turn-level node and 866 048 bytes per river-level node; the grid is
 * min(m, 256, 4 GiB / slice). */
#define PK_TS_MAX_NODES 128
int pk_solve_turn_d(int device, size_t m, const uint8_t *board_d /*[m][4]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                    const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t n, const uint8_t *kind /*[n], host*/, const uint8_t *child /*[n][4], host*/,
                    const uint32_t *put /*[n][2], host*/, uint32_t pot, uint32_t iters, uint16_t *strategy_d /*[m][D_t][4][1326]*/,
                    uint16_t *river_strategy_d /*[m][D_r][52][4][1326]*/, int64_t *value_d /*[m][2][1326]*/, int64_t *br_d, uint8_t *status_d,
                    void *stream);
int pk_solve_turn(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t n, const uint8_t *kind,
                  const uint8_t *child, const uint32_t *put, uint32_t pot, uint32_t iters, uint16_t *strategy, uint16_t *river_strategy,
                  int64_t *value, int64_t *br, uint8_t *status);
/* The grid pk_solve_turn uses for m spots of a tree with nt turn-level and nr river-level nodes (no output depends on it). */
unsigned pk_turn_grid(size_t m, uint32_t nt, uint32_t nr);

/* ---- River and turn solvers: a tree per spot.  The four calls below take `ntrees` trees and, per spot, the index
 * of its tree: spots of different pots, stacks, bet sizes and raise caps are solved in ONE call.
 * DEFINITION: spot i's outputs are byte for byte what pk_solve_river / pk_solve_turn give for that spot alone with tree tree_of[i]; only
 * the row strides of the strategies are the call's (below).
 * TREES: 1 <= ntrees <= PK_RS_MAX_TREES, in HOST memory in every form.  Tree k is row k of each array -- n u32 [ntrees], kind u8
 * [ntrees][64] (turn: [ntrees][128]), child u8 [ntrees][64][4], put u32 [ntrees][64][2], pot u32 [ntrees] -- and the entries past n[k] are
 * ignored.  EVERY tree passes the check of the one-tree call, whether or not a spot names it; a bad tree is PK_E_INVALID_ARG before any
 * device is looked at, with the one-tree call's text after "tree <k>: ".  ntrees out of range and a NULL n, pot or tree_of are refused the
 * same way.  The trees are packed on the host and copied to the device with the call: in the _d forms the caller may overwrite the host
 * tree arrays as soon as the call returns.
 * tree_of u32 [m]: in DEVICE memory in the _d forms, on the host otherwise.  A spot whose tree_of is >= ntrees reports PK_EQ_BAD_TREE,
 * gets all-zero outputs and disturbs no neighbour.
 * STRIDES: Dmax (river), Dtmax and Drmax (turn) are the largest D, D_t and D_r over ALL trees passed (pk_rs_trees_rows / pk_ts_trees_rows
 * compute them): strategy is u16 [m][Dmax][4][1326] (turn: [m][Dtmax][4][1326]), river_strategy u16 [m][Drmax][52][4][1326]; a spot's
 * rows at or past its own tree's count are written 0.
 * WORK SPACE: a workgroup's slice is sized for the largest tree of the call (the turn grid too: pk_turn_grid(m, max nt, max nr)), plus
 * the packed trees (968 / 2 192 bytes each).  Spots are dealt to workgroups by a fixed stride, whatever their trees' sizes. */
#define PK_RS_MAX_TREES 65536
#define PK_EQ_BAD_TREE 32u   /* a tree per spot: tree_of is >= ntrees (the value of PK_EQ_BAD_TABLE, which no spot form reports) */
int pk_solve_river_trees_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                           const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                           const uint8_t *kind /*[ntrees][64], host*/, const uint8_t *child /*[ntrees][64][4], host*/,
                           const uint32_t *put /*[ntrees][64][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                           const uint32_t *tree_of_d /*[m], DEVICE*/, uint32_t iters, uint16_t *strategy_d /*[m][Dmax][4][1326]*/,
                           int64_t *value_d /*[m][2][1326]*/, int64_t *br_d, uint8_t *status_d, void *stream);
int pk_solve_river_trees(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                         const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                         const uint32_t *tree_of /*[m], host*/, uint32_t iters, uint16_t *strategy, int64_t *value, int64_t *br, uint8_t *status);
int pk_solve_turn_trees_d(int device, size_t m, const uint8_t *board_d /*[m][4]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                          const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                          const uint8_t *kind /*[ntrees][128], host*/, const uint8_t *child /*[ntrees][128][4], host*/,
                          const uint32_t *put /*[ntrees][128][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                          const uint32_t *tree_of_d /*[m], DEVICE*/, uint32_t iters, uint16_t *strategy_d /*[m][Dtmax][4][1326]*/,
                          uint16_t *river_strategy_d /*[m][Drmax][52][4][1326]*/, int64_t *value_d /*[m][2][1326]*/, int64_t *br_d,
                          uint8_t *status_d, void *stream);
int pk_solve_turn_trees(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                        const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                        const uint32_t *tree_of /*[m], host*/, uint32_t iters, uint16_t *strategy, uint16_t *river_strategy, int64_t *value,
                        int64_t *br, uint8_t *status);
/* The row strides of the calls above: the largest number of decision nodes (turn: of turn-level and of river-level ones) over the trees.
 * They look at kind (and child) only; PK_E_INVALID_ARG for ntrees out of range, a NULL pointer, an n[k] out of range or (turn) a child index <= its parent or >= n[k]. */
int pk_rs_trees_rows(uint32_t ntrees, const uint32_t *n, const uint8_t *kind, uint32_t *Dmax);
int pk_ts_trees_rows(uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child, uint32_t *Dtmax, uint32_t *Drmax);

/* ---- Locked nodes: the river and turn solvers with rows of the strategy FIXED by the caller (the numpy restatement:
 * tests/solver_lock_spec.py).  "How exploitable is my policy here?", "he never bluff-raises; what do I do?", and a solution fed back into a
 * later call.  Everything of "River solver", "Turn solver" and "a tree per spot" holds except what is said here.
 * A call carries, beside the arguments of pk_solve_river_trees / pk_solve_turn_trees:
 *   lock   u8  [m][Dmax]            nonzero: row d of spot i is LOCKED (turn: the turn-level rows, stride Dtmax)
 *   locked u16 [m][Dmax][4][1326]   the layout and strides of the `strategy` output of the tree-per-spot calls
 *   river_lock u8 [m][Drmax], river_locked u16 [m][Drmax][52][4][1326] (turn only): the river-level rows, in the layout of river_strategy;
 *                                   a river-level row is locked for all river cards at once.
 * lock == NULL: nothing is locked and `locked` is not looked at; the same holds for the river_ pair.
 * DEFINITION: at a locked decision node n (row d, actor p), for every valid holding h, sigma[n][.][h] = the STRATEGY rule of "River solver"
 * applied to X[a] = locked[i][d][a][h] for a < nact, in every pass of every iteration and in the final passes: the uniform row where all X
 * are 0, otherwise sigma_a = (X_a << 15) // sum X for a >= 1 and sigma_0 = ONE - sum_{a >= 1} sigma_a (the rule's shift is 0 for 16-bit X).
 * So a row of a previous `strategy` output is reproduced unchanged (it sums to ONE), any non-negative weights are accepted, and X and 2X
 * give the same sigma.  NOT READ: action slots >= nact; invalid holdings; rows whose flag is 0; rows at or past the spot's own D; for the
 * turn solver, cards outside the pool and holdings that contain the river card.  Neither R nor A is updated at a locked node.  The
 * `strategy` / `river_strategy` output at a locked row is the sigma played.
 * value and br are defined as before on the final profile.  br IGNORES the locks: p maximises at all of its own nodes, so the
 * exploitability is that of the profile as played.
 * iters may be 0 .. PK_RS_MAX_ITERS in these calls (the calls above keep refusing 0).  With 0 iterations every free row is the uniform
 * row, because A = 0.  All rows locked with iters = 0 is a pure evaluation of a supplied strategy; all rows of q locked is the
 * best-response computation against q.  The BOUNDS are unchanged, because a locked sigma sums to ONE.
 * `locked` must not overlap an output: equal `locked` and `strategy` pointers are PK_E_INVALID_ARG, as is a non-NULL `lock` with a NULL
 * `locked`; the same for the river_ pair.
 * ONE FORM, the tree-per-spot form; ntrees = 1 with tree_of == NULL means every spot uses tree 0, which is the one-tree case.  The trees
 * are checked and packed as in the calls above, with their texts.  In the _d forms the lock arrays are DEVICE memory.  Status values and
 * the refused-spot rule are unchanged; a refused spot's lock data is never read. */
int pk_solve_river_locked_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                            const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                            const uint8_t *kind /*[ntrees][64], host*/, const uint8_t *child /*[ntrees][64][4], host*/,
                            const uint32_t *put /*[ntrees][64][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                            const uint32_t *tree_of_d /*[m], DEVICE; NULL with ntrees = 1: tree 0*/, uint32_t iters,
                            const uint8_t *lock_d /*[m][Dmax], DEVICE; NULL: none*/, const uint16_t *locked_d /*[m][Dmax][4][1326], DEVICE*/,
                            uint16_t *strategy_d /*[m][Dmax][4][1326]*/, int64_t *value_d /*[m][2][1326]*/, int64_t *br_d, uint8_t *status_d,
                            void *stream);
int pk_solve_river_locked(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                          const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                          const uint32_t *tree_of /*[m], host; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock,
                          const uint16_t *locked, uint16_t *strategy, int64_t *value, int64_t *br, uint8_t *status);
int pk_solve_turn_locked_d(int device, size_t m, const uint8_t *board_d /*[m][4]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                           const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                           const uint8_t *kind /*[ntrees][128], host*/, const uint8_t *child /*[ntrees][128][4], host*/,
                           const uint32_t *put /*[ntrees][128][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                           const uint32_t *tree_of_d /*[m], DEVICE; NULL with ntrees = 1: tree 0*/, uint32_t iters,
                           const uint8_t *lock_d /*[m][Dtmax], DEVICE; NULL: none*/, const uint16_t *locked_d /*[m][Dtmax][4][1326], DEVICE*/,
                           const uint8_t *river_lock_d /*[m][Drmax], DEVICE; NULL: none*/,
                           const uint16_t *river_locked_d /*[m][Drmax][52][4][1326], DEVICE*/, uint16_t *strategy_d /*[m][Dtmax][4][1326]*/,
                           uint16_t *river_strategy_d /*[m][Drmax][52][4][1326]*/, int64_t *value_d /*[m][2][1326]*/, int64_t *br_d,
                           uint8_t *status_d, void *stream);
int pk_solve_turn_locked(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                         const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                         const uint32_t *tree_of /*[m], host; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock,
                         const uint16_t *locked, const uint8_t *river_lock, const uint16_t *river_locked, uint16_t *strategy,
                         uint16_t *river_strategy, int64_t *value, int64_t *br, uint8_t *status);

/* ---- Re-solving: a subgame re-solved from a node of a solution (the numpy restatement: tests/resolve_spec.py).  A
 * caller who has solved a turn spot and then sees the river card, or has solved a coarse tree and meets a bet between its sizes, hands what the
 * first solve computed at that node to the next solve.  Everything of "River solver", "Turn solver", "a tree per spot" and "Locked nodes"
 * holds except what is said here.  A call carries, beside the arguments of pk_solve_river_locked / pk_solve_turn_locked, before `strategy`:
 *   reach   u32 [m][2][1326]   the root reaches in the solver's own units
 *   given   i64 [m][2][1326]   (river only) the values at the spot's GIVEN terminal
 *   at      u8  [m]            the node of the node outputs
 *   at_card u8  [m]            (turn only) the river card, a card code as on the board, under which a river-level `at` is reported
 * and after `br`:
 *   node_reach u32 [m][2][1326], node_value i64 [m][2][1326], node_br i64 [m][2][1326].
 * Each of them may be NULL.  PK_ABI_VERSION is unchanged: symbols are added only.
 * ROOT REACHES.  reach != NULL: `ranges` may be NULL and is not read; for valid h, r_p[root][h] = min(reach[i][p][h], LIM), without a shift,
 * LIM = 2^20 - 1 (river) and 2^17 - 1 (turn): the per-entry bounds of a shifted 16-bit weight, so every BOUND of the solvers holds
 * unchanged.  Invalid holdings are not read.  reach = ranges << 4 (turn: << 1) gives the locked call's outputs byte for byte.
 * NODE OUTPUTS.  `at` is NULL exactly when all three node outputs are (PK_E_INVALID_ARG otherwise).  They come from the final pass -- the
 * one that gives value and br -- at node at[i] of the spot's own tree: node_reach[p][h] = r_p[at][h], node_value[p][h] = u_p[at][h],
 * node_br[p][h] = the value the best-response pass of p carries at that node (at a terminal: u_p).  Invalid holdings are 0.  At the root
 * node_value = value, node_br = br and node_reach is the root reach.  Turn solver: at a turn-level node (a chance node is one) the values
 * are as they stand there, with the factor P - 4; at a river-level node the outputs are those of river card at_card[i], from that card's
 * pass (the factor P - 4 enters only when the chance node sums the cards), holdings that contain the card are 0; at_card is not read for a
 * turn-level `at`.  The sum over the pool's cards c of node_value at a chance node's child under c is node_value at the chance node.
 * STATUS: at[i] >= n of the spot's tree is PK_EQ_BAD_TREE; a river-level at[i] whose at_card[i] is no card of the pool (or a NULL at_card)
 * is PK_EQ_BAD_CARD; the spot is refused with all-zero outputs and no neighbour is disturbed.  Both are judged only for a spot that is not
 * refused for another reason.
 * GIVEN TERMINAL (pk_solve_river_resolve only).  Node kind 6 is a terminal, at most one per tree ("more than one given node"); its put is
 * not read for payoffs.  At it u_p[h] = clamp(given[i][p][h], +-(2^45 - 1)) for valid h, whatever the reaches, in every pass, the
 * best-response passes included -- the "terminate" leaf of the re-solving gadget (Burch, Johanson, Bowling 2014): an opponent node above it
 * chooses per holding between the value it was promised and playing on.  |u| < 2^45 is what every other terminal obeys, so the BOUNDS
 * hold.  A tree with a given node needs a non-NULL `given` (PK_E_INVALID_ARG); `given` is not read for a spot whose tree has none.  Every
 * other entry point, pk_solve_turn_resolve included, refuses kind 6 with its own text.
 * ROOT PUT: no check requires put[root] = 0 and nothing in the definitions does: a subtree re-rooted at one of its nodes keeps the pot
 * and every node's put, and its passes are those of the original tree below that node.
 * `reach` must not be `node_reach`, `given` none of value, br, node_value, node_br (PK_E_INVALID_ARG).  In the _d forms the new arrays
 * are DEVICE memory. */
int pk_solve_river_resolve_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                             const uint16_t *ranges_d /*[m][2][1326]; may be NULL with reach_d*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                             const uint8_t *kind /*[ntrees][64], host*/, const uint8_t *child /*[ntrees][64][4], host*/,
                             const uint32_t *put /*[ntrees][64][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                             const uint32_t *tree_of_d /*[m], DEVICE; NULL with ntrees = 1: tree 0*/, uint32_t iters,
                             const uint8_t *lock_d /*[m][Dmax], DEVICE; NULL: none*/, const uint16_t *locked_d /*[m][Dmax][4][1326], DEVICE*/,
                             const uint32_t *reach_d /*[m][2][1326]*/, const int64_t *given_d /*[m][2][1326]*/, const uint8_t *at_d /*[m]*/,
                             uint16_t *strategy_d /*[m][Dmax][4][1326]*/, int64_t *value_d /*[m][2][1326]*/, int64_t *br_d,
                             uint32_t *node_reach_d /*[m][2][1326]*/, int64_t *node_value_d, int64_t *node_br_d, uint8_t *status_d, void *stream);
int pk_solve_river_resolve(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                           const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                           const uint32_t *tree_of /*[m], host; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock,
                           const uint16_t *locked, const uint32_t *reach, const int64_t *given, const uint8_t *at, uint16_t *strategy,
                           int64_t *value, int64_t *br, uint32_t *node_reach, int64_t *node_value, int64_t *node_br, uint8_t *status);
int pk_solve_turn_resolve_d(int device, size_t m, const uint8_t *board_d /*[m][4]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                            const uint16_t *ranges_d /*[m][2][1326]; may be NULL with reach_d*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                            const uint8_t *kind /*[ntrees][128], host*/, const uint8_t *child /*[ntrees][128][4], host*/,
                            const uint32_t *put /*[ntrees][128][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                            const uint32_t *tree_of_d /*[m], DEVICE; NULL with ntrees = 1: tree 0*/, uint32_t iters,
                            const uint8_t *lock_d, const uint16_t *locked_d, const uint8_t *river_lock_d, const uint16_t *river_locked_d,
                            const uint32_t *reach_d /*[m][2][1326]*/, const uint8_t *at_d /*[m]*/, const uint8_t *at_card_d /*[m]*/,
                            uint16_t *strategy_d, uint16_t *river_strategy_d, int64_t *value_d /*[m][2][1326]*/, int64_t *br_d,
                            uint32_t *node_reach_d /*[m][2][1326]*/, int64_t *node_value_d, int64_t *node_br_d, uint8_t *status_d, void *stream);
int pk_solve_turn_resolve(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                          const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                          const uint32_t *tree_of /*[m], host; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock,
                          const uint16_t *locked, const uint8_t *river_lock, const uint16_t *river_locked, const uint32_t *reach,
                          const uint8_t *at, const uint8_t *at_card, uint16_t *strategy, uint16_t *river_strategy, int64_t *value, int64_t *br,
                          uint32_t *node_reach, int64_t *node_value, int64_t *node_br, uint8_t *status);

/* ---- Resuming a solve: the regrets R and the average accumulators A returned to the caller and taken back (the numpy
 * restatement: tests/resume_spec.py).  Solving until a target is met, a checkpoint, a warm start after the inputs moved a little, host work
 * between iterations.  Everything of the sections above holds except what is said here.  PK_ABI_VERSION is unchanged: symbols are added only.
 * pk_solve_river_resume(_d) / pk_solve_turn_resume(_d) take the arguments of pk_solve_river_resolve(_d) / pk_solve_turn_resolve(_d) and,
 * before `strategy`:
 *   t0       u32 [m]                  the iterations the state already holds; NULL: all 0
 *   regret   i64 [m][Dmax][4][1326]   R, in the shape and strides of `strategy` (turn: [m][Dtmax][4][1326], the turn-level rows)
 *   average  i64 [m][Dmax][4][1326]   A, likewise
 *   river_regret, river_average i64 [m][Drmax][52][4][1326]   (turn only) the river-level rows, in the shape of `river_strategy`: by the
 *                                     river card's canonical index (4.4 MB per row, spot and array)
 * The state arrays are IN/OUT, in place: DEVICE memory in the _d forms, host memory otherwise.  They are given all together or not at all
 * (PK_E_INVALID_ARG otherwise, and for a t0 without them, each with its own text).  With none the call IS the resolve call.  A state array
 * must be no other argument of the call and no other state array (PK_E_INVALID_ARG).
 * ITERATIONS: spot i runs t = t0[i] + 1 .. t0[i] + iters; t enters only A += t r_p.  iters may be 0.
 * LOAD, for a spot with t0[i] > 0, at every decision row d < D of the spot's tree that is not locked, action a < nact, valid h -- on the
 * turn's river level for every card c of the pool and every valid h without c: R = clamp(regret[i][d][a][h], 0, RMAX), A =
 * clamp(average[i][d][a][h], 0, AMAX); RMAX = 2^58 - 1, AMAX = 2^44 - 1 (river), RMAX = 2^60 - 1, AMAX = 2^41 - 1 (turn, both levels).  With
 * t0[i] = 0 nothing of the spot's state is read and R = A = 0.  A state this library wrote never meets the clamp.
 * STORE: after the last iteration and before the final passes the entries named under LOAD are written with R and A as they stand.  Every
 * OTHER entry of the spot's slices -- a >= nact, invalid holdings, rows at or past the spot's D, locked rows, cards outside the pool,
 * holdings that contain the card -- is written 0 by a call with t0[i] = 0 and left exactly as it is by a call with t0[i] > 0: a locked
 * row's state survives a locked call (the word in which the turn kernel keeps a locked river-level node's probabilities never leaves).
 * STATUS: PK_EQ_BAD_ITER marks t0[i] + iters > 4096, judged only for a spot that is not refused for another reason.  A refused spot, for
 * whatever reason, has all-zero outputs as before and ITS STATE IS NOT TOUCHED: a mistake destroys no checkpoint.  No neighbour is disturbed.
 * IDENTITIES: (i) state given with t0 = 0 leaves every other output what the resolve call gives, byte for byte; (ii) (t0 = 0, iters = a)
 * followed by (t0 = a, iters = b) on the same inputs leaves the state and every output of (t0 = 0, iters = a + b), whatever the grid, the
 * batch or the mix of t0 in it.
 * BOUNDS (river).  A regret moves by u_p[c] - u_p[n], |.| < 2^46, an iteration: from the clamp, 2^58 + 4096 * 2^46 = 2^59 < 2^63.  The
 * strategy rule shifts by bitlen(max) - 31, so the largest shifted entry is < 2^31 and a numerator < 2^46 whatever the size of X.  A grows
 * by t * reach with t <= 4096 and reach < 2^20: at most sum_{t <= 4096} t * 2^20 < 2^43 in one call, so A < 2^44 + 2^43 < 2^45.  The bounds
 * of "River solver" are what a state written by this library obeys, since its t never passes 4096; the clamps only keep a foreign state
 * inside int64_t.
 * BOUNDS (turn).  |u| < 2^46.7, so a regret moves by < 2^47.7 an iteration: 2^60 + 4096 * 2^47.7 < 2^60.3 < 2^63; the rule's numerator as
 * above.  A grows by t * reach, reach < 2^17: < 2^40 in one call, so A < 2^41 + 2^40 < 2^42. */
#define PK_EQ_BAD_ITER 16u   /* resuming: t0 + iters > 4096 (the value of PK_EQ_IN_FLIGHT, which no spot form reports) */
int pk_solve_river_resume_d(int device, size_t m, const uint8_t *board_d /*[m][5]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                            const uint16_t *ranges_d /*[m][2][1326]; may be NULL with reach_d*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                            const uint8_t *kind /*[ntrees][64], host*/, const uint8_t *child /*[ntrees][64][4], host*/,
                            const uint32_t *put /*[ntrees][64][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                            const uint32_t *tree_of_d /*[m], DEVICE; NULL with ntrees = 1: tree 0*/, uint32_t iters,
                            const uint8_t *lock_d /*[m][Dmax], DEVICE; NULL: none*/, const uint16_t *locked_d /*[m][Dmax][4][1326], DEVICE*/,
                            const uint32_t *reach_d /*[m][2][1326]*/, const int64_t *given_d /*[m][2][1326]*/, const uint8_t *at_d /*[m]*/,
                            const uint32_t *t0_d /*[m], DEVICE; NULL: all 0*/, int64_t *regret_d /*[m][Dmax][4][1326], DEVICE, in and out*/,
                            int64_t *average_d /*as regret_d*/, uint16_t *strategy_d /*[m][Dmax][4][1326]*/, int64_t *value_d /*[m][2][1326]*/,
                            int64_t *br_d, uint32_t *node_reach_d /*[m][2][1326]*/, int64_t *node_value_d, int64_t *node_br_d, uint8_t *status_d,
                            void *stream);
int pk_solve_river_resume(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                          const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                          const uint32_t *tree_of /*[m], host; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock,
                          const uint16_t *locked, const uint32_t *reach, const int64_t *given, const uint8_t *at, const uint32_t *t0,
                          int64_t *regret /*in and out*/, int64_t *average /*in and out*/, uint16_t *strategy, int64_t *value, int64_t *br,
                          uint32_t *node_reach, int64_t *node_value, int64_t *node_br, uint8_t *status);
int pk_solve_turn_resume_d(int device, size_t m, const uint8_t *board_d /*[m][4]*/, const uint64_t *dead_d /*[m]; NULL: none*/,
                           const uint16_t *ranges_d /*[m][2][1326]; may be NULL with reach_d*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                           const uint8_t *kind /*[ntrees][128], host*/, const uint8_t *child /*[ntrees][128][4], host*/,
                           const uint32_t *put /*[ntrees][128][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                           const uint32_t *tree_of_d /*[m], DEVICE; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock_d,
                           const uint16_t *locked_d, const uint8_t *river_lock_d, const uint16_t *river_locked_d,
                           const uint32_t *reach_d /*[m][2][1326]*/, const uint8_t *at_d /*[m]*/, const uint8_t *at_card_d /*[m]*/,
                           const uint32_t *t0_d /*[m], DEVICE; NULL: all 0*/, int64_t *regret_d /*[m][Dtmax][4][1326], DEVICE, in and out*/,
                           int64_t *average_d /*as regret_d*/, int64_t *river_regret_d /*[m][Drmax][52][4][1326], DEVICE, in and out*/,
                           int64_t *river_average_d /*as river_regret_d*/, uint16_t *strategy_d, uint16_t *river_strategy_d,
                           int64_t *value_d /*[m][2][1326]*/, int64_t *br_d, uint32_t *node_reach_d /*[m][2][1326]*/, int64_t *node_value_d,
                           int64_t *node_br_d, uint8_t *status_d, void *stream);
int pk_solve_turn_resume(int device, size_t m, const uint8_t *board, const uint64_t *dead, const uint16_t *ranges, uint32_t ntrees,
                         const uint32_t *n, const uint8_t *kind, const uint8_t *child, const uint32_t *put, const uint32_t *pot,
                         const uint32_t *tree_of /*[m], host; NULL with ntrees = 1: tree 0*/, uint32_t iters, const uint8_t *lock,
                         const uint16_t *locked, const uint8_t *river_lock, const uint16_t *river_locked, const uint32_t *reach,
                         const uint8_t *at, const uint8_t *at_card, const uint32_t *t0, int64_t *regret /*in and out*/,
                         int64_t *average /*in and out*/, int64_t *river_regret /*in and out*/, int64_t *river_average /*in and out*/,
                         uint16_t *strategy, uint16_t *river_strategy, int64_t *value, int64_t *br, uint32_t *node_reach, int64_t *node_value,
                         int64_t *node_br, uint8_t *status);

/* ---- Pre-flop solver: heads-up CFR+ over a betting tree with NO board, a showdown paid by the exact matchup table (DESIGN.md section 3.18;
 * the numpy restatement: tests/preflop_solver_spec.py).  Everything of "River solver" holds except what is said here.  PK_ABI_VERSION is
 * unchanged: symbols are added only.
 * SPOTS: a spot has no board and no dead mask: two ranges, u16 [2][1326], and a tree.  Every holding is valid, P = 52.  Player 0 acts
 * first, as the small blind does heads-up.  Root reach r_p[root][h] = w_p[h] << 4, as on the river.
 * TREES: the river solver's packed trees with kinds 0 .. 4 only.  Kind 5 (the turn solver's chance node) and kind 6 (a re-solving call's
 * given node) are refused, each with a text of its own; the rest of the river solver's host check applies unchanged (pot + max put <= 8191,
 * iters 1 .. 4096), before any device is looked at.  The root's put may be non-zero: the blinds are put[root] = (sb, bb), antes are pot.
 * A TREE PER SPOT: ntrees, the per-tree arrays and tree_of are taken as the calls of "a tree per spot" take them (at most PK_RS_MAX_TREES
 * trees, rows of 64 nodes, strategy strided by Dmax = pk_rs_trees_rows).  tree_of NULL: every spot uses tree 0.  tree_of[i] >= ntrees:
 * PK_EQ_BAD_TREE in status[i], all-zero outputs, no neighbour disturbed.  No other status exists.
 * FOLD TERMINALS: as the river solver's, with S_q(h) = the sum of r_q[n][h'] over the h' that share no card with h.
 * SHOWDOWN TERMINAL, the only new arithmetic.  B = PK_PREFLOP_BOARDS = 1 712 304, c = put[0] = put[1], win and tie the resident matchup table
 * ("Pre-flop matchups"; a pair that shares a card holds 0 in both, so card removal is in the table):
 *     E_q(h) = sum over h' of r_q[n][h'] (2 win[h][h'] + tie[h][h'])
 *     u_p[h] = floor((pot + 2c) E_q(h) / B) - 2c S_q(h), the floor of the exact product.
 * On the full table win + tie + lose = B for a disjoint pair, so this is the river solver's 2 (pot + c) W + pot T - 2c L with W, T, L the
 * reach times the share of boards won, tied and lost, floored once; the units are half-chips x opponent reach.  A showdown is paid as if
 * the hand were checked down to the river, whatever the puts: THERE IS NO POST-FLOP BETTING in this game.
 * BOUNDS: E < 2^52 (the 1 225 holdings disjoint from h, a reach < 2^20 each, times 2 B: below 2^51.97).  The product (pot + 2c) E can reach 2^66, so it is formed as
 * (pot + 2c) (E div B) + ((pot + 2c) (E mod B)) div B -- the same integer, every intermediate below 2^46.  |u| <= 2 (pot + c) S < 2^45, hence
 * |sum sigma u| < 2^60, |R| < 2^58 and A < 2^44 as on the river (measured at the corner: tests/preflop_solver_witness.py).  No sum depends
 * on its order: the output is bit-identical to the restatement whatever the grid.
 * OUTPUTS as the river solver's: strategy u16 [m][Dmax][4][1326], value and br i64 [m][2][1326], status u8 [m]; each optional except status.
 * The matchup table is built on the first call that needs it, as the other pre-flop entry points build it; the work space is sized by the
 * resident workgroups (59 136 bytes per node of the call's largest tree and workgroup), never by m.
 * NOT HERE: locks, re-solving (reach, at, given), resuming, a table form, more than two players, dead cards, post-flop play below a call. */
int pk_solve_preflop_d(int device, size_t m, const uint16_t *ranges_d /*[m][2][1326]*/, uint32_t ntrees, const uint32_t *n /*[ntrees], host*/,
                       const uint8_t *kind /*[ntrees][64], host*/, const uint8_t *child /*[ntrees][64][4], host*/,
                       const uint32_t *put /*[ntrees][64][2], host*/, const uint32_t *pot /*[ntrees], host*/,
                       const uint32_t *tree_of_d /*[m], DEVICE; NULL: tree 0*/, uint32_t iters, uint16_t *strategy_d /*[m][Dmax][4][1326]*/,
                       int64_t *value_d /*[m][2][1326]*/, int64_t *br_d, uint8_t *status_d, void *stream);
int pk_solve_preflop(int device, size_t m, const uint16_t *ranges, uint32_t ntrees, const uint32_t *n, const uint8_t *kind, const uint8_t *child,
                     const uint32_t *put, const uint32_t *pot, const uint32_t *tree_of /*[m], host; NULL: tree 0*/, uint32_t iters,
                     uint16_t *strategy, int64_t *value, int64_t *br, uint8_t *status);
/* Streams are recycled through a per-device pool when handles are destroyed (a process that opens and closes handles keeps its hardware
 * queues); the sub-batch streams of pk_set_env_batches are created at the HIGHEST stream priority (env PK_ENV_STREAM_PRIO=0: normal), so a
 * learner's normal-priority kernels on the same GPU yield to the env ranges while those run.  pk_stream_pool_drain destroys the pooled (idle)
 * streams of `device` (-1: all devices) and returns how many -- call it before hipDeviceReset, which would leave stale handles in the pool
 * -- any call on such a handle, a query included, crashes inside the HIP runtime -- or to give the queues back.  Seat belt for an application that
 * forgets: the pool keeps a small canary allocation per device and looks its ADDRESS up (hipMemGetAddressRange) before it hands a pooled stream out; a
 * canary that has vanished means the device was reset, and the pool forgets its handles instead of using them (a stream that cannot be synchronised when
 * its handle is destroyed is not pooled either). */
int pk_stream_pool_drain(int device);
/* Runs `reps` back-to-back fused rollouts of k_steps each (never coalesced) plus the flush of what they deferred and
 * returns the device time of all of it divided by `reps`, in milliseconds (events on the handle's stream): the time one
 * launch's k_steps of work take, the flush shared among the launches.  Diagnostic (tools/); bench.py's roofline leg
 * brackets its own timed region with events instead (pk_record_event + pk_get_launch_stats). */
int pk_time_rollout(pk_handle *h, int k_steps, int policy, int auto_reset, int fused, int reps, double *ms_per_launch,
                    uint64_t *counters);

#ifdef __cplusplus
}
#endif
#endif
