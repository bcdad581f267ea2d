// pk_util_kernels.hpp -- the __global__ kernels of libpokerl_hip.so that are NOT per-seat-count templates (included by pk_api.hip only): the
// counter sum, the exports and observation rows built from HBM, the batched hand evaluators and their test helpers.  gfx950 only.
#pragma once
#include "pk_device.hpp"

using namespace pk;

// Sums and clears the per-wave counter slots: one workgroup, grid-stride over the slots.
__global__ void __launch_bounds__(256) k_sum_counters(unsigned long long *slots, int nslots, unsigned long long *out) {
    __shared__ unsigned long long part[256][PK_NUM_COUNTERS];
    unsigned long long acc[PK_NUM_COUNTERS] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < nslots; i += 256)
        for (int c = 0; c < PK_NUM_COUNTERS; ++c) { acc[c] += slots[(size_t)i * PK_NUM_COUNTERS + c]; slots[(size_t)i * PK_NUM_COUNTERS + c] = 0; }
    for (int c = 0; c < PK_NUM_COUNTERS; ++c) part[threadIdx.x][c] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) for (int c = 0; c < PK_NUM_COUNTERS; ++c) part[threadIdx.x][c] += part[threadIdx.x + s][c];
        __syncthreads();
    }
    if (threadIdx.x < PK_NUM_COUNTERS) out[threadIdx.x] = part[0][threadIdx.x];
}

// ---- exports: device-side conversion from the SoA/bitmask layout to the reference's table-major arrays
__global__ void k_export_f64(const double *src, int T, int N, double *out) {  // [N][T] -> [T][N]
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * N) return;
    int t = i / N, p = i - t * N;
    out[i] = src[(size_t)p * T + t];
}
__global__ void k_export_states(const uint64_t *ss, int T, int N, uint8_t *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * N) return;
    int t = i / N, p = i - t * N;
    out[i] = SeatStates{ss[t]}.state_of(p);
}
__global__ void k_export_i32(State S, int field, int32_t *out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.T) return;
    const Cursor cur{S.cursors[t]};
    int32_t v = 0;
    switch (field) {
        case PK_I_ACTIVE_PLAYER: v = cur.active(); break;
        case PK_I_TURN: v = cur.turn(); break;
        case PK_I_DEALER_IDX: v = cur.dealer(); break;
        case PK_I_SMALL_BLIND_IDX: v = cur.sb(); break;
        case PK_I_BIG_BLIND_IDX: v = cur.bb(); break;
        case PK_I_HAND: v = S.hand[t]; break;
    }
    out[t] = v;
}
__global__ void k_export_cards(const uint32_t *cards, int T, int K, uint8_t *out) {  // [W][T] words -> [T][K] bytes
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * K) return;
    int t = i / K, c = i - t * K;
    out[i] = (uint8_t)card_byte(cards, T, t, c);
}
__global__ void k_export_show(const uint32_t *show, int T, int N, uint8_t *rank, uint32_t *kick) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * N) return;
    int t = i / N, p = i - t * N;
    uint32_t v = show[(size_t)p * T + t];
    rank[i] = (uint8_t)(v >> 20);
    kick[i] = v & 0xFFFFF;
}
// Game.get_valid_actions(player), game.py:339-383, of ANY seat as a bitmask (runtime N: export kernels are not
// templated).
__device__ inline uint32_t valid_bits_of(const State &S, int t, int N, int player) {
    const size_t T = (size_t)S.T;
    double high_bet = S.pending[t];                                               // :365 np.max
    for (int p = 1; p < N; ++p) { double x = S.pending[(size_t)p * T + t]; high_bet = (x > high_bet) ? x : high_bet; }
    return valid_bits(S.credits[(size_t)player * T + t], high_bet, S.min_raise[t]);        // :366
}
// player < 0: each table's active player (the cached mask); else that seat on every table.  out: one-hot [T][7]
__global__ void k_export_valid(State S, int N, int player, uint8_t *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.T * PK_NUM_MOVES) return;
    int t = i / PK_NUM_MOVES, a = i - t * PK_NUM_MOVES;
    uint32_t m = player < 0 ? S.valid[t] : valid_bits_of(S, t, N, player);
    out[i] = (m >> a) & 1;
}
// Game.StateView(game, player), game.py:117-131, as one dense f64 row per table (layout: pokerl_hip.h PK_OBS_DIM).
// player < 0: the active player of each table (what `game.active_state` is, game.py:323-332).
// The per-seat money of a table is LOADED FIRST, all of it (3 x 16 predicated loads in flight; runtime N: the export kernels are not templated),
// then stored: with one load -> store pair per seat in a loop (rounds 1-5) the compiler could not move a load above the previous seat's store
// (`out` may alias the state for all it knows) and the kernel ran at the latency of 3N dependent round trips -- 1.1 TB/s at 1 M tables.
struct SeatMoney { double credits[PK_MAX_PLAYERS], bets[PK_MAX_PLAYERS], pending[PK_MAX_PLAYERS]; };
__device__ __forceinline__ void load_seat_money(const State &S, int t, int N, SeatMoney &m) {
    const size_t T = (size_t)S.T;
#pragma unroll
    for (int p = 0; p < PK_MAX_PLAYERS; ++p) {
        const size_t i = (size_t)(p < N ? p : 0) * T + t;
        m.credits[p] = S.credits[i]; m.bets[p] = S.bets[i]; m.pending[p] = S.pending[i];
    }
}
__global__ void __launch_bounds__(64) k_obs(State S, int N, int player, double *__restrict__ out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.T) return;
    const int T = S.T, D = PK_OBS_DIM(N);
    double *o = out + (size_t)t * D;
    SeatMoney m;
    load_seat_money(S, t, N, m);
    const Cursor cur{S.cursors[t]};
    const int active = cur.active(), turn = cur.turn();
    const int who = player < 0 ? active : player;
    const uint32_t vm = player < 0 ? S.valid[t] : valid_bits_of(S, t, N, who);
    auto card = [&](int c) { return (double)card_byte(S.cards, T, t, c); };
    o[0] = who; o[1] = turn; o[2] = S.min_raise[t];
    for (int a = 0; a < PK_NUM_MOVES; ++a) o[3 + a] = (vm >> a) & 1;
    o[10] = card(5 + 2 * who); o[11] = card(6 + 2 * who);                          // game.py:385-389
    for (int c = 0; c < 5; ++c) o[12 + c] = community_visible(turn, c) ? card(c) : -1.0;
#pragma unroll
    for (int p = 0; p < PK_MAX_PLAYERS; ++p)
        if (p < N) { o[17 + p] = m.credits[p]; o[17 + N + p] = m.bets[p]; o[17 + 2 * N + p] = m.pending[p]; }
}
// The same row as k_obs, compact: 16 header bytes (seat, turn, valid-mask bits, 2 hole cards, 5 community cards with 0xFF for a
// card not yet visible, 6 zero bytes) + (3N+1) f64 (minimum_raise_value, credits, bets, pending_bets): pokerl_hip.h.
__global__ void __launch_bounds__(64) k_obs_packed(State S, int N, int player, uint8_t *__restrict__ out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.T) return;
    const int T = S.T;
    uint64_t *o = reinterpret_cast<uint64_t *>(out + (size_t)t * PK_OBS_PACKED_BYTES(N));
    SeatMoney sm;
    load_seat_money(S, t, N, sm);
    const Cursor cur{S.cursors[t]};
    const int active = cur.active(), turn = cur.turn();
    const int who = player < 0 ? active : player;
    const uint32_t vm = player < 0 ? S.valid[t] : valid_bits_of(S, t, N, who);
    auto card = [&](int c) { return card_byte(S.cards, T, t, c); };
    auto comm = [&](int c) { return community_visible(turn, c) ? card(c) : 0xffu; };
    o[0] = obs_packed_header0((uint32_t)who, (uint32_t)turn, vm, card(5 + 2 * who), card(6 + 2 * who), comm(0), comm(1), comm(2));
    o[1] = (uint64_t)comm(3) | ((uint64_t)comm(4) << 8);
    double *m = reinterpret_cast<double *>(o + 2);
    m[0] = S.min_raise[t];
#pragma unroll
    for (int p = 0; p < PK_MAX_PLAYERS; ++p)
        if (p < N) { m[1 + p] = sm.credits[p]; m[1 + N + p] = sm.bets[p]; m[1 + 2 * N + p] = sm.pending[p]; }
}
// Game.step's precondition (game.py:648-651) over a batch: the lowest table index whose action is not in its active player's mask.
__global__ void k_check_actions(const uint8_t *valid, const int32_t *actions, int T, int32_t *first_bad) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int a = actions[t];
    const bool ok = a >= 0 && a < PK_NUM_MOVES && ((valid[t] >> a) & 1);
    if (!ok) atomicMin(first_bad, t);
}
// Game.pot (np.sum(bets) in numpy's association order, game.py:281-284 + SURVEY A.5) / Game.high_bet
// (np.max(pending_bets), game.py:287-290) per table; Game.game_over (game.py:317-320).
__global__ void k_table_f64(State S, int N, int field, double *out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.T) return;
    const size_t T = (size_t)S.T;
    double r;
    if (field == PK_TF_POT) {
        const double *a = S.bets;
        if (N < 8) {
            r = a[t];
            for (int p = 1; p < N; ++p) r = r + a[(size_t)p * T + t];
        } else {   // numpy's pairwise_sum: eight partial sums over whole blocks of eight, the tree, then the tail
            double r8[8];
            for (int j = 0; j < 8; ++j) r8[j] = a[(size_t)j * T + t];
            int p = 8;
            for (; p + 8 <= N; p += 8)
                for (int j = 0; j < 8; ++j) r8[j] = r8[j] + a[(size_t)(p + j) * T + t];
            r = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
            for (; p < N; ++p) r = r + a[(size_t)p * T + t];
        }
    } else if (field == PK_TF_HIGH_BET) {
        r = S.pending[t];
        for (int p = 1; p < N; ++p) { double x = S.pending[(size_t)p * T + t]; r = (x > r) ? x : r; }
    } else r = S.min_raise[t];
    out[t] = r;
}
__global__ void k_game_over(const uint64_t *ss, int T, int N, uint8_t *out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    out[t] = __popc(~SeatStates{ss[t]}.broken() & ((1u << N) - 1)) == 1;
}

// pokerl.judger.eval_hand batched: one hand per lane, cards[M][7] bytes
__global__ void k_eval_hands(const uint8_t *cards, const uint8_t *ncards, size_t m, uint8_t *rank, uint32_t *kick, uint8_t *nkick) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint32_t c[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) c[j] = cards[i * 7 + j];
    int n = ncards ? ncards[i] : 7;
    n = n < 0 ? 0 : (n > 7 ? 7 : n);
    int nk;
    uint32_t v = eval_hand_any(c, n, nk);     // 3..7 distinct cards: the bitmask fast path; a repeated card, 0..2 cards: the literal scan
    rank[i] = (uint8_t)(v >> 20);
    kick[i] = v & 0xFFFFF;
    if (nkick) nkick[i] = (uint8_t)nk;
}
// The same op on the TABLE path (eval_tab_bits: ~two thirds of the instructions of the register evaluator, checks included):
// EVAL_TAB_BLOCK-thread workgroups with the 32 KB rank-mask table of the streaming evaluator in LDS, grid-stride, one hand per lane per
// iteration, nothing shared between lanes after the table copy (no barrier in the loop; eight waves per SIMD hide the lookups).  A hand's
// seven card bytes start at ANY byte offset: ONE unaligned 8-byte load per hand (gfx950 runs in unaligned-access mode; the eighth byte
// belongs to the next hand and is ignored -- the LAST hand of the buffer is read byte by byte instead, so nothing past cards[7m) is
// touched), the next iteration's load in flight while this one is evaluated.  3..7 distinct real cards: the table; 0..2 cards: the
// reference's first lines as selects (eval_small); a repeated card or a byte that is no card: the literal scan, executed by a wave only if
// one of its lanes needs it.  HAS_N == false: ncards == NULL, every hand holds seven cards.
// (Tried: two hands per lane per iteration as in the streaming kernel, 16-byte loads and paired stores -- no faster on seven-card hands,
// the kernel is bound by VALU issue, not by latency or memory instructions, and slower on mixed batches, where one short hand sends its
// partner down the slow branch too: profiles/r05_eval_hands_bench.txt.)
#define EVAL_TAB_BLOCK 512
template <bool HAS_N>
__global__ void __launch_bounds__(EVAL_TAB_BLOCK, 8) k_eval_hands_tab(const uint8_t *__restrict__ cards, const uint8_t *__restrict__ ncards, size_t m,
                                                                      uint8_t *__restrict__ rank, uint32_t *__restrict__ kick, uint8_t *__restrict__ nkick,
                                                                      const uint32_t *__restrict__ tab) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    for (int i = threadIdx.x; i < EVAL7_TAB_WORDS / 4; i += EVAL_TAB_BLOCK) reinterpret_cast<uint4 *>(T)[i] = reinterpret_cast<const uint4 *>(tab)[i];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * EVAL_TAB_BLOCK;
    auto fetch = [&](size_t i, uint64_t &w, int &n) {
        if (i + 1 < m) __builtin_memcpy(&w, cards + 7 * i, 8);            // global_load_dwordx2 at a byte address
        else { w = 0; for (int j = 0; j < 7; ++j) w |= (uint64_t)cards[7 * i + j] << (8 * j); }
        n = HAS_N ? ncards[i] : 7;
    };
    size_t i = (size_t)blockIdx.x * EVAL_TAB_BLOCK + threadIdx.x;
    uint64_t w = 0; int n = 0;
    if (i < m) fetch(i, w, n);
    for (; i < m; i += stride) {
        uint64_t wn = 0; int nn = 0;
        if (i + stride < m) fetch(i + stride, wn, nn);
        n = n > 7 ? 7 : n;                                                  // (u8: never negative)
        int nk = 0;
        uint32_t v;
        uint64_t bits;
        if (tab_bits_of<!HAS_N>(w, n, bits)) v = eval_tab_bits<!HAS_N>(bits, T, nk);
        else if (HAS_N && n < 3) v = eval_small(w, n, nk);
        else {
            const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
            const uint32_t c[7] = {lo & 0xff, (lo >> 8) & 0xff, (lo >> 16) & 0xff, lo >> 24, hi & 0xff, (hi >> 8) & 0xff, (hi >> 16) & 0xff};
            v = eval_hand(c, n, nk);
        }
        rank[i] = (uint8_t)(v >> 20);
        kick[i] = v & 0xFFFFF;
        if (nkick) nkick[i] = (uint8_t)nk;
        w = wn; n = nn;
    }
}
// pokerl.judger.compare_rankings batched: one list of n rankings per lane (judger.py:111-158)
__global__ void k_compare(const uint8_t *rank, const uint32_t *kick, int n, size_t m, uint8_t *onehot) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint32_t best_rank = HR_NONE, best_kicker = 0, win = 0;
    for (int p = 0; p < n; ++p) {
        uint32_t r = rank[i * n + p], k = kick[i * n + p];
        if (r < best_rank) { best_rank = r; best_kicker = k; win = 1u << p; }
        else if (r == best_rank) {
            if (k > best_kicker) win = 1u << p;  // line 148: best_kicker is not raised
            else if (k == best_kicker) win |= 1u << p;
        }
    }
    for (int p = 0; p < n; ++p) onehot[i * n + p] = (win >> p) & 1;
}
// Streaming evaluator: two hands per lane per iteration (one 16-byte load, one 8-byte store), grid-stride.
// VEC: hands 16-byte and out 8-byte aligned (any hipMalloc'ed base); otherwise one hand per lane per iteration.
template <bool DISTINCT, bool VEC>
__global__ void __launch_bounds__(256) k_eval7_stream(const uint64_t *__restrict__ hands, size_t m, uint32_t *__restrict__ out) {
    const size_t pairs = VEC ? m / 2 : 0, stride = (size_t)gridDim.x * blockDim.x;
    auto eval1 = [](uint64_t w) {
        uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
        uint32_t c[7] = {lo & 0xff, (lo >> 8) & 0xff, (lo >> 16) & 0xff, lo >> 24, hi & 0xff, (hi >> 8) & 0xff, (hi >> 16) & 0xff};
        int nk;
        return DISTINCT ? eval7_distinct(c) : eval_hand_any(c, 7, nk);
    };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const ulonglong2 w = reinterpret_cast<const ulonglong2 *>(hands)[i];
        uint2 r;
        r.x = eval1(w.x); r.y = eval1(w.y);
        reinterpret_cast<uint2 *>(out)[i] = r;
    }
    if constexpr (VEC) {
        if ((m & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[m - 1] = eval1(hands[m - 1]);
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) out[i] = eval1(hands[i]);
    }
}
// The table of eval7_tab (pk_device.hpp), built once per device into global memory; every workgroup of the streaming
// kernel below copies it into its LDS.
__global__ void k_make_eval7_tab(uint32_t *tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint32_t)EVAL7_TAB_WORDS) tab[i] = eval7_tab_entry(i);
}
// Streaming evaluator for 7 DISTINCT cards, table-driven (eval7_tab): 512-thread workgroups, four per CU (4 x 32 KB of LDS),
// eight waves per SIMD under the 64-register cap; same two-hands-per-lane 16-byte loads / 8-byte stores as above.
template <bool VEC>
__global__ void __launch_bounds__(512, 8) k_eval7_tab_stream(const uint64_t *__restrict__ hands, size_t m, uint32_t *__restrict__ out, const uint32_t *__restrict__ tab) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    for (int i = threadIdx.x; i < EVAL7_TAB_WORDS / 4; i += 512) reinterpret_cast<uint4 *>(T)[i] = reinterpret_cast<const uint4 *>(tab)[i];
    __syncthreads();
    const size_t pairs = VEC ? m / 2 : 0, stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4 w = i < pairs ? reinterpret_cast<const uint4 *>(hands)[i] : uint4{0, 0, 0, 0};
    for (; i < pairs; i += stride) {
        const size_t nx = i + stride;
        uint2 r;
        r.x = eval7_tab(w.x, w.y, T); r.y = eval7_tab(w.z, w.w, T);
        reinterpret_cast<uint2 *>(out)[i] = r;
        if (nx < pairs) w = reinterpret_cast<const uint4 *>(hands)[nx];
    }
    if constexpr (VEC) {
        if ((m & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[m - 1] = eval7_tab((uint32_t)hands[m - 1], (uint32_t)(hands[m - 1] >> 32), T);
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) out[i] = eval7_tab((uint32_t)hands[i], (uint32_t)(hands[i] >> 32), T);
    }
}
// hand i = first 7 cards of the RNG-spec deck of (table_id = i, hand_serial = 0): the deal of a 1-seat table
__global__ void __launch_bounds__(256) k_make_hands(Hot H, size_t m, uint64_t *out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        Table<1> tb;
        tb.hand_serial = 0;
        tb.deal(H, (uint32_t)i);
        out[i] = (uint64_t)tb.cards[0] | ((uint64_t)(tb.cards[1] & 0x00ffffffu) << 32);
    }
}

// Exhaustive 7-card sweep used by tests (digest definition: tests/golden/make_eval_digest.py): all hands with prefix
// (a, b); hand index within the prefix -> combination of 5 from the cards above b is decoded per lane.
__global__ void k_eval7_prefix(int a, int b, int fast, uint32_t count, uint32_t *out, const uint32_t *tab) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    // unrank i among 5-subsets of {b+1..51} in lexicographic order
    int n = 51 - b;  // pool size
    int sel5[5];
    uint32_t r = i;
    int start = 0;
    for (int k = 5; k >= 1; --k) {
        for (int x = start;; ++x) {
            // C(n - x - 1, k - 1) hands start with element x
            uint32_t cnt = 1;
            int top = n - x - 1;
            if (top < k - 1) cnt = 0;
            else for (int j = 0; j < k - 1; ++j) cnt = cnt * (uint32_t)(top - j) / (uint32_t)(j + 1);
            if (r < cnt) { sel5[5 - k] = x; start = x + 1; break; }
            r -= cnt;
        }
    }
    auto canon = [](int c) { return (uint32_t)(((c % 4) << 4) | (c / 4)); };
    uint32_t h[7] = {canon(a), canon(b), canon(b + 1 + sel5[0]), canon(b + 1 + sel5[1]), canon(b + 1 + sel5[2]),
                     canon(b + 1 + sel5[3]), canon(b + 1 + sel5[4])};
    int nk;
    // fast 1: the in-game evaluator; 0: the general (multiset) evaluator; 2: the table-driven evaluator of the streaming
    // kernel (cards rotated by the hand index so that every byte position of the packed word is exercised)
    if (fast == 2) {
        uint32_t r[7];
        for (int j = 0; j < 7; ++j) r[j] = h[(j + i) % 7];
        out[i] = eval7_tab(r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24), r[4] | (r[5] << 8) | (r[6] << 16) | 0xAB000000u, tab);
    } else if (fast == 4) {                                  // the table path of pk_eval_hands(_d), cards rotated likewise
        uint32_t r[7];
        for (int j = 0; j < 7; ++j) r[j] = h[(j + i) % 7];
        out[i] = eval_tab_n(r, 7, tab, nk);
    } else if (fast == 3) out[i] = eval_hand_any(h, 7, nk);   // pk_eval_hands' register dispatch (its fast path: eval_distinct_n)
    else out[i] = fast ? eval7_distinct(h) : eval_hand(h, 7, nk);
}
