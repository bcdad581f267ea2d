// pk_equity_ev.hip -- showdown EV in chips: Game.end_hand's side pots over every board still to come (include/pokerl_hip.h "Showdown EV",
// DESIGN.md section 3.7).  The pot is paid out in LEVELS (game.py:494-531): seats are visited in ascending bet order, each visit's amount
// depends on the bets alone, only its winner set depends on the board.  Three kernels per call:
//   k_ev_prep<N, TABLE>  one lane per spot: section 3.1's checks and descriptor, the bets (the table form: bets + pending_bets), the level
//                        loop in binary64 (np_sum<N>) -> level_seat, amount and the spot's level table; zeroes the share counters and cuts
//                        the spot into tasks (section 3.1's split rule, times the GROUPS of levels that hold a level to compare);
//   k_ev<N>              shaped like k_equity<N> (pk_equity.hip): a persistent grid of 512-thread workgroups, the evaluator table in LDS, the
//                        spot wave-uniform, the same unranking and stepping, ONE evaluation per live seat and board -- then per level of the
//                        task's group compare_rankings<N> on v masked by the level's remain mask (a scalar: the masking is a select), a
//                        32-bit share counter per (level, seat), wave sums, one 64-bit atomic per counter from lane 0;
//   k_ev_finish          one lane per (spot, seat): the last stand's share, then ev in the stated order, every operation rounded on its own.
// Ordinary vector stores and atomics only; no scratch memory (tests/test_equity_ev_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_ev.hpp"

using namespace pk;

#define EV_PREP_BLOCK 256
#define EV_FINISH_BLOCK 256

struct EvPrepArgs {
    EqSpots s;
    const double *bets;   // the explicit form: [m][N]
    EvTables t;
    EvOut out;
    EvWork w;
    int lpt;
    size_t m;
};

// negative (not -0.0), infinite or NaN: read from the bits -- the build does not honour NaNs in comparisons (build.py)
__device__ __forceinline__ bool ev_bad_bet(double b) {
    const uint64_t u = (uint64_t)__double_as_longlong(b);
    return ((u >> 63) && u != 0x8000000000000000ull) || ((u >> 52) & 0x7ffu) == 0x7ffu;
}

template <int N, bool TABLE>
__global__ void __launch_bounds__(EV_PREP_BLOCK) k_ev_prep(EvPrepArgs a) {
    const size_t tid = (size_t)blockIdx.x * EV_PREP_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * EV_PREP_BLOCK;
    constexpr int G = ev_group(N);
    // the share counters start at zero (k_ev adds to them); consecutive lanes, consecutive words
    const size_t cells = a.m * (size_t)(N * N);
    for (size_t e = tid; e < cells; e += nthreads) a.w.share[e] = 0;
    uint32_t ntask = 0, nch = 0, gmask = 0;
    if (tid < a.m) {
        const size_t i = tid;
        uint64_t *d = a.w.eq.desc + i * (size_t)(3 + N);
        uint32_t status = 0, live = 0;
        int nb = 0;
        uint64_t dead = 0, known = 0;
        double bets[N];
        PK_FOR(p, N) bets[p] = 0.0; PK_END
        // one card byte: its bit in the suit-lane layout (0 for "unknown"); marks it dead; a byte that is no card, or a card seen before, is refused
        auto card = [&](uint32_t c, bool required) -> uint64_t {
            if (c == 0xffu) { status |= required ? (uint32_t)PK_EQ_BAD_CARD : 0u; return 0; }
            if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; return 0; }
            const uint64_t bit = 1ull << ((c & 15u) * 4u + (c >> 4));              // canonical index (cards.py:77)
            status |= (dead & bit) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
            dead |= bit;
            return 4ull << c;
        };
        constexpr uint32_t seats = (1u << N) - 1u;
        bool readable = true;
        if constexpr (TABLE) {
            const int64_t t = a.t.t.tables ? (int64_t)a.t.t.tables[i] : (int64_t)i;
            if (t < 0 || t >= (int64_t)a.t.t.T) { status |= PK_EQ_BAD_TABLE; readable = false; }
            else {
                const size_t T = (size_t)a.t.t.T;
                const uint32_t cur = a.t.t.cursors[t];
                if (cur >> 20) status |= PK_EQ_IN_FLIGHT;
                const int turn = (int)Cursor{cur}.turn();
                nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);                 // game.py:266-278
                const uint64_t ss = a.t.t.seat_states[t];
                live = (uint32_t)(ss | (ss >> 16) | (ss >> 32)) & 0xffffu & seats;   // ACTIVE | CALLED | ALL_IN
                constexpr int K = 5 + 2 * N;
                uint32_t word = 0;
                uint64_t hb = 0;
                for (int pos = 0; pos < K; ++pos) {
                    if ((pos & 3) == 0) word = a.t.t.cards[(size_t)(pos >> 2) * T + t];
                    const uint32_t c = (word >> (8 * (pos & 3))) & 0xffu;
                    if (pos < 5) { if (pos < nb) known |= card(c, true); }           // (the future board cards the deck holds are unknown)
                    else {
                        hb |= card(c, true);
                        if (((pos - 5) & 1) == 1) { d[3 + ((pos - 5) >> 1)] = hb; hb = 0; }
                    }
                }
                PK_FOR(p, N) bets[p] = a.t.bets[(size_t)p * T + t] + a.t.pending[(size_t)p * T + t]; PK_END   // the commit of game.py:457
            }
        } else {
            const uint32_t nbv = a.s.nboard[i];
            if (nbv > 5u) status |= PK_EQ_BAD_NBOARD;
            nb = nbv > 5u ? 0 : (int)nbv;
            live = (uint32_t)a.s.live[i] & seats;
            for (int j = 0; j < nb; ++j) known |= card(a.s.board[i * 5 + j], true);
            for (int p = 0; p < N; ++p) {
                const bool lv = (live >> p) & 1u;
                const uint8_t *hc = a.s.holes + (i * (size_t)N + p) * 2;
                uint64_t hb = card(hc[0], lv);
                hb |= card(hc[1], lv);
                d[3 + p] = hb;
            }
            PK_FOR(p, N) bets[p] = a.bets[i * (size_t)N + p]; PK_END
        }
        if (readable && live == 0) status |= PK_EQ_NO_LIVE;
        bool bad = false;
        PK_FOR(p, N) bad = bad || ev_bad_bet(bets[p]); PK_END
        if (bad) status |= PK_EQ_BAD_BET;
        const uint32_t P = 52u - (uint32_t)__popcll(dead), k = (uint32_t)(5 - nb);
        const uint32_t boards = status ? 0u : eq_binom(P, k);
        d[0] = known;
        d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
        d[2] = (uint64_t)boards | ((uint64_t)live << 32) | ((uint64_t)k << 48) | ((uint64_t)P << 56);
        if (a.out.boards) a.out.boards[i] = boards;
        a.out.status[i] = (uint8_t)status;
        // ---- the levels (game.py:494-525): bets and live seats only
        double work[N];
        PK_FOR(p, N) work[p] = bets[p]; a.w.bets[i * (size_t)N + p] = bets[p]; PK_END
        uint32_t todo = status ? 0u : live, remain = live;
        int nrem = __popc(live);
        bool done = status != 0;
#pragma unroll 1
        for (int it = 0; it < N; ++it) {
            uint32_t rec = 0, seat = 0xffu;
            double amt = 0.0;
            if (!done && todo) {
                int s = 0; double best = 0.0, mx = 0.0; bool have = false;
                PK_FOR(p, N)                                                       // next seat in ascending bet order, stable (:495-496)
                    const bool cand = (todo >> p) & 1u;
                    const bool better = cand && (!have || bets[p] < best);
                    s = better ? p : s; best = better ? bets[p] : best; mx = better ? work[p] : mx;
                    have = have || cand;
                PK_END
                todo &= ~(1u << s);
                bool left = false;                                                 // any bet still > 0 (:499)
                PK_FOR(p, N) left = left || work[p] > 0.0; PK_END
                if (!left) done = true;
                else if (nrem == 1) {                                              // the last stand (:500-505)
                    amt = np_sum<N>(work);
                    rec = remain | ((uint32_t)s << 16) | EV_EXISTS | EV_LAST;
                    seat = (uint32_t)s;
                    done = true;
                } else {
                    double mb[N];                                                  // :509 np.clip(bets, 0, max_bet)
                    PK_FOR(p, N) double x = work[p]; x = (x < 0.0) ? 0.0 : x; x = (x > mx) ? mx : x; mb[p] = x; PK_END
                    amt = np_sum<N>(mb);
                    rec = remain | ((uint32_t)s << 16) | EV_EXISTS | (amt > 0.0 ? EV_COMPARE : 0u);
                    seat = (uint32_t)s;
                    gmask |= amt > 0.0 ? 1u << (it / G) : 0u;
                    remain &= ~(1u << s); nrem -= 1;                               // :522, :525
                    PK_FOR(p, N) work[p] = work[p] - mb[p]; PK_END                 // :523
                }
            }
            a.w.levels[i * (size_t)N + it] = rec;
            a.w.amount[i * (size_t)N + it] = amt;
            if (a.out.amount) a.out.amount[i * (size_t)N + it] = amt;
            if (a.out.level_seat) a.out.level_seat[i * (size_t)N + it] = (uint8_t)seat;
        }
        const uint32_t per = 64u * (uint32_t)a.lpt;
        nch = (boards + per - 1) / per;
        ntask = nch * (uint32_t)__popc(gmask);
    }
    // a range of the task list per spot: one atomic per wavefront (inclusive scan over its lanes)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t incl = ntask;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        incl += lane >= (uint32_t)off ? v : 0u;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(&a.w.eq.ctrl->ntasks, total);
    base = __shfl(base, 63);
    size_t slot = (size_t)base + incl - ntask;
    for (uint32_t g = 0; g < (uint32_t)ev_groups_max(N); ++g)
        if ((gmask >> g) & 1u)
            for (uint32_t c = 0; c < nch; ++c, ++slot)
                if (slot < a.w.eq.task_cap) a.w.eq.tasks[slot] = make_uint2((uint32_t)tid, c | (g << 24));
}


// registers per lane: as k_equity<N> -- its 3 N counters are this kernel's ev_group(N) * N
template <int N> constexpr int ev_min_waves() { return N <= 3 ? 8 : (N <= 8 ? 4 : 2); }

template <int N>
__global__ void __launch_bounds__(EQ_BLOCK, ev_min_waves<N>()) k_ev(const uint32_t *__restrict__ tab, EvWork W, int lpt_max) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t pool[EQ_WAVES][64];
    __shared__ uint32_t wt[32];
    constexpr int G = ev_group(N);
    const uint32_t listed = W.eq.ctrl->ntasks;
    const uint32_t ntasks = listed < W.eq.task_cap ? listed : (uint32_t)W.eq.task_cap;
    if (blockIdx.x * EQ_WAVES >= ntasks) return;                 // (the whole workgroup: before the table is staged)
    stage_eval7_tab<EQ_BLOCK>(T, tab);
    fill_share_weights(wt);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6), nwaves = gridDim.x * EQ_WAVES;
    uint64_t *mypool = pool[PK_IDX(wave, EQ_WAVES, "pool")];
    // tasks are taken in runs, as k_equity takes them
    const uint32_t take = ntasks >= 8u * nwaves ? 4u : 1u;
    uint32_t t = (blockIdx.x * EQ_WAVES + wave) * take, left = take, fetched = 0;
    while (t < ntasks) {
        if (left == take) {
            fetched = 0;
            if (lane == 0) fetched = atomicAdd(&W.eq.ctrl->next, 1u);
        }
        const uint2 task = W.eq.tasks[t];
        const uint32_t spot = uniform(task.x), ty = uniform(task.y), chunk = ty & 0xffffffu, first = (ty >> 24) * (uint32_t)G;
        const uint64_t *d = W.eq.desc + (size_t)spot * (3 + N);
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        uint64_t hole[N];
        PK_FOR(p, N) hole[p] = uniform(d[3 + p]); PK_END
        // the levels of this task's group: remain mask and flags, scalars (0: no level here)
        uint32_t lv[G];
        PK_FOR(c, G)
            lv[c] = 0;
            if (first + c < (uint32_t)N) lv[c] = uniform(W.levels[(size_t)spot * N + first + c]);
        PK_END
        const uint32_t boards = (uint32_t)meta, mhi = (uint32_t)(meta >> 32), live = mhi & 0xffffu, k = (mhi >> 16) & 0xffu, P = mhi >> 24;
        // this task's boards [start, end) of the spot's, and this lane's [s, s + cnt) of those
        const uint32_t per_max = 64u * (uint32_t)lpt_max, nch = (boards + per_max - 1) / per_max, per = (boards + nch - 1) / nch;
        const uint32_t start = chunk * per, end = min(boards, start + per), nt = end > start ? end - start : 0u;
        const uint32_t l = (nt + 63u) / 64u, s = start + lane * l;
        const uint32_t cnt = s < end ? min(l, end - s) : 0u;
        eq_fill_wave_pool(mypool, avail, lane);
        // combination levels 0 .. 4 (ascending pool indices c0 < c1 < c2 < c3 < j), the first 5 - k of them frozen on the empty slot;
        // lim[t]: the highest index level t may still be raised FROM (-1: never)
        const int f = 5 - (int)k;
        const int lim0 = f <= 0 ? (int)P - 5 : -1, lim1 = f <= 1 ? (int)P - 4 : -1, lim2 = f <= 2 ? (int)P - 3 : -1, lim3 = f <= 3 ? (int)P - 2 : -1;
        uint32_t c0 = COMB_FROZEN, c1 = COMB_FROZEN, c2 = COMB_FROZEN, c3 = COMB_FROZEN, j = COMB_FROZEN;
        if (cnt) {     // unrank board index s (lexicographic): C(P - 1 - x, levels left) boards start with x at a level
            uint32_t r = s, x = 0;
            auto level = [&](auto jc) {
                constexpr int J = decltype(jc)::value;
                while (x < P) {
                    const uint32_t c = binom_c<J>(P - 1u - x);
                    if (r < c) break;
                    r -= c; ++x;
                }
                return x++;
            };
            if (f <= 0) c0 = level(std::integral_constant<int, 4>{});
            if (f <= 1) c1 = level(std::integral_constant<int, 3>{});
            if (f <= 2) c2 = level(std::integral_constant<int, 2>{});
            if (f <= 3) c3 = level(std::integral_constant<int, 1>{});
            if (f <= 4) j = x + r;
        }
        uint64_t base = known | mypool[PK_IDX(c0, 64, "mypool")] | mypool[PK_IDX(c1, 64, "mypool")] | mypool[PK_IDX(c2, 64, "mypool")] | mypool[PK_IDX(c3, 64, "mypool")];
        uint32_t sh[G][N];
        PK_FOR(c, G) PK_FOR(p, N) sh[c][p] = 0; PK_END PK_END
        for (uint32_t n = 0; n < cnt; ++n) {
            const uint64_t bits = base | mypool[PK_IDX(j, 64, "mypool") & 63u];
            uint32_t v[N];
            PK_FOR(p, N)
                v[p] = NONE_V;                                                        // eval_hand([]) of a seat that does not show down
                if ((live >> p) & 1u) v[p] = eval7_tab_back(eval7_tab_front_bits(bits | hole[p], T), T);
            PK_END
            PK_FOR(c, G)
                if (lv[c] & EV_COMPARE) {                                             // (a scalar: the whole wavefront takes the branch)
                    uint32_t vm[N];
                    PK_FOR(p, N) vm[p] = ((lv[c] >> p) & 1u) ? v[p] : NONE_V; PK_END   // :522 the seats paid out below this level
                    int nw;
                    const uint32_t win = compare_rankings<N>(vm, nw);
                    const uint32_t w = wt[PK_IDX(nw, 32, "wt")];
                    PK_FOR(p, N) sh[c][p] += ((win >> p) & 1u) ? w : 0u; PK_END
                }
            PK_END
            // next combination: the last card moves on; when it runs out, the deepest level that can still rise does, and the ones after it follow
            ++j;
            if (j >= P) {
                if ((int)c3 < lim3) { ++c3; }
                else if ((int)c2 < lim2) { ++c2; c3 = c2 + 1; }
                else if ((int)c1 < lim1) { ++c1; c2 = c1 + 1; c3 = c2 + 1; }
                else if ((int)c0 < lim0) { ++c0; c1 = c0 + 1; c2 = c1 + 1; c3 = c2 + 1; }
                else { c3 = COMB_FROZEN - 1; }                                          // (past the spot's last board: never evaluated)
                j = c3 + 1;
                base = known | mypool[PK_IDX(c0, 64, "mypool") & 63u] | mypool[PK_IDX(c1, 64, "mypool") & 63u] | mypool[PK_IDX(c2, 64, "mypool") & 63u] | mypool[PK_IDX(c3, 64, "mypool") & 63u];
            }
        }
        // per level and seat in its remain mask: the wavefront's sum, then one atomic from lane 0
        PK_FOR(c, G)
            if (lv[c] & EV_COMPARE) {
                PK_FOR(p, N)
                    if ((lv[c] >> p) & 1u) {
                        const uint64_t wsh = wave_sum((uint64_t)sh[c][p]);
                        if (lane == 0 && wsh)
                            atomicAdd(reinterpret_cast<unsigned long long *>(&W.share[((size_t)spot * N + first + c) * N + p]), (unsigned long long)wsh);
                    }
                PK_END
            }
        PK_END
        if (--left == 0) { t = (uniform(fetched) + nwaves) * take; left = take; }
        else ++t;
    }
}

// One lane per (spot, seat p): the last stand's share row, then
//   acc = +0.0;  for i ascending: acc = acc + (amount[i] * (double)share[i][p]) / (720720.0 * (double)boards);  ev[p] = acc - bets[p]
// every operation rounded on its own (-ffp-contract=off).  A refused spot (boards = 0): ev = 0.
__global__ void __launch_bounds__(EV_FINISH_BLOCK) k_ev_finish(EvWork W, double *__restrict__ ev, int N, size_t m) {
    const size_t e = (size_t)blockIdx.x * EV_FINISH_BLOCK + threadIdx.x;
    if (e >= m * (size_t)N) return;
    const size_t spot = e / (size_t)N;
    const uint32_t p = (uint32_t)(e - spot * (size_t)N);
    const uint32_t boards = (uint32_t)W.eq.desc[spot * (size_t)(3 + N) + 2];
    double acc = 0.0;
    if (boards) {
        const double den = (double)EQ_SHARE_UNIT * (double)boards;
        for (int i = 0; i < N; ++i) {
            const uint32_t rec = W.levels[spot * (size_t)N + i];
            uint64_t *cell = &W.share[(spot * (size_t)N + i) * N + p];
            uint64_t sh = *cell;
            if ((rec & EV_LAST) && ((rec >> 16) & 0xffu) == p) { sh = (uint64_t)EQ_SHARE_UNIT * boards; *cell = sh; }
            acc = acc + (W.amount[spot * (size_t)N + i] * (double)sh) / den;
        }
        acc = acc - W.bets[e];
    }
    if (ev) ev[e] = acc;
}

namespace pk {

size_t ev_task_cap(int N, size_t m, int lpt, int pool_max) {
    return m * (((size_t)eq_binom((uint32_t)pool_max, 5) + 64 * (size_t)lpt - 1) / (64 * (size_t)lpt)) * (size_t)ev_groups_max(N);
}

size_t ev_layout(int N, size_t m, int lpt, int pool_max, bool own_share, char *base, EvWork *w) {
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t cap = ev_task_cap(N, m, lpt, pool_max);
    size_t off = 0;
    EvWork r{};
    r.eq.ctrl = (EqCtrl *)(base + off); off += align(sizeof(EqCtrl));
    r.eq.desc = (uint64_t *)(base + off); off += align(m * (size_t)(3 + N) * 8);
    r.levels = (uint32_t *)(base + off); off += align(m * (size_t)N * 4);
    r.bets = (double *)(base + off); off += align(m * (size_t)N * 8);
    r.amount = (double *)(base + off); off += align(m * (size_t)N * 8);
    if (own_share) { r.share = (uint64_t *)(base + off); off += align(m * (size_t)N * N * 8); }
    r.eq.tasks = (uint2 *)(base + off); off += align(cap * sizeof(uint2));
    r.eq.task_cap = cap;
    if (w) *w = r;
    return off;
}

template <int N>
static bool ev_dispatch(int n, hipStream_t stream, bool table, unsigned pgrid, const EvPrepArgs &a, unsigned grid, const uint32_t *tab) {
    if constexpr (N > PK_MAX_PLAYERS) return false;
    else {
        if (n == N) {
            if constexpr (EQ_SEAT_ENABLED(N)) {
                if (table) hipLaunchKernelGGL((k_ev_prep<N, true>), dim3(pgrid), dim3(EV_PREP_BLOCK), 0, stream, a);
                else hipLaunchKernelGGL((k_ev_prep<N, false>), dim3(pgrid), dim3(EV_PREP_BLOCK), 0, stream, a);
                hipLaunchKernelGGL(k_ev<N>, dim3(grid), dim3(EQ_BLOCK), 0, stream, tab, a.w, a.lpt);
                return true;
            } else return false;
        }
        return ev_dispatch<N + 1>(n, stream, table, pgrid, a, grid, tab);
    }
}

hipError_t ev_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const double *bets, const EvTables *tables, int N, size_t m,
                     const EvOut &out, const EvWork &w_in, int lpt) {
    if (m == 0) return hipSuccess;
    EvWork w = w_in;
    if (out.share) w.share = out.share;      // the counters are the caller's array where there is one
    if (!out.status || !w.share || lpt < 1 || lpt > EQ_LPT_MAX || w.eq.task_cap > EQ_TASKS_MAX) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(w.eq.ctrl, 0, sizeof(EqCtrl), stream);
    if (e != hipSuccess) return e;
    EvPrepArgs a{};
    if (spots) a.s = *spots;
    a.bets = bets;
    if (tables) a.t = *tables;
    a.out = out; a.w = w; a.lpt = lpt; a.m = m;
    const unsigned pgrid = (unsigned)((m + EV_PREP_BLOCK - 1) / EV_PREP_BLOCK);
    // no more workgroups than there can be tasks for (each stages the 32 KB table); the grid is persistent beyond that
    const size_t want = (w.eq.task_cap + EQ_WAVES - 1) / EQ_WAVES;
    const unsigned grid = (unsigned)(want < (size_t)EQ_GRID_MAX ? want : (size_t)EQ_GRID_MAX);
    if (!ev_dispatch<PK_MIN_PLAYERS>(N, stream, tables != nullptr, pgrid, a, grid, tab)) return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t lanes = m * (size_t)N;
    hipLaunchKernelGGL(k_ev_finish, dim3((unsigned)((lanes + EV_FINISH_BLOCK - 1) / EV_FINISH_BLOCK)), dim3(EV_FINISH_BLOCK), 0, stream, w, out.ev, N, m);
    return hipGetLastError();
}

}  // namespace pk
