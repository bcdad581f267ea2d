// pk_equity.hip -- showdown equity by exhaustive enumeration of the boards still to come (include/pokerl_hip.h "Showdown equity",
// DESIGN.md section 3.1).  Two kernels per call:
//   k_equity_prep   one lane per spot: reads the spot (explicit arrays, or a handle's own tables), checks it, writes its descriptor (bit
//                   sets, pool, board count), its `boards` / `status`, zeroes the count outputs and cuts the spot into TASKS of one
//                   wavefront each (eq_lpt: a spot of up to 64 * lpt boards is one task, a pre-flop spot many);
//   k_equity<N>     a persistent grid of 512-thread workgroups, each with the 32 KB rank-mask table of eval7_tab in LDS (staged once per
//                   workgroup, whatever the number of spots).  A wavefront takes one task at a time: the spot is WAVE-UNIFORM (hole bit sets,
//                   live mask, known board in scalar registers; the pool as 64-bit card bits in LDS), every lane owns a contiguous range
//                   of board indices, unranks its first board once and then steps to the next combination.  A hand is
//                   board_bits | hole_bits[p]: no card bytes, no memory traffic per hand.  Counts are kept per lane, summed over the
//                   wavefront, and added to the outputs with 3 integer atomics per live seat and task.
// Ordinary vector stores and atomics only; no scratch memory (tests/test_equity_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity.hpp"

using namespace pk;

#define EQ_PREP_BLOCK 256

struct EqPrepArgs {
    EqSpots s;
    EqTables t;
    EqOut out;
    EqWork w;
    int N, lpt;
    size_t m;
};

template <bool TABLE>
__global__ void __launch_bounds__(EQ_PREP_BLOCK) k_equity_prep(EqPrepArgs a) {
    const size_t tid = (size_t)blockIdx.x * EQ_PREP_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * EQ_PREP_BLOCK;
    const int N = a.N;
    // the count outputs start at zero (k_equity adds to them); consecutive lanes, consecutive words
    const size_t cells = a.m * (size_t)N;
    for (size_t e = tid; e < cells; e += nthreads) {
        if (a.out.win) a.out.win[e] = 0;
        if (a.out.tie) a.out.tie[e] = 0;
        if (a.out.share) a.out.share[e] = 0;
    }
    uint32_t ntask = 0;
    if (tid < a.m) {
        const size_t i = tid;
        uint64_t *d = a.w.desc + i * (size_t)(3 + N);
        uint32_t status = 0, live = 0;
        int nb = 0;
        uint64_t dead = 0, known = 0;
        // one card byte: its bit in the suit-lane layout (0 for "unknown"); marks it dead; a byte that is no card, or a card seen before, is refused
        auto card = [&](uint32_t c, bool required) -> uint64_t {
            if (c == 0xffu) { status |= required ? (uint32_t)PK_EQ_BAD_CARD : 0u; return 0; }
            if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; return 0; }
            const uint64_t bit = 1ull << ((c & 15u) * 4u + (c >> 4));              // canonical index (cards.py:77)
            status |= (dead & bit) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
            dead |= bit;
            return 4ull << c;
        };
        const uint32_t seats = (1u << N) - 1u;
        bool readable = true;
        if constexpr (TABLE) {
            const int64_t t = a.t.tables ? (int64_t)a.t.tables[i] : (int64_t)i;
            if (t < 0 || t >= (int64_t)a.t.T) { status |= PK_EQ_BAD_TABLE; readable = false; }
            else {
                // (Cursor::in_flight(), SeatStates' masks, card_byte() by hand: through them this kernel is scheduled differently; its code is kept as it is)
                const Cursor cur{a.t.cursors[t]};
                if (cur.w >> 20) status |= PK_EQ_IN_FLIGHT;
                const int turn = (int)cur.turn();
                nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);                 // game.py:266-278
                const uint64_t ss = a.t.seat_states[t];
                live = (uint32_t)(ss | (ss >> 16) | (ss >> 32)) & 0xffffu & seats;   // ACTIVE | CALLED | ALL_IN
                const int K = 5 + 2 * N;
                uint32_t word = 0;
                uint64_t hb = 0;
                for (int pos = 0; pos < K; ++pos) {
                    if ((pos & 3) == 0) word = a.t.cards[(size_t)(pos >> 2) * a.t.T + t];
                    const uint32_t c = (word >> (8 * (pos & 3))) & 0xffu;
                    if (pos < 5) { if (pos < nb) known |= card(c, true); }           // (the future board cards the deck holds are unknown)
                    else {
                        hb |= card(c, true);
                        if (((pos - 5) & 1) == 1) { d[3 + ((pos - 5) >> 1)] = hb; hb = 0; }
                    }
                }
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
        }
        if (readable && live == 0) status |= PK_EQ_NO_LIVE;
        const uint32_t P = 52u - (uint32_t)__popcll(dead), k = (uint32_t)(5 - nb);
        const uint32_t boards = status ? 0u : eq_binom(P, k);
        d[0] = known;
        d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
        d[2] = (uint64_t)boards | ((uint64_t)live << 32) | ((uint64_t)k << 48) | ((uint64_t)P << 56);
        if (a.out.boards) a.out.boards[i] = boards;
        if (a.out.status) a.out.status[i] = (uint8_t)status;
        const uint32_t per = 64u * (uint32_t)a.lpt;
        ntask = (boards + per - 1) / per;
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
    if (lane == 63 && total) base = atomicAdd(&a.w.ctrl->ntasks, total);
    base = __shfl(base, 63);
    const size_t first = (size_t)base + incl - ntask;
    for (uint32_t c = 0; c < ntask; ++c)
        if (first + c < a.w.task_cap) a.w.tasks[first + c] = make_uint2((uint32_t)tid, c);
}


// registers per lane: eight waves per SIMD (64) up to three seats, four (128) up to eight, two beyond -- no spill at any seat count
template <int N> constexpr int eq_min_waves() { return N <= 3 ? 8 : (N <= 8 ? 4 : 2); }

template <int N>
__global__ void __launch_bounds__(EQ_BLOCK, eq_min_waves<N>()) k_equity(const uint32_t *__restrict__ tab, EqWork W, EqOut out, int lpt_max) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t pool[EQ_WAVES][64];
    __shared__ uint32_t wt[32];
    const uint32_t listed = W.ctrl->ntasks;
    const uint32_t ntasks = listed < W.task_cap ? listed : (uint32_t)W.task_cap;
    if (blockIdx.x * EQ_WAVES >= ntasks) return;                 // (the whole workgroup: before the table is staged)
    stage_eval7_tab<EQ_BLOCK>(T, tab);
    fill_share_weights(wt);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6), nwaves = gridDim.x * EQ_WAVES;
    uint64_t *mypool = pool[PK_IDX(wave, EQ_WAVES, "pool")];
    // Tasks are taken in runs of `take` consecutive ones: a wavefront's first run is its own number, the next ones come from the counter,
    // fetched one run ahead.  One task per run while there are few (a lone pre-flop spot must spread over every CU); four once there are
    // eight per wavefront -- 65 536 one-task spots would otherwise queue 65 536 atomics on ONE address.
    const uint32_t take = ntasks >= 8u * nwaves ? 4u : 1u;
    uint32_t t = (blockIdx.x * EQ_WAVES + wave) * take, left = take, fetched = 0;
    while (t < ntasks) {
        if (left == take) {
            fetched = 0;
            if (lane == 0) fetched = atomicAdd(&W.ctrl->next, 1u);
        }
        const uint2 task = W.tasks[t];
        const uint32_t spot = uniform(task.x), chunk = uniform(task.y);
        const uint64_t *d = W.desc + (size_t)spot * (3 + N);
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        uint64_t hole[N];
        PK_FOR(p, N) hole[p] = uniform(d[3 + p]); PK_END
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
        uint32_t sole[N], inw[N], sh[N];
        PK_FOR(p, N) sole[p] = 0; inw[p] = 0; sh[p] = 0; PK_END
        for (uint32_t n = 0; n < cnt; ++n) {
            const uint64_t bits = base | mypool[PK_IDX(j, 64, "mypool") & 63u];
            uint32_t v[N];
            PK_FOR(p, N)
                v[p] = NONE_V;                                                        // eval_hand([]) of a seat that does not show down
                if ((live >> p) & 1u) v[p] = eval7_tab_back(eval7_tab_front_bits(bits | hole[p], T), T);
            PK_END
            int nw;
            const uint32_t win = compare_rankings<N>(v, nw);
            const uint32_t w = wt[PK_IDX(nw, 32, "wt")];
            PK_FOR(p, N)
                if ((live >> p) & 1u) {
                    const bool in = (win >> p) & 1u;
                    sole[p] += win == (1u << p) ? 1u : 0u;
                    inw[p] += in ? 1u : 0u;
                    sh[p] += in ? w : 0u;
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
        // per seat: the wavefront's sums, then one atomic per output from lane 0
        PK_FOR(p, N)
            if ((live >> p) & 1u) {
                const uint32_t ws = wave_sum(sole[p]), wi = wave_sum(inw[p]);
                const uint64_t wsh = wave_sum((uint64_t)sh[p]);
                if (lane == 0) {
                    const size_t o = (size_t)spot * N + p;
                    if (out.win && ws) atomicAdd(&out.win[o], ws);
                    if (out.tie && wi != ws) atomicAdd(&out.tie[o], wi - ws);
                    if (out.share && wsh) atomicAdd(reinterpret_cast<unsigned long long *>(&out.share[o]), (unsigned long long)wsh);
                }
            }
        PK_END
        if (--left == 0) { t = (uniform(fetched) + nwaves) * take; left = take; }
        else ++t;
    }
}

namespace pk {

int eq_lpt(size_t m) { return m < 16 ? 16 : (m < 256 ? 64 : 1024); }

size_t eq_task_cap(size_t m, int lpt, int pool_max) {
    return m * (((size_t)eq_binom((uint32_t)pool_max, 5) + 64 * (size_t)lpt - 1) / (64 * (size_t)lpt));
}

size_t eq_layout(int N, size_t m, int lpt, int pool_max, char *base, EqWork *w) {
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t cap = eq_task_cap(m, lpt, pool_max);
    size_t off = 0;
    EqWork r{};
    r.ctrl = (EqCtrl *)(base + off); off += align(sizeof(EqCtrl));
    r.desc = (uint64_t *)(base + off); off += align(m * (size_t)(3 + N) * 8);
    r.tasks = (uint2 *)(base + off); off += align(cap * sizeof(uint2));
    r.task_cap = cap;
    if (w) *w = r;
    return off;
}

template <int N>
static bool eq_dispatch(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const EqWork &w, const EqOut &out, int lpt) {
    if constexpr (N > PK_MAX_PLAYERS) return false;
    else {
        if (n == N) {
            if constexpr (EQ_SEAT_ENABLED(N)) { hipLaunchKernelGGL(k_equity<N>, dim3(grid), dim3(EQ_BLOCK), 0, stream, tab, w, out, lpt); return true; }
            else return false;
        }
        return eq_dispatch<N + 1>(n, stream, grid, tab, w, out, lpt);
    }
}

hipError_t eq_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const EqTables *tables, int N, size_t m, const EqOut &out,
                     const EqWork &w, int lpt) {
    if (m == 0) return hipSuccess;
    if (lpt < 1 || lpt > EQ_LPT_MAX || w.task_cap > EQ_TASKS_MAX) return hipErrorInvalidValue;   // (32-bit share sums per lane, 32-bit task count)
    hipError_t e = hipMemsetAsync(w.ctrl, 0, sizeof(EqCtrl), stream);
    if (e != hipSuccess) return e;
    EqPrepArgs a{};
    if (spots) a.s = *spots;
    if (tables) a.t = *tables;
    a.out = out; a.w = w; a.N = N; a.lpt = lpt; a.m = m;
    const dim3 pgrid((unsigned)((m + EQ_PREP_BLOCK - 1) / EQ_PREP_BLOCK));
    if (tables) hipLaunchKernelGGL(k_equity_prep<true>, pgrid, dim3(EQ_PREP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_equity_prep<false>, pgrid, dim3(EQ_PREP_BLOCK), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // no more workgroups than there can be tasks for (each stages the 32 KB table); the grid is persistent beyond that
    const size_t want = (w.task_cap + EQ_WAVES - 1) / EQ_WAVES;
    const unsigned grid = (unsigned)(want < (size_t)EQ_GRID_MAX ? want : (size_t)EQ_GRID_MAX);
    if (!eq_dispatch<PK_MIN_PLAYERS>(N, stream, grid, tab, w, out, lpt)) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace pk
