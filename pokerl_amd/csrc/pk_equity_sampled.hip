// pk_equity_sampled.hip -- showdown equity by Monte Carlo sampling: hole cards a seat cannot see are DRAWN, not enumerated
// (include/pokerl_hip.h "Sampled showdown equity").  Two kernels per call:
//   k_eqs_prep   one lane per spot: reads the spot (explicit arrays, or a handle's own tables as one seat sees them), checks it, writes its
//                descriptor (known bit sets, hidden-byte mask, pool, counts, stream id), its `samples` / `status`, and zeroes the count outputs;
//   k_eqs<N>     a persistent grid of 512-thread workgroups, each with the 32 KB rank-mask table of eval7_tab in LDS.  Every valid spot is
//                cut into the same number of tasks, so task -> (spot, chunk) is a division: no task list.  A wavefront takes one task at a
//                time: the spot is WAVE-UNIFORM (scalar registers), every lane owns a contiguous run of sample indices.  Per sample a lane
//                generates its Philox blocks, draws the hidden cards by selecting the c-th set bit of its remaining-pool mask (registers
//                only), ORs them into the board / hole bit sets and evaluates every live seat.  Counts are kept per lane, summed over the
//                wavefront, and added to the outputs with 3 integer atomics per live seat and task.
// Ordinary vector stores and atomics only; no scratch memory (tests/test_equity_sampled_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_sampled.hpp"

using namespace pk;

#define EQS_PREP_BLOCK 256

struct EqsPrepArgs {
    EqSpots s;
    EqTables t;
    EqsStream rng;
    EqsOut out;
    uint64_t *desc;
    int N, observer;
    size_t m;
};

template <bool TABLE>
__global__ void __launch_bounds__(EQS_PREP_BLOCK) k_eqs_prep(EqsPrepArgs a) {
    const size_t tid = (size_t)blockIdx.x * EQS_PREP_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * EQS_PREP_BLOCK;
    const int N = a.N;
    // the count outputs start at zero (k_eqs adds to them); consecutive lanes, consecutive words
    const size_t cells = a.m * (size_t)N;
    for (size_t e = tid; e < cells; e += nthreads) {
        if (a.out.win) a.out.win[e] = 0;
        if (a.out.tie) a.out.tie[e] = 0;
        if (a.out.share) a.out.share[e] = 0;
    }
    if (tid >= a.m) return;
    const size_t i = tid;
    uint64_t *d = a.desc + i * (size_t)eqs_desc_words(N);
    uint32_t status = 0, live = 0, hidden = 0, id = 0;
    int nb = 0;
    uint64_t dead = 0, known = 0;
    // one card byte: its bit in the suit-lane layout (0 for 0xFF); marks it dead; a byte that is no card, or a card seen before, is refused
    auto card = [&](uint32_t c, bool required) -> uint64_t {
        if (c == 0xffu) { status |= required ? (uint32_t)PK_EQ_BAD_CARD : 0u; return 0; }
        if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; return 0; }
        const uint64_t bit = 1ull << ((c & 15u) * 4u + (c >> 4));              // canonical index (cards.py:77)
        status |= (dead & bit) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
        dead |= bit;
        return 4ull << c;
    };
    // seat p's two hole bytes: a card is known and dead; 0xFF is hidden (drawn) at a live seat and simply in the pool at any other
    auto seat = [&](int p, uint32_t c0, uint32_t c1) {
        const uint32_t lv = (live >> p) & 1u;
        d[4 + p] = card(c0, false) | card(c1, false);
        hidden |= (lv && c0 == 0xffu ? 1u : 0u) << (2 * p);
        hidden |= (lv && c1 == 0xffu ? 2u : 0u) << (2 * p);
    };
    const uint32_t seats = (1u << N) - 1u;
    bool readable = true;
    if constexpr (TABLE) {
        const int64_t t = a.t.tables ? (int64_t)a.t.tables[i] : (int64_t)i;
        id = a.rng.id_base + (uint32_t)t;
        if (t < 0 || t >= (int64_t)a.t.T) { status |= PK_EQ_BAD_TABLE; readable = false; }   // (k_eqs reads no further than the valid bit)
        else {
            const Cursor cur{a.t.cursors[t]};
            if (cur.in_flight()) status |= PK_EQ_IN_FLIGHT;
            const int turn = (int)cur.turn();
            nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);                 // game.py:266-278
            const SeatStates ss{a.t.seat_states[t]};
            live = (ss.active() | ss.called() | ss.allin()) & seats;
            const int who = a.observer == PK_OBSERVER_ACTIVE ? (int)cur.active() : a.observer;   // PK_OBSERVER_NONE (-1): every seat's cards are known
            for (int j = 0; j < nb; ++j) known |= card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, j), true);
            for (int p = 0; p < N; ++p) {
                const bool seen = who < 0 || p == who;                             // (another seat's cards are not read at all: the observer never saw them)
                const uint32_t c0 = seen ? card_byte(a.t.cards, (size_t)a.t.T, (int)t, 5 + 2 * p) : 0xffu;
                const uint32_t c1 = seen ? card_byte(a.t.cards, (size_t)a.t.T, (int)t, 6 + 2 * p) : 0xffu;
                if (seen) { d[4 + p] = card(c0, true) | card(c1, true); }           // (a dealt deck holds no 0xFF)
                else seat(p, c0, c1);
            }
        }
    } else {
        id = a.rng.ids ? a.rng.ids[i] : (uint32_t)i;
        const uint32_t nbv = a.s.nboard[i];
        if (nbv > 5u) status |= PK_EQ_BAD_NBOARD;
        nb = nbv > 5u ? 0 : (int)nbv;
        live = (uint32_t)a.s.live[i] & seats;
        for (int j = 0; j < nb; ++j) known |= card(a.s.board[i * 5 + j], true);
        for (int p = 0; p < N; ++p) {
            const uint8_t *hc = a.s.holes + (i * (size_t)N + p) * 2;
            seat(p, hc[0], hc[1]);
        }
    }
    if (readable && live == 0) status |= PK_EQ_NO_LIVE;
    const uint32_t P = 52u - (uint32_t)__popcll(dead), k = (uint32_t)(5 - nb);
    d[0] = known;
    d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
    d[2] = (uint64_t)hidden | ((uint64_t)live << 32) | ((uint64_t)k << 48) | ((uint64_t)P << 56);
    d[3] = (uint64_t)id | ((uint64_t)(status ? 0u : 1u) << 32);
    if (a.out.samples) a.out.samples[i] = status ? 0u : a.rng.samples;
    if (a.out.status) a.out.status[i] = (uint8_t)status;
}


// registers per lane: the caps of k_equity<N> (eight waves per SIMD up to three seats, four up to eight, two beyond) -- no spill at any seat count
template <int N> constexpr int eqs_min_waves() { return N <= 3 ? 8 : (N <= 8 ? 4 : 2); }

template <int N>
__global__ void __launch_bounds__(EQ_BLOCK, eqs_min_waves<N>()) k_eqs(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, EqsOut out,
                                                                     EqsStream rng, uint32_t ntasks, uint32_t nch, uint32_t per) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint32_t wt[32];
    stage_eval7_tab<EQ_BLOCK>(T, tab);
    fill_share_weights(wt);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6), nwaves = gridDim.x * EQ_WAVES;
    const uint32_t S = rng.samples;
    // every task costs the same, so the tasks are dealt round robin: no counter
    for (uint32_t t = blockIdx.x * EQ_WAVES + wave; t < ntasks; t += nwaves) {
        const uint32_t spot = t / nch, chunk = t - spot * nch;
        const uint64_t *d = desc + (size_t)spot * eqs_desc_words(N);
        const uint64_t m3 = uniform(d[3]);
        if (!(m3 >> 32)) continue;                                   // a refused spot: no samples
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        uint64_t hole[N];
        PK_FOR(p, N) hole[p] = uniform(d[4 + p]); PK_END
        const uint32_t hidden = (uint32_t)meta, mhi = (uint32_t)(meta >> 32), live = mhi & 0xffffu, k = (mhi >> 16) & 0xffu, P = mhi >> 24;
        const uint32_t id = (uint32_t)m3, D = k + (uint32_t)__builtin_popcount(hidden);
        // this task's samples [start, end) of the spot's, and this lane's [s, s + cnt) of those
        const uint32_t start = chunk * per, end = min(S, start + per), nt = end - start;
        const uint32_t l = (nt + 63u) / 64u, s = start + lane * l;
        const uint32_t cnt = s < end ? min(l, end - s) : 0u;
        uint32_t sole[N], inw[N], sh[N];
        PK_FOR(p, N) sole[p] = 0; inw[p] = 0; sh[p] = 0; PK_END
        for (uint32_t n = 0; n < cnt; ++n) {
            // the 64-bit words of this sample's draws, 9 draws each: X[2b], X[2b + 1] of Philox block b (a queue: static indices only)
            uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0;
            uint32_t w[4];
            if (D > 0u) {
                philox4x32_10(id, s + n, STREAM_EQS, rng.nonce, rng.key0, rng.key1, w);
                q0 = (uint64_t)w[0] | ((uint64_t)w[1] << 32); q1 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            }
            if (D > 18u) {
                philox4x32_10(id, s + n, STREAM_EQS + 1u, rng.nonce, rng.key0, rng.key1, w);
                q2 = (uint64_t)w[0] | ((uint64_t)w[1] << 32); q3 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            }
            if (D > 36u) {
                philox4x32_10(id, s + n, STREAM_EQS + 2u, rng.nonce, rng.key0, rng.key1, w);
                q4 = (uint64_t)w[0] | ((uint64_t)w[1] << 32); q5 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            }
            uint64_t rem = avail;
            uint32_t xlo = 0, xhi = 0;
            // draw i (wave-uniform, ascending over the sample): the c_i-th card still in the pool, as its bit in the suit-lane layout
            auto draw = [&](uint32_t i) -> uint64_t {
                if (i % 9u == 0u) {
                    xlo = (uint32_t)q0; xhi = (uint32_t)(q0 >> 32);
                    q0 = q1; q1 = q2; q2 = q3; q3 = q4; q4 = q5;
                }
                const uint32_t left = P - i;                                       // chained multiply-high: c = (x * left) >> 64, x = the low 64 bits
                const uint64_t a = (uint64_t)xlo * left, b = (uint64_t)xhi * left + (a >> 32);
                xlo = (uint32_t)a; xhi = (uint32_t)b;
                const uint32_t c = select(rem, (uint32_t)(b >> 32));
                rem &= ~(1ull << c);
                return 4ull << (((c & 3u) << 4) | (c >> 2));
            };
            uint64_t bits = known;
            PK_FOR(j, 5) if ((uint32_t)j < k) bits |= draw((uint32_t)j); PK_END
            uint32_t v[N];
            PK_FOR(p, N)
                v[p] = NONE_V;                                                        // eval_hand([]) of a seat that does not show down
                if ((live >> p) & 1u) {
                    uint64_t h = bits | hole[p];
                    const uint32_t before = k + (uint32_t)__builtin_popcount(hidden & ((1u << (2 * p)) - 1u));
                    if ((hidden >> (2 * p)) & 1u) h |= draw(before);
                    if ((hidden >> (2 * p + 1)) & 1u) h |= draw(before + ((hidden >> (2 * p)) & 1u));
                    v[p] = eval7_tab_back(eval7_tab_front_bits(h, T), T);
                }
            PK_END
            int nw;
            const uint32_t win = compare_rankings<N>(v, nw);
            const uint32_t wsh = wt[PK_IDX(nw, 32, "wt")];
            PK_FOR(p, N)
                if ((live >> p) & 1u) {
                    const bool in = (win >> p) & 1u;
                    sole[p] += win == (1u << p) ? 1u : 0u;
                    inw[p] += in ? 1u : 0u;
                    sh[p] += in ? wsh : 0u;
                }
            PK_END
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
    }
}

namespace pk {

int eqs_lpt(size_t m, uint32_t samples) {
    const uint64_t runs = eqs_task_bound(m, samples);               // lane runs of 64 samples in the whole call
    const uint64_t lpt = (runs + EQS_TASKS_TARGET - 1) / EQS_TASKS_TARGET;
    return (int)(lpt < (uint64_t)EQS_LPT_MIN ? (uint64_t)EQS_LPT_MIN : (lpt > (uint64_t)EQS_LPT_MAX ? (uint64_t)EQS_LPT_MAX : lpt));
}

template <int N>
static bool eqs_dispatch(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const uint64_t *desc, const EqsOut &out, const EqsStream &rng,
                         uint32_t ntasks, uint32_t nch, uint32_t per) {
    if constexpr (N > PK_MAX_PLAYERS) return false;
    else {
        if (n == N) {
            if constexpr (EQ_SEAT_ENABLED(N)) {
                hipLaunchKernelGGL(k_eqs<N>, dim3(grid), dim3(EQ_BLOCK), 0, stream, tab, desc, out, rng, ntasks, nch, per);
                return true;
            } else return false;
        }
        return eqs_dispatch<N + 1>(n, stream, grid, tab, desc, out, rng, ntasks, nch, per);
    }
}

hipError_t eqs_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const EqTables *tables, int observer, const EqsStream &rng,
                      int N, size_t m, const EqsOut &out, uint64_t *desc) {
    if (m == 0) return hipSuccess;
    const uint32_t S = rng.samples;
    if (S == 0 || S > EQS_SAMPLES_MAX || eqs_task_bound(m, S) > EQ_TASKS_MAX) return hipErrorInvalidValue;
    EqsPrepArgs a{};
    if (spots) a.s = *spots;
    if (tables) a.t = *tables;
    a.rng = rng; a.out = out; a.desc = desc; a.N = N; a.observer = observer; a.m = m;
    const dim3 pgrid((unsigned)((m + EQS_PREP_BLOCK - 1) / EQS_PREP_BLOCK));
    if (tables) hipLaunchKernelGGL(k_eqs_prep<true>, pgrid, dim3(EQS_PREP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_eqs_prep<false>, pgrid, dim3(EQS_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t per = 64u * (uint32_t)eqs_lpt(m, S), nch = (S + per - 1) / per;
    const uint32_t ntasks = (uint32_t)m * nch;                       // (<= eqs_task_bound: fits)
    // no more workgroups than there are tasks for (each stages the 32 KB table); the grid is persistent beyond that
    const uint32_t want = (ntasks + EQ_WAVES - 1) / EQ_WAVES;
    const unsigned grid = want < (uint32_t)EQ_GRID_MAX ? want : (unsigned)EQ_GRID_MAX;
    if (!eqs_dispatch<PK_MIN_PLAYERS>(N, stream, grid, tab, desc, out, rng, ntasks, nch, per)) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace pk
