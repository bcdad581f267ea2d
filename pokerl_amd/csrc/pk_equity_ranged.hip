// pk_equity_ranged.hip -- sampled showdown equity against weighted ranges: every hidden seat draws its HOLDING from a u16 [1326] range, the
// attempts whose holdings collide are rejected, the board is drawn from what is left (include/pokerl_hip.h "Ranged sampled equity", DESIGN.md
// section 3.6).  Three kernels per call:
//   k_eqw_cdf    one wavefront per range row: the cumulative sums u32 [R][1326] into the call's work space;
//   k_eqw_prep   one lane per spot: k_eqs_prep's checks plus the three rules of this family (a half-hidden live seat, a range row >= R at a
//                hidden seat: PK_EQ_BAD_CARD); writes the descriptor (hidden-seat mask, range rows), `status`, and zeroes the counts;
//   k_eqw<N, RC> k_eqs<N>'s shape -- a persistent grid of 512-thread workgroups, eval7_tab staged once per workgroup, the spot wave-uniform,
//                task -> (spot, chunk) by division, a run of attempt indices per lane, 32-bit lane counters, wave sums, integer atomics from
//                lane 0 -- with the call's cumulative rows (RC = 0, 8 or 16 of them: the LDS size class) and a 1326-entry holding -> cards
//                table in LDS beside the evaluator table.  A lane finds its holding by a branch-free binary search of 11 LDS reads; a
//                rejected attempt skips the board draw and the evaluations.
// Ordinary vector stores, LDS operations and integer atomics only; no scratch memory (tests/test_equity_ranged_host.py reads the code objects).
// -DPK_EQW_CLASS=0 | 8 | 16: an object file with the sampling kernels of ONE size class (class 0 carries the shared kernels and eqw_launch).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_ranged.hpp"

using namespace pk;

#if !defined(PK_EQW_CLASS) || PK_EQW_CLASS == 0
#define EQW_SHARED_PART 1
#else
#define EQW_SHARED_PART 0
#endif
#ifdef PK_EQW_CLASS
#define EQW_HAS_CLASS(rc) ((rc) == (PK_EQW_CLASS))
#else
#define EQW_HAS_CLASS(rc) 1
#endif

#define EQW_PREP_BLOCK 256
#define EQW_CDF_PER_LANE 21      // 64 lanes x 21 >= 1326 holdings
static_assert(64 * EQW_CDF_PER_LANE >= EQW_HOLDINGS, "a wavefront covers a row");

struct EqwPrepArgs {
    EqSpots s;
    EqTables t;
    EqsStream rng;
    EqwRanges r;
    EqwOut out;
    uint64_t *desc;
    int N, observer;
    size_t m;
};

#if EQW_SHARED_PART
// cum[r][h] = sum of w[r][0 .. h]: a lane sums its run of 21 holdings, the wavefront scans the 64 run totals, the lane writes its run
__global__ void __launch_bounds__(64) k_eqw_cdf(const uint16_t *__restrict__ weights, uint32_t *__restrict__ cum, uint32_t R) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = blockIdx.x; r < R; r += gridDim.x) {
        const uint16_t *w = weights + (size_t)r * EQW_HOLDINGS;
        uint32_t *c = cum + (size_t)r * EQW_HOLDINGS;
        const uint32_t first = lane * EQW_CDF_PER_LANE;
        uint32_t run = 0;
        for (uint32_t i = 0; i < EQW_CDF_PER_LANE; ++i) run += first + i < (uint32_t)EQW_HOLDINGS ? (uint32_t)w[first + i] : 0u;
        uint32_t incl = run;                                            // inclusive scan over the lanes
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl(incl, (int)(lane >= off ? lane - off : lane));
            incl += lane >= off ? up : 0u;
        }
        uint32_t acc = incl - run;
        for (uint32_t i = 0; i < EQW_CDF_PER_LANE; ++i)
            if (first + i < (uint32_t)EQW_HOLDINGS) { acc += (uint32_t)w[first + i]; c[first + i] = acc; }
    }
}

template <bool TABLE>
__global__ void __launch_bounds__(EQW_PREP_BLOCK) k_eqw_prep(EqwPrepArgs a) {
    const size_t tid = (size_t)blockIdx.x * EQW_PREP_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * EQW_PREP_BLOCK;
    const int N = a.N;
    // the count outputs start at zero (k_eqw adds to them); consecutive lanes, consecutive words
    const size_t cells = a.m * (size_t)N;
    for (size_t e = tid; e < cells; e += nthreads) {
        if (a.out.win) a.out.win[e] = 0;
        if (a.out.tie) a.out.tie[e] = 0;
        if (a.out.share) a.out.share[e] = 0;
    }
    if (tid >= a.m) return;
    const size_t i = tid;
    uint64_t *d = a.desc + i * (size_t)eqw_desc_words(N);
    uint32_t status = 0, live = 0, hidden = 0, id = 0;
    int nb = 0;
    uint64_t dead = 0, known = 0;
    d[4] = d[5] = d[6] = d[7] = ~0ull;                                          // every seat's range row: EQW_UNIFORM until a hidden seat names one
    // one card byte: its bit in the suit-lane layout (0 for 0xFF); marks it dead; a byte that is no card, or a card seen before, is refused
    auto card = [&](uint32_t c, bool required) -> uint64_t {
        if (c == 0xffu) { status |= required ? (uint32_t)PK_EQ_BAD_CARD : 0u; return 0; }
        if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; return 0; }
        const uint64_t bit = 1ull << ((c & 15u) * 4u + (c >> 4));              // canonical index (cards.py:77)
        status |= (dead & bit) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
        dead |= bit;
        return 4ull << c;
    };
    // seat p's two hole bytes: a card is known and dead; a live seat hides BOTH (its holding is drawn from its range) or none; at a seat that
    // is not live 0xFF is simply in the pool.  The seat's range row is read only where the seat is hidden.
    auto seat = [&](int p, uint32_t c0, uint32_t c1) {
        const uint32_t lv = (live >> p) & 1u;
        d[8 + p] = card(c0, false) | card(c1, false);
        const bool h0 = c0 == 0xffu, h1 = c1 == 0xffu;
        if (lv && h0 != h1) status |= PK_EQ_BAD_CARD;                           // half a holding: no weighted draw is defined for it
        if (lv && h0 && h1) {
            hidden |= 1u << p;
            const uint32_t ro = a.r.range_of ? (uint32_t)a.r.range_of[(a.r.per_spot ? i * (size_t)N : (size_t)0) + p] : EQW_UNIFORM;
            if (ro != EQW_UNIFORM && ro >= a.r.R) status |= PK_EQ_BAD_CARD;     // (the status word has no bit left: a row that does not exist is a bad input byte)
            d[4 + (p >> 2)] = (d[4 + (p >> 2)] & ~(0xffffull << (16 * (p & 3)))) | ((uint64_t)ro << (16 * (p & 3)));
        }
    };
    const uint32_t seats = (1u << N) - 1u;
    bool readable = true;
    if constexpr (TABLE) {
        const int64_t t = a.t.tables ? (int64_t)a.t.tables[i] : (int64_t)i;
        id = a.rng.id_base + (uint32_t)t;
        if (t < 0 || t >= (int64_t)a.t.T) { status |= PK_EQ_BAD_TABLE; readable = false; }   // (k_eqw reads no further than the valid bit)
        else {
            const Cursor cur{a.t.cursors[t]};
            if (cur.in_flight()) status |= PK_EQ_IN_FLIGHT;
            const int turn = (int)cur.turn();
            nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);                 // game.py:266-278
            const SeatStates ss{a.t.seat_states[t]};
            live = (ss.active() | ss.called() | ss.allin()) & seats;
            const int who = a.observer == PK_OBSERVER_ACTIVE ? (int)cur.active() : a.observer;
            for (int j = 0; j < nb; ++j) known |= card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, j), true);
            for (int p = 0; p < N; ++p) {
                if (p == who) {                                                   // (a dealt deck holds no 0xFF)
                    const uint32_t c0 = card_byte(a.t.cards, (size_t)a.t.T, (int)t, 5 + 2 * p), c1 = card_byte(a.t.cards, (size_t)a.t.T, (int)t, 6 + 2 * p);
                    d[8 + p] = card(c0, true) | card(c1, true);
                } else seat(p, 0xffu, 0xffu);                                     // (another seat's cards are not read at all: the observer never saw them)
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
    if (a.out.accepted) a.out.accepted[i] = 0;
    if (a.out.status) a.out.status[i] = (uint8_t)status;
}
#endif  // EQW_SHARED_PART

// The number of h with row[h] <= u over a non-decreasing row of 1326 sums: 11 dependent LDS reads, no branch.  u < row[1325]: the result <= 1325.
__device__ __forceinline__ uint32_t eqw_search(const uint32_t *row, uint32_t u) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = 1024; step >= 1; step >>= 1) {
        const uint32_t idx = pos + step - 1u;
        const bool in = idx < (uint32_t)EQW_HOLDINGS;
        const uint32_t v = row[PK_IDX(in ? idx : (uint32_t)EQW_HOLDINGS - 1u, (uint32_t)EQW_HOLDINGS, "cumulative row")];
        pos += (in && v <= u) ? step : 0u;
    }
    return pos;
}
// the card of canonical index c as its bit in the suit-lane layout (4 << Card.value)
__device__ __forceinline__ uint64_t eqw_card_bit(uint32_t c) { return 4ull << (((c & 3u) << 4) | (c >> 2)); }

// registers per lane: the caps of k_eqs<N> (taken from it, not measured for this kernel)
template <int N> constexpr int eqw_min_waves() { return N <= 3 ? 8 : (N <= 8 ? 4 : 2); }

template <int N, int RC>
__global__ void __launch_bounds__(EQ_BLOCK, eqw_min_waves<N>()) k_eqw(const uint32_t *__restrict__ tab, const uint32_t *__restrict__ cum,
                                                                     const uint64_t *__restrict__ desc, EqwOut out, EqsStream rng, uint32_t R,
                                                                     uint32_t ntasks, uint32_t nch, uint32_t per) {
    constexpr uint32_t CUM_WORDS = RC ? (uint32_t)RC * EQW_HOLDINGS : 1u;
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint32_t CUM[CUM_WORDS];
    __shared__ uint16_t HC[EQW_HOLDINGS];                             // holding h -> its cards' canonical indices a | b << 8
    __shared__ uint32_t wt[32];
    stage_eval7_tab<EQ_BLOCK>(T, tab);
    if constexpr (RC > 0) {
        const uint32_t words = (R < (uint32_t)RC ? R : (uint32_t)RC) * EQW_HOLDINGS;
        for (uint32_t i = threadIdx.x; i < words; i += EQ_BLOCK) CUM[PK_IDX(i, CUM_WORDS, "CUM")] = cum[i];
    }
    for (uint32_t h = threadIdx.x; h < (uint32_t)EQW_HOLDINGS; h += EQ_BLOCK) {
        uint32_t b = 1;                                                // b (b - 1) / 2 <= h < b (b + 1) / 2: once per workgroup, three holdings a lane
        while (b * (b + 1u) / 2u <= h) ++b;
        HC[PK_IDX(h, EQW_HOLDINGS, "HC")] = (uint16_t)((h - b * (b - 1u) / 2u) | (b << 8));
    }
    fill_share_weights(wt);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = uniform(threadIdx.x >> 6), nwaves = gridDim.x * EQ_WAVES;
    const uint32_t S = rng.samples;
    // every task costs about the same, so the tasks are dealt round robin: no counter
    for (uint32_t t = blockIdx.x * EQ_WAVES + wave; t < ntasks; t += nwaves) {
        const uint32_t spot = t / nch, chunk = t - spot * nch;
        const uint64_t *d = desc + (size_t)spot * eqw_desc_words(N);
        const uint64_t m3 = uniform(d[3]);
        if (!(m3 >> 32)) continue;                                   // a refused spot: no attempts
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        uint64_t rw[(N + 3) / 4];
        PK_FOR(q, (N + 3) / 4) rw[q] = uniform(d[4 + q]); PK_END
        uint64_t hole[N];
        PK_FOR(p, N) hole[p] = uniform(d[8 + p]); PK_END
        const uint32_t hid = (uint32_t)meta & 0xffffu, mhi = (uint32_t)(meta >> 32), live = mhi & 0xffffu, k = (mhi >> 16) & 0xffu, P = mhi >> 24;
        const uint32_t id = (uint32_t)m3, H = (uint32_t)__builtin_popcount(hid), Pb = P - 2u * H;
        // per hidden seat: the row's first word in CUM (EQW_UNIFORM: none) and its total T_j; a range with no weight left accepts nothing
        uint32_t tot[N];
        bool none = false;
        PK_FOR(p, N)
            tot[p] = 0;
            if ((hid >> p) & 1u) {
                const uint32_t row = (uint32_t)(rw[p / 4] >> (16 * (p % 4))) & 0xffffu;
                tot[p] = (uint32_t)EQW_HOLDINGS;
                if constexpr (RC > 0) {
                    if (row != EQW_UNIFORM) tot[p] = uniform(CUM[PK_IDX(row * (uint32_t)EQW_HOLDINGS + (uint32_t)EQW_HOLDINGS - 1u, CUM_WORDS, "CUM total")]);
                }
                none = none || tot[p] == 0u;
            }
        PK_END
        if (none) continue;
        // this task's attempts [start, end) of the spot's, and this lane's [s, s + cnt) of those
        const uint32_t start = chunk * per, end = min(S, start + per), nt = end - start;
        const uint32_t l = (nt + 63u) / 64u, s = start + lane * l;
        const uint32_t cnt = s < end ? min(l, end - s) : 0u;
        uint32_t sole[N], inw[N], sh[N], acc = 0;
        PK_FOR(p, N) sole[p] = 0; inw[p] = 0; sh[p] = 0; PK_END
        for (uint32_t n = 0; n < cnt; ++n) {
            // 64-bit word j of the attempt: X[2b] / X[2b + 1] of Philox block b = j / 2, generated when its first word is asked for (j is
            // wave-uniform and ascending: only the blocks the spot needs)
            uint32_t w[4] = {0, 0, 0, 0};
            uint32_t xlo = 0, xhi = 0;
            auto word = [&](uint32_t j) {
                if (!(j & 1u)) philox4x32_10(id, s + n, STREAM_EQW + (j >> 1), rng.nonce, rng.key0, rng.key1, w);
                xlo = (j & 1u) ? w[2] : w[0];
                xhi = (j & 1u) ? w[3] : w[1];
            };
            uint64_t rem = avail;
            bool rej = false;
            uint64_t dh[N];
            PK_FOR(p, N)
                dh[p] = 0;
                if ((hid >> p) & 1u) {
                    word((uint32_t)__builtin_popcount(hid & ((1u << p) - 1u)));
                    const uint64_t a = (uint64_t)xlo * tot[p], b = (uint64_t)xhi * tot[p] + (a >> 32);
                    uint32_t h = (uint32_t)(b >> 32);                                  // u = (X * T) >> 64; the uniform row: cum[h] = h + 1, so h = u
                    if constexpr (RC > 0) {
                        const uint32_t row = (uint32_t)(rw[p / 4] >> (16 * (p % 4))) & 0xffffu;
                        if (row != EQW_UNIFORM) h = eqw_search(CUM + PK_IDX(row * (uint32_t)EQW_HOLDINGS, CUM_WORDS, "CUM row"), h);
                    }
                    const uint32_t ab = HC[PK_IDX(h, EQW_HOLDINGS, "HC")], ca = ab & 0xffu, cb = ab >> 8;
                    const uint64_t two = (1ull << ca) | (1ull << cb);
                    rej = rej || (two & ~rem) != 0;                                     // a dead card, or a card of an earlier seat's holding
                    rem &= ~two;
                    dh[p] = eqw_card_bit(ca) | eqw_card_bit(cb);
                }
            PK_END
            if (!rej) {
                // the board: k chained draws from the one word X[H] over the Pb cards left
                uint64_t bits = known;
                if (k > 0u) {
                    word(H);
                    PK_FOR(j, 5)
                        if ((uint32_t)j < k) {
                            const uint32_t left = Pb - (uint32_t)j;
                            const uint64_t a = (uint64_t)xlo * left, b = (uint64_t)xhi * left + (a >> 32);
                            xlo = (uint32_t)a; xhi = (uint32_t)b;
                            const uint32_t c = select(rem, (uint32_t)(b >> 32));
                            rem &= ~(1ull << c);
                            bits |= eqw_card_bit(c);
                        }
                    PK_END
                }
                uint32_t v[N];
                PK_FOR(p, N)
                    v[p] = NONE_V;                                                    // eval_hand([]) of a seat that does not show down
                    if ((live >> p) & 1u) {
                        const uint64_t h7 = bits | (((hid >> p) & 1u) ? dh[p] : hole[p]);
                        v[p] = eval7_tab_back(eval7_tab_front_bits(h7, T), T);
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
                acc += 1u;
            }
        }
        // per seat: the wavefront's sums, then one atomic per output from lane 0; one more for the accepted attempts
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
        const uint32_t wacc = wave_sum(acc);
        if (lane == 0 && out.accepted && wacc) atomicAdd(&out.accepted[spot], wacc);
    }
}

namespace pk {

template <int N, int RC>
static bool eqw_dispatch(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const uint32_t *cum, const uint64_t *desc, const EqwOut &out,
                         const EqsStream &rng, uint32_t R, uint32_t ntasks, uint32_t nch, uint32_t per) {
    if constexpr (N > PK_MAX_PLAYERS) return false;
    else {
        if (n == N) {
            if constexpr (EQ_SEAT_ENABLED(N)) {
                hipLaunchKernelGGL((k_eqw<N, RC>), dim3(grid), dim3(EQ_BLOCK), 0, stream, tab, cum, desc, out, rng, R, ntasks, nch, per);
                return true;
            } else return false;
        }
        return eqw_dispatch<N + 1, RC>(n, stream, grid, tab, cum, desc, out, rng, R, ntasks, nch, per);
    }
}

template <int RC>
bool eqw_run_class(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const uint32_t *cum, const uint64_t *desc, const EqwOut &out,
                   const EqsStream &rng, uint32_t R, uint32_t ntasks, uint32_t nch, uint32_t per) {
    return eqw_dispatch<PK_MIN_PLAYERS, RC>(n, stream, grid, tab, cum, desc, out, rng, R, ntasks, nch, per);
}
#if EQW_HAS_CLASS(0)
template bool eqw_run_class<0>(int, hipStream_t, unsigned, const uint32_t *, const uint32_t *, const uint64_t *, const EqwOut &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#else
extern template bool eqw_run_class<0>(int, hipStream_t, unsigned, const uint32_t *, const uint32_t *, const uint64_t *, const EqwOut &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#endif
#if EQW_HAS_CLASS(8)
template bool eqw_run_class<8>(int, hipStream_t, unsigned, const uint32_t *, const uint32_t *, const uint64_t *, const EqwOut &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#else
extern template bool eqw_run_class<8>(int, hipStream_t, unsigned, const uint32_t *, const uint32_t *, const uint64_t *, const EqwOut &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#endif
#if EQW_HAS_CLASS(16)
template bool eqw_run_class<16>(int, hipStream_t, unsigned, const uint32_t *, const uint32_t *, const uint64_t *, const EqwOut &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#else
extern template bool eqw_run_class<16>(int, hipStream_t, unsigned, const uint32_t *, const uint32_t *, const uint64_t *, const EqwOut &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#endif

#if EQW_SHARED_PART
hipError_t eqw_launch_cdf(hipStream_t stream, const uint16_t *weights, uint32_t *cum, uint32_t R) {
    if (R) hipLaunchKernelGGL(k_eqw_cdf, dim3(R), dim3(64), 0, stream, weights, cum, R);
    return hipGetLastError();
}

hipError_t eqw_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const EqTables *tables, int observer, const EqsStream &rng,
                      const EqwRanges &ranges, int N, size_t m, const EqwOut &out, char *work) {
    if (m == 0) return hipSuccess;
    const uint32_t S = rng.samples, R = ranges.R;
    if (S == 0 || S > EQS_SAMPLES_MAX || eqs_task_bound(m, S) > EQ_TASKS_MAX || R > (uint32_t)EQW_MAX_RANGES || (R && !ranges.weights)) return hipErrorInvalidValue;
    uint32_t *cum = reinterpret_cast<uint32_t *>(work);
    uint64_t *desc = reinterpret_cast<uint64_t *>(work + eqw_cum_bytes(R));
    if (R) hipLaunchKernelGGL(k_eqw_cdf, dim3(R), dim3(64), 0, stream, ranges.weights, cum, R);
    EqwPrepArgs a{};
    if (spots) a.s = *spots;
    if (tables) a.t = *tables;
    a.rng = rng; a.r = ranges; a.out = out; a.desc = desc; a.N = N; a.observer = observer; a.m = m;
    const dim3 pgrid((unsigned)((m + EQW_PREP_BLOCK - 1) / EQW_PREP_BLOCK));
    if (tables) hipLaunchKernelGGL(k_eqw_prep<true>, pgrid, dim3(EQW_PREP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_eqw_prep<false>, pgrid, dim3(EQW_PREP_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t per = 64u * (uint32_t)eqs_lpt(m, S), nch = (S + per - 1) / per;
    const uint32_t ntasks = (uint32_t)m * nch;                       // (<= eqs_task_bound: fits)
    // no more workgroups than there are tasks for, and no more than fit the CUs at this class's LDS (4, 2 or 1 per CU); persistent beyond that
    const int rc = eqw_class(R);
    const uint32_t want = (ntasks + EQ_WAVES - 1) / EQ_WAVES, cap = (uint32_t)EQ_GRID_MAX / (rc == 0 ? 1u : (rc == 8 ? 2u : 4u));
    const unsigned grid = want < cap ? want : cap;
    const bool ok = rc == 0   ? eqw_run_class<0>(N, stream, grid, tab, cum, desc, out, rng, R, ntasks, nch, per)
                    : rc == 8 ? eqw_run_class<8>(N, stream, grid, tab, cum, desc, out, rng, R, ntasks, nch, per)
                              : eqw_run_class<16>(N, stream, grid, tab, cum, desc, out, rng, R, ntasks, nch, per);
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}
#endif

}  // namespace pk
