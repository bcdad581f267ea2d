// pk_ev_ranged.hip -- ranged showdown EV in chips: what every seat is paid out of the side pots of Game.end_hand, over attempts in which every
// hidden seat draws its HOLDING from a u16 [1326] range (include/pokerl_hip.h "Ranged showdown EV").  The draw is
// section 3.6's (pk_equity_ranged.hip: stream 'EQW0', cumulative search, rejection, the board from word X[H]), the levels and ev are section
// 3.7's (pk_equity_ev.hip).  Four kernels per call:
//   k_eqw_cdf            (pk_equity_ranged.hip) one wavefront per range row: the cumulative sums into the call's work space;
//   k_evw_prep<N, TABLE> one lane per spot: k_eqw_prep's checks and descriptor (hidden-seat mask, range rows, pool, stream id), k_ev_prep's
//                        bet checks and level loop in registers -> level_seat, amount, the level table, the bets as used; zeroes `share` and
//                        `accepted`;
//   k_evw<N, RC>         k_eqw<N, RC>'s shape -- a persistent grid of 512-thread workgroups, eval7_tab, RC cumulative rows and the holding
//                        table staged once per workgroup, the spot wave-uniform, a run of attempts per lane, rejection under a divergent
//                        branch -- where a task is (spot, chunk of attempts, GROUP of ev_group(N) levels): per accepted attempt ONE evaluation
//                        per live seat, then per level of the group compare_rankings<N> on v masked by the level's remain mask (a scalar: the
//                        masking is a select), a 32-bit share counter per (level, seat), wave sums, one 64-bit atomic per counter from lane 0.
//                        A group re-draws its chunk's attempts (the stream is counter-based: exact); only group 0 adds to `accepted`;
//   k_evw_finish         one lane per (spot, seat): the last stand's share cell, then ev in the stated order, every operation rounded on its own.
// Tasks are ENUMERATED (m * nch * ev_groups_max(N)); a task whose group has no level to compare ends at a scalar branch.
// Ordinary vector stores, LDS operations and integer atomics only; no scratch memory (tests/test_ranged_ev_host.py reads the code objects).
// -DPK_EVW_CLASS=0 | 8 | 16: an object file with the sampling kernels of ONE size class (class 0 carries the shared kernels and evw_launch).
// The device helpers below (search, card bit, bad bet, the register caps) are copies of the parents': the parents' translation units stay
// as they are, so that their kernels' code does not move.
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_ev_ranged.hpp"

using namespace pk;

#if !defined(PK_EVW_CLASS) || PK_EVW_CLASS == 0
#define EVW_SHARED_PART 1
#else
#define EVW_SHARED_PART 0
#endif
#ifdef PK_EVW_CLASS
#define EVW_HAS_CLASS(rc) ((rc) == (PK_EVW_CLASS))
#else
#define EVW_HAS_CLASS(rc) 1
#endif

#define EVW_PREP_BLOCK 256
#define EVW_FINISH_BLOCK 256

struct EvwPrepArgs {
    EqSpots s;
    const double *bets;   // the explicit form: [m][N]
    EvTables t;
    EqsStream rng;
    EqwRanges r;
    EvwOut out;
    EvwWork w;
    int observer;
    size_t m;
};

#if EVW_SHARED_PART
// negative (not -0.0), infinite or NaN: read from the bits, as ev_bad_bet (pk_equity_ev.hip) -- the build does not honour NaNs in comparisons
__device__ __forceinline__ bool evw_bad_bet(double b) {
    const uint64_t u = (uint64_t)__double_as_longlong(b);
    return ((u >> 63) && u != 0x8000000000000000ull) || ((u >> 52) & 0x7ffu) == 0x7ffu;
}

template <int N, bool TABLE>
__global__ void __launch_bounds__(EVW_PREP_BLOCK) k_evw_prep(EvwPrepArgs a) {
    const size_t tid = (size_t)blockIdx.x * EVW_PREP_BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * EVW_PREP_BLOCK;
    constexpr int G = ev_group(N);
    // the share counters start at zero (k_evw adds to them); consecutive lanes, consecutive words
    const size_t cells = a.m * (size_t)(N * N);
    for (size_t e = tid; e < cells; e += nthreads) a.w.share[e] = 0;
    if (tid >= a.m) return;
    const size_t i = tid;
    uint64_t *d = a.w.desc + i * (size_t)eqw_desc_words(N);
    uint32_t status = 0, live = 0, hidden = 0, id = 0;
    int nb = 0;
    uint64_t dead = 0, known = 0;
    double bets[N];
    PK_FOR(p, N) bets[p] = 0.0; PK_END
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
    // seat p's two hole bytes, as k_eqw_prep reads them: a live seat hides BOTH (its holding is drawn from its range) or none
    auto seat = [&](int p, uint32_t c0, uint32_t c1) {
        const uint32_t lv = (live >> p) & 1u;
        d[8 + p] = card(c0, false) | card(c1, false);
        const bool h0 = c0 == 0xffu, h1 = c1 == 0xffu;
        if (lv && h0 != h1) status |= PK_EQ_BAD_CARD;                           // half a holding
        if (lv && h0 && h1) {
            hidden |= 1u << p;
            const uint32_t ro = a.r.range_of ? (uint32_t)a.r.range_of[(a.r.per_spot ? i * (size_t)N : (size_t)0) + p] : EQW_UNIFORM;
            if (ro != EQW_UNIFORM && ro >= a.r.R) status |= PK_EQ_BAD_CARD;     // a row that does not exist
            d[4 + (p >> 2)] = (d[4 + (p >> 2)] & ~(0xffffull << (16 * (p & 3)))) | ((uint64_t)ro << (16 * (p & 3)));
        }
    };
    constexpr uint32_t seats = (1u << N) - 1u;
    bool readable = true;
    if constexpr (TABLE) {
        const int64_t t = a.t.t.tables ? (int64_t)a.t.t.tables[i] : (int64_t)i;
        id = a.rng.id_base + (uint32_t)t;
        if (t < 0 || t >= (int64_t)a.t.t.T) { status |= PK_EQ_BAD_TABLE; readable = false; }
        else {
            const size_t T = (size_t)a.t.t.T;
            const Cursor cur{a.t.t.cursors[t]};
            if (cur.in_flight()) status |= PK_EQ_IN_FLIGHT;
            const int turn = (int)cur.turn();
            nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);                 // game.py:266-278
            const SeatStates ss{a.t.t.seat_states[t]};
            live = (ss.active() | ss.called() | ss.allin()) & seats;
            const int who = a.observer == PK_OBSERVER_ACTIVE ? (int)cur.active() : a.observer;
            for (int j = 0; j < nb; ++j) known |= card(card_byte(a.t.t.cards, T, (int)t, j), true);
            for (int p = 0; p < N; ++p) {
                if (p == who) {                                                   // (a dealt deck holds no 0xFF)
                    const uint32_t c0 = card_byte(a.t.t.cards, T, (int)t, 5 + 2 * p), c1 = card_byte(a.t.t.cards, T, (int)t, 6 + 2 * p);
                    d[8 + p] = card(c0, true) | card(c1, true);
                } else seat(p, 0xffu, 0xffu);                                     // (another seat's cards are not read at all)
            }
            PK_FOR(p, N) bets[p] = a.t.bets[(size_t)p * T + t] + a.t.pending[(size_t)p * T + t]; PK_END   // the commit of game.py:457
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
        PK_FOR(p, N) bets[p] = a.bets[i * (size_t)N + p]; PK_END
    }
    if (readable && live == 0) status |= PK_EQ_NO_LIVE;
    bool bad = false;
    PK_FOR(p, N) bad = bad || evw_bad_bet(bets[p]); PK_END
    if (bad) status |= PK_EQ_BAD_BET;
    // a -0.0 bet is a zero and is read as +0.0: np.clip and np.sum do not agree between numpy builds on the sign of a zero amount otherwise
    PK_FOR(p, N) bets[p] = (uint64_t)__double_as_longlong(bets[p]) == 0x8000000000000000ull ? 0.0 : bets[p]; PK_END
    // ---- the levels (game.py:494-525), exactly k_ev_prep's loop: bets and live seats only
    double work[N];
    PK_FOR(p, N) work[p] = bets[p]; a.w.bets[i * (size_t)N + p] = bets[p]; PK_END
    uint32_t todo = status ? 0u : live, remain = live, gmask = 0;
    int nrem = __popc(live);
    bool done = status != 0;
#pragma unroll 1
    for (int it = 0; it < N; ++it) {
        uint32_t rec = 0, lseat = 0xffu;
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
                lseat = (uint32_t)s;
                done = true;
            } else {
                double mb[N];                                                  // :509 np.clip(bets, 0, max_bet)
                PK_FOR(p, N) double x = work[p]; x = (x < 0.0) ? 0.0 : x; x = (x > mx) ? mx : x; mb[p] = x; PK_END
                amt = np_sum<N>(mb);
                rec = remain | ((uint32_t)s << 16) | EV_EXISTS | (amt > 0.0 ? EV_COMPARE : 0u);
                lseat = (uint32_t)s;
                gmask |= amt > 0.0 ? 1u << (it / G) : 0u;
                remain &= ~(1u << s); nrem -= 1;                               // :522, :525
                PK_FOR(p, N) work[p] = work[p] - mb[p]; PK_END                 // :523
            }
        }
        a.w.levels[i * (size_t)N + it] = rec;
        a.w.amount[i * (size_t)N + it] = amt;
        if (a.out.amount) a.out.amount[i * (size_t)N + it] = amt;
        if (a.out.level_seat) a.out.level_seat[i * (size_t)N + it] = (uint8_t)lseat;
    }
    const uint32_t P = 52u - (uint32_t)__popcll(dead), k = (uint32_t)(5 - nb);
    d[0] = known;
    d[1] = ~dead & 0x000FFFFFFFFFFFFFull;
    d[2] = (uint64_t)hidden | ((uint64_t)live << 32) | ((uint64_t)k << 48) | ((uint64_t)P << 56);
    d[3] = (uint64_t)id | ((uint64_t)(status ? 0u : 1u) << 32) | ((uint64_t)gmask << 40);
    a.w.accepted[i] = 0;
    a.out.status[i] = (uint8_t)status;
}

// One lane per (spot, seat p): the last stand's share cell (720720 * accepted at its seat), then
//   acc = +0.0;  for i ascending: acc = acc + (amount[i] * (double)share[i][p]) / (720720.0 * (double)accepted);  ev[p] = acc - bets[p]
// every operation rounded on its own (-ffp-contract=off).  A refused spot, or one with nothing accepted: ev = +0.0.
__global__ void __launch_bounds__(EVW_FINISH_BLOCK) k_evw_finish(EvwWork W, double *__restrict__ ev, int N, size_t m) {
    const size_t e = (size_t)blockIdx.x * EVW_FINISH_BLOCK + threadIdx.x;
    if (e >= m * (size_t)N) return;
    const size_t spot = e / (size_t)N;
    const uint32_t p = (uint32_t)(e - spot * (size_t)N);
    const uint32_t accepted = W.accepted[spot];
    double acc = 0.0;
    if (accepted) {
        const double den = (double)EQ_SHARE_UNIT * (double)accepted;
        for (int i = 0; i < N; ++i) {
            const uint32_t rec = W.levels[spot * (size_t)N + i];
            uint64_t *cell = &W.share[(spot * (size_t)N + i) * N + p];
            uint64_t sh = *cell;
            if ((rec & EV_LAST) && ((rec >> 16) & 0xffu) == p) { sh = (uint64_t)EQ_SHARE_UNIT * accepted; *cell = sh; }
            acc = acc + (W.amount[spot * (size_t)N + i] * (double)sh) / den;
        }
        acc = acc - W.bets[e];
    }
    if (ev) ev[e] = acc;
}
#endif  // EVW_SHARED_PART

// The number of h with row[h] <= u over a non-decreasing row of 1326 sums: 11 dependent LDS reads, no branch (eqw_search's copy)
__device__ __forceinline__ uint32_t evw_search(const uint32_t *row, uint32_t u) {
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
__device__ __forceinline__ uint64_t evw_card_bit(uint32_t c) { return 4ull << (((c & 3u) << 4) | (c >> 2)); }

// registers per lane: the caps of k_eqw<N, RC> (eqw_min_waves), TAKEN from it, not measured for this kernel -- its 3 N counters are this
// kernel's ev_group(N) * N
template <int N> constexpr int evw_min_waves() { return N <= 3 ? 8 : (N <= 8 ? 4 : 2); }

template <int N, int RC>
__global__ void __launch_bounds__(EQ_BLOCK, evw_min_waves<N>()) k_evw(const uint32_t *__restrict__ tab, EvwWork W, EqsStream rng, uint32_t R,
                                                                     uint32_t ntasks, uint32_t nch, uint32_t per) {
    constexpr uint32_t CUM_WORDS = RC ? (uint32_t)RC * EQW_HOLDINGS : 1u;
    constexpr int G = ev_group(N);
    constexpr uint32_t GM = (uint32_t)ev_groups_max(N);
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint32_t CUM[CUM_WORDS];
    __shared__ uint16_t HC[EQW_HOLDINGS];                             // holding h -> its cards' canonical indices a | b << 8
    __shared__ uint32_t wt[32];
    stage_eval7_tab<EQ_BLOCK>(T, tab);
    if constexpr (RC > 0) {
        const uint32_t words = (R < (uint32_t)RC ? R : (uint32_t)RC) * EQW_HOLDINGS;
        for (uint32_t i = threadIdx.x; i < words; i += EQ_BLOCK) CUM[PK_IDX(i, CUM_WORDS, "CUM")] = W.cum[i];
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
    // tasks are dealt round robin: task -> (group, (spot, chunk)) by division, the group outermost -- a wavefront's stride is a multiple of
    // eight, so with the group innermost a wavefront would meet one group only, and the groups that are skipped cost nothing; no counter, no list
    const uint32_t nsc = ntasks / GM;
    for (uint32_t t = blockIdx.x * EQ_WAVES + wave; t < ntasks; t += nwaves) {
        const uint32_t grp = t / nsc, sc = t - grp * nsc, spot = sc / nch, chunk = sc - spot * nch, first = grp * (uint32_t)G;
        const uint64_t *d = W.desc + (size_t)spot * eqw_desc_words(N);
        const uint64_t m3 = uniform(d[3]);
        if (!((m3 >> 32) & 1u)) continue;                            // a refused spot: no attempts
        const uint32_t groups = (uint32_t)(m3 >> 40) & 0xffu;
        const bool cmp = (groups >> grp) & 1u;
        if (!cmp && grp != 0u) continue;                             // nothing to compare here (group 0 still counts the accepted attempts)
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        uint64_t rw[(N + 3) / 4];
        PK_FOR(q, (N + 3) / 4) rw[q] = uniform(d[4 + q]); PK_END
        uint64_t hole[N];
        PK_FOR(p, N) hole[p] = uniform(d[8 + p]); PK_END
        // the levels of this task's group: remain mask and flags, scalars (0: no level here)
        uint32_t lv[G];
        PK_FOR(c, G)
            lv[c] = 0;
            if (first + c < (uint32_t)N) lv[c] = uniform(W.levels[(size_t)spot * N + first + c]);
        PK_END
        const uint32_t hid = (uint32_t)meta & 0xffffu, mhi = (uint32_t)(meta >> 32), live = mhi & 0xffffu, k = (mhi >> 16) & 0xffu, P = mhi >> 24;
        const uint32_t id = (uint32_t)m3, H = (uint32_t)__builtin_popcount(hid), Pb = P - 2u * H;
        // per hidden seat: the row's total T_j; a range with no weight left accepts nothing
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
        // this task's attempts [start, end) of the spot's, and this lane's [s, s + cnt) of those: at most per / 64 <= EQS_LPT_MAX a lane
        const uint32_t start = chunk * per, end = min(S, start + per), nt = end - start;
        const uint32_t l = (nt + 63u) / 64u, s = start + lane * l;
        const uint32_t cnt = s < end ? min(l, end - s) : 0u;
        uint32_t sh[G][N], acc = 0;
        PK_FOR(c, G) PK_FOR(p, N) sh[c][p] = 0; PK_END PK_END
        for (uint32_t n = 0; n < cnt; ++n) {
            // 64-bit word j of the attempt: X[2b] / X[2b + 1] of Philox block b = j / 2, generated when its first word is asked for
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
                        if (row != EQW_UNIFORM) h = evw_search(CUM + PK_IDX(row * (uint32_t)EQW_HOLDINGS, CUM_WORDS, "CUM row"), h);
                    }
                    const uint32_t ab = HC[PK_IDX(h, EQW_HOLDINGS, "HC")], ca = ab & 0xffu, cb = ab >> 8;
                    const uint64_t two = (1ull << ca) | (1ull << cb);
                    rej = rej || (two & ~rem) != 0;                                     // a dead card, or a card of an earlier seat's holding
                    rem &= ~two;
                    dh[p] = evw_card_bit(ca) | evw_card_bit(cb);
                }
            PK_END
            if (!rej) {
                acc += 1u;
                if (cmp) {                                                             // (a scalar: a group 0 with nothing to compare evaluates no hand)
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
                                bits |= evw_card_bit(c);
                            }
                        PK_END
                    }
                    uint32_t v[N];
                    PK_FOR(p, N)
                        v[p] = NONE_V;                                                // eval_hand([]) of a seat that does not show down
                        if ((live >> p) & 1u) {
                            const uint64_t h7 = bits | (((hid >> p) & 1u) ? dh[p] : hole[p]);
                            v[p] = eval7_tab_back(eval7_tab_front_bits(h7, T), T);
                        }
                    PK_END
                    PK_FOR(c, G)
                        if (lv[c] & EV_COMPARE) {                                     // (a scalar: the whole wavefront takes the branch)
                            uint32_t vm[N];
                            PK_FOR(p, N) vm[p] = ((lv[c] >> p) & 1u) ? v[p] : NONE_V; PK_END   // :522 the seats paid out below this level
                            int nw;
                            const uint32_t win = compare_rankings<N>(vm, nw);
                            const uint32_t wsh = wt[PK_IDX(nw, 32, "wt")];
                            PK_FOR(p, N) sh[c][p] += ((win >> p) & 1u) ? wsh : 0u; PK_END
                        }
                    PK_END
                }
            }
        }
        // per level and seat in its remain mask: the wavefront's sum, then one atomic from lane 0; group 0: one more for the accepted attempts
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
        if (grp == 0u) {
            const uint32_t wacc = wave_sum(acc);
            if (lane == 0 && wacc) atomicAdd(&W.accepted[spot], wacc);
        }
    }
}

namespace pk {

template <int N, int RC>
static bool evw_dispatch(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const EvwWork &w, const EqsStream &rng, uint32_t R,
                         uint32_t ntasks, uint32_t nch, uint32_t per) {
    if constexpr (N > PK_MAX_PLAYERS) return false;
    else {
        if (n == N) {
            if constexpr (EQ_SEAT_ENABLED(N)) {
                hipLaunchKernelGGL((k_evw<N, RC>), dim3(grid), dim3(EQ_BLOCK), 0, stream, tab, w, rng, R, ntasks, nch, per);
                return true;
            } else return false;
        }
        return evw_dispatch<N + 1, RC>(n, stream, grid, tab, w, rng, R, ntasks, nch, per);
    }
}

template <int RC>
bool evw_run_class(int n, hipStream_t stream, unsigned grid, const uint32_t *tab, const EvwWork &w, const EqsStream &rng, uint32_t R, uint32_t ntasks,
                   uint32_t nch, uint32_t per) {
    return evw_dispatch<PK_MIN_PLAYERS, RC>(n, stream, grid, tab, w, rng, R, ntasks, nch, per);
}
#if EVW_HAS_CLASS(0)
template bool evw_run_class<0>(int, hipStream_t, unsigned, const uint32_t *, const EvwWork &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#else
extern template bool evw_run_class<0>(int, hipStream_t, unsigned, const uint32_t *, const EvwWork &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#endif
#if EVW_HAS_CLASS(8)
template bool evw_run_class<8>(int, hipStream_t, unsigned, const uint32_t *, const EvwWork &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#else
extern template bool evw_run_class<8>(int, hipStream_t, unsigned, const uint32_t *, const EvwWork &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#endif
#if EVW_HAS_CLASS(16)
template bool evw_run_class<16>(int, hipStream_t, unsigned, const uint32_t *, const EvwWork &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#else
extern template bool evw_run_class<16>(int, hipStream_t, unsigned, const uint32_t *, const EvwWork &, const EqsStream &, uint32_t, uint32_t, uint32_t, uint32_t);
#endif

#if EVW_SHARED_PART
size_t evw_layout(int N, size_t m, uint32_t R, bool own_share, bool own_accepted, char *base, EvwWork *w) {
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    EvwWork r{};
    r.cum = (uint32_t *)(base + off); off += align(eqw_cum_bytes(R));
    r.desc = (uint64_t *)(base + off); off += align(m * (size_t)eqw_desc_words(N) * 8);
    r.levels = (uint32_t *)(base + off); off += align(m * (size_t)N * 4);
    r.bets = (double *)(base + off); off += align(m * (size_t)N * 8);
    r.amount = (double *)(base + off); off += align(m * (size_t)N * 8);
    if (own_share) { r.share = (uint64_t *)(base + off); off += align(m * (size_t)N * N * 8); }
    if (own_accepted) { r.accepted = (uint32_t *)(base + off); off += align(m * 4); }
    if (w) *w = r;
    return off;
}

template <int N>
static bool evw_prep_dispatch(int n, hipStream_t stream, bool table, unsigned pgrid, const EvwPrepArgs &a) {
    if constexpr (N > PK_MAX_PLAYERS) return false;
    else {
        if (n == N) {
            if constexpr (EQ_SEAT_ENABLED(N)) {
                if (table) hipLaunchKernelGGL((k_evw_prep<N, true>), dim3(pgrid), dim3(EVW_PREP_BLOCK), 0, stream, a);
                else hipLaunchKernelGGL((k_evw_prep<N, false>), dim3(pgrid), dim3(EVW_PREP_BLOCK), 0, stream, a);
                return true;
            } else return false;
        }
        return evw_prep_dispatch<N + 1>(n, stream, table, pgrid, a);
    }
}

hipError_t evw_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const double *bets, const EvTables *tables, int observer,
                      const EqsStream &rng, const EqwRanges &ranges, int N, size_t m, const EvwOut &out, const EvwWork &w_in) {
    if (m == 0) return hipSuccess;
    const uint32_t S = rng.samples, R = ranges.R;
    EvwWork w = w_in;
    if (out.share) w.share = out.share;            // the counters are the caller's arrays where there are any
    if (out.accepted) w.accepted = out.accepted;
    if (!out.status || !w.share || !w.accepted || S == 0 || S > EQS_SAMPLES_MAX || evw_task_bound(N, m, S) > EQ_TASKS_MAX ||
        R > (uint32_t)EQW_MAX_RANGES || (R && !ranges.weights))
        return hipErrorInvalidValue;
    hipError_t e = eqw_launch_cdf(stream, ranges.weights, w.cum, R);
    if (e != hipSuccess) return e;
    EvwPrepArgs a{};
    if (spots) a.s = *spots;
    a.bets = bets;
    if (tables) a.t = *tables;
    a.rng = rng; a.r = ranges; a.out = out; a.w = w; a.observer = observer; a.m = m;
    const unsigned pgrid = (unsigned)((m + EVW_PREP_BLOCK - 1) / EVW_PREP_BLOCK);
    if (!evw_prep_dispatch<PK_MIN_PLAYERS>(N, stream, tables != nullptr, pgrid, a)) return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the split is the ranged family's (eqs_lpt); a lane's 32-bit share counters hold its run of attempts: lpt * 720720 < 2^32
    const int lpt = eqs_lpt(m, S);
    static_assert((uint64_t)EQS_LPT_MAX * EQ_SHARE_UNIT < (1ull << 32), "a lane's 32-bit share sum must hold EQS_LPT_MAX attempts of a sole winner");
    if (lpt < 1 || lpt > EQS_LPT_MAX) return hipErrorInvalidValue;
    const uint32_t per = 64u * (uint32_t)lpt, nch = (S + per - 1) / per;
    const uint32_t ntasks = (uint32_t)m * nch * (uint32_t)ev_groups_max(N);   // (<= evw_task_bound: fits)
    // no more workgroups than there are tasks for, and no more than fit the CUs at this class's LDS (4, 2 or 1 per CU: k_eqw's caps, taken)
    const int rc = eqw_class(R);
    const uint32_t want = (ntasks + EQ_WAVES - 1) / EQ_WAVES, cap = (uint32_t)EQ_GRID_MAX / (rc == 0 ? 1u : (rc == 8 ? 2u : 4u));
    const unsigned grid = want < cap ? want : cap;
    const bool ok = rc == 0   ? evw_run_class<0>(N, stream, grid, tab, w, rng, R, ntasks, nch, per)
                    : rc == 8 ? evw_run_class<8>(N, stream, grid, tab, w, rng, R, ntasks, nch, per)
                              : evw_run_class<16>(N, stream, grid, tab, w, rng, R, ntasks, nch, per);
    if (!ok) return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t lanes = m * (size_t)N;
    hipLaunchKernelGGL(k_evw_finish, dim3((unsigned)((lanes + EVW_FINISH_BLOCK - 1) / EVW_FINISH_BLOCK)), dim3(EVW_FINISH_BLOCK), 0, stream, w, out.ev, N, m);
    return hipGetLastError();
}
#endif

}  // namespace pk
