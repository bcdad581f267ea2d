// pk_preflop.hip -- pre-flop hand strength: the exact matchup table of every ordered pair of holdings over all C(52, 5) boards, and the two
// families that read it (include/pokerl_hip.h "Pre-flop matchups").  Five kernels:
//   k_pfm_rank    for a chunk of boards: the 24-bit order key (pk::order_key: larger = stronger, equal = tie) of EVERY holding on every board of
//                 the chunk, keys[board][PFM_STRIDE] in the work space.  A workgroup stages the 32 KB rank-mask table of eval7_tab in LDS,
//                 unranks its first board once and steps (Comb<5, 0> over the 52 canonical indices); a lane ranks the same 6 holdings on every
//                 board (their cards are unpaired once).  A holding that shares a card with the board, and the 82 pad slots, get PFM_SENT.
//   k_pfm_count   the hot path, a register-tiled comparison "GEMM".  A workgroup owns a 128 x 128 tile of (hero x villain) holdings and one
//                 slice of the chunk's boards; it stages the two key strips of 32 boards in LDS (coalesced 16-byte loads) and each of its
//                 16 x 16 lanes keeps an 8 x 8 block of ordered pairs with win / tie counters in registers: per pair and board one compare +
//                 add-with-carry for `>` and one for `==`.  The sentinel is all ones on the villain side and selected to 0 on the hero side
//                 when a strip is staged, so that both comparisons are false when either holding is out of play: no branch in the loop.
//                 The tile's counts go to the output with integer atomics (exact in any order) -- or, for the first slice of a call that
//                 overwrites, with plain stores by a launch of one slice.  Pairs that share a card, the diagonal included, get 0 there.
//   k_pfm_prep    one lane per spot of pre-flop range equity: reads the hero's two cards (explicit, or a handle's table as one seat sees it,
//                 whatever its turn), checks them, writes the holding index (or PFM_NO_HOLDING) and `boards` / `status`;
//   k_pfm_hero    one spot per workgroup at a time: row `hero` of the table to win / tie, the weighted sums reduced in 64 bits;
//   k_pfm_rvr     the integer mat-vec u32 x u16 -> u64: a workgroup keeps PFM_RVR_ROWS rows of the table in registers and reuses them across
//                 every weight row of the call.
// Ordinary vector loads / stores, LDS and global integer atomics only; no scratch memory (tests/test_preflop_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_preflop.hpp"

using namespace pk;

// the two cards of holding h < 1326 as a mask over canonical indices
__device__ __forceinline__ uint64_t pfm_cards(uint32_t h) {
    uint32_t a, b;
    unpair(h, a, b);
    return (1ull << a) | (1ull << b);
}

__global__ void __launch_bounds__(PFM_RANK_BLOCK) k_pfm_rank(const uint32_t *__restrict__ tab, uint32_t first, uint32_t n, uint32_t *__restrict__ keys) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    stage_eval7_tab<PFM_RANK_BLOCK>(T, tab);
    const uint32_t tid = threadIdx.x;
    uint64_t hbits[PFM_RANK_PER_LANE], hmask[PFM_RANK_PER_LANE];   // this lane's holdings: suit-lane bits, canonical mask (all ones: a pad slot)
#pragma unroll
    for (int j = 0; j < PFM_RANK_PER_LANE; ++j) {
        const uint32_t h = tid + (uint32_t)j * PFM_RANK_BLOCK;
        hbits[j] = 0; hmask[j] = ~0ull;
        if (h < (uint32_t)PFM_HOLDINGS) {
            uint32_t a, b;
            unpair(h, a, b);
            hbits[j] = card_bit(a) | card_bit(b);
            hmask[j] = (1ull << a) | (1ull << b);
        }
    }
    __syncthreads();
    const uint32_t b0 = blockIdx.x * PFM_RANK_BOARDS;
    if (b0 >= n) return;
    const uint32_t cnt = min((uint32_t)PFM_RANK_BOARDS, n - b0);
    Comb<5, 0> cb;
    cb.start(52u, 0, first + b0, true);
    for (uint32_t i = 0; i < cnt; ++i) {
        uint64_t bits = 0, mask = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) { bits |= card_bit(cb.c[t]); mask |= 1ull << cb.c[t]; }
        uint32_t *row = keys + (size_t)(b0 + i) * PFM_STRIDE;
#pragma unroll
        for (int j = 0; j < PFM_RANK_PER_LANE; ++j) {
            const uint32_t h = tid + (uint32_t)j * PFM_RANK_BLOCK;
            if (h < (uint32_t)PFM_STRIDE) {
                uint32_t key = PFM_SENT;
                if (!(hmask[j] & mask)) key = order_key(eval7_tab_back(eval7_tab_front_bits(bits | hbits[j], T), T));
                row[PK_IDX(h, PFM_STRIDE, "keys")] = key;
            }
        }
        cb.next(52u, [] {});
    }
}

// the holding of a lane's block entry e = 0 .. 7 along one side of the tile: 4 consecutive holdings at q * 4, 4 more at 64 + q * 4 (q = the lane's
// coordinate 0 .. 15 on that side), so that a lane's keys are two 16-byte LDS loads and a wave's loads fall on consecutive banks
__device__ __forceinline__ uint32_t pfm_tile_slot(uint32_t q, int e) { return (e < 4 ? 0u : 64u) + q * 4u + (uint32_t)(e & 3); }

// One hero key against a lane's eight villain keys on one board: w[j] += kh > kv[j], t[j] += kh == kv[j].  On the device the instructions are
// spelled out, two pairs at a time: four compares into four scalar masks, then the four add-with-carry that consume them.  Left to the
// compiler, the 128 compares of a board are hoisted ahead of their adds and their masks spilled (869 scalar spills and scratch memory,
// read off the ISA).  A compare's mask -> the add's carry-in is interlocked by the hardware; no wait state is owed.
#define PFM_PAIR2(J, K)                                           \
    "v_cmp_gt_u32_e64 %[a], %[h], %[v" #J "]\n\t"                  \
    "v_cmp_eq_u32_e64 %[b], %[h], %[v" #J "]\n\t"                  \
    "v_cmp_gt_u32_e64 %[c], %[h], %[v" #K "]\n\t"                  \
    "v_cmp_eq_u32_e64 %[d], %[h], %[v" #K "]\n\t"                  \
    "v_addc_co_u32_e64 %[w" #J "], %[a], 0, %[w" #J "], %[a]\n\t"  \
    "v_addc_co_u32_e64 %[t" #J "], %[b], 0, %[t" #J "], %[b]\n\t"  \
    "v_addc_co_u32_e64 %[w" #K "], %[c], 0, %[w" #K "], %[c]\n\t"  \
    "v_addc_co_u32_e64 %[t" #K "], %[d], 0, %[t" #K "], %[d]\n\t"
__device__ __forceinline__ void pfm_tally_row(uint32_t (&w)[8], uint32_t (&t)[8], uint32_t kh, const uint32_t (&kv)[8]) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(PK_HOST_SIM)
    uint64_t a, b, c, d;
    asm(PFM_PAIR2(0, 1) PFM_PAIR2(2, 3) PFM_PAIR2(4, 5) PFM_PAIR2(6, 7)
        : [w0] "+v"(w[0]), [w1] "+v"(w[1]), [w2] "+v"(w[2]), [w3] "+v"(w[3]), [w4] "+v"(w[4]), [w5] "+v"(w[5]), [w6] "+v"(w[6]), [w7] "+v"(w[7]),
          [t0] "+v"(t[0]), [t1] "+v"(t[1]), [t2] "+v"(t[2]), [t3] "+v"(t[3]), [t4] "+v"(t[4]), [t5] "+v"(t[5]), [t6] "+v"(t[6]), [t7] "+v"(t[7]),
          [a] "=&s"(a), [b] "=&s"(b), [c] "=&s"(c), [d] "=&s"(d)
        : [h] "v"(kh), [v0] "v"(kv[0]), [v1] "v"(kv[1]), [v2] "v"(kv[2]), [v3] "v"(kv[3]), [v4] "v"(kv[4]), [v5] "v"(kv[5]), [v6] "v"(kv[6]), [v7] "v"(kv[7]));
#else
    for (int j = 0; j < 8; ++j) {
        w[j] += kh > kv[j] ? 1u : 0u;
        t[j] += kh == kv[j] ? 1u : 0u;
    }
#endif
}
#undef PFM_PAIR2

// registers per lane: 128 counters + 16 keys; two waves per SIMD (two workgroups per CU) leave a lane 256
template <bool STORE>
__global__ void __launch_bounds__(PFM_COUNT_BLOCK, 2) k_pfm_count(const uint32_t *__restrict__ keys, uint32_t n, uint32_t slice, uint32_t *__restrict__ win,
                                                                  uint32_t *__restrict__ tie) {
    __shared__ uint4 sH[PFM_RUN * PFM_TILE / 4], sV[PFM_RUN * PFM_TILE / 4];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t tile = blockIdx.x % (PFM_STRIPS * PFM_STRIPS), th = tile / PFM_STRIPS, tv = tile % PFM_STRIPS;   // the grid: tiles x slices
    const uint32_t b0 = blockIdx.x / (PFM_STRIPS * PFM_STRIPS) * slice, b1 = min(b0 + slice, n);
    uint32_t w[8][8], t[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) { w[i][j] = 0; t[i][j] = 0; }
    const uint4 *keys4 = reinterpret_cast<const uint4 *>(keys);
    for (uint32_t run = b0; run < b1; run += PFM_RUN) {
        __syncthreads();                              // (the run before is done with)
        // stage: PFM_RUN rows of 32 uint4 per side; a board past the slice is out of play for everybody
#pragma unroll
        for (int i = 0; i < PFM_RUN * PFM_TILE / 4 / PFM_COUNT_BLOCK; ++i) {
            const uint32_t idx = tid + (uint32_t)i * PFM_COUNT_BLOCK, row = idx >> 5, col = idx & 31u, b = run + row;
            uint4 h, v;
            h.x = PFM_SENT; h.y = PFM_SENT; h.z = PFM_SENT; h.w = PFM_SENT;
            v = h;
            if (b < b1) {
                const size_t base = (size_t)b * (PFM_STRIDE / 4);
                h = keys4[base + th * (PFM_TILE / 4) + col];
                v = keys4[base + tv * (PFM_TILE / 4) + col];
            }
            h.x = h.x == PFM_SENT ? 0u : h.x; h.y = h.y == PFM_SENT ? 0u : h.y; h.z = h.z == PFM_SENT ? 0u : h.z; h.w = h.w == PFM_SENT ? 0u : h.w;
            sH[PK_IDX(idx, PFM_RUN * PFM_TILE / 4, "sH")] = h;
            sV[PK_IDX(idx, PFM_RUN * PFM_TILE / 4, "sV")] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t r = 0; r < (uint32_t)PFM_RUN; ++r) {
            const uint4 h0 = sH[PK_IDX(r * 32u + ty, PFM_RUN * PFM_TILE / 4, "sH")], h1 = sH[PK_IDX(r * 32u + 16u + ty, PFM_RUN * PFM_TILE / 4, "sH")];
            const uint4 v0 = sV[PK_IDX(r * 32u + tx, PFM_RUN * PFM_TILE / 4, "sV")], v1 = sV[PK_IDX(r * 32u + 16u + tx, PFM_RUN * PFM_TILE / 4, "sV")];
            const uint32_t kh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w}, kv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) pfm_tally_row(w[i], t[i], kh[i], kv);
        }
    }
    // ---- the tile's counts: pairs that share a card (the diagonal too) are 0
    uint64_t cv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t o = tv * PFM_TILE + pfm_tile_slot(tx, j);
        cv[j] = o < (uint32_t)PFM_HOLDINGS ? pfm_cards(o) : ~0ull;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t h = th * PFM_TILE + pfm_tile_slot(ty, i);
        if (h >= (uint32_t)PFM_HOLDINGS) continue;
        const uint64_t ch = pfm_cards(h);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t o = tv * PFM_TILE + pfm_tile_slot(tx, j);
            if (o >= (uint32_t)PFM_HOLDINGS) continue;
            const bool share = (ch & cv[j]) != 0ull;
            const uint32_t wv = share ? 0u : w[i][j], tv_ = share ? 0u : t[i][j];
            const size_t cell = PK_IDX((size_t)h * PFM_HOLDINGS + o, PFM_CELLS, "matchup cell");
            if constexpr (STORE) {
                if (win) win[cell] = wv;
                if (tie) tie[cell] = tv_;
            } else {
                if (win && wv) atomicAdd(&win[cell], wv);
                if (tie && tv_) atomicAdd(&tie[cell], tv_);
            }
        }
    }
}

#define PFM_PREP_BLOCK 256

struct PfmPrepArgs {
    const uint8_t *hero;
    EqTables t;
    PfmOut out;
    uint32_t *desc;
    int N, observer;
    size_t m;
};

template <bool TABLE>
__global__ void __launch_bounds__(PFM_PREP_BLOCK) k_pfm_prep(PfmPrepArgs a) {
    const size_t i = (size_t)blockIdx.x * PFM_PREP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    uint32_t status = 0, lo = 52, hi = 0;
    uint64_t seen = 0;
    // one card byte: a byte that is no card (0xFF too), or a card seen before, is refused
    auto card = [&](uint32_t c) {
        if (c >= 0x40u || (c & 15u) >= 13u) { status |= PK_EQ_BAD_CARD; return; }
        const uint32_t k = (c & 15u) * 4u + (c >> 4);                           // canonical index (cards.py:77)
        status |= ((seen >> k) & 1ull) ? (uint32_t)PK_EQ_DUP_CARD : 0u;
        seen |= 1ull << k;
        lo = k < lo ? k : lo; hi = k > hi ? k : hi;
    };
    if constexpr (TABLE) {
        const int64_t t = a.t.tables ? (int64_t)a.t.tables[i] : (int64_t)i;
        if (t < 0 || t >= (int64_t)a.t.T) status |= PK_EQ_BAD_TABLE;            // (nothing is read)
        else {
            const Cursor cur{a.t.cursors[t]};
            if (cur.in_flight()) status |= PK_EQ_IN_FLIGHT;
            const int who = a.observer == PK_OBSERVER_ACTIVE ? (int)cur.active() : a.observer;
            if (who < 0 || who >= a.N) status |= PK_EQ_BAD_CARD;                // (a cursor no game writes: there is no such seat to read)
            else {
                card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, 5 + 2 * who));   // (the board is not read: the starting hand, at whatever turn)
                card(card_byte(a.t.cards, (size_t)a.t.T, (int)t, 6 + 2 * who));
            }
        }
    } else {
        card(a.hero[i * 2]);
        card(a.hero[i * 2 + 1]);
    }
    a.desc[i] = status ? PFM_NO_HOLDING : tri(hi) + lo;
    if (a.out.boards) a.out.boards[i] = status ? 0u : (uint32_t)PK_PREFLOP_BOARDS;
    if (a.out.status) a.out.status[i] = (uint8_t)status;
}

__global__ void __launch_bounds__(PFM_READ_BLOCK) k_pfm_hero(const uint32_t *__restrict__ M, const uint32_t *__restrict__ desc, PfmWeights wts, PfmOut out,
                                                             uint32_t m) {
    __shared__ uint64_t red[PFM_READ_WAVES][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    uint64_t oc[PFM_READ_PER_LANE];                   // the cards of the villain holdings this lane reads: o = tid + 256 j
#pragma unroll
    for (int j = 0; j < PFM_READ_PER_LANE; ++j) {
        const uint32_t o = tid + (uint32_t)j * PFM_READ_BLOCK;
        oc[j] = o < (uint32_t)PFM_HOLDINGS ? pfm_cards(o) : ~0ull;
    }
    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        const uint32_t h = uniform(desc[spot]);
        const bool ok = h != PFM_NO_HOLDING;          // (a refused spot: zeros)
        const uint64_t hc = ok ? pfm_cards(h) : ~0ull;
        const uint32_t *rw = M + (size_t)(ok ? h : 0u) * PFM_HOLDINGS, *rt = rw + PFM_CELLS;
        const uint16_t *wv = wts.w ? wts.w + (wts.per_spot ? (size_t)spot * PFM_HOLDINGS : 0) : nullptr;
        uint64_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
        for (int j = 0; j < PFM_READ_PER_LANE; ++j) {
            const uint32_t o = tid + (uint32_t)j * PFM_READ_BLOCK;
            if (o < (uint32_t)PFM_HOLDINGS) {
                const uint32_t w = ok ? rw[PK_IDX(o, PFM_HOLDINGS, "row")] : 0u, t = ok ? rt[PK_IDX(o, PFM_HOLDINGS, "row")] : 0u;
                if (out.win) out.win[(size_t)spot * PFM_HOLDINGS + o] = w;
                if (out.tie) out.tie[(size_t)spot * PFM_HOLDINGS + o] = t;
                if (out.agg) {
                    const uint64_t wt = wv ? (uint64_t)wv[o] : 1ull;
                    a0 += wt * w; a1 += wt * t; a2 += (hc & oc[j]) ? 0ull : wt;
                }
            }
        }
        if (out.agg) {
            a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
            __syncthreads();                          // (the spot before has read the sums)
            if (lane == 0) { red[PK_IDX(wave, PFM_READ_WAVES, "red")][0] = a0; red[wave][1] = a1; red[wave][2] = a2; }
            __syncthreads();
            if (tid == 0) {
                uint64_t r0 = 0, r1 = 0, r2 = 0;
                for (int v = 0; v < PFM_READ_WAVES; ++v) { r0 += red[PK_IDX(v, PFM_READ_WAVES, "red")][0]; r1 += red[v][1]; r2 += red[v][2]; }
                out.agg[(size_t)spot * 3] = r0;
                out.agg[(size_t)spot * 3 + 1] = r1;
                out.agg[(size_t)spot * 3 + 2] = (uint64_t)PK_PREFLOP_BOARDS * r2;
            }
        }
    }
}

__global__ void __launch_bounds__(PFM_READ_BLOCK) k_pfm_rvr(const uint32_t *__restrict__ M, const uint16_t *__restrict__ weights, uint32_t m,
                                                            uint64_t *__restrict__ win, uint64_t *__restrict__ tie, uint64_t *__restrict__ tot) {
    __shared__ uint64_t red[PFM_READ_WAVES][PFM_RVR_ROWS][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    const uint32_t h0 = blockIdx.x * PFM_RVR_ROWS;    // this workgroup's rows h0 .. h0 + PFM_RVR_ROWS - 1 (1326 is a multiple of PFM_RVR_ROWS)
    uint32_t mw[PFM_RVR_ROWS][PFM_READ_PER_LANE], mt[PFM_RVR_ROWS][PFM_READ_PER_LANE];
    bool apart[PFM_RVR_ROWS][PFM_READ_PER_LANE];      // holding o shares no card with row r
#pragma unroll
    for (int r = 0; r < PFM_RVR_ROWS; ++r) {
        const uint64_t hc = pfm_cards(h0 + (uint32_t)r);
        const uint32_t *rw = M + (size_t)(h0 + (uint32_t)r) * PFM_HOLDINGS, *rt = rw + PFM_CELLS;
#pragma unroll
        for (int j = 0; j < PFM_READ_PER_LANE; ++j) {
            const uint32_t o = tid + (uint32_t)j * PFM_READ_BLOCK;
            const bool in = o < (uint32_t)PFM_HOLDINGS;
            mw[r][j] = in ? rw[PK_IDX(o, PFM_HOLDINGS, "row")] : 0u;
            mt[r][j] = in ? rt[PK_IDX(o, PFM_HOLDINGS, "row")] : 0u;
            apart[r][j] = in && !(hc & pfm_cards(in ? o : 0u));
        }
    }
    for (uint32_t spot = 0; spot < m; ++spot) {
        const uint16_t *wv = weights ? weights + (size_t)spot * PFM_HOLDINGS : nullptr;
        uint32_t wt[PFM_READ_PER_LANE];
#pragma unroll
        for (int j = 0; j < PFM_READ_PER_LANE; ++j) {
            const uint32_t o = tid + (uint32_t)j * PFM_READ_BLOCK;
            wt[j] = o < (uint32_t)PFM_HOLDINGS ? (wv ? (uint32_t)wv[o] : 1u) : 0u;
        }
        uint64_t a[PFM_RVR_ROWS][3];
#pragma unroll
        for (int r = 0; r < PFM_RVR_ROWS; ++r) {
            a[r][0] = 0; a[r][1] = 0; a[r][2] = 0;
#pragma unroll
            for (int j = 0; j < PFM_READ_PER_LANE; ++j) {
                a[r][0] += (uint64_t)wt[j] * mw[r][j];
                a[r][1] += (uint64_t)wt[j] * mt[r][j];
                a[r][2] += apart[r][j] ? (uint64_t)wt[j] : 0ull;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) a[r][c] = wave_sum(a[r][c]);
        }
        __syncthreads();                              // (the spot before has read the sums)
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < PFM_RVR_ROWS; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) red[PK_IDX(wave, PFM_READ_WAVES, "red")][r][c] = a[r][c];
        }
        __syncthreads();
        if (tid < (uint32_t)PFM_RVR_ROWS * 3u) {
            const uint32_t r = tid / 3u, c = tid % 3u;
            uint64_t s = 0;
            for (int v = 0; v < PFM_READ_WAVES; ++v) s += red[PK_IDX(v, PFM_READ_WAVES, "red")][r][c];
            const size_t cell = (size_t)spot * PFM_HOLDINGS + h0 + r;
            if (c == 0u && win) win[cell] = s;
            if (c == 1u && tie) tie[cell] = s;
            if (c == 2u && tot) tot[cell] = (uint64_t)PK_PREFLOP_BOARDS * s;
        }
    }
}

namespace pk {

hipError_t pfm_count_launch(hipStream_t stream, const uint32_t *tab, uint32_t first, uint32_t n, int accumulate, uint32_t chunk, uint32_t *keys,
                            uint32_t *win, uint32_t *tie) {
    if (!(win || tie)) return hipSuccess;
    const uint32_t slice = pfm_slice_boards(chunk);
    bool store = accumulate == 0;
    for (uint32_t pos = first, end = first + n; pos < end;) {
        const uint32_t cap = store && slice < chunk ? slice : chunk, cn = end - pos < cap ? end - pos : cap;   // (a storing launch is one slice deep, one workgroup per tile; never more boards than `keys` holds)
        hipLaunchKernelGGL(k_pfm_rank, dim3((cn + PFM_RANK_BOARDS - 1) / PFM_RANK_BOARDS), dim3(PFM_RANK_BLOCK), 0, stream, tab, pos, cn, keys);
        const dim3 grid(PFM_STRIPS * PFM_STRIPS * ((cn + slice - 1) / slice));
        if (store) hipLaunchKernelGGL(k_pfm_count<true>, grid, dim3(PFM_COUNT_BLOCK), 0, stream, (const uint32_t *)keys, cn, slice, win, tie);
        else hipLaunchKernelGGL(k_pfm_count<false>, grid, dim3(PFM_COUNT_BLOCK), 0, stream, (const uint32_t *)keys, cn, slice, win, tie);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        store = false;
        pos += cn;
    }
    return hipSuccess;
}

hipError_t pfm_hero_launch(hipStream_t stream, const uint32_t *M, const uint8_t *hero, const EqTables *tables, int N, int observer,
                           const PfmWeights &weights, size_t m, const PfmOut &out, uint32_t *desc) {
    if (m == 0) return hipSuccess;
    PfmPrepArgs a{};
    a.hero = hero;
    if (tables) a.t = *tables;
    a.out = out; a.desc = desc; a.N = N; a.observer = observer; a.m = m;
    const dim3 pgrid((unsigned)((m + PFM_PREP_BLOCK - 1) / PFM_PREP_BLOCK));
    if (tables) hipLaunchKernelGGL(k_pfm_prep<true>, pgrid, dim3(PFM_PREP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_pfm_prep<false>, pgrid, dim3(PFM_PREP_BLOCK), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !(out.agg || out.win || out.tie)) return e;   // (boards / status alone: the preparation kernel has written them)
    const unsigned grid = (unsigned)(m < (size_t)PFM_HERO_GRID_MAX ? m : (size_t)PFM_HERO_GRID_MAX);
    hipLaunchKernelGGL(k_pfm_hero, dim3(grid), dim3(PFM_READ_BLOCK), 0, stream, M, (const uint32_t *)desc, weights, out, (uint32_t)m);
    return hipGetLastError();
}

hipError_t pfm_rvr_launch(hipStream_t stream, const uint32_t *M, const uint16_t *weights, size_t m, uint64_t *win, uint64_t *tie, uint64_t *tot) {
    static_assert(PFM_HOLDINGS % PFM_RVR_ROWS == 0, "every workgroup has PFM_RVR_ROWS rows");
    if (m == 0 || !(win || tie || tot)) return hipSuccess;
    hipLaunchKernelGGL(k_pfm_rvr, dim3(PFM_HOLDINGS / PFM_RVR_ROWS), dim3(PFM_READ_BLOCK), 0, stream, M, weights, (uint32_t)m, win, tie, tot);
    return hipGetLastError();
}

}  // namespace pk
