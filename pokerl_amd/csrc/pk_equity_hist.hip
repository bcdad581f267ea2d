// pk_equity_hist.hip -- strength histograms: for EVERY holding the hero can have on a public board, how its river strength against a
// weighted opponent range is distributed over the completions of the board (include/pokerl_hip.h "Strength histograms", DESIGN.md section
// 3.5).  The spots are checked by range vs range's own preparation kernel (k_rvr_prep, pk_equity_rvr.hip: the same descriptor, the same
// status).  Two kernels here:
//   k_hist_counts  one lane per spot: completions = C(P - 2, k) from the descriptor (0 for a refused spot);
//   k_hist         k_rvr's grid, workgroup and LDS layout (a persistent grid of 512-thread workgroups, the 32 KB rank-mask table of eval7_tab
//                  in LDS, ONE SPOT PER WORKGROUP at a time, holdings indexed by pool slots) and, per completion of the board, k_rvr's three
//                  stages, copied (k_rvr itself is untouched):
//                    rank      every pool holding that shares no card with the completion is evaluated once; key and sort slot;
//                    order     workgroup bitonic sort of the slots; an exclusive prefix sum of the weights in sorted order, whose grand
//                              total is the completion's live weight;
//                    combine   per holding h a lane owns: the weight below and equal by binary search, the 2 (P - 2) card-sharing holdings
//                              and h itself taken back out by their own keys -- and out of the live weight, which gives den.
//                  Then, instead of adding below / equal up: bin = min(nbins - 1, nbins (2 below + equal) / (2 den)) in 32-bit integers and
//                  ONE u16 load / add / store in h's own output row (den = 0: a `void` counter in a register).  The workgroup zeroes the
//                  spot's rows first, coalesced; a row belongs to one lane from then on, so there are no atomics, and one lane's accesses to
//                  one address stay in order.
// Ordinary vector loads / stores and LDS loads / stores only; no atomics, no scratch memory (tests/test_hist_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_hist.hpp"

using namespace pk;



__global__ void __launch_bounds__(HIST_COUNTS_BLOCK) k_hist_counts(const uint64_t *__restrict__ desc, uint32_t *__restrict__ completions, size_t m) {
    const size_t i = (size_t)blockIdx.x * HIST_COUNTS_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint64_t meta = desc[i * (size_t)RVR_DESC_WORDS + 2];
    const uint32_t boards = (uint32_t)meta, k = (uint32_t)(meta >> 48) & 0xffu, P = (uint32_t)(meta >> 56);
    completions[i] = boards ? binom2(P - 2u, k) : 0u;                      // (boards != 0: the spot is good, P >= k + 4)
}


// registers per lane: four waves per SIMD (two 512-thread workgroups per CU, what the group segment allows) cap a lane at 128 registers
__global__ void __launch_bounds__(RVR_BLOCK, 4) k_hist(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, RvrWeights wts, HistOut out,
                                                       uint32_t nbins, uint32_t m) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t slot[RVR_SLOTS];              // key << 11 | pool holding, sorted per completion; all ones = no holding
    __shared__ uint32_t pre[RVR_PREFIX];              // pre[i]: the weight of sorted positions 0 .. i - 1
    __shared__ uint32_t keyw[RVR_POOL_HOLDINGS];      // this completion's key per pool holding (RVR_SENT: shares a card with the completion)
    __shared__ uint16_t wp[RVR_POOL_HOLDINGS];        // the spot's weights per pool holding
    __shared__ uint64_t pool[64];                     // card j of the pool (canonical order) as its bit in the suit-lane layout
    __shared__ uint32_t canon[64];                    // ... and its canonical index
    __shared__ uint32_t wsum[RVR_WAVES];
    stage_eval7_tab<RVR_BLOCK>(T, tab);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uniform(tid >> 6);
    const uint32_t row_words = (uint32_t)RVR_HOLDINGS * nbins;                // u16 entries of one spot's rows: at most 42 432
    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                              // (the table; the spot before: its pool, weights, keys and sums are done with)
        const uint64_t *d = desc + (size_t)spot * RVR_DESC_WORDS;
        const uint64_t known = uniform(d[0]), avail = uniform(d[1]), meta = uniform(d[2]);
        const uint32_t boards = (uint32_t)meta, k = (uint32_t)(meta >> 48) & 0xffu, P = (uint32_t)(meta >> 56);
        uint16_t *rows = out.hist ? out.hist + (size_t)spot * row_words : nullptr;
        // ---- every entry of the spot's rows is written: zeros first, by the whole workgroup (a refused spot, an invalid holding: they stay)
        if (rows)
            for (uint32_t i = tid; i < row_words; i += RVR_BLOCK) rows[i] = 0;
        uint32_t voidc[RVR_PER_LANE];
#pragma unroll
        for (int j = 0; j < RVR_PER_LANE; ++j) voidc[j] = 0;
        if (boards) {                                 // (a refused spot: zeros)
            fill_pool(pool, canon, avail, tid);
            __syncthreads();                          // (... and the zeros above are in place before any lane counts in its rows)
            const uint32_t nh = tri(P), nreal = tri(P - k);   // pool holdings; those a completion leaves in play
            uint32_t npad = 64;
            while (npad < nh) npad <<= 1;                             // (> nh: C(P, 2) is no power of two for P >= 3, so a pad slot always exists)
            // ---- per spot: the pool holdings this lane ranks (ea < eb pool slots), the weights by pool holding, the pad slots
            const uint16_t *wv = wts.w ? wts.w + (wts.per_spot ? (size_t)spot * RVR_HOLDINGS : 0) : nullptr;
            uint64_t ebits[RVR_PER_LANE];
            uint32_t ea[RVR_PER_LANE], eb[RVR_PER_LANE];
#pragma unroll
            for (int j = 0; j < RVR_PER_LANE; ++j) {
                const uint32_t ph = tid + (uint32_t)j * RVR_BLOCK;
                ea[j] = RVR_NONE; eb[j] = RVR_NONE; ebits[j] = 0;
                if (ph < nh) {
                    unpair(ph, ea[j], eb[j]);
                    ebits[j] = pool[PK_IDX(ea[j], 64, "pool")] | pool[PK_IDX(eb[j], 64, "pool")];
                    const uint32_t gh = tri(canon[PK_IDX(eb[j], 64, "canon")]) + canon[PK_IDX(ea[j], 64, "canon")];
                    const uint32_t w = wv ? (uint32_t)wv[PK_IDX(gh, RVR_HOLDINGS, "weights")] : 1u;
                    wp[PK_IDX(ph, RVR_POOL_HOLDINGS, "wp")] = (uint16_t)w;
                }
            }
            for (uint32_t i = nh + tid; i < npad; i += RVR_BLOCK) slot[PK_IDX(i, RVR_SLOTS, "slot")] = ~0ull;   // (stay all ones: every sorted position >= nreal is)
            // ... the holdings this lane OWNS (h = tid + 512 j of the fixed index space) as pool slots ha < hb; hph: their pool holding
            uint32_t ha[RVR_PER_LANE], hb[RVR_PER_LANE], hph[RVR_PER_LANE];
            bool hvalid[RVR_PER_LANE];
#pragma unroll
            for (int j = 0; j < RVR_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * RVR_BLOCK;
                uint32_t ca = 0, cb = 1;
                if (h < (uint32_t)RVR_HOLDINGS) unpair(h, ca, cb);
                hvalid[j] = h < (uint32_t)RVR_HOLDINGS && ((avail >> ca) & (avail >> cb) & 1ull);
                ha[j] = (uint32_t)__popcll(avail & ((1ull << ca) - 1ull));
                hb[j] = (uint32_t)__popcll(avail & ((1ull << cb) - 1ull));
                hph[j] = hvalid[j] ? tri(hb[j]) + ha[j] : 0u;
            }
            // ---- the completions: {ci < cj} in pair order (k = 2), {c} (k = 1), {} (k = 0)
            const uint32_t ncomp = binom2(P, k);
            uint32_t ci = 0, cj = 1;
            for (uint32_t c = 0; c < ncomp; ++c) {
                const uint32_t x0 = k == 2u ? ci : (k == 1u ? c : RVR_NONE), x1 = k == 2u ? cj : RVR_NONE;
                const uint64_t board = known | pool[PK_IDX(x0, 64, "pool")] | pool[PK_IDX(x1, 64, "pool")];
                // rank
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    const uint32_t ph = tid + (uint32_t)j * RVR_BLOCK;
                    if (ph < nh) {
                        const bool gone = ea[j] == x0 || ea[j] == x1 || eb[j] == x0 || eb[j] == x1;
                        uint32_t key = RVR_SENT;
                        if (!gone) key = order_key(eval7_tab_back(eval7_tab_front_bits(board | ebits[j], T), T));
                        keyw[PK_IDX(ph, RVR_POOL_HOLDINGS, "keyw")] = key;
                        slot[PK_IDX(ph, RVR_SLOTS, "slot")] = gone ? ~0ull : (((uint64_t)key << 11) | ph);
                    }
                }
                __syncthreads();
                // order: bitonic sort of slot[0 .. npad), ascending
                for (uint32_t kk = 2; kk <= npad; kk <<= 1) {
                    for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
                        for (uint32_t t = tid; t < (npad >> 1); t += RVR_BLOCK) {
                            const uint32_t lo = ((t & ~(jj - 1u)) << 1) | (t & (jj - 1u)), hi = lo | jj;
                            const uint64_t a = slot[PK_IDX(lo, RVR_SLOTS, "slot")], b = slot[PK_IDX(hi, RVR_SLOTS, "slot")];
                            const bool up = (lo & kk) == 0u;
                            if ((a > b) == up) { slot[PK_IDX(lo, RVR_SLOTS, "slot")] = b; slot[PK_IDX(hi, RVR_SLOTS, "slot")] = a; }
                        }
                        __syncthreads();
                    }
                }
                // exclusive prefix sum of the weights in sorted order: three positions per lane, a wave scan, the waves' totals
                uint32_t v[RVR_PER_LANE], mine = 0;
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    const uint32_t i = tid * RVR_PER_LANE + (uint32_t)j;
                    v[j] = 0;
                    if (i < nreal) v[j] = wp[PK_IDX((uint32_t)slot[PK_IDX(i, RVR_SLOTS, "slot")] & 2047u, RVR_POOL_HOLDINGS, "wp")];
                    mine += v[j];
                }
                uint32_t inc = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t y = __shfl_up(inc, off);
                    inc += lane >= (uint32_t)off ? y : 0u;
                }
                if (lane == 63u) wsum[PK_IDX(wave, RVR_WAVES, "wsum")] = inc;
                __syncthreads();
                uint32_t run = inc - mine, live = 0;  // live: the weight of every holding in play on this completion
#pragma unroll
                for (int w = 0; w < RVR_WAVES; ++w) {
                    const uint32_t s = wsum[PK_IDX(w, RVR_WAVES, "wsum")];
                    run += (uint32_t)w < wave ? s : 0u;
                    live += s;
                }
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    pre[PK_IDX(tid * RVR_PER_LANE + (uint32_t)j, RVR_PREFIX, "pre")] = run;
                    run += v[j];
                }
                __syncthreads();
                // combine, bin, count
#pragma unroll
                for (int j = 0; j < RVR_PER_LANE; ++j) {
                    if (!hvalid[j]) continue;
                    const uint32_t kh = keyw[PK_IDX(hph[j], RVR_POOL_HOLDINGS, "keyw")];
                    if (kh == RVR_SENT) continue;                                  // (h shares a card with this completion)
                    uint32_t lb = 0, ub = 0;                                        // sorted positions with a key < kh, <= kh
                    for (uint32_t step = npad >> 1; step > 0; step >>= 1) {
                        const uint32_t kl = (uint32_t)(slot[PK_IDX(lb + step - 1u, RVR_SLOTS, "slot")] >> 11);
                        const uint32_t ku = (uint32_t)(slot[PK_IDX(ub + step - 1u, RVR_SLOTS, "slot")] >> 11);
                        lb += kl < kh ? step : 0u;
                        ub += ku <= kh ? step : 0u;
                    }
                    const uint32_t below0 = pre[PK_IDX(lb, RVR_PREFIX, "pre")];
                    uint32_t below = below0, equal = pre[PK_IDX(ub, RVR_PREFIX, "pre")] - below0, den = live;
                    // card removal: h itself, and every holding {ha, x}, {hb, x} that is in play
                    const uint32_t wh = wp[PK_IDX(hph[j], RVR_POOL_HOLDINGS, "wp")];
                    equal -= wh;
                    den -= wh;
                    const uint32_t ta = tri(ha[j]), tb = tri(hb[j]);
                    for (uint32_t x = 0; x < P; ++x) {
                        if (x == ha[j] || x == hb[j]) continue;
                        const uint32_t tx = tri(x);
                        const uint32_t p0 = PK_IDX(pair(ha[j], ta, x, tx), RVR_POOL_HOLDINGS, "pair"), p1 = PK_IDX(pair(hb[j], tb, x, tx), RVR_POOL_HOLDINGS, "pair");
                        const uint32_t k0 = keyw[p0], k1 = keyw[p1], w0 = wp[p0], w1 = wp[p1];   // (p0, p1: checked above)
                        below -= (k0 < kh ? w0 : 0u) + (k1 < kh ? w1 : 0u);
                        equal -= (k0 == kh ? w0 : 0u) + (k1 == kh ? w1 : 0u);
                        den -= (k0 != RVR_SENT ? w0 : 0u) + (k1 != RVR_SENT ? w1 : 0u);
                    }
                    if (den == 0u) { ++voidc[j]; continue; }
                    // nbins (2 below + equal) <= 32 * 2 * 65 535 * 990 < 2^32; 2 below + equal <= 2 den, so the quotient is at most nbins
                    uint32_t bin = nbins * (2u * below + equal) / (2u * den);
                    bin = bin < nbins - 1u ? bin : nbins - 1u;
                    if (rows) {
                        uint16_t *cell = rows + PK_IDX((tid + (uint32_t)j * RVR_BLOCK) * nbins + bin, row_words, "hist");
                        *cell = (uint16_t)(*cell + 1u);                             // this lane's own row: at most C(47, 2) = 1 081 per cell
                    }
                }
                __syncthreads();                      // (the keys and slots are rewritten by the next completion)
                ++ci;
                if (ci == cj) { ci = 0; ++cj; }
            }
        }
        // ---- output: every holding's void count (zeros included)
        if (out.void_) {
#pragma unroll
            for (int j = 0; j < RVR_PER_LANE; ++j) {
                const uint32_t h = tid + (uint32_t)j * RVR_BLOCK;
                if (h < (uint32_t)RVR_HOLDINGS) out.void_[(size_t)spot * RVR_HOLDINGS + h] = (uint16_t)voidc[j];
            }
        }
    }
}

namespace pk {

hipError_t hist_launch(hipStream_t stream, const uint32_t *tab, const RvrSpots *spots, const EqTables *tables, const RvrWeights &weights, size_t m,
                       int nbins, const HistOut &out, uint64_t *desc) {
    if (m == 0) return hipSuccess;
    hipError_t e = rvr_prep_launch(stream, spots, tables, m, RvrOut{nullptr, nullptr, nullptr, nullptr, out.status}, desc);
    if (e != hipSuccess) return e;
    if (out.completions) {
        hipLaunchKernelGGL(k_hist_counts, dim3((unsigned)((m + HIST_COUNTS_BLOCK - 1) / HIST_COUNTS_BLOCK)), dim3(HIST_COUNTS_BLOCK), 0, stream,
                           (const uint64_t *)desc, out.completions, m);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!(out.hist || out.void_)) return hipSuccess;                           // (completions / status alone: the one-lane-per-spot kernels have written them)
    const unsigned grid = (unsigned)(m < (size_t)RVR_GRID_MAX ? m : (size_t)RVR_GRID_MAX);
    hipLaunchKernelGGL(k_hist, dim3(grid), dim3(RVR_BLOCK), 0, stream, tab, (const uint64_t *)desc, weights, out, (uint32_t)nbins, (uint32_t)m);
    return hipGetLastError();
}

}  // namespace pk
