// pk_equity_hist_hero.hip -- the hero form of the strength histograms: how ONE seat's river strength against a weighted opponent range is
// distributed over the completions of the board (include/pokerl_hip.h "Hero strength histogram") -- row h of
// pk_equity_hist for the one holding that is wanted, at the cost of pk_equity_range.  The spots are checked by range equity's own preparation
// kernel (k_eqr_prep through pk::eqr_prep_launch: the same descriptor, the same status).  Two kernels here (k_hero_hist*, not k_hist_hero*:
// the names that begin with k_hist are the public form's, and tests/test_hist_host.py counts them):
//   k_hero_hist_counts  one lane per spot: completions = C(P, k) from the descriptor (0 for a refused spot);
//   k_hero_hist         k_eqr's shape, and its hero and villain passes themselves (pk_equity_range.hpp: eqr_hero_pass, eqr_villain_pass with another
//                       callable): a persistent grid of 512-thread workgroups, the 32 KB rank-mask table
//                       of eval7_tab in LDS (staged once per workgroup), ONE SPOT PER WORKGROUP at a time, spots dealt round robin.  Per spot:
//                         weights       the spot's weight vector into LDS in the fixed 1 326 index space, 0 at the holdings that are not valid;
//                                       on the way the weight of the holdings that hold each card, W[card] (LDS atomics, 2 per holding);
//                         hero pass     the hero's ranking word on each of the C(P, k) completions, into LDS at the completion's pair / single
//                                       index; one wave adds the W[card] up: total = the weight of all valid holdings (each counted twice);
//                         villain pass  lanes enumerate the sets S of k + 2 pool cards (a contiguous index range per lane, unranked once, then
//                                       stepped), evaluate board | S ONCE, and for each of the C(k + 2, 2) splits of S into "board to come" and
//                                       "hole cards" look the hero's word of that completion up, decide with compare_rankings<2> and add the
//                                       HOLDING's weight to the counters of that split's COMPLETION -- below[comp] on a win, equal[comp] on a
//                                       tie (u32 LDS atomics).  That is the one difference from k_eqr, whose counters are the holding's;
//                         bin pass      one lane per completion: den by inclusion-exclusion, total - W[ci] - W[cj] + w[{ci, cj}] (k = 2),
//                                       total - W[c] (k = 1), total (k = 0); the integer bin rule with one unsigned 32-bit division; nbins + 1
//                                       u32 counters in LDS (the last is `void`); below / equal cleared for the next spot;
//                         output        hist / void from LDS (a refused spot: the zeros the counters hold); the counters cleared.
//                       den is NOT accumulated like below / equal: that would be a third atomic on EVERY split (the other two fire only on a
//                       win or a tie), and a third 4 324-byte array.  The per-card sums cost 2 x 1 326 atomics per spot against 6 x 178 365.
// The workgroup width and LDS atomics (against per-lane private accumulation) are TAKEN from k_eqr, not measured for this kernel.
// Ordinary vector loads / stores and LDS integer atomics only; no scratch memory (tests/test_hero_hist_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_equity_common.hpp"
#include "pk_equity_hist_hero.hpp"

using namespace pk;

constexpr int HH_CARDS = 52;
static_assert(HH_MAX_BINS + 1 <= 64 && HH_CARDS + 1 <= 64, "one wave clears the counters");


__global__ void __launch_bounds__(HH_COUNTS_BLOCK) k_hero_hist_counts(const uint64_t *__restrict__ desc, uint32_t *__restrict__ completions, size_t m) {
    const size_t i = (size_t)blockIdx.x * HH_COUNTS_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint64_t meta = desc[i * (size_t)EQR_DESC_WORDS + 3];
    const uint32_t boards = (uint32_t)meta, k = (uint32_t)(meta >> 48) & 0xffu, P = (uint32_t)(meta >> 56);
    completions[i] = boards ? binom2(P, k) : 0u;                           // (boards != 0: the spot is good, P >= k + 2)
}


// registers per lane: six waves per SIMD (three 512-thread workgroups per CU, what the group segment allows) caps a lane at 80 registers
__global__ void __launch_bounds__(HH_BLOCK, 6) k_hero_hist(const uint32_t *__restrict__ tab, const uint64_t *__restrict__ desc, EqrWeights wts, HeroHistOut out,
                                                           uint32_t nbins, uint32_t m) {
    __shared__ uint32_t T[EVAL7_TAB_WORDS];
    __shared__ uint64_t pool[64];                 // card j of the pool (canonical order) as its bit in the suit-lane layout
    __shared__ uint32_t canon[64];                // ... and its canonical index
    __shared__ uint32_t hero_w[EQR_COMPLETIONS];  // the hero's ranking word per completion of the board
    __shared__ uint32_t below[EQR_COMPLETIONS], equal[EQR_COMPLETIONS];   // per completion: the weight the hero beats / ties
    __shared__ uint16_t wt[EQR_HOLDINGS];         // the spot's weights; 0 at a holding that is not valid
    __shared__ uint32_t wcard[64];                // [c < 52] the weight of the valid holdings that hold card c; [52] the weight of all of them
    __shared__ uint32_t cnt[64];                  // [b < nbins] the histogram, [nbins] void
    stage_eval7_tab<HH_BLOCK>(T, tab);
    for (int c = threadIdx.x; c < EQR_COMPLETIONS; c += HH_BLOCK) { below[PK_IDX(c, EQR_COMPLETIONS, "below")] = 0; equal[PK_IDX(c, EQR_COMPLETIONS, "equal")] = 0; }
    if (threadIdx.x < 64u) { wcard[threadIdx.x] = 0; cnt[threadIdx.x] = 0; }
    const uint32_t tid = threadIdx.x, wave = uniform(tid >> 6);
    for (uint32_t spot = blockIdx.x; spot < m; spot += gridDim.x) {
        __syncthreads();                          // (the table and the cleared counters; the spot before: everything of it is done with)
        const uint64_t *d = desc + (size_t)spot * EQR_DESC_WORDS;
        const uint64_t known = uniform(d[0]), hero = uniform(d[1]), avail = uniform(d[2]), meta = uniform(d[3]);
        const uint32_t boards = (uint32_t)meta, k = (uint32_t)(meta >> 48) & 0xffu, P = (uint32_t)(meta >> 56);
        if (boards) {                             // (a refused spot: its counters stay zero)
            fill_pool(pool, canon, avail, tid);
            // ---- weights: the fixed index space, 0 where a card of the holding is not in the pool; the per-card sums
            const uint16_t *wv = wts.w ? wts.w + (wts.per_spot ? (size_t)spot * EQR_HOLDINGS : 0) : nullptr;
            for (uint32_t h = tid; h < (uint32_t)EQR_HOLDINGS; h += HH_BLOCK) {
                uint32_t ca, cb;
                unpair(h, ca, cb);
                const bool valid = (avail >> ca) & (avail >> cb) & 1ull;
                const uint32_t w = valid ? (wv ? (uint32_t)wv[h] : 1u) : 0u;
                wt[PK_IDX(h, EQR_HOLDINGS, "wt")] = (uint16_t)w;
                if (w) { atomicAdd(&wcard[PK_IDX(ca, HH_CARDS, "wcard")], w); atomicAdd(&wcard[PK_IDX(cb, HH_CARDS, "wcard")], w); }   // (at most 51 * 65 535 each)
            }
            __syncthreads();
            // ---- hero pass: the hero's word per completion; one wave adds the W[card] up
            const uint32_t ncomp = binom2(P, k);
            eqr_hero_pass(T, pool, hero_w, known | hero, k, ncomp, tid);
            if (wave == HH_WAVES - 1) {           // every holding is in two cards' sums: total = half their sum, at most 65 535 * 1 326
                const uint32_t c = tid & 63u;
                const uint32_t s = wave_sum(c < (uint32_t)HH_CARDS ? wcard[c] : 0u);
                if (c == 0u) wcard[HH_CARDS] = s >> 1;
            }
            __syncthreads();
            // ---- villain pass: a split adds its HOLDING's weight to the counters of its COMPLETION
            eqr_villain_pass(T, pool, canon, hero_w, known, k, P, tid, [&](uint32_t comp, uint32_t h, uint32_t win) {
                const uint32_t w = wt[h];
                if (win == 1u) atomicAdd(&below[comp], w);
                else if (win == 3u) atomicAdd(&equal[comp], w);
            });
            __syncthreads();
            // ---- bin pass: one lane per completion; den = the weight of the valid holdings that share no card with it
            const uint32_t total = wcard[HH_CARDS];
            for (uint32_t c = tid; c < ncomp; c += HH_BLOCK) {
                uint32_t den = total;
                if (k == 2u) {
                    uint32_t ci, cj;
                    unpair(c, ci, cj);
                    const uint32_t a = canon[PK_IDX(ci, 64, "canon") & 63u], b = canon[PK_IDX(cj, 64, "canon") & 63u];   // (a < b: the pool is in canonical order)
                    den = den - wcard[PK_IDX(a, HH_CARDS, "wcard")] - wcard[PK_IDX(b, HH_CARDS, "wcard")] + wt[PK_IDX(tri(b) + a, EQR_HOLDINGS, "wt")];
                } else if (k == 1u) den -= wcard[PK_IDX(canon[PK_IDX(c, 64, "canon") & 63u], HH_CARDS, "wcard")];
                const uint32_t lo = below[PK_IDX(c, EQR_COMPLETIONS, "below")], eq = equal[PK_IDX(c, EQR_COMPLETIONS, "equal")];
                below[c] = 0; equal[c] = 0;
                // nbins (2 below + equal) <= 32 * 2 * 65 535 * 990 < 2^32; 2 below + equal <= 2 den, so the quotient is at most nbins
                uint32_t bin = nbins;                                                    // (den = 0: void)
                if (den) { bin = nbins * (2u * lo + eq) / (2u * den); bin = bin < nbins - 1u ? bin : nbins - 1u; }
                atomicAdd(&cnt[PK_IDX(bin, HH_MAX_BINS + 1, "cnt")], 1u);
            }
            __syncthreads();
        }
        // ---- output: every bin and the void count (zeros included), and the counters cleared for the next spot
        if (tid < 64u) {
            const uint32_t v = cnt[tid];
            cnt[tid] = 0; wcard[tid] = 0;
            if (tid < nbins) { if (out.hist) out.hist[(size_t)spot * nbins + tid] = (uint16_t)v; }
            else if (tid == nbins && out.void_) out.void_[spot] = (uint16_t)v;
        }
    }
}

namespace pk {

static size_t hh_al(size_t b) { return (b + 255) & ~(size_t)255; }

size_t hh_work_bytes(size_t m, int nbins, const HeroHistOut &out, const HeroHistBucket &bk) {
    size_t t = hh_al(eqr_work_bytes(m));
    if (bk.K > 0 && (bk.label || bk.dist)) {
        if (!out.hist) t += hh_al(m * (size_t)nbins * 2);
        if (!bk.label) t += hh_al(m * 2);
        t += cl_work_bytes(m, nbins, bk.K, false, false);
    }
    return t;
}

hipError_t hh_launch(hipStream_t stream, const uint32_t *tab, const EqrSpots *spots, const EqTables *tables, int N, int observer,
                     const EqrWeights &weights, size_t m, int nbins, const HeroHistOut &out, const HeroHistBucket &bk, char *work) {
    if (m == 0) return hipSuccess;
    uint64_t *desc = (uint64_t *)work;
    work += hh_al(eqr_work_bytes(m));
    hipError_t e = eqr_prep_launch(stream, spots, tables, N, observer, m, EqrOut{nullptr, nullptr, nullptr, nullptr, out.status}, desc);
    if (e != hipSuccess) return e;
    if (out.completions) {
        hipLaunchKernelGGL(k_hero_hist_counts, dim3((unsigned)((m + HH_COUNTS_BLOCK - 1) / HH_COUNTS_BLOCK)), dim3(HH_COUNTS_BLOCK), 0, stream,
                           (const uint64_t *)desc, out.completions, m);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const bool bucket = bk.K > 0 && (bk.label || bk.dist);
    if (!(out.hist || out.void_ || bucket)) return hipSuccess;                 // (completions / status alone: the one-lane-per-spot kernels have written them)
    HeroHistOut o = out;
    if (bucket && !o.hist) { o.hist = (uint16_t *)work; work += hh_al(m * (size_t)nbins * 2); }   // the rows live in the work space
    const unsigned grid = (unsigned)(m < (size_t)HH_GRID_MAX ? m : (size_t)HH_GRID_MAX);
    hipLaunchKernelGGL(k_hero_hist, dim3(grid), dim3(HH_BLOCK), 0, stream, tab, (const uint64_t *)desc, weights, o, (uint32_t)nbins, (uint32_t)m);
    if ((e = hipGetLastError()) != hipSuccess || !bucket) return e;
    uint16_t *label = bk.label;
    if (!label) { label = (uint16_t *)work; work += hh_al(m * 2); }            // (k_cl_assign always writes labels)
    return cl_assign_launch(stream, m, nbins, o.hist, bk.K, bk.centroids, label, bk.dist, cl_work(work, m, nbins, bk.K, false, false));
}

}  // namespace pk
