// pk_equity_common.hpp -- the small device helpers every kernel of the equity family (pk_equity*.hip) uses: wave-uniform values, sums over a
// wavefront, bit selection, the binomials of the unranking, pair indices, the two-seat order key, the evaluator table and share weights
// into LDS, a pool card's bit, the pool fill of the one-spot-per-workgroup kernels, and the combination walker (Comb) of the four kernels
// that enumerate boards or card sets.  Every one inlined.
#pragma once
#include <cstdint>

#include "pk_device.hpp"

// a development library holds one seat count (build.py: -DPK_ONLY_SEATS): the per-seat-count kernels of every other one are not instantiated
#ifdef PK_ONLY_SEATS
#define EQ_SEAT_ENABLED(N) ((N) == (PK_ONLY_SEATS))
#else
#define EQ_SEAT_ENABLED(N) 1
#endif

namespace pk {

// a value every lane of the wavefront holds, moved to scalar registers
__device__ __forceinline__ uint32_t uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uniform(uint64_t x) { return (uint64_t)uniform((uint32_t)x) | ((uint64_t)uniform((uint32_t)(x >> 32)) << 32); }
// every lane gets the wavefront's sum (every lane of the wave takes part)
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
// Index of the c-th (0-based) set bit of m, c < popcount(m): popcount bisection, 32 -> 1 bits.  Registers only.
__device__ __forceinline__ uint32_t select(uint64_t m, uint32_t c) {
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    uint32_t p = (uint32_t)__popc(lo);
    bool up = c >= p;
    uint32_t w = up ? hi : lo, base = up ? 32u : 0u;
    c -= up ? p : 0u;
#pragma unroll
    for (uint32_t sh = 16; sh >= 1; sh >>= 1) {
        p = (uint32_t)__popc(w & ((1u << sh) - 1u));
        up = c >= p;
        c -= up ? p : 0u;
        w = up ? w >> sh : w;
        base += up ? sh : 0u;
    }
    return base;
}
// C(n, J) for the unranking, J a compile-time 1 .. 4 (n <= 51); 0 where n < J
template <int J>
__device__ __forceinline__ uint32_t binom_c(uint32_t n) {
    if constexpr (J == 1) return n;
    else if constexpr (J == 2) return n * (n - 1u) / 2u;                     // (n = 0: 0 * 0xffffffff = 0)
    else if constexpr (J == 3) return n < 3u ? 0u : n * (n - 1u) * (n - 2u) / 6u;
    else return n < 4u ? 0u : n * (n - 1u) * (n - 2u) * (n - 3u) / 24u;
}
// C(n, k), 0 <= k <= 2
__device__ __forceinline__ uint32_t binom2(uint32_t n, uint32_t k) { return k == 0 ? 1u : (k == 1 ? n : n * (n - 1u) / 2u); }
__device__ __forceinline__ uint32_t tri(uint32_t n) { return n * (n - 1u) / 2u; }   // (n = 0: 0 * 0xffffffff = 0)
// t = b (b - 1) / 2 + a with a < b (a holding index, a completion's pair index) -> (a, b); t < 2^20
__device__ __forceinline__ void unpair(uint32_t t, uint32_t &a, uint32_t &b) {
    b = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
    b = b < 1u ? 1u : b;
    while (tri(b) > t) --b;
    while (tri(b + 1u) <= t) ++b;
    a = t - tri(b);
}
// the index of the pair {a, x}, a != x
__device__ __forceinline__ uint32_t pair(uint32_t a, uint32_t tri_a, uint32_t x, uint32_t tri_x) { return x < a ? tri_a + x : tri_x + a; }
// The two-seat order: compare_rankings<2> on ranking words rank << 20 | kickers lets the lower rank number win, then the
// larger kickers value, and ties equal words.  So the hero beats exactly the words whose key is SMALLER, and ties exactly the equal key.
__device__ __forceinline__ uint32_t order_key(uint32_t word) { return ((15u - (word >> 20)) << 20) | (word & 0xFFFFFu); }

// the 32 KB rank-mask table of eval7_tab into the workgroup's LDS copy T, by a workgroup of BLOCK threads (a barrier follows at the caller's)
template <int BLOCK>
__device__ __forceinline__ void stage_eval7_tab(uint32_t *T, const uint32_t *__restrict__ tab) {
    for (int i = threadIdx.x; i < EVAL7_TAB_WORDS / 4; i += BLOCK) reinterpret_cast<uint4 *>(T)[PK_IDX(i, EVAL7_TAB_WORDS / 4, "T")] = reinterpret_cast<const uint4 *>(tab)[i];
}
// wt[nw]: a board's pot share of one of nw = 1 .. 16 winners, PK_EQ_SHARE_UNIT / nw exactly; 0 elsewhere (32 entries)
__device__ __forceinline__ void fill_share_weights(uint32_t *wt) {
    if (threadIdx.x < 32) wt[PK_IDX(threadIdx.x, 32, "wt")] = (threadIdx.x >= 1 && threadIdx.x <= 16) ? (uint32_t)PK_EQ_SHARE_UNIT / threadIdx.x : 0u;
}
// the card of canonical index c (rank0 * 4 + suit) as its bit in the suit-lane layout, 4 << Card.value
__device__ __forceinline__ uint64_t card_bit(uint32_t c) { return 4ull << (((c & 3u) << 4) | (c >> 2)); }

constexpr uint32_t COMB_FROZEN = 63;   // pool slot that holds no card: the index of a combination level that does not exist

// The pool of a one-spot-per-workgroup kernel: card j (canonical order) of the cards not dead as its bit in pool[j] and its canonical index
// in canon[j]; the empty slot holds none.  Lanes 0 .. 63 of the workgroup; a barrier follows at the caller's.
__device__ __forceinline__ void fill_pool(uint64_t *pool, uint32_t *canon, uint64_t avail, uint32_t tid) {
    if (tid < 52u && ((avail >> tid) & 1ull)) {
        const uint32_t slot = (uint32_t)__popcll(avail & ((1ull << tid) - 1ull));
        pool[PK_IDX(slot, 64, "pool")] = card_bit(tid);
        canon[PK_IDX(slot, 64, "canon")] = tid;
    }
    if (tid == COMB_FROZEN) { pool[COMB_FROZEN] = 0; canon[COMB_FROZEN] = 0; }
}

// The combination walker: the (L - f)-subsets of pool slots 0 .. P - 1 in lexicographic order, as ascending indices c[0] < ... < c[L - 1].
// The first f levels do not exist and stay frozen on the empty slot; the last MIN levels exist in every call (f <= L - MIN), so that their
// code carries no test of f.  start() unranks once, next() steps: the last level moves on; when it runs out, the deepest level that can
// still rise does, the ones after it follow, and the caller is told (a callable: what it derived from the levels above the last is stale).
// Past the last combination the state is c[L - 2] = COMB_FROZEN - 1, c[L - 1] = COMB_FROZEN: still indices of the pool's 64 slots, never
// evaluated.  Comb<4, 2>: the card sets of k_eqr / k_hero_hist (pk_equity_range.hpp).  Comb<5, 0> is the board walk k_equity<N> and k_ev<N>
// spell out themselves (sharing it cost them legs of their A/B against the parent: profiles/equity_shared_ab.json); tested all the same.
template <int L, int MIN>
struct Comb {
    static_assert(L >= 2 && MIN >= 0 && MIN <= L, "levels");
    uint32_t c[L];
    int lim[L - 1];      // lim[t]: the highest index level t may still be raised FROM (-1: never)

    static constexpr bool always(int t) { return t >= L - MIN; }
    // one level of the unranking: C(P - 1 - x, J) combinations start with x at a level that has J levels after it
    template <int J>
    static __device__ __forceinline__ uint32_t level(uint32_t P, uint32_t &r, uint32_t &x) {
        while (x < P) {
            const uint32_t n = binom_c<J>(P - 1u - x);
            if (r < n) break;
            r -= n; ++x;
        }
        return x++;
    }
    // the combination of index `rank`; any = false (a lane without work): every level stays frozen
    __device__ __forceinline__ void start(uint32_t P, int f, uint32_t rank, bool any) {
        unroll<L - 1>([&](auto tc) { constexpr int t = decltype(tc)::value; lim[t] = (always(t) || f <= t) ? (int)P - (L - t) : -1; });
        unroll<L>([&](auto tc) { c[decltype(tc)::value] = COMB_FROZEN; });
        if (any) {
            uint32_t r = rank, x = 0;
            unroll<L - 1>([&](auto tc) { constexpr int t = decltype(tc)::value; if (always(t) || f <= t) c[t] = level<L - 1 - t>(P, r, x); });
            if (always(L - 1) || f <= L - 1) c[L - 1] = x + r;
        }
    }
    template <int T>
    __device__ __forceinline__ void carry() {
        if ((int)c[T] < lim[T]) {
            ++c[T];
            unroll<L - 2 - T>([&](auto uc) { constexpr int u = T + 1 + decltype(uc)::value; c[u] = c[u - 1] + 1; });
        } else if constexpr (T > 0) carry<T - 1>();
        else { c[L - 2] = COMB_FROZEN - 1; }
    }
    // the next combination; moved(): a level above the last one moved (what the caller derives from c[0 .. L - 2] is stale)
    template <typename F>
    __device__ __forceinline__ void next(uint32_t P, F &&moved) {
        ++c[L - 1];
        if (c[L - 1] >= P) {
            carry<L - 2>();
            c[L - 1] = c[L - 2] + 1;
            moved();
        }
    }
};

}  // namespace pk
