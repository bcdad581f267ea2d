// pk_equity_common.hpp -- the small device helpers every kernel of the equity family (pk_equity*.hip) uses: wave-uniform values, sums over a
// wavefront, bit selection, the binomials of the unranking, pair indices and the two-seat order key.  Registers only, every one inlined.
#pragma once
#include <cstdint>

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

}  // namespace pk
