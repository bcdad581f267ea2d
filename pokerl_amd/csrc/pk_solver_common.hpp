// pk_solver_common.hpp -- what the solver kernels (pk_river_solver.hip, pk_turn_solver.hip) share on the device: the corrected 64-bit
// division and the strategy rule (include/pokerl_hip.h "River solver": STRATEGY FROM NON-NEGATIVE INTEGERS).  Both inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pk_river_solver.hpp"

namespace {

// floor(num / den), num < 2^46, 0 < den < 2^33: the double quotient is within one of it
__device__ __forceinline__ uint32_t rs_div(uint64_t num, uint64_t den) {
    uint64_t q = (uint64_t)((double)num / (double)den);
    if (q * den > num) --q;
    else if ((q + 1u) * den <= num) ++q;
    return (uint32_t)q;
}

// The strategy rule: X[0 .. nact) non-negative -> sig[0 .. nact) summing to RS_ONE (the slots from nact on: 0)
__device__ __forceinline__ void rs_sigma(const int64_t (&X)[4], uint32_t nact, uint32_t (&sig)[4]) {
    uint64_t mx = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) mx = ((uint32_t)a < nact && (uint64_t)X[a] > mx) ? (uint64_t)X[a] : mx;
    const uint32_t hi = (uint32_t)(mx >> 32), bl = hi ? 64u - (uint32_t)__clz((int)hi) : 32u - (uint32_t)__clz((int)(uint32_t)mx), sh = bl > 31u ? bl - 31u : 0u;
    uint64_t S = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) S += (uint32_t)a < nact ? (uint64_t)X[a] >> sh : 0ull;
    const uint32_t even = pk::RS_ONE / nact;
    uint32_t rest = pk::RS_ONE;
    sig[0] = 0;
#pragma unroll
    for (int a = 1; a < 4; ++a) {
        sig[a] = 0;
        if ((uint32_t)a < nact) sig[a] = mx ? rs_div(((uint64_t)X[a] >> sh) << 15, S) : even;
        rest -= sig[a];
    }
    sig[0] = rest;
}

}  // namespace
