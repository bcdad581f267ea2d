// Dev-only: wg_shim.h checked against itself -- what the equity drivers rely on, on kernels small enough to read.  Built and run by
// tests/test_equity_sim_host.py (plain) and by sanitize_equity.sh (both sanitizer builds).
//   g++ -std=c++20 -O1 -DPK_HOST_SIM -I tools/host_sim/stub -include tools/host_sim/wg_shim.h tools/host_sim/wg_shim_selftest.cpp
//   wg_shim_selftest ok | split-barrier | split-wave | left-lane | index | race | race-ahead
// ok: exits 0.  split-barrier, split-wave, left-lane: the shim reports and exits 3.  index: PK_IDX aborts.  race: a hand-off between two waves
// without __syncthreads; race-ahead: a lane that runs on to the NEXT barrier reads what a lane resumed after it then writes (the lanes are
// fibres, run one after the other: the late lane must not inherit the early one's clock) -- both exit 0 on a plain build and are a reported
// data race under TSan.
#include "../../pokerl_amd/csrc/pk_device.hpp"

using namespace pk;

static unsigned long long g_sum;     // "global memory"
static uint32_t g_seen_garbage;

__global__ void k_selftest(int mode) {
    __shared__ uint32_t box[8];
    __shared__ uint64_t wide[64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0 && box[3] == 0x2D2D2D2Du) atomicAdd(&g_seen_garbage, 1u);          // LDS starts from garbage, in every workgroup
    __syncthreads();
    if (mode == 0) {
        // shuffles, 32 and 64 bits; a lane below `off` keeps its own value
        uint32_t inc = lane + 1u;
        for (int off = 1; off < 64; off <<= 1) { const uint32_t y = __shfl_up(inc, off); inc += lane >= (uint32_t)off ? y : 0u; }
        if (inc != (lane + 1u) * (lane + 2u) / 2u) abort();
        uint64_t x = (uint64_t)tid << 33;
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
        if (x != ((uint64_t)(wave * 64u * 64u + 2016u) << 33)) abort();
        if (__shfl(tid, 63) != wave * 64u + 63u) abort();
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)tid) != wave * 64u) abort();
        // a hand-off between waves through LDS, with its barrier; an LDS atomic; a global atomic
        if (lane == 0) box[PK_IDX(wave, 8, "box")] = wave + 100u;
        if (wave == 0) wide[PK_IDX(lane, 64, "wide")] = 0;
        __syncthreads();
        uint32_t all = 0;
        for (uint32_t w = 0; w < blockDim.x / 64u; ++w) all += box[w];
        if (all != (blockDim.x / 64u) * 100u + (blockDim.x / 64u) * (blockDim.x / 64u - 1u) / 2u) abort();
        atomicAdd(reinterpret_cast<unsigned long long *>(&wide[lane]), 1ull);
        __syncthreads();
        if (wide[lane] != blockDim.x / 64u) abort();
        if (tid >= 100u) return;                                                      // lanes that have left drop out of every later rendezvous
        __syncthreads();
        atomicAdd(&g_sum, (unsigned long long)(blockIdx.x * 1000u + tid));
    } else if (mode == 1) {
        if (tid & 1u) __syncthreads();                                                // two sites
        else __syncthreads();
    } else if (mode == 2) {
        if (lane < 7u) (void)__shfl_xor(tid, 1); else __syncthreads();
    } else if (mode == 3) {
        if (lane == 5u) return;
        (void)__shfl(tid, 5);
    } else if (mode == 4) {
        if (lane == 0) box[PK_IDX(wave + 1u, 8, "box")] = 1;                                         // wave 7: index 8
    } else if (mode == 5) {
        if (tid == 0) box[0] = 7;                                                     // wave 0 writes ...
        (void)__shfl_xor(tid, 1);                                                     // (a wave collective orders nothing between waves)
        if (tid == 64u && box[0] == 12345u) abort();                                  // ... wave 1 reads: no barrier in between
    } else if (mode == 6) {
        if (tid == 0 && box[1] == 12345u) abort();                                    // lane 0 runs first: it reads, and arrives at the barrier below
        if (tid == 64u) box[1] = 5;                                                   // lane 64 is resumed after that and writes
        __syncthreads();
    }
}

int main(int argc, char **argv) {
    const std::string m = argc > 1 ? argv[1] : "";
    static const char *names[] = {"ok", "split-barrier", "split-wave", "left-lane", "index", "race", "race-ahead"};
    int mode = -1;
    for (int i = 0; i < 7; ++i) if (m == names[i]) mode = i;
    if (mode < 0) { fprintf(stderr, "usage: wg_shim_selftest ok | split-barrier | split-wave | left-lane | index | race | race-ahead\n"); return 2; }
    if (pk_sim::lds_find({"10k_selftesti"}) != 8 * 4 + 64 * 8) { fprintf(stderr, "wg_shim_selftest: lds_find did not find box[] and wide[]\n"); return 1; }
    pk_sim::launch(3, 512, [=] { k_selftest(mode); });
    if (mode == 0) {
        pk_sim::launch(2, 256, [=] { k_selftest(0); });
        unsigned long long want = 0;
        for (unsigned b = 0; b < 3; ++b) for (unsigned t = 0; t < 100; ++t) want += b * 1000u + t;
        for (unsigned b = 0; b < 2; ++b) for (unsigned t = 0; t < 100; ++t) want += b * 1000u + t;
        if (g_sum != want || g_seen_garbage != 5) { fprintf(stderr, "wg_shim_selftest: sum %llu (want %llu), garbage seen by %u of 5 workgroups\n", g_sum, want, g_seen_garbage); return 1; }
    }
    printf("wg_shim_selftest %s: done\n", names[mode]);
    return 0;
}
