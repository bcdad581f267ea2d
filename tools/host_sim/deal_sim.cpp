// Dev-only: the REAL Table<N>::deal_cards of pk_device.hpp -- Philox block(s), chained bounded draws, packed Lehmer decode, index -> Card.value --
// for every seat count 2 .. 16 on the CPU (hip_shim.h: one lane), for tests/test_deal_decode_host.py to hold against oracle/rng_spec.py.
//   g++ -std=c++20 -O1 -DPK_HOST_SIM -include tools/host_sim/hip_shim.h tools/host_sim/deal_sim.cpp -o deal_sim
//   deal_sim < triples      one line "seed table_id hand_serial" (decimal or 0x...) per triple
//   -> per triple and seat count one line "N <2 * (5 + 2 N) hex digits>": Card.value of the deck's first 5 + 2 N cards, in deck order
#include <cstdio>
#include <cstdlib>
#define HIP_INCLUDE_HIP_HIP_RUNTIME_H
#include "../../pokerl_amd/csrc/pk_device.hpp"
using namespace pk;

template <int N>
static void one(uint64_t seed, uint32_t table_id, uint64_t hand_serial) {
    constexpr int K = 5 + 2 * N, W = (K + 3) / 4;
    Hot H{};
    H.key0 = (uint32_t)seed; H.key1 = (uint32_t)(seed >> 32);
    uint32_t cards[W];
    Table<N>::deal_cards(H, table_id, hand_serial, cards);
    printf("%d ", N);
    for (int i = 0; i < K; ++i) printf("%02x", (cards[i >> 2] >> (8 * (i & 3))) & 0xffu);
    printf("\n");
}

int main() {
    char a[64], b[64], c[64];
    while (scanf("%63s %63s %63s", a, b, c) == 3) {
        const uint64_t seed = strtoull(a, nullptr, 0), hs = strtoull(c, nullptr, 0);
        const uint32_t tid = (uint32_t)strtoull(b, nullptr, 0);
        pk::unroll<15>([&](auto n) { one<decltype(n)::value + 2>(seed, tid, hs); });
    }
    return 0;
}
