// Dev-only: the seat and serial arithmetic of a betting pass -- ActionRing::half_of and Table<N>'s rotr / window_of / wrap / unwrap / first_playing /
// scan of pk_device.hpp -- on the CPU (hip_shim.h: one lane), exhaustively against the plain forms they replaced, for tests/test_seat_arith_host.py.
//   g++ -std=c++20 -O1 -DPK_HOST_SIM -include tools/host_sim/hip_shim.h tools/host_sim/seat_arith_sim.cpp -o seat_arith_sim
//   seat_arith_sim -> "half_of: <cases> cases", one line "N=<n>: <cases> cases" per seat count 2 .. 16, "seat_arith_sim: ok"; exit status 1 and the
//   first mismatch on stderr otherwise
#include <cstdio>
#include <cstdlib>
#define HIP_INCLUDE_HIP_HIP_RUNTIME_H
#include "../../pokerl_amd/csrc/pk_device.hpp"
using namespace pk;

[[noreturn]] static void fail(const char *what, int n, unsigned long long a, unsigned long long b, unsigned long long c, long long got, long long want) {
    fprintf(stderr, "seat_arith_sim: %s N=%d (%#llx, %llu, %llu): got %lld, want %lld\n", what, n, a, b, c, got, want);
    exit(1);
}

// the plain forms
static uint32_t plain_half(uint32_t word, uint32_t serial) { return (serial & 1) ? (word >> 16) : (word & 0xffffu); }
template <int N> static uint32_t plain_rotr(uint32_t m, int a) { return ((m >> a) | (m << (N - a))) & ((1u << N) - 1u); }
template <int N> static int plain_first_playing(uint32_t broken, int idx) {
    int i = idx >= N ? idx - N : idx;
    uint32_t nb = ~broken & ((1u << N) - 1u);
    int r = i + (__ffs(plain_rotr<N>(nb, i)) - 1);
    r = r >= N ? r - N : r;
    return nb ? r : i;
}
template <int N> static bool plain_scan(uint32_t st_active, int &active, int current) {
    int d = current - active; d = d < 0 ? d + N : d;
    uint32_t window = plain_rotr<N>(st_active, active) & ((2u << d) - 1);
    int a = active + (__ffs(window) - 1); a = a >= N ? a - N : a;
    active = window ? a : current;
    return window != 0;
}

static unsigned long long half_cases() {
    // every 16-bit pattern in either half (the other half its complement, so that a draw taken from the wrong half never matches), both parities,
    // and serials whose upper bits must drop out of `serial << 4`
    const uint32_t upper[] = {0u, 2u, 0x10u, 0x0ffffff0u, 0x10000000u, 0x7ffffffeu, 0x80000000u, 0xfffffffeu};
    unsigned long long cases = 0;
    for (uint32_t v = 0; v < 0x10000u; ++v)
        for (uint32_t bit = 0; bit < 2; ++bit) {
            const uint32_t words[] = {v | ((~v & 0xffffu) << 16), (v << 16) | (~v & 0xffffu)};
            for (uint32_t word : words)
                for (uint32_t up : upper) {
                    const uint32_t serial = up | bit;
                    const uint32_t got = ActionRing::half_of(word, serial), want = plain_half(word, serial);
                    if (got != want) fail("half_of", 0, word, serial, 0, got, want);
                }
            ++cases;
        }
    return cases;
}

template <int N>
static unsigned long long seat_cases() {
    using Tb = Table<N>;
    unsigned long long cases = 0;
    for (int x = 0; x < 2 * N; ++x) if (Tb::wrap(x) != x % N) fail("wrap", N, 0, (unsigned long long)x, 0, Tb::wrap(x), x % N);
    for (int d = -(N - 1); d < N; ++d) if (Tb::unwrap(d) != (d + N) % N) fail("unwrap", N, 0, 0, (unsigned long long)(d + N), Tb::unwrap(d), (d + N) % N);
    Tb tb{};
    for (uint32_t m = 0; m <= Tb::FULL; ++m) {
        for (int a = 0; a < N; ++a) {
            const uint32_t r = Tb::rotr(m, a), rw = plain_rotr<N>(m, a);
            if (r != rw) fail("rotr", N, m, (unsigned long long)a, 0, r, rw);
            for (int c = 0; c < N; ++c) {
                tb.st_active = m; tb.active = a; tb.current = c;
                int want_active = a;
                const bool want = plain_scan<N>(m, want_active, c);
                const bool got = tb.scan();
                if (got != want) fail("scan (found)", N, m, (unsigned long long)a, (unsigned long long)c, got, want);
                if (tb.active != want_active) fail("scan (active)", N, m, (unsigned long long)a, (unsigned long long)c, tb.active, want_active);
                tb.st_active = m; tb.active = a; tb.current = c; tb.lstate = LS_SCAN;      // the branch-free half of k_rollout's pass
                tb.scan_first();
                if ((tb.lstate == LS_DONE) != want || tb.active != (want ? want_active : a))
                    fail("scan_first", N, m, (unsigned long long)a, (unsigned long long)c, tb.active, want ? want_active : a);
                ++cases;
            }
        }
        tb.st_broken = m;
        for (int idx = 0; idx <= N; ++idx) {
            const int got = tb.first_playing(idx), want = plain_first_playing<N>(m, idx);
            if (got != want) fail("first_playing", N, m, (unsigned long long)idx, 0, got, want);
        }
    }
    return cases;
}

int main() {
    printf("half_of: %llu cases\n", half_cases());
    pk::unroll<15>([&](auto n) { constexpr int N = decltype(n)::value + 2; printf("N=%d: %llu cases\n", N, seat_cases<N>()); });
    printf("seat_arith_sim: ok\n");
    return 0;
}
