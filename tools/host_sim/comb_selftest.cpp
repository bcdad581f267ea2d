// Dev-only: the combination walker of the equity kernels (pk::Comb, pokerl_amd/csrc/pk_equity_common.hpp) against a plain enumeration, on the
// CPU.  Built and run by tests/test_comb_walker_host.py, plain and under ASan + UBSan.
//   g++ -std=c++20 -O1 -DPK_HOST_SIM -I tools/host_sim/stub -include tools/host_sim/wg_shim.h tools/host_sim/comb_selftest.cpp
// Comb<L, MIN> walks the n = L - f subsets of pool slots 0 .. P - 1 (f levels frozen on the empty slot 63).  The forms the kernels use:
// <5, 0> with f = 0 .. 5 (k_equity, k_ev) and <4, 2> with f = 0 .. 2 (k_eqr, k_hero_hist).  Per form, f and pool size P:
//   * start(rank) is the rank-th subset in lexicographic order, for every rank; the frozen levels hold 63; a lane without work gets 63s;
//   * next() from rank 0 visits all C(P, n) subsets in order, and calls back exactly when a level above the last one changed;
//   * past the last subset the state is c[L - 2] = 62, c[L - 1] = 63: every index still one of the pool's 64 slots.
// P runs over n .. n + 4 (the walk's ends and carries at every depth) and 47 (a full-pool flop: up to C(47, 5) = 1 533 939 boards).
#include "../../pokerl_amd/csrc/pk_equity_common.hpp"

using namespace pk;

static int g_fail;
static unsigned long long g_cases, g_subsets;

#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { fprintf(stderr, "comb_selftest: " __VA_ARGS__); fputc('\n', stderr); } } } while (0)

// the reference: n ascending indices below P, stepped the textbook way; false after the last
static bool ref_next(uint32_t *a, int n, uint32_t P) {
    int i = n - 1;
    while (i >= 0 && a[i] == P - (uint32_t)(n - i)) --i;
    if (i < 0) return false;
    ++a[i];
    for (int u = i + 1; u < n; ++u) a[u] = a[u - 1] + 1;
    return true;
}

template <int L, int MIN>
static bool same(const Comb<L, MIN> &w, int f, const uint32_t *a) {
    for (int t = 0; t < L; ++t)
        if (w.c[t] != (t < f ? COMB_FROZEN : a[t - f])) return false;
    return true;
}

template <int L, int MIN>
static void check(int f, uint32_t P) {
    const int n = L - f;
    ++g_cases;
    Comb<L, MIN> idle;
    idle.start(P, f, 0, false);
    for (int t = 0; t < L; ++t) CHECK(idle.c[t] == COMB_FROZEN, "<%d,%d> f %d P %u: a lane without work holds %u at level %d", L, MIN, f, P, idle.c[t], t);
    uint32_t a[L > 0 ? L : 1], prev[L > 0 ? L : 1];
    for (int i = 0; i < n; ++i) a[i] = (uint32_t)i;
    Comb<L, MIN> w;
    w.start(P, f, 0, true);
    uint32_t rank = 0;
    for (;;) {
        ++g_subsets;
        CHECK(same(w, f, a), "<%d,%d> f %d P %u: the walk at rank %u is %u %u %u %u ...", L, MIN, f, P, rank, w.c[0], w.c[1], w.c[2], w.c[3]);
        for (int i = 0; i < n; ++i) prev[i] = a[i];
        const bool more_to_come = ref_next(a, n, P);   // (a: the subset after this one, prev: this one)
        Comb<L, MIN> s;
        s.start(P, f, rank, true);
        CHECK(same(s, f, prev), "<%d,%d> f %d P %u: start(%u) is %u %u %u %u ...", L, MIN, f, P, rank, s.c[0], s.c[1], s.c[2], s.c[3]);
        bool moved = false;
        w.next(P, [&] { moved = true; });
        if (!more_to_come) {
            // past the end: a carry out of every level, the state the kernels index the pool's 64 slots with
            CHECK(moved, "<%d,%d> f %d P %u: next() past the last subset reports no carry", L, MIN, f, P);
            for (int t = 0; t < L; ++t) CHECK(w.c[t] <= 63u, "<%d,%d> f %d P %u: index %u at level %d past the end", L, MIN, f, P, w.c[t], t);
            CHECK(w.c[L - 2] == COMB_FROZEN - 1 && w.c[L - 1] == COMB_FROZEN, "<%d,%d> f %d P %u: past the end levels %d, %d hold %u, %u", L, MIN, f, P, L - 2, L - 1, w.c[L - 2], w.c[L - 1]);
            break;
        }
        bool above = false;                   // did a level above the last one change?
        for (int i = 0; i + 1 < n; ++i) above = above || a[i] != prev[i];
        CHECK(moved == above, "<%d,%d> f %d P %u: next() after rank %u calls back: %d, levels above the last %s", L, MIN, f, P, rank, (int)moved, above ? "changed" : "did not change");
        ++rank;
    }
    unsigned long long want = 1;
    for (int i = 0; i < n; ++i) want = want * (P - (uint32_t)i) / (uint32_t)(i + 1);
    CHECK(rank + 1ull == want, "<%d,%d> f %d P %u: %llu subsets visited, C(P, %d) = %llu", L, MIN, f, P, rank + 1ull, n, want);
}

template <int L, int MIN>
static void form() {
    for (int f = 0; f <= L - MIN; ++f) {
        const int n = L - f;
        for (uint32_t P = (uint32_t)n; P <= (uint32_t)n + 4u; ++P) check<L, MIN>(f, P);
        check<L, MIN>(f, 47);
    }
}

int main() {
    form<5, 0>();
    form<4, 2>();
    printf("comb_selftest: %llu cases, %llu subsets, %d failed checks\n", g_cases, g_subsets, g_fail);
    return g_fail ? 1 : 0;
}
