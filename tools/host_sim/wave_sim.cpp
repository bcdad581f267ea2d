// Dev-only: the REAL rollout_body<...> of pk_table_kernels.hpp -- the body of k_rollout, k_rollout_allin, k_rollout_call, k_rollout_tab,
// k_rollout_allin_tab, k_rollout_single, k_step and k_step_async, with the template arguments pk_table_kernels.hpp gives them -- run 64 lanes
// wide on the CPU (wave_shim.h: one thread per lane, one wave at a time) on a State this program owns, and compared with the oracle after
// every launch that runs to completion: every state field, the rankings of the last showdown, the valid-action masks, the error bits, the
// serials, State::owed, the step-in-flight bits and the four counters.  (A deferring launch, slack < 64, leaves steps in flight by design: the comparison
// follows the flush that completes them.)  Built plain by tests/test_wave_sim_host.py and under ASan + UBSan and TSan by sanitize_wave.sh.
//   g++ -std=c++20 -O1 -pthread -ffp-contract=off -DPK_HOST_SIM -include tools/host_sim/wave_shim.h -DPK_WS_PART=100 -DPK_WS_MAIN \
//       tools/host_sim/wave_sim.cpp oracle/pokerl_oracle.c
//   wave_sim [family [N]] [--quick] [--steps K] [--deep]      families: rollout allin call tab allin_tab single step step_async
//   --deep (step, step_async): the actions of the oracle's never-fold caller (oracle/rng_spec.py POLICY_DEEP, policy 14 of orc_pick_actions) on
//   per-seat fractional stacks -- raises on every street, all-ins on different streets, multi-way river showdowns with side pots; 60 steps
//   --ring-stats (the random-agent rollout families): three complete launches of --steps (default 1 024) steps on 192 tables -- three waves of 64
//   live lanes -- with the headline's stacks and blinds (100, 2 / 1) and parking threshold (28); prints the Philox passes of ActionRing::ensure per
//   loop iteration and the lanes each pass filled.  The step machine is deterministic: the counts are the device's.
// One translation unit per family and seat group (-DPK_WS_PART=1..11; 100: the three instantiations of the suite's test), main with -DPK_WS_MAIN.
#define HIP_INCLUDE_HIP_HIP_RUNTIME_H
#include "../../pokerl_amd/csrc/pk_table_kernels.hpp"
extern "C" {
#include "../../oracle/pokerl_oracle.h"
}
#include <string>

enum Family : int { F_ROLLOUT, F_ALLIN, F_CALL, F_TAB, F_ALLIN_TAB, F_SINGLE, F_STEP, F_STEP_ASYNC };
static const char *const kFamilyName[] = {"rollout", "allin", "call", "tab", "allin_tab", "single", "step", "step_async"};
struct Opts { bool quick = false; int steps = 0; bool deep = false; bool ring = false; };
struct Case { int family, n; int (*fn)(const Opts &); };
std::vector<Case> &registry();
#ifdef PK_WS_MAIN
std::vector<Case> &registry() { static std::vector<Case> r; return r; }
#endif

// an allocation of exactly n elements, so that ASan bounds every State array
template <typename T>
struct Arr {
    T *p; size_t n;
    explicit Arr(size_t n_, T fill = T()) : p((T *)malloc((n_ ? n_ : 1) * sizeof(T))), n(n_) { for (size_t i = 0; i < n; ++i) p[i] = fill; }
    ~Arr() { free(p); }
    Arr(const Arr &) = delete;
    T &operator[](size_t i) { return p[i]; }
};

struct Cfg { double start[16]; double bb, sb; uint32_t base; uint64_t seed; const char *name; };
// per-seat stacks and fractional blinds out of host_sim's fuzz tables (short stacks below the blinds included), and equal stacks: with
// all-in agents every seat of every lane then reaches the first showdowns (queues of 64 * N hands: pair rounds only at ten seats)
static Cfg fuzz_cfg(int n) {
    static const double stacks[] = {0.5, 1, 2, 3, 5, 10, 37.5, 100, 1000, 1e6};
    Cfg c; for (int p = 0; p < 16; ++p) c.start[p] = stacks[(2 * p + 3 + n) % 10];
    c.bb = 7.5; c.sb = 0.25; c.base = 0x7fffff00u; c.seed = 0x706F6B65726Cull + (uint64_t)n; c.name = "per-seat stacks";
    return c;
}
// blinds above every stack: each hand posts the blinds all-in and ends before anybody can act, so one Game.step rolls through hand after hand --
// what a bounded launch (k_step_async, max_end = 1) must leave in flight
static Cfg rolling_cfg(int n) {
    static const double stacks[] = {3, 5, 10, 37.5, 2, 5, 3, 10};
    Cfg c; for (int p = 0; p < 16; ++p) c.start[p] = stacks[(p + n) % 8];
    c.bb = 40; c.sb = 7.5; c.base = 77; c.seed = 0x5EEDull + (uint64_t)n; c.name = "blinds above the stacks";
    return c;
}
// the deep configuration of tests/seat_matrix.py: stacks 7.5 (p + 1) + 0.25 (p % 3), blinds 2 / 1, table ids that wrap 2^32 inside the batch
static Cfg deep_cfg(int n) {
    Cfg c; for (int p = 0; p < 16; ++p) c.start[p] = 7.5 * (p + 1) + 0.25 * (p % 3);
    c.bb = 2; c.sb = 1; c.base = 0xffffff9cu; c.seed = 0xDEE9ull + (uint64_t)n; c.name = "deep caller, per-seat fractional stacks";
    return c;
}
static Cfg equal_cfg(int n) {
    Cfg c; for (int p = 0; p < 16; ++p) c.start[p] = 100.0;
    c.bb = 2; c.sb = 1; c.base = 0; c.seed = 4400 + (uint64_t)n; c.name = "equal stacks";
    return c;
}

template <int N, int FAM>
struct Sim {
    static constexpr int KK = 5 + 2 * N, W = (KK + 3) / 4;
    static constexpr int POLICY = (FAM == F_ALLIN || FAM == F_ALLIN_TAB) ? PK_POLICY_ALLIN : (FAM == F_CALL ? PK_POLICY_CALL : PK_POLICY_RANDOM);
    static constexpr bool TAB = FAM == F_TAB || FAM == F_ALLIN_TAB;
    using LDS = std::conditional_t<TAB, LdsTab<N, FAM == F_TAB>, Lds<N>>;
    const int T, grid;
    const Cfg cfg;
    Arr<double> cr, be, pe, pa, mr, startc;
    Arr<uint64_t> ss, hs, st;
    Arr<uint32_t> cur, cards, show, owed, mid, evtab;
    Arr<int32_t> hand, actions;
    Arr<uint8_t> valid, terr, flags, terr_out, ready, flags2, terr2, ready2;
    Arr<unsigned long long> counters;
    Arr<Fresh> fresh;
    Arr<State> Sdev;
    State &S;
    Hot H{};
    orc_game *o;
    uint64_t oc4[4] = {0, 0, 0, 0};
    int orc_err = 0;
    long inflight_seen = 0;

    Sim(int T_, const Cfg &c)
        : T(T_), grid((T_ + 63) / 64), cfg(c), cr(N * T_), be(N * T_), pe(N * T_), pa(N * T_), mr(T_), startc(N), ss(T_), hs(T_), st(T_), cur(T_), cards(W * T_),
          show(N * T_, NONE_V), owed(T_), mid(T_), evtab(EVAL7_TAB_WORDS), hand(T_), actions(T_), valid(T_), terr(T_), flags(T_), terr_out(T_), ready(T_),
          flags2(T_), terr2(T_), ready2(T_), counters((size_t)((T_ + 63) / 64) * PK_NUM_COUNTERS), fresh(1), Sdev(1), S(Sdev[0]) {
        memset(&S, 0, sizeof(S));
        S.credits = cr.p; S.bets = be.p; S.pending = pe.p; S.payoffs = pa.p; S.min_raise = mr.p; S.seat_states = ss.p; S.cursors = cur.p; S.hand = hand.p;
        S.hand_serial = hs.p; S.step_serial = st.p; S.cards = cards.p; S.show = show.p; S.owed = owed.p; S.mid = mid.p; S.valid = valid.p; S.terr = terr.p;
        S.counters = counters.p; S.evtab = TAB ? evtab.p : nullptr;
        for (int m = 0; m < EVAL7_TAB_WORDS; ++m) evtab[m] = eval7_tab_entry((uint32_t)m);
        for (int p = 0; p < N; ++p) { S.start_credits[p] = cfg.start[p]; startc[p] = cfg.start[p]; }
        S.big_blind = cfg.bb; S.small_blind = cfg.sb; S.key0 = (uint32_t)cfg.seed; S.key1 = (uint32_t)(cfg.seed >> 32); S.table_id_base = cfg.base; S.T = T;
        H.big_blind = cfg.bb; H.small_blind = cfg.sb; H.start_credits = startc.p; H.show = show.p; H.key0 = S.key0; H.key1 = S.key1; H.table_id_base = cfg.base;
        H.T = T; H.tpb = 64; H.start_uniform = cfg.start[0]; H.start_is_uniform = 1;
        for (int p = 1; p < N; ++p) if (cfg.start[p] != cfg.start[0]) H.start_is_uniform = 0;
        {   // k_make_fresh
            Table<N> f0; f0.blank(); f0.reset_state(H, 0);
            Fresh &fr = fresh[0]; memset(&fr, 0, sizeof(fr));
            for (int p = 0; p < N; ++p) { fr.credits[p] = f0.credits[p]; fr.pending[p] = f0.pending[p]; }
            fr.min_raise = f0.min_raise; fr.st_active = f0.st_active; fr.st_called = f0.st_called; fr.st_allin = f0.st_allin; fr.st_broken = f0.st_broken;
            fr.active = f0.active; fr.dealer = f0.dealer; fr.sb = f0.sb; fr.bb = f0.bb;
        }
        H.fresh = fresh.p;
        o = orc_create(T, N, cfg.start, cfg.bb, cfg.sb, cfg.seed, cfg.base);
        orc_reset(o, nullptr, 0);
        Arr<uint8_t> all(T, 1);
        reset(all.p);
    }
    ~Sim() { orc_destroy(o); }
    void reset(const uint8_t *mask) {   // k_reset (no cross-lane code in it)
        for (int t = 0; t < T; ++t)
            if (mask[t]) {
                Table<N> tb; tb.load(S, t); tb.reset_state(H, 0); tb.deal(H, cfg.base + (uint32_t)t); tb.store(S, t);
                double hb; valid[t] = (uint8_t)tb.valid_mask(hb); terr[t] = 0;
            }
    }
    void launch_rollout(int K, int park, int slack, int clear_terr) {
        const State *Sp = &S; const Hot &Hr = H;
        pk_sim::launch(grid, sizeof(LDS), [=, &Hr] {
            if constexpr (FAM == F_SINGLE) rollout_body<N, false, PK_POLICY_RANDOM, 1>(Sp, Hr, K, 1, park, slack, clear_terr);
            else rollout_body<N, true, POLICY, 0, false, TAB>(Sp, Hr, K, 1, park, slack, clear_terr);
        });
    }
    void launch_step(const int32_t *act, uint8_t *fl, uint8_t *te, uint8_t *rd, int park, int max_end) {
        const StepKernArgs ka{&S, H, act, fl, te, park, 0, rd, max_end, nullptr, nullptr};
        const StepKernArgs *kp = &ka;
        pk_sim::launch(grid, sizeof(LDS), [=] {
            if constexpr (FAM == F_STEP_ASYNC) rollout_body<N, false, PK_POLICY_EXTERNAL, 1, true>(kp->Sp, kp->H, 0, kp->auto_reset, kp->park, PK_WAVE, 1, kp->actions, kp);
            else rollout_body<N, false, PK_POLICY_EXTERNAL, 1>(kp->Sp, kp->H, 0, kp->auto_reset, kp->park, PK_WAVE, 1, kp->actions, kp);
        });
    }
    // every field against the oracle; 0 = equal
    int compare(const char *where, bool check_terr_word) {
        Arr<double> f(N * T); Arr<uint8_t> ost(N * T), ocards((size_t)T * KK), orank(N * T), ovalid(T); Arr<int32_t> ocur(6 * T); Arr<uint32_t> okick(N * T);
        Arr<uint64_t> ohs(T), ost2(T);
        int bad = 0;
        auto fail = [&](const char *what, int t, int p, double a, double b) {
            if (bad++ < 5) printf("MISMATCH %s N=%d %s: %s table %d seat %d: oracle %.17g sim %.17g\n", kFamilyName[FAM], N, where, what, t, p, a, b);
        };
        const double *mine[4] = {cr.p, be.p, pe.p, pa.p}; const char *nm[4] = {"credits", "bets", "pending", "payoffs"};
        for (int k = 0; k < 4; ++k) {
            orc_get_f64(o, k, f.p);
            for (int t = 0; t < T; ++t) for (int p = 0; p < N; ++p) if (memcmp(&f[t * N + p], &mine[k][(size_t)p * T + t], 8)) fail(nm[k], t, p, f[t * N + p], mine[k][(size_t)p * T + t]);
        }
        orc_get_min_raise(o, f.p);
        for (int t = 0; t < T; ++t) if (memcmp(&f[t], &mr[t], 8)) fail("min_raise", t, -1, f[t], mr[t]);
        orc_get_states(o, ost.p); orc_get_cursors(o, ocur.p); orc_get_serials(o, ohs.p, ost2.p); orc_get_cards(o, ocards.p); orc_get_showdown(o, orank.p, okick.p);
        orc_valid_actions(o, ovalid.p);
        for (int t = 0; t < T; ++t) {
            const SeatStates s{ss[t]}; const Cursor c{cur[t]};
            for (int p = 0; p < N; ++p) {
                if (s.state_of(p) != ost[t * N + p]) fail("player state", t, p, ost[t * N + p], s.state_of(p));
                const uint32_t want = ((uint32_t)orank[t * N + p] << 20) | okick[t * N + p];
                if (show[(size_t)p * T + t] != want) fail("show", t, p, want, show[(size_t)p * T + t]);
            }
            const int32_t got[6] = {(int32_t)c.active(), (int32_t)c.turn(), (int32_t)c.dealer(), (int32_t)c.sb(), (int32_t)c.bb(), hand[t]};
            static const char *cn[6] = {"active", "turn", "dealer", "sb", "bb", "hand"};
            for (int k = 0; k < 6; ++k) if (got[k] != ocur[6 * t + k]) fail(cn[k], t, -1, ocur[6 * t + k], got[k]);
            if (c.in_flight()) fail("cursor: a step is in flight after a complete launch", t, -1, 0, cur[t] >> 20);
            if (hs[t] != ohs[t]) fail("hand_serial", t, -1, (double)ohs[t], (double)hs[t]);
            if (st[t] != ost2[t]) fail("step_serial", t, -1, (double)ost2[t], (double)st[t]);
            for (int i = 0; i < KK; ++i) if (card_byte(cards.p, (size_t)T, t, i) != ocards[(size_t)t * KK + i]) fail("card", t, i, ocards[(size_t)t * KK + i], card_byte(cards.p, (size_t)T, t, i));
            if (valid[t] != ovalid[t]) fail("valid", t, -1, ovalid[t], valid[t]);
            if (owed[t] != 0) fail("owed", t, -1, 0, owed[t]);
        }
        if (check_terr_word) {   // a rollout's State::terr accumulates over its launches; the oracle returns the OR over tables and steps
            int got = 0; for (int t = 0; t < T; ++t) got |= terr[t];
            if (got != orc_err) fail("terr (OR over the tables)", -1, -1, orc_err, got);
            unsigned long long sum[4] = {0, 0, 0, 0};
            for (int w = 0; w < grid; ++w) for (int k = 0; k < 4; ++k) sum[k] += counters[(size_t)w * PK_NUM_COUNTERS + k];
            static const char *kn[4] = {"counter steps", "counter hands", "counter evals", "counter games"};
            for (int k = 0; k < 4; ++k) if (sum[k] != oc4[k]) fail(kn[k], -1, -1, (double)oc4[k], (double)sum[k]);
        }
        return bad;
    }
};

// One run of a fused-rollout family: K steps as the launches of `split`; the ones before the last defer (slack < 64), then a flush (K = 0) completes them.
template <int N, int FAM>
static int run_rollout(int T, const Cfg &cfg, int K, int park, bool split) {
    Sim<N, FAM> s(T, cfg);
    char where[96];
    int bad = 0;
    if (FAM == F_SINGLE) {      // pk_rollout(fused = 0): K complete single-step launches
        for (int k = 0; k < K && !bad; ++k) {
            s.launch_rollout(1, park, PK_WAVE, 1);
            s.orc_err = orc_rollout(s.o, 1, 0, 1, s.oc4);
            snprintf(where, sizeof where, "T=%d park=%d launch %d", T, park, k);
            bad = s.compare(where, true);
        }
    } else if (!split) {
        s.launch_rollout(K, park, PK_WAVE, 1);
        s.orc_err = orc_rollout(s.o, K, Sim<N, FAM>::POLICY, 1, s.oc4);
        snprintf(where, sizeof where, "T=%d park=%d launches {%d}", T, park, K);
        bad = s.compare(where, true);
        // ... and once more on the tables that launch left (lds.show starts from garbage again: store_show writes only what this launch showed)
        s.launch_rollout(5, park, PK_WAVE, 1);
        s.orc_err = orc_rollout(s.o, 5, Sim<N, FAM>::POLICY, 1, s.oc4);
        bad += s.compare(where, true);
    } else {
        const int ks[3] = {1, 7, K - 8}, slacks[3] = {40, 16, 57};
        for (int i = 0; i < 3; ++i) s.launch_rollout(ks[i], park, slacks[i], i == 0);
        long left = 0; for (int t = 0; t < T; ++t) left += s.owed[t] != 0 || (s.cur[t] >> 20) != 0;
        s.inflight_seen = left;
        s.launch_rollout(0, park, PK_WAVE, 0);
        s.orc_err = orc_rollout(s.o, K, Sim<N, FAM>::POLICY, 1, s.oc4);
        snprintf(where, sizeof where, "T=%d park=%d launches {1,7,%d} + flush (%ld tables had work deferred)", T, park, K - 8, left);
        bad = s.compare(where, true);
    }
    return bad;
}
// Game.step with the caller's actions (the oracle's random agent's, one table in 23 an invalid one); finished games are reset as a caller does.
// ASYNC: every step is a bounded launch (max_end = 1) followed by a drain (actions == NULL) that completes what stayed in flight.
template <int N, int FAM>
static int run_step(int T, const Cfg &cfg, int K, int park, long *inflight, bool deep = false, long *river = nullptr) {
    Sim<N, FAM> s(T, cfg);
    Arr<uint8_t> of(T), oe(T), m(T);
    Arr<int32_t> ocur(6 * (size_t)T);
    Arr<uint8_t> ostates((size_t)T * N);
    char where[96];
    int bad = 0;
    for (int k = 0; k < K && !bad; ++k) {
        orc_pick_actions(s.o, deep ? 14 : 0, s.actions.p);
        if (river) { orc_get_cursors(s.o, ocur.p); orc_get_states(s.o, ostates.p); }
        for (int t = 0; t < T; ++t) if ((t + 3 * k) % 23 == 5) s.actions[t] = (k & 1) ? PK_NUM_MOVES : -1;
        orc_step(s.o, s.actions.p, of.p, oe.p);
        if (river)      // hand ends at the river among three or more seats still in the hand (two at a two-seat table)
            for (int t = 0; t < T; ++t) {
                int live = 0;
                for (int p = 0; p < N; ++p) live += ostates[(size_t)t * N + p] >= 1 && ostates[(size_t)t * N + p] <= 3;
                *river += (of[t] & 2) && ocur[6 * t + 1] == 3 && live >= (N < 3 ? N : 3);
            }
        if (FAM == F_STEP) s.launch_step(s.actions.p, s.flags.p, s.terr_out.p, nullptr, park, 0);
        else {
            // the bounded launch; one more bounded launch that steps nothing (an invalid action for every table: the ones whose step has returned come
            // back untouched, the ones in flight ignore it and carry on); then the drain.  A table's outputs are the ones of the launch it got ready in.
            Arr<int32_t> none(T, -1);
            Arr<uint8_t> done(T, 0);
            s.launch_step(s.actions.p, s.flags.p, s.terr_out.p, s.ready.p, park, 1);
            for (int t = 0; t < T; ++t) { done[t] = s.ready[t]; *inflight += !s.ready[t]; }
            for (int pass = 0; pass < 2; ++pass) {
                s.launch_step(pass == 0 ? none.p : nullptr, s.flags2.p, s.terr2.p, s.ready2.p, park, pass == 0 ? 1 : 0);
                for (int t = 0; t < T; ++t)
                    if (!done[t] && s.ready2[t]) { done[t] = 1; s.flags[t] = s.flags2[t]; s.terr_out[t] = s.terr2[t]; }
                    else if (done[t] && (!s.ready2[t] || s.terr2[t] != PK_TERR_INVALID_ACTION)) { if (bad++ < 5) printf("MISMATCH step_async N=%d: idle table %d not refused by a launch that steps nothing\n", N, t); }
            }
            for (int t = 0; t < T; ++t) if (!done[t]) { if (bad++ < 5) printf("MISMATCH step_async N=%d: table %d not ready after the drain\n", N, t); }
        }
        snprintf(where, sizeof where, "T=%d park=%d step %d", T, park, k);
        for (int t = 0; t < T; ++t) {
            if (s.flags[t] != of[t] || s.terr_out[t] != oe[t]) { if (bad++ < 5) printf("MISMATCH %s N=%d %s: table %d flags %d/%d terr %d/%d\n", kFamilyName[FAM], N, where, t, of[t], s.flags[t], oe[t], s.terr_out[t]); }
            if (FAM == F_STEP && s.terr[t] != oe[t]) { if (bad++ < 5) printf("MISMATCH step N=%d %s: table %d State::terr %d/%d\n", N, where, t, oe[t], s.terr[t]); }
            m[t] = of[t] & 1;
        }
        bad += s.compare(where, false);
        orc_reset(s.o, m.p, 0); s.reset(m.p);
    }
    return bad;
}

template <int N, int FAM>
static int run_case(const Opts &op) {
    constexpr bool allin = FAM == F_ALLIN || FAM == F_ALLIN_TAB, stepf = FAM == F_STEP || FAM == F_STEP_ASYNC;
    const int K = op.steps > 0 ? op.steps : (stepf && op.deep ? 60 : (stepf || FAM == F_SINGLE ? 24 : 48));
    int bad = 0, runs = 0;
    long inflight = 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::string ran;
    if (op.ring) {
        if constexpr (FAM == F_ROLLOUT || FAM == F_TAB) {
            const int Kr = op.steps > 0 ? op.steps : 1024;
            Sim<N, FAM> s(192, equal_cfg(N));
            for (auto &c : pk_sim::ring_count) c.store(0);
            for (int i = 0; i < 3 && !bad; ++i) {
                s.launch_rollout(Kr, 28, PK_WAVE, 1);
                s.orc_err = orc_rollout(s.o, Kr, Sim<N, FAM>::POLICY, 1, s.oc4);
                bad = s.compare("ring-stats", true);
            }
            const double it = (double)pk_sim::ring_count[0].load(), ps = (double)pk_sim::ring_count[1].load(), ln = (double)pk_sim::ring_count[2].load();
            printf("%s N=%d ring-stats: 3 launches of %d steps, 192 tables, park 28: %.0f loop iterations, %.0f Philox passes = %.3f per iteration, %.1f lanes filled per pass, "
                   "%.3f wave-steps per iteration%s\n", kFamilyName[FAM], N, Kr, it, ps, ps / it, ps > 0 ? ln / ps : 0.0, 3.0 * Kr * 3 / it, bad ? ": MISMATCH" : ": wave-sim == oracle");
        }
        return bad != 0;
    }
    if (op.deep) {
        if constexpr (stepf) {
            long river = 0;
            const Cfg cfg = deep_cfg(N);
            for (int T : {64 * 3 + 7, 1})
                for (int park : {1, 28, 64}) {
                    if (op.quick && !(T > 1 && park == 28)) continue;
                    const int b = run_step<N, FAM>(T, cfg, K, park, &inflight, true, &river);
                    if (b) printf("  ^ %s, T=%d park=%d K=%d\n", cfg.name, T, park, K);
                    bad += b; ++runs;
                }
            if (river == 0) { printf("%s N=%d deep: no hand ended at the river among three or more seats: nothing deep was compared\n", kFamilyName[FAM], N); ++bad; }
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (!bad) printf("%s N=%d deep: %d runs (%s; %d steps; %ld multi-way river hand ends): wave-sim == oracle  [%.1f s]\n", kFamilyName[FAM], N, runs, cfg.name, K, river, sec);
            else printf("%s N=%d deep: %d mismatches\n", kFamilyName[FAM], N, bad);
            fflush(stdout);
            return bad != 0;
        } else {
            return 0;      // (the rollout families play the product's own agents: nothing deep to run)
        }
    }
    for (int ci = 0; ci < (op.quick ? 1 : (stepf ? 3 : 2)); ++ci) {
        // quick (the suite's test): the configuration that matters most for the family -- equal stacks for the all-in agents (all-showdown queues)
        const Cfg cfg = ci == 2 ? rolling_cfg(N) : ((op.quick ? allin : ci == 1) ? equal_cfg(N) : fuzz_cfg(N));
        for (int T : {64 * 3 + 7, 1})
            for (int park : {1, 28, 64})
                for (int split = 0; split < 2; ++split) {
                    if (op.quick && !(T > 1 && park == 28 && split == (stepf ? 0 : 1))) continue;
                    if ((stepf || FAM == F_SINGLE) && split) continue;      // (every launch of these kernels is one complete step)
                    int b;
                    if constexpr (stepf) b = run_step<N, FAM>(T, cfg, K, park, &inflight);
                    else b = run_rollout<N, FAM>(T, cfg, K, park, split != 0);
                    if (b) printf("  ^ %s, T=%d park=%d split=%d K=%d\n", cfg.name, T, park, split, K);
                    bad += b; ++runs;
                    if (runs <= 1) ran = std::string(cfg.name) + ", T=" + std::to_string(T) + ", park " + std::to_string(park) + (stepf || FAM == F_SINGLE ? ", one launch per step" : (split ? ", launches {1,7,K-8} + flush" : ", one launch"));
                }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (FAM == F_STEP_ASYNC) {
        printf("  (step_async: %ld steps stayed in flight after their bounded launch and were completed by later launches)\n", inflight);
        if (!op.quick && inflight == 0) { printf("step_async N=%d: no step ever stayed in flight: the bounded path was not reached\n", N); ++bad; }
    }
    if (runs > 1) ran = "per-seat / equal" + std::string(stepf ? " / above-the-stacks-blinds" : "") + " stacks, T = 199 and 1, park 1/28/64" + (stepf || FAM == F_SINGLE ? ", one launch per step" : ", launches {K} and {1,7,K-8} + flush");
    if (!bad) printf("%s N=%d: %d runs (%s; %d steps): wave-sim == oracle  [%.1f s]\n", kFamilyName[FAM], N, runs, ran.c_str(), K, sec);
    else printf("%s N=%d: %d mismatches\n", kFamilyName[FAM], N, bad);
    fflush(stdout);
    return bad != 0;
}

#define WS_CASE(FAM, N) static const bool ws_reg_##FAM##_##N = (registry().push_back(Case{FAM, N, &run_case<N, FAM>}), true);
#ifndef PK_WS_PART
#error "compile with -DPK_WS_PART=<0 (no case: main alone) | 1..11 | 100>"
#endif
#if PK_WS_PART == 1
WS_CASE(F_ROLLOUT, 2) WS_CASE(F_ROLLOUT, 6) WS_CASE(F_ROLLOUT, 10)
#elif PK_WS_PART == 2
WS_CASE(F_ROLLOUT, 13) WS_CASE(F_ROLLOUT, 16)
#elif PK_WS_PART == 3
WS_CASE(F_ALLIN, 2) WS_CASE(F_ALLIN, 6) WS_CASE(F_ALLIN, 10)
#elif PK_WS_PART == 4
WS_CASE(F_ALLIN, 13) WS_CASE(F_ALLIN, 16)
#elif PK_WS_PART == 5
WS_CASE(F_CALL, 2) WS_CASE(F_CALL, 6) WS_CASE(F_CALL, 10)
#elif PK_WS_PART == 6
WS_CASE(F_CALL, 13) WS_CASE(F_CALL, 16)
#elif PK_WS_PART == 7
WS_CASE(F_TAB, 2) WS_CASE(F_TAB, 6)
#elif PK_WS_PART == 8
WS_CASE(F_ALLIN_TAB, 2) WS_CASE(F_ALLIN_TAB, 9) WS_CASE(F_ALLIN_TAB, 10)
#elif PK_WS_PART == 9
WS_CASE(F_SINGLE, 2) WS_CASE(F_SINGLE, 6) WS_CASE(F_SINGLE, 16)
#elif PK_WS_PART == 10
WS_CASE(F_STEP, 2) WS_CASE(F_STEP, 6) WS_CASE(F_STEP, 16)
#elif PK_WS_PART == 11
WS_CASE(F_STEP_ASYNC, 6)
#elif PK_WS_PART == 100
WS_CASE(F_TAB, 6) WS_CASE(F_ALLIN_TAB, 9) WS_CASE(F_STEP, 6)
#endif

#ifdef PK_WS_MAIN
int main(int argc, char **argv) {
    Opts op;
    std::string fam;
    int n = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--quick") op.quick = true;
        else if (a == "--deep") op.deep = true;
        else if (a == "--ring-stats") op.ring = true;
        else if (a == "--steps" && i + 1 < argc) op.steps = atoi(argv[++i]);
        else if (fam.empty()) fam = a;
        else n = atoi(argv[i]);
    }
    std::sort(registry().begin(), registry().end(), [](const Case &a, const Case &b) { return a.family != b.family ? a.family < b.family : a.n < b.n; });
    int rc = 0, ran = 0;
    for (const Case &c : registry())
        if ((fam.empty() || fam == kFamilyName[c.family]) && (n == 0 || n == c.n) && (!op.deep || c.family == F_STEP || c.family == F_STEP_ASYNC)) { rc |= c.fn(op); ++ran; }
    if (!ran) { fprintf(stderr, "wave_sim: no such case in this build\n"); return 2; }
    printf(rc ? "wave_sim: FAILED\n" : "wave_sim: %d cases == oracle\n", ran);
    return rc;
}
#endif
