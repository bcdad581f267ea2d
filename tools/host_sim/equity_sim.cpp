// Dev-only: the REAL equity kernels -- k_equity<N>, k_eqs<N>, k_eqr, k_rvr, k_hist, k_hero_hist, k_eqw<N, RC> and their preparation kernels, the text of
// pokerl_amd/csrc/pk_equity*.hip, and k_pfm_rank / k_pfm_count of pk_preflop.hip -- run on the CPU as workgroups of 8 waves x 64 lanes (wg_shim.h: a fibre per lane, every collective and
// barrier a checked rendezvous, garbage LDS before every workgroup, PK_IDX active).  One case per run: the case file names the family, the
// spots, the weights / bins / samples, the grid and which outputs are wanted; the preparation kernel runs, then the main kernel, and every
// output array goes to the out file.  Expected values are NOT computed here: tools/host_sim/equity_cases.py writes the case files and compares
// the outputs with the numpy specs of tests/.  Every input, work and output array is an allocation of exactly its size (ASan bounds it); work
// and output arrays start from a non-zero pattern (device memory is not zeroed, and the kernels promise to write every entry).
//   g++ -std=c++20 -O1 -ffp-contract=off -DPK_HOST_SIM -I tools/host_sim/stub -include tools/host_sim/wg_shim.h tools/host_sim/equity_sim.cpp
//   equity_sim <case file> <out file>
// Case file: lines "name dtype count" (dtype u8 u16 u32 u64 i32) each followed by a line of `count` decimal values, and
// "family <name>" / "outputs <name> ..." lines.  Out file: the same array format.
// -DPK_ES_ONLY=1 .. 22: a build of ONE family (equity, sampled, range, rvr, hist, ranged, ev, cluster, herohist, preflop, rangedev, riversolve, turnsolve, rivertrees, turntrees, riverlock, turnlock, riverresolve, turnresolve, riverresume, turnresume, pfsolve), so that a test can compile them side by side.
// The pfsolve family (pk_preflop_solver.hip: k_preflop_solve) takes the trees as rivertrees does, an optional tree_of (none: every spot uses tree 0)
// and ranges; the table it reads is the readers' fixed pattern (fill_table), which has none of the real table's structure: the kernel must not lean on any.
// The riverresume / turnresume families (k_resume_prep, k_resume_river_solve / k_resume_turn_solve) take what riverresolve / turnresolve take and the state arrays,
// which go in and come out: allocations of exactly their size, holding what the case put there.
// The riverresolve / turnresolve families (k_resolve_prep, k_resolve_river_solve / k_resolve_turn_solve) take what riverlock / turnlock take (ranges optional) and
// the optional reach, given (river), at and at_card (turn) arrays, each in an allocation of exactly its size; the node outputs node_reach (u32), node_value, node_br (i64 as u64).
// The riverlock / turnlock families (k_lock_river_solve / k_lock_turn_solve) take the trees as rivertrees / turntrees do, an optional tree_of (none: every
// spot uses tree 0 and k_trees_prep is not queued) and the optional lock / locked (turn: river_lock / river_locked too) arrays, each in an allocation of exactly its size.
// The rivertrees / turntrees families (k_rs_prep / k_ts_prep, k_trees_prep, k_trees_river_solve / k_trees_turn_solve) take ntrees trees as rows of 64 / 128 nodes, as the
// C ABI's tree-per-spot calls do, and tree_of per spot; the outputs have the call's row strides.  The work space is sized for the call's largest tree, as the library sizes it.
// The turnsolve family (pk_turn_solver.hip: k_ts_prep, k_turn_solve) takes the tree as riversolve does; the driver derives nact, row, river and idx as the host check does.
// The riversolve family (pk_river_solver.hip: k_rs_prep, k_river_solve) takes the tree's arrays as the C ABI does; the driver derives nact and row as the host check does.  Its
// int64 outputs (value, br) travel as their bit patterns, dtype u64.
// The preflop family (pk_preflop.hip) is the partial count: the driver queues k_pfm_rank and k_pfm_count chunk by chunk in the order of
// pk::pfm_count_launch, with the case's board range, chunk and `accumulate` (the outputs start from 0xA5 bytes: an accumulating case adds to them).
// Its readers are the families pfhero (k_pfm_prep, k_pfm_hero) and pfrvr (k_pfm_rvr) of the same build; the table they read is a fixed pattern
// (fill_table; equity_cases.py preflop_table restates it), not a counted one: what the readers do with the numbers is what is checked.
// The herohist family (pk_equity_hist_hero.hip) checks its spots with k_eqr_prep; its optional bucket stage is the cluster family's assign and is not run here.
// The cluster family (pk_hist_cluster.hip) has no preparation kernel: the driver queues its kernels in the order of pk::cl_seed_launch /
// cl_assign_launch / cl_cluster_launch (`op` 0 / 1 / 2), with the case's grid, seeding chunk and choice of the update kernel.
// f64 arrays (the bets, amounts and ev of the ev family) travel as their bit patterns, dtype u64.
#ifndef PK_ES_ONLY
#define PK_ES_ONLY 0
#endif
#define PK_ES_HAS(n) (PK_ES_ONLY == 0 || PK_ES_ONLY == (n))
#if PK_ES_HAS(1)
#include "../../pokerl_amd/csrc/pk_equity.hip"
#endif
#if PK_ES_HAS(2)
#include "../../pokerl_amd/csrc/pk_equity_sampled.hip"
#endif
#if PK_ES_HAS(3) || PK_ES_HAS(9)
#include "../../pokerl_amd/csrc/pk_equity_range.hip"     // (the hero histograms check their spots with k_eqr_prep)
#endif
#if PK_ES_HAS(4) || PK_ES_HAS(5)
#include "../../pokerl_amd/csrc/pk_equity_rvr.hip"      // (the histograms check their spots with k_rvr_prep)
#endif
#if PK_ES_HAS(5)
#include "../../pokerl_amd/csrc/pk_equity_hist.hip"
#endif
#if PK_ES_HAS(6) || PK_ES_HAS(11)
#if !PK_ES_HAS(2)
#include "../../pokerl_amd/csrc/pk_equity_sampled.hip"  // (the ranged families split their tasks with pk::eqs_lpt)
#endif
#include "../../pokerl_amd/csrc/pk_equity_ranged.hip"   // (the ranged EV sums its rows with k_eqw_cdf)
#endif

#if PK_ES_HAS(7)
#include "../../pokerl_amd/csrc/pk_equity_ev.hip"
#endif

#if PK_ES_HAS(11)
#include "../../pokerl_amd/csrc/pk_ev_ranged.hip"
#endif

#if PK_ES_HAS(8) || PK_ES_HAS(9)
#include "../../pokerl_amd/csrc/pk_equity.hpp"          // (EqTables, which the driver's table_form names)
#include "../../pokerl_amd/csrc/pk_hist_cluster.hip"    // (pk::hh_launch names pk::cl_assign_launch)
#endif

#if PK_ES_HAS(9)
#include "../../pokerl_amd/csrc/pk_equity_hist_hero.hip"
#endif

#if PK_ES_HAS(10)
#include "../../pokerl_amd/csrc/pk_preflop.hip"
#endif
#if PK_ES_HAS(12) || PK_ES_HAS(14) || PK_ES_HAS(13) || PK_ES_HAS(15) || PK_ES_HAS(16) || PK_ES_HAS(17) || PK_ES_HAS(18) || PK_ES_HAS(19) || PK_ES_HAS(20) || PK_ES_HAS(21)
#include "../../pokerl_amd/csrc/pk_river_solver.hip"     // (the turn solver's tree-per-spot launch queues k_trees_prep)
#endif
#if PK_ES_HAS(13) || PK_ES_HAS(15) || PK_ES_HAS(17) || PK_ES_HAS(19) || PK_ES_HAS(21)
#include "../../pokerl_amd/csrc/pk_turn_solver.hip"
#endif
#if PK_ES_HAS(22)
#include "../../pokerl_amd/csrc/pk_preflop_solver.hip"
#endif
#include <chrono>
#include <climits>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>

namespace {

[[noreturn]] void die(const std::string &what) { fprintf(stderr, "equity_sim: %s\n", what.c_str()); exit(2); }

struct Buf {
    std::string dtype;
    size_t count = 0, width = 0;
    void *p = nullptr;
    Buf(const std::string &dt, size_t n, int fill) : dtype(dt), count(n) {
        width = dt == "u8" ? 1 : (dt == "u16" ? 2 : (dt == "u32" || dt == "i32" ? 4 : (dt == "u64" ? 8 : 0)));
        if (!width) die("dtype " + dt);
        p = malloc(n * width ? n * width : 1);                       // exactly its size
        memset(p, fill, n * width);
    }
    ~Buf() { free(p); }
    Buf(const Buf &) = delete;
    void set(size_t i, unsigned long long v) {
        if (width == 1) ((uint8_t *)p)[i] = (uint8_t)v; else if (width == 2) ((uint16_t *)p)[i] = (uint16_t)v;
        else if (width == 4) ((uint32_t *)p)[i] = (uint32_t)v; else ((uint64_t *)p)[i] = v;
    }
    unsigned long long get(size_t i) const {
        return width == 1 ? ((uint8_t *)p)[i] : (width == 2 ? ((uint16_t *)p)[i] : (width == 4 ? ((uint32_t *)p)[i] : ((uint64_t *)p)[i]));
    }
};

struct Case {
    std::string family;
    std::vector<std::string> outputs;
    std::map<std::string, std::unique_ptr<Buf>> in;
    std::vector<std::pair<std::string, std::unique_ptr<Buf>>> out;

    explicit Case(const char *path) {
        std::ifstream f(path);
        if (!f) die(std::string("cannot read ") + path);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream h(line);
            std::string name, dt;
            if (!(h >> name)) continue;
            if (name == "family") { h >> family; continue; }
            if (name == "outputs") { std::string o; while (h >> o) outputs.push_back(o); continue; }
            size_t n;
            if (!(h >> dt >> n)) die("bad header line: " + line);
            auto b = std::make_unique<Buf>(dt, n, 0);
            if (!std::getline(f, line)) die("no values for " + name);
            std::istringstream v(line);
            for (size_t i = 0; i < n; ++i) {
                std::string tok;
                if (!(v >> tok)) die("too few values for " + name);
                b->set(i, dt == "i32" ? (unsigned long long)(long long)std::stoll(tok) : std::stoull(tok));
            }
            in[name] = std::move(b);
        }
    }
    template <typename T> const T *arr(const char *name, size_t want) const {
        auto it = in.find(name);
        if (it == in.end()) return nullptr;
        if (it->second->width != sizeof(T) || it->second->count != want) die(std::string(name) + ": " + std::to_string(it->second->count) + " x " + it->second->dtype + ", the kernel reads " + std::to_string(want) + " elements of " + std::to_string(sizeof(T)) + " bytes");
        return (const T *)it->second->p;
    }
    template <typename T> const T *need(const char *name, size_t want) const {
        const T *p = arr<T>(name, want);
        if (!p) die(std::string("the case has no ") + name);
        return p;
    }
    long long num(const char *name, long long dflt = LLONG_MIN) const {
        auto it = in.find(name);
        if (it == in.end()) { if (dflt == LLONG_MIN) die(std::string("the case has no ") + name); return dflt; }
        return it->second->dtype == "i32" ? (long long)(int32_t)it->second->get(0) : (long long)it->second->get(0);
    }
    // an output array: NULL unless the case wants it; starts from 0xA5 bytes
    template <typename T> T *output(const char *name, const char *dt, size_t n) {
        if (std::find(outputs.begin(), outputs.end(), name) == outputs.end()) return nullptr;
        out.emplace_back(name, std::make_unique<Buf>(dt, n, 0xA5));
        return (T *)out.back().second->p;
    }
    // an array that goes in AND comes out (a solver's state): the case's own values, an allocation of exactly its size, written with the outputs
    template <typename T> T *inout(const char *name, size_t n) {
        auto it = in.find(name);
        if (it == in.end()) return nullptr;
        if (it->second->width != sizeof(T) || it->second->count != n) die(std::string(name) + ": not the size the kernel works in");
        if (std::find(outputs.begin(), outputs.end(), name) == outputs.end()) die(std::string(name) + " goes in and must come out: name it among the outputs");
        out.emplace_back(name, std::move(it->second));
        in.erase(it);
        return (T *)out.back().second->p;
    }
    void write(const char *path) const {
        FILE *f = fopen(path, "w");
        if (!f) die(std::string("cannot write ") + path);
        for (const auto &o : out) {
            fprintf(f, "%s %s %zu\n", o.first.c_str(), o.second->dtype.c_str(), o.second->count);
            for (size_t i = 0; i < o.second->count; ++i) fprintf(f, i ? " %llu" : "%llu", o.second->get(i));
            fprintf(f, "\n");
        }
        fclose(f);
    }
};

// a work array of the call (descriptors, task list): exactly its size, 0x5A bytes
template <typename T> struct Work {
    T *p; size_t n;
    explicit Work(size_t n_) : p((T *)malloc(n_ * sizeof(T) ? n_ * sizeof(T) : 1)), n(n_) { memset((void *)p, 0x5A, n * sizeof(T)); }
    ~Work() { free(p); }
    Work(const Work &) = delete;
};

// the table form's arrays (a handle's own state, hand-built by the case): cards [W][T] words, seat_states [T], cursors [T], tables [m] or none
bool table_form(const Case &c, int N, size_t m, EqTables &t) {
    if (c.in.find("cursors") == c.in.end()) return false;
    const int T = (int)c.num("T"), W = (5 + 2 * N + 3) / 4;
    t.T = T;
    t.cards = c.need<uint32_t>("cards", (size_t)W * T);
    t.seat_states = c.need<uint64_t>("seat_states", (size_t)T);
    t.cursors = c.need<uint32_t>("cursors", (size_t)T);
    t.tables = c.arr<int32_t>("tables", m);
    return true;
}
unsigned prep_grid(size_t m, unsigned block) { return (unsigned)((m + block - 1) / block); }

#if PK_ES_HAS(1)
template <int N>
void run_equity(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const int lpt = (int)c.num("lpt"), pool_max = (int)c.num("pool_max");
    const unsigned grid = (unsigned)c.num("grid");
    EqPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t);
    if (!tbl) { a.s.holes = c.need<uint8_t>("holes", m * N * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.live = c.need<uint16_t>("live", m); }
    EqOut out{c.output<uint32_t>("win", "u32", m * N), c.output<uint32_t>("tie", "u32", m * N), c.output<uint64_t>("share", "u64", m * N),
              c.output<uint32_t>("boards", "u32", m), c.output<uint8_t>("status", "u8", m)};
    Work<EqCtrl> ctrl(1);
    memset(ctrl.p, 0, sizeof(EqCtrl));                               // (eq_launch's hipMemsetAsync)
    Work<uint64_t> desc(m * (size_t)(3 + N));
    Work<uint2> tasks(pk::eq_task_cap(m, lpt, pool_max));
    const EqWork w{ctrl.p, desc.p, tasks.p, tasks.n};
    a.out = out; a.w = w; a.N = N; a.lpt = lpt; a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EQ_PREP_BLOCK), EQ_PREP_BLOCK, [&] { k_equity_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, EQ_PREP_BLOCK), EQ_PREP_BLOCK, [&] { k_equity_prep<false>(a); });
    printf("tasks %u take %u\n", ctrl.p->ntasks, ctrl.p->ntasks >= 8u * grid * EQ_WAVES ? 4u : 1u);
    pk_sim::launch(grid, EQ_BLOCK, [&] { k_equity<N>(tab, w, out, lpt); });
}

#endif

#if PK_ES_HAS(2)
template <int N>
void run_sampled(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    EqsPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t);
    if (!tbl) { a.s.holes = c.need<uint8_t>("holes", m * N * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.live = c.need<uint16_t>("live", m); }
    EqsStream rng{(uint32_t)c.num("key0"), (uint32_t)c.num("key1"), (uint32_t)c.num("nonce"), (uint32_t)c.num("samples"), (uint32_t)c.num("id_base", 0), c.arr<uint32_t>("ids", m)};
    EqsOut out{};
    out.win = c.output<uint32_t>("win", "u32", m * N); out.tie = c.output<uint32_t>("tie", "u32", m * N); out.share = c.output<uint64_t>("share", "u64", m * N);
    out.samples = c.output<uint32_t>("samples", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * (size_t)eqs_desc_words(N));
    a.rng = rng; a.out = out; a.desc = desc.p; a.N = N; a.observer = (int)c.num("observer", PK_OBSERVER_NONE); a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EQS_PREP_BLOCK), EQS_PREP_BLOCK, [&] { k_eqs_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, EQS_PREP_BLOCK), EQS_PREP_BLOCK, [&] { k_eqs_prep<false>(a); });
    const long long lpt_case = c.num("lpt", 0);
    const uint32_t S = rng.samples, per = 64u * (uint32_t)(lpt_case ? lpt_case : pk::eqs_lpt(m, S)), nch = (S + per - 1) / per, ntasks = (uint32_t)m * nch;
    printf("tasks %u (%u per spot)\n", ntasks, nch);
    const uint64_t *dp = desc.p;
    pk_sim::launch(grid, EQ_BLOCK, [&] { k_eqs<N>(tab, dp, out, rng, ntasks, nch, per); });
}

#endif

#if PK_ES_HAS(3)
void run_range(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const int N = (int)c.num("N", 2);
    EqrPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t);
    if (!tbl) { a.s.hero = c.need<uint8_t>("hero", m * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.dead = c.arr<uint64_t>("dead", m); }
    const int per_spot = (int)c.num("per_spot", 0);
    const EqrWeights wts{c.arr<uint16_t>("weights", per_spot ? m * EQR_HOLDINGS : (size_t)EQR_HOLDINGS), per_spot};
    EqrOut out{};
    out.agg = c.output<uint64_t>("agg", "u64", m * 3); out.win = c.output<uint32_t>("win", "u32", m * EQR_HOLDINGS); out.tie = c.output<uint32_t>("tie", "u32", m * EQR_HOLDINGS);
    out.boards = c.output<uint32_t>("boards", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * EQR_DESC_WORDS);
    a.out = out; a.desc = desc.p; a.N = N; a.observer = (int)c.num("observer", 0); a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EQR_PREP_BLOCK), EQR_PREP_BLOCK, [&] { k_eqr_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, EQR_PREP_BLOCK), EQR_PREP_BLOCK, [&] { k_eqr_prep<false>(a); });
    const uint64_t *dp = desc.p;
    if (out.agg || out.win || out.tie) pk_sim::launch(grid, EQR_BLOCK, [&] { k_eqr(tab, dp, wts, out, (uint32_t)m); });
}

#endif

#if PK_ES_HAS(4) || PK_ES_HAS(5)
// k_rvr_prep for range vs range and the histograms alike
void run_rvr_prep(Case &c, size_t m, const RvrOut &out, uint64_t *desc) {
    RvrPrepArgs a{};
    const bool tbl = table_form(c, (int)c.num("N", 2), m, a.t);
    if (!tbl) { a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.dead = c.arr<uint64_t>("dead", m); }
    a.out = out; a.desc = desc; a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, RVR_PREP_BLOCK), RVR_PREP_BLOCK, [&] { k_rvr_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, RVR_PREP_BLOCK), RVR_PREP_BLOCK, [&] { k_rvr_prep<false>(a); });
}

#endif

#if PK_ES_HAS(4)
void run_rvr(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const int per_spot = (int)c.num("per_spot", 0);
    const RvrWeights wts{c.arr<uint16_t>("weights", per_spot ? m * RVR_HOLDINGS : (size_t)RVR_HOLDINGS), per_spot};
    RvrOut out{};
    out.win = c.output<uint64_t>("win", "u64", m * RVR_HOLDINGS); out.tie = c.output<uint64_t>("tie", "u64", m * RVR_HOLDINGS); out.tot = c.output<uint64_t>("tot", "u64", m * RVR_HOLDINGS);
    out.boards = c.output<uint32_t>("boards", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RVR_DESC_WORDS);
    run_rvr_prep(c, m, out, desc.p);
    const uint64_t *dp = desc.p;
    if (out.win || out.tie || out.tot) pk_sim::launch(grid, RVR_BLOCK, [&] { k_rvr(tab, dp, wts, out, (uint32_t)m); });
}

#endif

#if PK_ES_HAS(5)
void run_hist(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t bins = (uint32_t)c.num("bins");
    const int per_spot = (int)c.num("per_spot", 0);
    const RvrWeights wts{c.arr<uint16_t>("weights", per_spot ? m * RVR_HOLDINGS : (size_t)RVR_HOLDINGS), per_spot};
    HistOut out{};
    out.hist = c.output<uint16_t>("hist", "u16", m * RVR_HOLDINGS * bins); out.void_ = c.output<uint16_t>("void", "u16", m * RVR_HOLDINGS);
    out.completions = c.output<uint32_t>("completions", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RVR_DESC_WORDS);
    run_rvr_prep(c, m, RvrOut{nullptr, nullptr, nullptr, nullptr, out.status}, desc.p);
    const uint64_t *dp = desc.p;
    if (out.completions) pk_sim::launch(prep_grid(m, HIST_COUNTS_BLOCK), HIST_COUNTS_BLOCK, [&] { k_hist_counts(dp, out.completions, m); });
    if (out.hist || out.void_) pk_sim::launch(grid, RVR_BLOCK, [&] { k_hist(tab, dp, wts, out, bins, (uint32_t)m); });
}
#endif


#if PK_ES_HAS(9)
// k_eqr_prep (status alone), k_hero_hist_counts, k_hero_hist
void run_hero_hist(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t bins = (uint32_t)c.num("bins");
    const int N = (int)c.num("N", 2);
    EqrPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t);
    if (!tbl) { a.s.hero = c.need<uint8_t>("hero", m * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.dead = c.arr<uint64_t>("dead", m); }
    const int per_spot = (int)c.num("per_spot", 0);
    const EqrWeights wts{c.arr<uint16_t>("weights", per_spot ? m * EQR_HOLDINGS : (size_t)EQR_HOLDINGS), per_spot};
    HeroHistOut out{};
    out.hist = c.output<uint16_t>("hist", "u16", m * bins); out.void_ = c.output<uint16_t>("void", "u16", m);
    out.completions = c.output<uint32_t>("completions", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * EQR_DESC_WORDS);
    a.out = EqrOut{nullptr, nullptr, nullptr, nullptr, out.status}; a.desc = desc.p; a.N = N; a.observer = (int)c.num("observer", 0); a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EQR_PREP_BLOCK), EQR_PREP_BLOCK, [&] { k_eqr_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, EQR_PREP_BLOCK), EQR_PREP_BLOCK, [&] { k_eqr_prep<false>(a); });
    const uint64_t *dp = desc.p;
    if (out.completions) pk_sim::launch(prep_grid(m, HH_COUNTS_BLOCK), HH_COUNTS_BLOCK, [&] { k_hero_hist_counts(dp, out.completions, m); });
    if (out.hist || out.void_) pk_sim::launch(grid, HH_BLOCK, [&] { k_hero_hist(tab, dp, wts, out, bins, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(6)
// k_eqw_cdf, k_eqw_prep, k_eqw<N, RC>: RC is the size class of the case's R, as eqw_launch picks it
template <int N, int RC>
void run_ranged_class(const uint32_t *tab, const uint32_t *cum, const uint64_t *desc, const EqwOut &out, const EqsStream &rng, uint32_t R, unsigned grid,
                      uint32_t ntasks, uint32_t nch, uint32_t per) {
    pk_sim::launch(grid, EQ_BLOCK, [&] { k_eqw<N, RC>(tab, cum, desc, out, rng, R, ntasks, nch, per); });
}
template <int N>
void run_ranged(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t R = (uint32_t)c.num("R", 0);
    EqwPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t);
    if (!tbl) { a.s.holes = c.need<uint8_t>("holes", m * N * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.live = c.need<uint16_t>("live", m); }
    const int per_spot = (int)c.num("per_spot", tbl ? 0 : 1);
    const EqwRanges ranges{R ? c.need<uint16_t>("weights", (size_t)R * EQW_HOLDINGS) : nullptr, R, c.arr<uint16_t>("range_of", (per_spot ? m : (size_t)1) * N), per_spot};
    EqsStream rng{(uint32_t)c.num("key0"), (uint32_t)c.num("key1"), (uint32_t)c.num("nonce"), (uint32_t)c.num("samples"), (uint32_t)c.num("id_base", 0), c.arr<uint32_t>("ids", m)};
    EqwOut out{};
    out.win = c.output<uint32_t>("win", "u32", m * N); out.tie = c.output<uint32_t>("tie", "u32", m * N); out.share = c.output<uint64_t>("share", "u64", m * N);
    out.accepted = c.output<uint32_t>("accepted", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint32_t> cum((size_t)R * EQW_HOLDINGS);
    Work<uint64_t> desc(m * (size_t)eqw_desc_words(N));
    if (R) pk_sim::launch(R, 64, [&] { k_eqw_cdf(ranges.weights, cum.p, R); });
    a.rng = rng; a.r = ranges; a.out = out; a.desc = desc.p; a.N = N; a.observer = (int)c.num("observer", PK_OBSERVER_ACTIVE); a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EQW_PREP_BLOCK), EQW_PREP_BLOCK, [&] { k_eqw_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, EQW_PREP_BLOCK), EQW_PREP_BLOCK, [&] { k_eqw_prep<false>(a); });
    const long long lpt_case = c.num("lpt", 0);
    const uint32_t S = rng.samples, per = 64u * (uint32_t)(lpt_case ? lpt_case : pk::eqs_lpt(m, S)), nch = (S + per - 1) / per, ntasks = (uint32_t)m * nch;
    const int rc = pk::eqw_class(R);
    printf("tasks %u (%u per spot), size class %d\n", ntasks, nch, rc);
    if (rc == 0) run_ranged_class<N, 0>(tab, cum.p, desc.p, out, rng, R, grid, ntasks, nch, per);
    else if (rc == 8) run_ranged_class<N, 8>(tab, cum.p, desc.p, out, rng, R, grid, ntasks, nch, per);
    else run_ranged_class<N, 16>(tab, cum.p, desc.p, out, rng, R, grid, ntasks, nch, per);
}
#endif

#if PK_ES_HAS(7)
// k_ev_prep<N, TABLE>, k_ev<N>, k_ev_finish; the share counters are the caller's array, or a work array when the case does not want them
template <int N>
void run_ev(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const int lpt = (int)c.num("lpt"), pool_max = (int)c.num("pool_max");
    const unsigned grid = (unsigned)c.num("grid");
    EvPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t.t);
    if (tbl) { a.t.bets = (const double *)c.need<uint64_t>("bets", (size_t)N * a.t.t.T); a.t.pending = (const double *)c.need<uint64_t>("pending", (size_t)N * a.t.t.T); }
    else {
        a.s.holes = c.need<uint8_t>("holes", m * N * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.live = c.need<uint16_t>("live", m);
        a.bets = (const double *)c.need<uint64_t>("bets", m * N);
    }
    EvOut out{c.output<uint64_t>("share", "u64", m * N * N), c.output<uint8_t>("level_seat", "u8", m * N), (double *)c.output<uint64_t>("amount", "u64", m * N),
              (double *)c.output<uint64_t>("ev", "u64", m * N), c.output<uint32_t>("boards", "u32", m), c.output<uint8_t>("status", "u8", m)};
    if (!out.status) die("the ev family needs the status output");
    Work<EqCtrl> ctrl(1);
    memset(ctrl.p, 0, sizeof(EqCtrl));                               // (ev_launch's hipMemsetAsync)
    Work<uint64_t> desc(m * (size_t)(3 + N));
    Work<uint32_t> levels(m * N);
    Work<double> wbets(m * N), wamount(m * N);
    Work<uint64_t> wshare(out.share ? 0 : m * N * N);
    Work<uint2> tasks(pk::ev_task_cap(N, m, lpt, pool_max));
    const EvWork w{EqWork{ctrl.p, desc.p, tasks.p, tasks.n}, levels.p, wbets.p, wamount.p, out.share ? out.share : wshare.p};
    a.out = out; a.w = w; a.lpt = lpt; a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EV_PREP_BLOCK), EV_PREP_BLOCK, [&] { k_ev_prep<N, true>(a); });
    else pk_sim::launch(prep_grid(m, EV_PREP_BLOCK), EV_PREP_BLOCK, [&] { k_ev_prep<N, false>(a); });
    printf("tasks %u take %u groups of %d levels\n", ctrl.p->ntasks, ctrl.p->ntasks >= 8u * grid * EQ_WAVES ? 4u : 1u, pk::ev_group(N));
    pk_sim::launch(grid, EQ_BLOCK, [&] { k_ev<N>(tab, w, lpt); });
    pk_sim::launch(prep_grid(m * N, EV_FINISH_BLOCK), EV_FINISH_BLOCK, [&] { k_ev_finish(w, out.ev, N, m); });
}
#endif

#if PK_ES_HAS(11)
// k_eqw_cdf, k_evw_prep<N, TABLE>, k_evw<N, RC>, k_evw_finish: RC is the size class of the case's R, as evw_launch picks it; `share` and
// `accepted` are the caller's arrays, or work arrays when the case does not want them
template <int N, int RC>
void run_rangedev_class(const uint32_t *tab, const EvwWork &w, const EqsStream &rng, uint32_t R, unsigned grid, uint32_t ntasks, uint32_t nch, uint32_t per) {
    pk_sim::launch(grid, EQ_BLOCK, [&] { k_evw<N, RC>(tab, w, rng, R, ntasks, nch, per); });
}
template <int N>
void run_rangedev(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t R = (uint32_t)c.num("R", 0);
    EvwPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t.t);
    if (tbl) { a.t.bets = (const double *)c.need<uint64_t>("bets", (size_t)N * a.t.t.T); a.t.pending = (const double *)c.need<uint64_t>("pending", (size_t)N * a.t.t.T); }
    else {
        a.s.holes = c.need<uint8_t>("holes", m * N * 2); a.s.board = c.need<uint8_t>("board", m * 5); a.s.nboard = c.need<uint8_t>("nboard", m); a.s.live = c.need<uint16_t>("live", m);
        a.bets = (const double *)c.need<uint64_t>("bets", m * N);
    }
    const int per_spot = (int)c.num("per_spot", tbl ? 0 : 1);
    const EqwRanges ranges{R ? c.need<uint16_t>("weights", (size_t)R * EQW_HOLDINGS) : nullptr, R, c.arr<uint16_t>("range_of", (per_spot ? m : (size_t)1) * N), per_spot};
    EqsStream rng{(uint32_t)c.num("key0"), (uint32_t)c.num("key1"), (uint32_t)c.num("nonce"), (uint32_t)c.num("samples"), (uint32_t)c.num("id_base", 0), c.arr<uint32_t>("ids", m)};
    EvwOut out{c.output<uint64_t>("share", "u64", m * N * N), c.output<uint8_t>("level_seat", "u8", m * N), (double *)c.output<uint64_t>("amount", "u64", m * N),
               (double *)c.output<uint64_t>("ev", "u64", m * N), c.output<uint32_t>("accepted", "u32", m), c.output<uint8_t>("status", "u8", m)};
    if (!out.status) die("the rangedev family needs the status output");
    Work<uint32_t> cum((size_t)R * EQW_HOLDINGS);
    Work<uint64_t> desc(m * (size_t)eqw_desc_words(N));
    Work<uint32_t> levels(m * N);
    Work<double> wbets(m * N), wamount(m * N);
    Work<uint64_t> wshare(out.share ? 0 : m * N * N);
    Work<uint32_t> waccepted(out.accepted ? 0 : m);
    const EvwWork w{cum.p, desc.p, levels.p, wbets.p, wamount.p, out.share ? out.share : wshare.p, out.accepted ? out.accepted : waccepted.p};
    if (R) pk_sim::launch(R, 64, [&] { k_eqw_cdf(ranges.weights, cum.p, R); });
    a.rng = rng; a.r = ranges; a.out = out; a.w = w; a.observer = (int)c.num("observer", PK_OBSERVER_ACTIVE); a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, EVW_PREP_BLOCK), EVW_PREP_BLOCK, [&] { k_evw_prep<N, true>(a); });
    else pk_sim::launch(prep_grid(m, EVW_PREP_BLOCK), EVW_PREP_BLOCK, [&] { k_evw_prep<N, false>(a); });
    const long long lpt_case = c.num("lpt", 0);
    const uint32_t S = rng.samples, per = 64u * (uint32_t)(lpt_case ? lpt_case : pk::eqs_lpt(m, S)), nch = (S + per - 1) / per;
    const uint32_t ntasks = (uint32_t)m * nch * (uint32_t)pk::ev_groups_max(N);
    const int rc = pk::eqw_class(R);
    printf("tasks %u (%u chunks x %d groups of %d levels per spot), size class %d\n", ntasks, nch, pk::ev_groups_max(N), pk::ev_group(N), rc);
    if (rc == 0) run_rangedev_class<N, 0>(tab, w, rng, R, grid, ntasks, nch, per);
    else if (rc == 8) run_rangedev_class<N, 8>(tab, w, rng, R, grid, ntasks, nch, per);
    else run_rangedev_class<N, 16>(tab, w, rng, R, grid, ntasks, nch, per);
    pk_sim::launch(prep_grid(m * N, EVW_FINISH_BLOCK), EVW_FINISH_BLOCK, [&] { k_evw_finish(w, out.ev, N, m); });
}
#endif

#if PK_ES_HAS(8)
template <int P = 1, typename F>
void cl_with_pairs(int pairs, F f) {
    if constexpr (P <= CL_ROW_DWORDS) {
        if (pairs == P) f(std::integral_constant<int, P>{}); else cl_with_pairs<P + 1>(pairs, f);
    } else die("pairs outside 1 .. 16");
}
void run_cluster(Case &c) {
    const size_t n = (size_t)c.num("n");
    const int nbins = (int)c.num("nbins"), K = (int)c.num("K"), op = (int)c.num("op"), pairs = pk::cl_pairs(nbins);
    const unsigned grid = (unsigned)c.num("grid");
    const size_t skew = (size_t)c.num("skew", 0);                    // u16 entries before the first row: an array that is not 16-byte aligned
    const uint16_t *hist = c.need<uint16_t>("hist", n * nbins + skew) + skew;
    Work<uint32_t> q(n * pairs), cp((size_t)K * CL_ROW_DWORDS);
    pk_sim::launch(grid, CL_BLOCK, [&] { k_cl_quant(hist, q.p, (uint32_t)nbins, (uint64_t)n); });
    const uint32_t *qp = q.p, *cpp = cp.p;
    auto assign = [&](uint16_t *label, uint32_t *dist, int mode, uint32_t *changed, uint64_t *inertia) {
        cl_with_pairs(pairs, [&](auto pc) {
            pk_sim::launch(grid, CL_BLOCK, [&] { k_cl_assign<decltype(pc)::value>(qp, cpp, (uint32_t)K, (uint64_t)n, label, dist, mode, changed, (cl_u64 *)inertia); });
        });
    };
    if (op == 0) {
        const uint64_t chunk = (uint64_t)c.num("chunk", (long long)pk::cl_chunk_rows(n));
        if (chunk == 0 || chunk % CL_BLOCK) die("chunk: a multiple of the workgroup's width");
        const uint32_t nchunks = (uint32_t)((n + chunk - 1) / chunk);
        Work<uint32_t> mind(n);
        Work<uint64_t> part(nchunks), rows(nchunks);
        uint16_t *cen = c.output<uint16_t>("centroids", "u16", (size_t)K * nbins);
        if (!cen) die("seeding needs the centroids output");
        const uint32_t key0 = (uint32_t)c.num("key0"), key1 = (uint32_t)c.num("key1"), nonce = (uint32_t)c.num("nonce");
        for (int j = 0; j < K; ++j) {
            const uint32_t *newest = j ? cp.p + (size_t)(j - 1) * CL_ROW_DWORDS : nullptr;
            uint64_t *out = j ? part.p : rows.p;
            const int mode = j == 0 ? 0 : (j == 1 ? 1 : 2);
            cl_with_pairs(pairs, [&](auto pc) {
                pk_sim::launch(nchunks, CL_BLOCK, [&] { k_cl_seed_dist<decltype(pc)::value>(qp, newest, mind.p, out, (uint64_t)n, chunk, mode); });
            });
            pk_sim::launch(1, CL_BLOCK, [&] { k_cl_seed_pick(qp, mind.p, part.p, rows.p, nchunks, chunk, (uint64_t)n, (uint32_t)j, key0, key1, nonce, (uint32_t)nbins, cen, cp.p); });
        }
        return;
    }
    const uint16_t *cin = c.need<uint16_t>("centroids", (size_t)K * nbins);
    uint16_t *label = c.output<uint16_t>("label", "u16", n);
    uint32_t *dist = c.output<uint32_t>("dist", "u32", n);
    if (!label) die("assign and cluster need the label output");
    if (op == 1) {
        pk_sim::launch((unsigned)((K * CL_ROW_DWORDS + CL_BLOCK - 1) / CL_BLOCK), CL_BLOCK, [&] { k_cl_pack(cin, cp.p, (uint32_t)nbins, (uint32_t)K); });
        assign(label, dist, 0, nullptr, nullptr);
        return;
    }
    const int iters = (int)c.num("iters");
    uint16_t *cen = c.output<uint16_t>("centroids_out", "u16", (size_t)K * nbins);
    uint64_t *inertia = c.output<uint64_t>("inertia", "u64", (size_t)iters + 1);
    uint32_t *changed = c.output<uint32_t>("changed", "u32", (size_t)iters);
    if (!cen) die("cluster needs the centroids_out output");
    memcpy(cen, cin, (size_t)K * nbins * 2);                         // (in: seeds, out: result)
    Work<uint64_t> sums((size_t)K * nbins);
    Work<uint32_t> counts((size_t)K);
    memset(sums.p, 0, sums.n * 8); memset(counts.p, 0, counts.n * 4);   // (cl_cluster_launch's fills)
    if (inertia) memset(inertia, 0, ((size_t)iters + 1) * 8);
    if (changed) memset(changed, 0, (size_t)iters * 4);
    const bool lds = c.num("lds", (size_t)K * nbins <= (size_t)CL_LDS_SUMS) != 0;
    if (lds && (size_t)K * nbins > (size_t)CL_LDS_SUMS) die("lds: K * nbins does not fit");
    pk_sim::launch((unsigned)((K * CL_ROW_DWORDS + CL_BLOCK - 1) / CL_BLOCK), CL_BLOCK, [&] { k_cl_pack(cin, cp.p, (uint32_t)nbins, (uint32_t)K); });
    for (int t = 0; t < iters; ++t) {
        assign(label, nullptr, t == 0 ? 1 : 2, changed ? changed + t : nullptr, inertia ? inertia + t : nullptr);
        if (lds) pk_sim::launch(grid, CL_BLOCK, [&] { k_cl_update<true>(qp, label, (uint32_t)nbins, (uint32_t)K, (uint64_t)n, (cl_u64 *)sums.p, counts.p); });
        else pk_sim::launch(grid, CL_BLOCK, [&] { k_cl_update<false>(qp, label, (uint32_t)nbins, (uint32_t)K, (uint64_t)n, (cl_u64 *)sums.p, counts.p); });
        pk_sim::launch((unsigned)((K + CL_BLOCK - 1) / CL_BLOCK), CL_BLOCK, [&] { k_cl_finalise((cl_u64 *)sums.p, counts.p, cen, cp.p, (uint32_t)nbins, (uint32_t)K); });
    }
    assign(label, dist, 0, nullptr, inertia ? inertia + iters : nullptr);
}
#endif

#if PK_ES_HAS(10)
// k_pfm_rank, k_pfm_count<STORE>: the launches of pk::pfm_count_launch
void run_preflop(Case &c, const uint32_t *tab) {
    const uint32_t first = (uint32_t)c.num("first"), n = (uint32_t)c.num("n"), chunk = (uint32_t)c.num("chunk");
    const int accumulate = (int)c.num("accumulate", 0);
    uint32_t *win = c.output<uint32_t>("win", "u32", PFM_CELLS), *tie = c.output<uint32_t>("tie", "u32", PFM_CELLS);
    // the key work space holds ONE chunk.  Under ASan it is exactly that; otherwise a run of untouched rows follows it and is looked at
    // afterwards, so that a launch that ranks more boards than a chunk is caught by any build
#if defined(__SANITIZE_ADDRESS__)
    const size_t guard = 0;
#else
    const size_t guard = (size_t)PFM_RUN * PFM_STRIDE;
#endif
    const size_t nkeys = (size_t)chunk * PFM_STRIDE;
    Work<uint32_t> keys(nkeys + guard);
    const uint32_t slice = pk::pfm_slice_boards(chunk);
    bool store = accumulate == 0;
    unsigned launches = 0;
    for (uint32_t pos = first, end = first + n; pos < end;) {
        const uint32_t cap = store && slice < chunk ? slice : chunk, cn = end - pos < cap ? end - pos : cap;
        uint32_t *kp = keys.p;
        pk_sim::launch((cn + PFM_RANK_BOARDS - 1) / PFM_RANK_BOARDS, PFM_RANK_BLOCK, [&] { k_pfm_rank(tab, pos, cn, kp); });
        const unsigned grid = PFM_STRIPS * PFM_STRIPS * ((cn + slice - 1) / slice);
        if (store) pk_sim::launch(grid, PFM_COUNT_BLOCK, [&] { k_pfm_count<true>(kp, cn, slice, win, tie); });
        else pk_sim::launch(grid, PFM_COUNT_BLOCK, [&] { k_pfm_count<false>(kp, cn, slice, win, tie); });
        store = false;
        pos += cn;
        ++launches;
    }
    for (size_t i = 0; i < guard; ++i)
        if (keys.p[nkeys + i] != 0x5A5A5A5Au) die("the key work space of one chunk was overrun at word " + std::to_string(nkeys + i));
    printf("chunks %u (slice %u boards)\n", launches, slice);
}

#endif

#if PK_ES_HAS(10) || PK_ES_HAS(22)
// the readers' table: win, then tie, a fixed pattern
void fill_table(uint32_t *M) {
    for (size_t i = 0; i < PFM_CELLS; ++i) {
        M[i] = ((uint32_t)i * 2654435761u) >> 11;
        M[PFM_CELLS + i] = ((uint32_t)i * 40503u + 7u) & 1023u;
    }
}
#endif

#if PK_ES_HAS(10)

// k_pfm_prep<TABLE>, k_pfm_hero
void run_preflop_hero(Case &c) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const int N = (int)c.num("N", 2);
    PfmPrepArgs a{};
    const bool tbl = table_form(c, N, m, a.t);
    if (!tbl) a.hero = c.need<uint8_t>("hero", m * 2);
    const int per_spot = (int)c.num("per_spot", 0);
    const PfmWeights wts{c.arr<uint16_t>("weights", per_spot ? m * PFM_HOLDINGS : (size_t)PFM_HOLDINGS), per_spot};
    PfmOut out{};
    out.agg = c.output<uint64_t>("agg", "u64", m * 3); out.win = c.output<uint32_t>("win", "u32", m * PFM_HOLDINGS); out.tie = c.output<uint32_t>("tie", "u32", m * PFM_HOLDINGS);
    out.boards = c.output<uint32_t>("boards", "u32", m); out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint32_t> desc(m), M(2 * PFM_CELLS);
    fill_table(M.p);
    a.out = out; a.desc = desc.p; a.N = N; a.observer = (int)c.num("observer", 0); a.m = m;
    if (tbl) pk_sim::launch(prep_grid(m, PFM_PREP_BLOCK), PFM_PREP_BLOCK, [&] { k_pfm_prep<true>(a); });
    else pk_sim::launch(prep_grid(m, PFM_PREP_BLOCK), PFM_PREP_BLOCK, [&] { k_pfm_prep<false>(a); });
    const uint32_t *dp = desc.p, *mp = M.p;
    if (out.agg || out.win || out.tie) pk_sim::launch(grid, PFM_READ_BLOCK, [&] { k_pfm_hero(mp, dp, wts, out, (uint32_t)m); });
}

// k_pfm_rvr: the grid is the kernel's own, PFM_RVR_ROWS rows per workgroup
void run_preflop_rvr(Case &c) {
    const size_t m = (size_t)c.num("m");
    const uint16_t *w = c.arr<uint16_t>("weights", m * PFM_HOLDINGS);
    uint64_t *win = c.output<uint64_t>("win", "u64", m * PFM_HOLDINGS), *tie = c.output<uint64_t>("tie", "u64", m * PFM_HOLDINGS), *tot = c.output<uint64_t>("tot", "u64", m * PFM_HOLDINGS);
    Work<uint32_t> M(2 * PFM_CELLS);
    fill_table(M.p);
    const uint32_t *mp = M.p;
    pk_sim::launch(PFM_HOLDINGS / PFM_RVR_ROWS, PFM_READ_BLOCK, [&] { k_pfm_rvr(mp, w, (uint32_t)m, win, tie, tot); });
}
#endif

#if PK_ES_HAS(12) || PK_ES_HAS(14) || PK_ES_HAS(16) || PK_ES_HAS(18) || PK_ES_HAS(20) || PK_ES_HAS(22)
// nact and row as the host check derives them -> the number of decision nodes
size_t pack_river_tree(RsTree &t, uint32_t n, uint32_t pot, const uint8_t *kind, const uint8_t *child, const uint32_t *put) {
    t = RsTree{};
    t.n = n; t.pot = pot;
    size_t D = 0;
    for (uint32_t v = 0; v < n; ++v) {
        t.kind[v] = kind[v]; t.put[v][0] = put[v * 2]; t.put[v][1] = put[v * 2 + 1];
        for (int a = 0; a < 4; ++a) { t.child[v][a] = child[v * 4 + a]; t.nact[v] += child[v * 4 + a] != 0xFF; }
        if (kind[v] <= RS_P1) t.row[v] = (uint8_t)D++;
    }
    return D;
}
#endif

#if PK_ES_HAS(13) || PK_ES_HAS(15) || PK_ES_HAS(17) || PK_ES_HAS(19) || PK_ES_HAS(21)
// nact, row, river and idx as the host check derives them; D[0] / D[1]: turn-level / river-level decision nodes
void pack_turn_tree(TsTree &t, uint32_t n, uint32_t pot, const uint8_t *kind, const uint8_t *child, const uint32_t *put, size_t (&D)[2]) {
    t = TsTree{};
    t.n = n; t.pot = pot;
    D[0] = D[1] = 0;
    for (uint32_t v = 0; v < n; ++v) {
        t.kind[v] = kind[v]; t.put[v][0] = put[v * 2]; t.put[v][1] = put[v * 2 + 1];
        for (int a = 0; a < 4; ++a) {
            const uint8_t ch = child[v * 4 + a];
            t.child[v][a] = ch; t.nact[v] += ch != 0xFF;
            if (ch != 0xFF && ch < n) t.river[ch] = t.river[v] || kind[v] == TS_CHANCE;
        }
        t.idx[v] = (uint8_t)(t.river[v] ? t.nr++ : t.nt++);
        if (kind[v] <= RS_P1) t.row[v] = (uint8_t)D[t.river[v]]++;
    }
}
#endif

#if PK_ES_HAS(14)
void run_river_trees(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("rivertrees: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.need<uint32_t>("tree_of", m);
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * RS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * RS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * RS_MAX_NODES * 2);
    Work<RsTree> trees(ntrees);                                       // exactly ntrees: an index past them is ASan's to see
    uint32_t nmax = 0;
    size_t Dmax = 0;
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)RS_MAX_NODES) die("rivertrees: n outside 1 .. 64");
        const size_t row = (size_t)k * RS_MAX_NODES;
        Dmax = std::max(Dmax, pack_river_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2));
        nmax = std::max(nmax, n[k]);
    }
    const RsSpots spots{c.need<uint8_t>("board", m * 5), c.arr<uint64_t>("dead", m), c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    RsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * Dmax * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * rs_group_bytes(nmax));              // sized by the grid and the largest tree, as pk_solve_river_trees sizes it
    const RsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_rs_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    const RsTrees tt{trees.p, tree_of, nmax, (uint32_t)Dmax};
    if (out.strategy || out.value || out.br) pk_sim::launch(grid, RS_BLOCK, [&] { k_trees_river_solve(tab, dp, tt, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(22)
// k_preflop_solve: ONE launch, which writes the status too (pk::ps_launch)
void run_preflop_solve(Case &c) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("pfsolve: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * RS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * RS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * RS_MAX_NODES * 2);
    Work<RsTree> trees(ntrees);                                       // exactly ntrees: an index past them is ASan's to see
    uint32_t nmax = 0;
    size_t Dmax = 0;
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)RS_MAX_NODES) die("pfsolve: n outside 1 .. 64");
        const size_t row = (size_t)k * RS_MAX_NODES;
        Dmax = std::max(Dmax, pack_river_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2));
        nmax = std::max(nmax, n[k]);
    }
    const uint16_t *ranges = c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS);
    RsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * Dmax * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    const bool solve = out.strategy || out.value || out.br;
    Work<char> ws(solve ? (size_t)grid * ps_group_bytes(nmax) : 0);   // sized by the grid and the largest tree, as pk_solve_preflop sizes it
    Work<uint32_t> M(2 * PFM_CELLS);
    fill_table(M.p);
    const uint32_t *mp = M.p;
    char *wp = ws.p;
    const RsTrees tt{trees.p, tree_of, nmax, (uint32_t)Dmax};
    pk_sim::launch(grid, PS_BLOCK, [&] { k_preflop_solve(mp, ranges, tt, ntrees, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(15)
void run_turn_trees(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("turntrees: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.need<uint32_t>("tree_of", m);
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * TS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * TS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * TS_MAX_NODES * 2);
    Work<TsTree> trees(ntrees);
    TsTrees tt{trees.p, tree_of, 0, 0, 0, 0};
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)TS_MAX_NODES) die("turntrees: n outside 1 .. 128");
        const size_t row = (size_t)k * TS_MAX_NODES;
        size_t D[2];
        pack_turn_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2, D);
        tt.ntmax = std::max(tt.ntmax, trees.p[k].nt); tt.nrmax = std::max(tt.nrmax, trees.p[k].nr);
        tt.Dtmax = std::max(tt.Dtmax, (uint32_t)D[0]); tt.Drmax = std::max(tt.Drmax, (uint32_t)D[1]);
    }
    const TsSpots spots{c.need<uint8_t>("board", m * 4), c.arr<uint64_t>("dead", m), c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    TsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * tt.Dtmax * 4 * RS_HOLDINGS);
    out.river_strategy = c.output<uint16_t>("river_strategy", "u16", m * tt.Drmax * 52 * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * ts_group_bytes(tt.ntmax, tt.nrmax));  // sized by the grid and the call's largest levels, as pk_solve_turn_trees sizes it
    const TsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, TS_PREP_BLOCK), TS_PREP_BLOCK, [&] { k_ts_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    if (out.strategy || out.river_strategy || out.value || out.br) pk_sim::launch(grid, RS_BLOCK, [&] { k_trees_turn_solve(tab, dp, tt, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(16)
void run_river_lock(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("riverlock: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    if (!tree_of && ntrees != 1) die("riverlock: no tree_of with more than one tree");
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * RS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * RS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * RS_MAX_NODES * 2);
    Work<RsTree> trees(ntrees);
    uint32_t nmax = 0;
    size_t Dmax = 0;
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)RS_MAX_NODES) die("riverlock: n outside 1 .. 64");
        const size_t row = (size_t)k * RS_MAX_NODES;
        Dmax = std::max(Dmax, pack_river_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2));
        nmax = std::max(nmax, n[k]);
    }
    const RsSpots spots{c.need<uint8_t>("board", m * 5), c.arr<uint64_t>("dead", m), c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    const RsLock lk{c.arr<uint8_t>("lock", m * Dmax), c.arr<uint16_t>("locked", m * Dmax * 4 * RS_HOLDINGS)};
    if (lk.lock && !lk.locked) die("riverlock: lock without locked");
    RsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * Dmax * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * rs_group_bytes(nmax));
    const RsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_rs_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    if (tree_of) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    const RsTrees tt{trees.p, tree_of, nmax, (uint32_t)Dmax};
    if (out.strategy || out.value || out.br) pk_sim::launch(grid, RS_BLOCK, [&] { k_lock_river_solve(tab, dp, tt, lk, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(17)
void run_turn_lock(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("turnlock: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    if (!tree_of && ntrees != 1) die("turnlock: no tree_of with more than one tree");
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * TS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * TS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * TS_MAX_NODES * 2);
    Work<TsTree> trees(ntrees);
    TsTrees tt{trees.p, tree_of, 0, 0, 0, 0};
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)TS_MAX_NODES) die("turnlock: n outside 1 .. 128");
        const size_t row = (size_t)k * TS_MAX_NODES;
        size_t D[2];
        pack_turn_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2, D);
        tt.ntmax = std::max(tt.ntmax, trees.p[k].nt); tt.nrmax = std::max(tt.nrmax, trees.p[k].nr);
        tt.Dtmax = std::max(tt.Dtmax, (uint32_t)D[0]); tt.Drmax = std::max(tt.Drmax, (uint32_t)D[1]);
    }
    const TsSpots spots{c.need<uint8_t>("board", m * 4), c.arr<uint64_t>("dead", m), c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    const TsLock lk{c.arr<uint8_t>("lock", m * tt.Dtmax), c.arr<uint16_t>("locked", m * tt.Dtmax * 4 * RS_HOLDINGS), c.arr<uint8_t>("river_lock", m * tt.Drmax),
                    c.arr<uint16_t>("river_locked", m * tt.Drmax * 52 * 4 * RS_HOLDINGS)};
    if ((lk.lock && !lk.locked) || (lk.river_lock && !lk.river_locked)) die("turnlock: a lock array without its locked array");
    TsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * tt.Dtmax * 4 * RS_HOLDINGS);
    out.river_strategy = c.output<uint16_t>("river_strategy", "u16", m * tt.Drmax * 52 * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * ts_group_bytes(tt.ntmax, tt.nrmax));
    const TsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, TS_PREP_BLOCK), TS_PREP_BLOCK, [&] { k_ts_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    if (tree_of) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    if (out.strategy || out.river_strategy || out.value || out.br) pk_sim::launch(grid, RS_BLOCK, [&] { k_lock_turn_solve(tab, dp, tt, lk, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(18)
void run_river_resolve(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("riverresolve: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    if (!tree_of && ntrees != 1) die("riverresolve: no tree_of with more than one tree");
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * RS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * RS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * RS_MAX_NODES * 2);
    Work<RsTree> trees(ntrees);
    uint32_t nmax = 0;
    size_t Dmax = 0;
    bool given_node = false;
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)RS_MAX_NODES) die("riverresolve: n outside 1 .. 64");
        const size_t row = (size_t)k * RS_MAX_NODES;
        Dmax = std::max(Dmax, pack_river_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2));
        nmax = std::max(nmax, n[k]);
        for (uint32_t v = 0; v < n[k]; ++v) given_node = given_node || kind[row + v] == RS_GIVEN;
    }
    const RsSpots spots{c.need<uint8_t>("board", m * 5), c.arr<uint64_t>("dead", m), c.arr<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    const RsLock lk{c.arr<uint8_t>("lock", m * Dmax), c.arr<uint16_t>("locked", m * Dmax * 4 * RS_HOLDINGS)};
    if (lk.lock && !lk.locked) die("riverresolve: lock without locked");
    RsResolve rz{c.arr<uint32_t>("reach", m * 2 * RS_HOLDINGS), (const int64_t *)c.arr<uint64_t>("given", m * 2 * RS_HOLDINGS), c.arr<uint8_t>("at", m), nullptr, nullptr, nullptr};
    if (!spots.ranges && !rz.reach) die("riverresolve: neither ranges nor reach");
    if (given_node && !rz.given) die("riverresolve: a given node without given");
    RsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * Dmax * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    rz.node_reach = c.output<uint32_t>("node_reach", "u32", m * 2 * RS_HOLDINGS);
    rz.node_value = (int64_t *)c.output<uint64_t>("node_value", "u64", m * 2 * RS_HOLDINGS);
    rz.node_br = (int64_t *)c.output<uint64_t>("node_br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    if ((rz.at != nullptr) != (rz.node_reach || rz.node_value || rz.node_br)) die("riverresolve: at comes with a node output, and only with one");
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * rs_group_bytes(nmax));
    const RsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_rs_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    if (tree_of) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const ResolvePrepArgs ra{(const char *)trees.p, (uint32_t)sizeof(RsTree), 0u, tree_of, rz.at, nullptr, dw, st, m};
    if (rz.at) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_resolve_prep(ra); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    const RsTrees tt{trees.p, tree_of, nmax, (uint32_t)Dmax};
    if (out.strategy || out.value || out.br || rz.at) pk_sim::launch(grid, RS_BLOCK, [&] { k_resolve_river_solve(tab, dp, tt, lk, rz, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(19)
void run_turn_resolve(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("turnresolve: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    if (!tree_of && ntrees != 1) die("turnresolve: no tree_of with more than one tree");
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * TS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * TS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * TS_MAX_NODES * 2);
    Work<TsTree> trees(ntrees);
    TsTrees tt{trees.p, tree_of, 0, 0, 0, 0};
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)TS_MAX_NODES) die("turnresolve: n outside 1 .. 128");
        const size_t row = (size_t)k * TS_MAX_NODES;
        size_t D[2];
        pack_turn_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2, D);
        tt.ntmax = std::max(tt.ntmax, trees.p[k].nt); tt.nrmax = std::max(tt.nrmax, trees.p[k].nr);
        tt.Dtmax = std::max(tt.Dtmax, (uint32_t)D[0]); tt.Drmax = std::max(tt.Drmax, (uint32_t)D[1]);
    }
    const TsSpots spots{c.need<uint8_t>("board", m * 4), c.arr<uint64_t>("dead", m), c.arr<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    const TsLock lk{c.arr<uint8_t>("lock", m * tt.Dtmax), c.arr<uint16_t>("locked", m * tt.Dtmax * 4 * RS_HOLDINGS), c.arr<uint8_t>("river_lock", m * tt.Drmax),
                    c.arr<uint16_t>("river_locked", m * tt.Drmax * 52 * 4 * RS_HOLDINGS)};
    if ((lk.lock && !lk.locked) || (lk.river_lock && !lk.river_locked)) die("turnresolve: a lock array without its locked array");
    TsResolve rz{c.arr<uint32_t>("reach", m * 2 * RS_HOLDINGS), c.arr<uint8_t>("at", m), c.arr<uint8_t>("at_card", m), nullptr, nullptr, nullptr};
    if (!spots.ranges && !rz.reach) die("turnresolve: neither ranges nor reach");
    TsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * tt.Dtmax * 4 * RS_HOLDINGS);
    out.river_strategy = c.output<uint16_t>("river_strategy", "u16", m * tt.Drmax * 52 * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    rz.node_reach = c.output<uint32_t>("node_reach", "u32", m * 2 * RS_HOLDINGS);
    rz.node_value = (int64_t *)c.output<uint64_t>("node_value", "u64", m * 2 * RS_HOLDINGS);
    rz.node_br = (int64_t *)c.output<uint64_t>("node_br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    if ((rz.at != nullptr) != (rz.node_reach || rz.node_value || rz.node_br)) die("turnresolve: at comes with a node output, and only with one");
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * ts_group_bytes(tt.ntmax, tt.nrmax));
    const TsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, TS_PREP_BLOCK), TS_PREP_BLOCK, [&] { k_ts_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    if (tree_of) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const ResolvePrepArgs ra{(const char *)trees.p, (uint32_t)sizeof(TsTree), (uint32_t)offsetof(TsTree, river), tree_of, rz.at, rz.at_card, dw, st, m};
    if (rz.at) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_resolve_prep(ra); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    if (out.strategy || out.river_strategy || out.value || out.br || rz.at)
        pk_sim::launch(grid, RS_BLOCK, [&] { k_resolve_turn_solve(tab, dp, tt, lk, rz, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(20)
// The riverresume family (k_resume_prep, k_resume_river_solve): what riverresolve takes, and t0 u32 [m] (optional), regret / average
// u64 [m][Dmax][4][1326], which go in and come out.  The solve kernel always runs: the state is an output.
void run_river_resume(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("riverresume: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    if (!tree_of && ntrees != 1) die("riverresume: no tree_of with more than one tree");
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * RS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * RS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * RS_MAX_NODES * 2);
    Work<RsTree> trees(ntrees);
    uint32_t nmax = 0;
    size_t Dmax = 0;
    bool given_node = false;
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)RS_MAX_NODES) die("riverresume: n outside 1 .. 64");
        const size_t row = (size_t)k * RS_MAX_NODES;
        Dmax = std::max(Dmax, pack_river_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2));
        nmax = std::max(nmax, n[k]);
        for (uint32_t v = 0; v < n[k]; ++v) given_node = given_node || kind[row + v] == RS_GIVEN;
    }
    const RsSpots spots{c.need<uint8_t>("board", m * 5), c.arr<uint64_t>("dead", m), c.arr<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    const RsLock lk{c.arr<uint8_t>("lock", m * Dmax), c.arr<uint16_t>("locked", m * Dmax * 4 * RS_HOLDINGS)};
    if (lk.lock && !lk.locked) die("riverresume: lock without locked");
    RsResolve rz{c.arr<uint32_t>("reach", m * 2 * RS_HOLDINGS), (const int64_t *)c.arr<uint64_t>("given", m * 2 * RS_HOLDINGS), c.arr<uint8_t>("at", m), nullptr, nullptr, nullptr};
    if (!spots.ranges && !rz.reach) die("riverresume: neither ranges nor reach");
    if (given_node && !rz.given) die("riverresume: a given node without given");
    const RsResume rm{c.arr<uint32_t>("t0", m), (int64_t *)c.inout<uint64_t>("regret", m * Dmax * 4 * RS_HOLDINGS), (int64_t *)c.inout<uint64_t>("average", m * Dmax * 4 * RS_HOLDINGS)};
    if (!rm.regret || !rm.average) die("riverresume: the case has no state");
    RsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * Dmax * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    rz.node_reach = c.output<uint32_t>("node_reach", "u32", m * 2 * RS_HOLDINGS);
    rz.node_value = (int64_t *)c.output<uint64_t>("node_value", "u64", m * 2 * RS_HOLDINGS);
    rz.node_br = (int64_t *)c.output<uint64_t>("node_br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    if ((rz.at != nullptr) != (rz.node_reach || rz.node_value || rz.node_br)) die("riverresume: at comes with a node output, and only with one");
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * rs_group_bytes(nmax));
    const RsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_rs_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    if (tree_of) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const ResolvePrepArgs ra{(const char *)trees.p, (uint32_t)sizeof(RsTree), 0u, tree_of, rz.at, nullptr, dw, st, m};
    if (rz.at) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_resolve_prep(ra); });
    const uint32_t *t0 = rm.t0;
    if (t0) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_resume_prep(t0, iters, dw, st, m); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    const RsTrees tt{trees.p, tree_of, nmax, (uint32_t)Dmax};
    pk_sim::launch(grid, RS_BLOCK, [&] { k_resume_river_solve(tab, dp, tt, lk, rz, rm, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(21)
// The turnresume family (k_resume_prep, k_resume_turn_solve): what turnresolve takes, and t0, regret / average u64 [m][Dtmax][4][1326], river_regret /
// river_average u64 [m][Drmax][52][4][1326], which go in and come out.
void run_turn_resume(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t ntrees = (uint32_t)c.num("ntrees"), iters = (uint32_t)c.num("iters");
    if (ntrees < 1 || grid < 1) die("turnresume: no tree, or no workgroup");
    const uint32_t *n = c.need<uint32_t>("n", ntrees), *pot = c.need<uint32_t>("pot", ntrees), *tree_of = c.arr<uint32_t>("tree_of", m);
    if (!tree_of && ntrees != 1) die("turnresume: no tree_of with more than one tree");
    const uint8_t *kind = c.need<uint8_t>("kind", (size_t)ntrees * TS_MAX_NODES), *child = c.need<uint8_t>("child", (size_t)ntrees * TS_MAX_NODES * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)ntrees * TS_MAX_NODES * 2);
    Work<TsTree> trees(ntrees);
    TsTrees tt{trees.p, tree_of, 0, 0, 0, 0};
    for (uint32_t k = 0; k < ntrees; ++k) {
        if (n[k] < 1 || n[k] > (uint32_t)TS_MAX_NODES) die("turnresume: n outside 1 .. 128");
        const size_t row = (size_t)k * TS_MAX_NODES;
        size_t D[2];
        pack_turn_tree(trees.p[k], n[k], pot[k], kind + row, child + row * 4, put + row * 2, D);
        tt.ntmax = std::max(tt.ntmax, trees.p[k].nt); tt.nrmax = std::max(tt.nrmax, trees.p[k].nr);
        tt.Dtmax = std::max(tt.Dtmax, (uint32_t)D[0]); tt.Drmax = std::max(tt.Drmax, (uint32_t)D[1]);
    }
    const TsSpots spots{c.need<uint8_t>("board", m * 4), c.arr<uint64_t>("dead", m), c.arr<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    const TsLock lk{c.arr<uint8_t>("lock", m * tt.Dtmax), c.arr<uint16_t>("locked", m * tt.Dtmax * 4 * RS_HOLDINGS), c.arr<uint8_t>("river_lock", m * tt.Drmax),
                    c.arr<uint16_t>("river_locked", m * tt.Drmax * 52 * 4 * RS_HOLDINGS)};
    if ((lk.lock && !lk.locked) || (lk.river_lock && !lk.river_locked)) die("turnresume: a lock array without its locked array");
    TsResolve rz{c.arr<uint32_t>("reach", m * 2 * RS_HOLDINGS), c.arr<uint8_t>("at", m), c.arr<uint8_t>("at_card", m), nullptr, nullptr, nullptr};
    if (!spots.ranges && !rz.reach) die("turnresume: neither ranges nor reach");
    const size_t trows = m * tt.Dtmax * 4 * RS_HOLDINGS, rrows = m * tt.Drmax * 52 * 4 * RS_HOLDINGS;
    const TsResume rm{c.arr<uint32_t>("t0", m), (int64_t *)c.inout<uint64_t>("regret", trows), (int64_t *)c.inout<uint64_t>("average", trows),
                      (int64_t *)c.inout<uint64_t>("river_regret", rrows), (int64_t *)c.inout<uint64_t>("river_average", rrows)};
    if (!rm.regret || !rm.average || !rm.river_regret || !rm.river_average) die("turnresume: the case has no state");
    TsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", trows);
    out.river_strategy = c.output<uint16_t>("river_strategy", "u16", rrows);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    rz.node_reach = c.output<uint32_t>("node_reach", "u32", m * 2 * RS_HOLDINGS);
    rz.node_value = (int64_t *)c.output<uint64_t>("node_value", "u64", m * 2 * RS_HOLDINGS);
    rz.node_br = (int64_t *)c.output<uint64_t>("node_br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    if ((rz.at != nullptr) != (rz.node_reach || rz.node_value || rz.node_br)) die("turnresume: at comes with a node output, and only with one");
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * ts_group_bytes(tt.ntmax, tt.nrmax));
    const TsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, TS_PREP_BLOCK), TS_PREP_BLOCK, [&] { k_ts_prep(a); });
    uint64_t *dw = desc.p;
    uint8_t *st = out.status;
    if (tree_of) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_trees_prep(tree_of, ntrees, dw, st, m); });
    const ResolvePrepArgs ra{(const char *)trees.p, (uint32_t)sizeof(TsTree), (uint32_t)offsetof(TsTree, river), tree_of, rz.at, rz.at_card, dw, st, m};
    if (rz.at) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_resolve_prep(ra); });
    const uint32_t *t0 = rm.t0;
    if (t0) pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_resume_prep(t0, iters, dw, st, m); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    pk_sim::launch(grid, RS_BLOCK, [&] { k_resume_turn_solve(tab, dp, tt, lk, rz, rm, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(12)
void run_river(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t n = (uint32_t)c.num("n"), iters = (uint32_t)c.num("iters");
    if (n < 1 || n > (uint32_t)RS_MAX_NODES || grid < 1) die("riversolve: n outside 1 .. 64, or no workgroup");
    const uint8_t *kind = c.need<uint8_t>("kind", n), *child = c.need<uint8_t>("child", (size_t)n * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)n * 2);
    RsTree t;
    const size_t D = pack_river_tree(t, n, (uint32_t)c.num("pot"), kind, child, put);
    const RsSpots spots{c.need<uint8_t>("board", m * 5), c.arr<uint64_t>("dead", m), c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    RsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * D * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * rs_group_bytes(n));                 // sized by the grid, as pk::rs_work_bytes sizes it
    const RsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, RS_PREP_BLOCK), RS_PREP_BLOCK, [&] { k_rs_prep(a); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    if (out.strategy || out.value || out.br) pk_sim::launch(grid, RS_BLOCK, [&] { k_river_solve(tab, dp, t, spots, out, wp, iters, (uint32_t)m); });
}
#endif

#if PK_ES_HAS(13)
void run_turn(Case &c, const uint32_t *tab) {
    const size_t m = (size_t)c.num("m");
    const unsigned grid = (unsigned)c.num("grid");
    const uint32_t n = (uint32_t)c.num("n"), iters = (uint32_t)c.num("iters");
    if (n < 1 || n > (uint32_t)TS_MAX_NODES || grid < 1) die("turnsolve: n outside 1 .. 128, or no workgroup");
    const uint8_t *kind = c.need<uint8_t>("kind", n), *child = c.need<uint8_t>("child", (size_t)n * 4);
    const uint32_t *put = c.need<uint32_t>("put", (size_t)n * 2);
    TsTree t;
    size_t D[2];
    pack_turn_tree(t, n, (uint32_t)c.num("pot"), kind, child, put, D);
    const TsSpots spots{c.need<uint8_t>("board", m * 4), c.arr<uint64_t>("dead", m), c.need<uint16_t>("ranges", m * 2 * RS_HOLDINGS)};
    TsOut out{};
    out.strategy = c.output<uint16_t>("strategy", "u16", m * D[0] * 4 * RS_HOLDINGS);
    out.river_strategy = c.output<uint16_t>("river_strategy", "u16", m * D[1] * 52 * 4 * RS_HOLDINGS);
    out.value = (int64_t *)c.output<uint64_t>("value", "u64", m * 2 * RS_HOLDINGS);
    out.br = (int64_t *)c.output<uint64_t>("br", "u64", m * 2 * RS_HOLDINGS);
    out.status = c.output<uint8_t>("status", "u8", m);
    Work<uint64_t> desc(m * RS_DESC_WORDS);
    Work<char> ws((size_t)grid * ts_group_bytes(t.nt, t.nr));       // sized by the grid, as pk::ts_work_bytes sizes it
    const TsPrepArgs a{spots, out.status, desc.p, m};
    pk_sim::launch(prep_grid(m, TS_PREP_BLOCK), TS_PREP_BLOCK, [&] { k_ts_prep(a); });
    const uint64_t *dp = desc.p;
    char *wp = ws.p;
    if (out.strategy || out.river_strategy || out.value || out.br) pk_sim::launch(grid, RS_BLOCK, [&] { k_turn_solve(tab, dp, t, spots, out, wp, iters, (uint32_t)m); });
}
#endif

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) die("usage: equity_sim <case file> <out file>");
    Case c(argv[1]);
    // the function-local __shared__ arrays of the main kernels (the preparation kernels have none)
    const size_t lds = pk_sim::lds_find({"8k_equityILi", "5k_eqsILi", "5k_eqrPKj", "5k_rvrPKj", "6k_histPKj", "11k_hero_histPKj", "5k_eqwILi", "4k_evILi", "5k_evwILi", "10k_cl_quant", "11k_cl_assign",
                                        "11k_cl_update", "14k_cl_seed_dist", "14k_cl_seed_pick", "10k_pfm_rank", "11k_pfm_count", "10k_pfm_hero", "9k_pfm_rvr", "13rs_solve_bodyILb", "13ts_solve_bodyILb", "15k_preflop_solve"});
    Work<uint32_t> tab(EVAL7_TAB_WORDS);
    for (int i = 0; i < EVAL7_TAB_WORDS; ++i) tab.p[i] = eval7_tab_entry((uint32_t)i);
    const auto t0 = std::chrono::steady_clock::now();
    const int N = (int)c.num("N", 2);
    bool ran = false;
    (void)N;
#if PK_ES_HAS(1)
    if (c.family == "equity") {
        if (N == 2) run_equity<2>(c, tab.p); else if (N == 3) run_equity<3>(c, tab.p); else if (N == 9) run_equity<9>(c, tab.p); else if (N == 16) run_equity<16>(c, tab.p);
        else die("k_equity<N>: this build has N = 2, 3, 9, 16");
        ran = true;
    }
#endif
#if PK_ES_HAS(2)
    if (c.family == "sampled") {
        if (N == 2) run_sampled<2>(c, tab.p); else if (N == 6) run_sampled<6>(c, tab.p); else if (N == 16) run_sampled<16>(c, tab.p);
        else die("k_eqs<N>: this build has N = 2, 6, 16");
        ran = true;
    }
#endif
#if PK_ES_HAS(3)
    if (c.family == "range") { run_range(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(4)
    if (c.family == "rvr") { run_rvr(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(5)
    if (c.family == "hist") { run_hist(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(6)
    if (c.family == "ranged") {
        if (N == 2) run_ranged<2>(c, tab.p); else if (N == 3) run_ranged<3>(c, tab.p); else if (N == 6) run_ranged<6>(c, tab.p); else if (N == 16) run_ranged<16>(c, tab.p);
        else die("k_eqw<N, RC>: this build has N = 2, 3, 6, 16");
        ran = true;
    }
#endif
#if PK_ES_HAS(7)
    if (c.family == "ev") {
        if (N == 2) run_ev<2>(c, tab.p); else if (N == 3) run_ev<3>(c, tab.p); else if (N == 5) run_ev<5>(c, tab.p); else if (N == 9) run_ev<9>(c, tab.p); else if (N == 16) run_ev<16>(c, tab.p);
        else die("k_ev<N>: this build has N = 2, 3, 5, 9, 16");
        ran = true;
    }
#endif
#if PK_ES_HAS(11)
    if (c.family == "rangedev") {
        if (N == 2) run_rangedev<2>(c, tab.p); else if (N == 3) run_rangedev<3>(c, tab.p); else if (N == 5) run_rangedev<5>(c, tab.p); else if (N == 9) run_rangedev<9>(c, tab.p);
        else if (N == 16) run_rangedev<16>(c, tab.p);
        else die("k_evw<N, RC>: this build has N = 2, 3, 5, 9, 16");
        ran = true;
    }
#endif
#if PK_ES_HAS(8)
    if (c.family == "cluster") { run_cluster(c); ran = true; }
#endif
#if PK_ES_HAS(9)
    if (c.family == "herohist") { run_hero_hist(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(10)
    if (c.family == "preflop") { run_preflop(c, tab.p); ran = true; }
    if (c.family == "pfhero") { run_preflop_hero(c); ran = true; }
    if (c.family == "pfrvr") { run_preflop_rvr(c); ran = true; }
#endif
#if PK_ES_HAS(12)
    if (c.family == "riversolve") { run_river(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(13)
    if (c.family == "turnsolve") { run_turn(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(14)
    if (c.family == "rivertrees") { run_river_trees(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(15)
    if (c.family == "turntrees") { run_turn_trees(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(16)
    if (c.family == "riverlock") { run_river_lock(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(17)
    if (c.family == "turnlock") { run_turn_lock(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(18)
    if (c.family == "riverresolve") { run_river_resolve(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(19)
    if (c.family == "turnresolve") { run_turn_resolve(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(20)
    if (c.family == "riverresume") { run_river_resume(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(21)
    if (c.family == "turnresume") { run_turn_resume(c, tab.p); ran = true; }
#endif
#if PK_ES_HAS(22)
    if (c.family == "pfsolve") { run_preflop_solve(c); ran = true; }
#endif
    if (!ran) die("family " + c.family + ": not in this build");
    c.write(argv[2]);
    printf("equity_sim: %s done: %zu LDS bytes in %zu arrays refilled per workgroup, %llu __syncthreads, %llu wave collectives  [%.2f s]\n", c.family.c_str(), lds,
           pk_sim::g_lds.size(), pk_sim::g.barriers, pk_sim::g.rendezvous, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
