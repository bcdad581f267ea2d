#!/bin/bash
# Dev-only: the 8-wave CPU build of the equity kernels (equity_sim.cpp on wg_shim.h) under ASan + UBSan and under TSan, EVERY case of
# equity_cases.py -- all_cases(), the ranged family's ranged_cases(), the EV family's ev_cases(), the ranged EV's ranged_ev_cases(), the histogram clustering's cluster_cases(), the hero histograms' hero_hist_cases(), the pre-flop count pass's preflop_cases() the river solver's river_cases(), the turn solver's turn_cases() and the tree-per-spot solvers' river_trees_cases() and turn_trees_cases() and the locked solvers' river_lock_cases() and turn_lock_cases() and the re-solving calls' river_resolve_cases() and turn_resolve_cases() and the pre-flop solver's pfsolve_cases() -- on both builds, each compared with the numpy specs; exits 0 only if
# every case on both builds does.  Stand-alone programs, run directly on the CPU; the two builds are compiled side by side (2 jobs, never more
# than 16).  The committed outputs: profiles/equity_sim_sanitizers.txt (the five earlier families) and, from `--only ranged`,
# profiles/equity_ranged_sim_sanitizers.txt, and from `--only ev-` profiles/equity_ev_sim_sanitizers.txt, and from `--only evw-` profiles/ranged_ev_sim_sanitizers.txt, and from `--only cluster` profiles/hist_cluster_sim_sanitizers.txt, and from `--only herohist` profiles/hero_hist_sim_sanitizers.txt, and from `--only preflop` profiles/preflop_sim_sanitizers.txt, and from `--only rsolve` profiles/river_solver_sim_sanitizers.txt, and from `--only tsolve` profiles/turn_solver_sim_sanitizers.txt, and from `--only trees` profiles/solver_trees_sim_sanitizers.txt, and from `--only lock-` profiles/solver_lock_sim_sanitizers.txt, and from `--only res-` profiles/solver_resolve_sim_sanitizers.txt, and from `--only sum-` (the resuming calls' river_resume_cases() and turn_resume_cases()) profiles/solver_resume_sim_sanitizers.txt, and from `--only arith-` (the solvers' arithmetic: river_arith_cases() and turn_arith_cases()) profiles/solver_arith_sim_sanitizers.txt, and from `--only pfsolve` (the pre-flop solver: pfsolve_cases()) profiles/preflop_solver_sim_sanitizers.txt.
#   tools/host_sim/sanitize_equity.sh [out-dir] [equity_cases.py options, e.g. --only rvr]      (default out-dir /tmp/equity_sim_san)
set -e -o pipefail
cd "$(dirname "$0")/../.."
OUT=${1:-/tmp/equity_sim_san}
shift || true
JOBS=${PK_BUILD_JOBS:-$(n=$(nproc); echo $(( n < 16 ? n : 16 )))}
mkdir -p "$OUT"
CXX="g++ -std=c++20 -O1 -g -ffp-contract=off -fno-omit-frame-pointer -DPK_HOST_SIM -I tools/host_sim/stub -include tools/host_sim/wg_shim.h"
t0=$SECONDS
printf '%s\n' "asan -fsanitize=address,undefined -fno-sanitize-recover=undefined" "tsan -fsanitize=thread" | xargs -P "$JOBS" -L 1 sh -c \
    "$CXX \$1 \$2 tools/host_sim/equity_sim.cpp -o $OUT/equity_sim_\$0 2>$OUT/build_\$0.log" \
    || { for f in "$OUT"/build_*.log; do [ -s "$f" ] && { echo "== $f"; cat "$f"; }; done; echo "build FAILED"; exit 1; }
$CXX -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/host_sim/wg_shim_selftest.cpp -o "$OUT/selftest_asan"
$CXX -fsanitize=thread tools/host_sim/wg_shim_selftest.cpp -o "$OUT/selftest_tsan"
echo "build asan + tsan: $((SECONDS - t0)) s ($JOBS jobs at most)"
g++ --version | head -1
export UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 ASAN_OPTIONS=detect_leaks=1 TSAN_OPTIONS=halt_on_error=1:second_deadlock_stack=1
# the shim against itself: clean on both builds; a missing barrier between waves must be a race TSan reports (that run is MEANT to fail)
"$OUT/selftest_asan" ok
"$OUT/selftest_tsan" ok
for mode in race race-ahead; do
    if "$OUT/selftest_tsan" $mode >"$OUT/selftest_$mode.log" 2>&1; then echo "wg_shim_selftest $mode: TSan reported NO race"; exit 1; fi
    grep -q "ThreadSanitizer: data race" "$OUT/selftest_$mode.log" || { cat "$OUT/selftest_$mode.log"; exit 1; }
    echo "wg_shim_selftest $mode: TSan reports the race (as it must)"
done
t0=$SECONDS
python3 tools/host_sim/equity_cases.py --exe "$OUT/equity_sim_asan" --exe "$OUT/equity_sim_tsan" --keep "$OUT/cases" "$@"
echo "run asan + tsan: $((SECONDS - t0)) s"
