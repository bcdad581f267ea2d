#!/bin/bash
# Dev-only: the 64-lane CPU build of the table kernels' bodies (wave_sim.cpp on wave_shim.h) under ASan + UBSan and under TSan, every
# configuration of the driver and the step families' deep variant, all must exit 0.  One translation unit per family and seat group, at most 16 compiles at once.
#   tools/host_sim/sanitize_wave.sh [out-dir]        (default /tmp/wave_sim_san; prints build and run times)
set -e -o pipefail
cd "$(dirname "$0")/../.."
OUT=${1:-/tmp/wave_sim_san}
JOBS=${PK_BUILD_JOBS:-$(n=$(nproc); echo $(( n < 16 ? n : 16 )))}
mkdir -p "$OUT"
CXX="g++ -std=c++20 -O1 -g -pthread -ffp-contract=off -fno-omit-frame-pointer -DPK_HOST_SIM -include tools/host_sim/wave_shim.h"
build() {   # name, sanitizer flags
    local name=$1 san=$2 t0=$SECONDS
    gcc -O1 -g -std=gnu11 -ffp-contract=off $san -c oracle/pokerl_oracle.c -o "$OUT/oracle_$name.o"
    printf '%s\n' 0 1 2 3 4 5 6 7 8 9 10 11 | xargs -P "$JOBS" -I{} sh -c \
        "$CXX $san -DPK_WS_PART={} \$([ {} = 0 ] && echo -DPK_WS_MAIN) -c tools/host_sim/wave_sim.cpp -o $OUT/part{}_$name.o 2>$OUT/part{}_$name.log" \
        || { for f in "$OUT"/part*_"$name".log; do [ -s "$f" ] && { echo "== $f"; cat "$f"; }; done; echo "build $name FAILED"; exit 1; }
    g++ -pthread $san "$OUT"/part*_"$name".o "$OUT/oracle_$name.o" -o "$OUT/wave_sim_$name"
    echo "build $name: $((SECONDS - t0)) s ($JOBS jobs)"
}
run() {
    local name=$1 t0=$SECONDS
    "$OUT/wave_sim_$name"
    "$OUT/wave_sim_$name" --deep --steps 120      # the step families on the never-fold caller's actions (deep hands)
    echo "run $name: $((SECONDS - t0)) s"
}
build asan "-fsanitize=address,undefined -fno-sanitize-recover=undefined"
build tsan "-fsanitize=thread"
UBSAN_OPTIONS=print_stacktrace=1 run asan
run tsan
