#!/bin/bash
# Runs ON THE GPU BOX: the bench lines DESIGN.md section 6 quotes (no profiling; tools/refresh_round.sh does both).
# usage: RES=<folder for the bench lines> tools/refresh_bench_lines.sh <round tag>
set -u
R=$1
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
cd $ROOT
RES=${RES:?"set RES to the folder for the bench lines"}
python bench.py --gpus 1 --steps 20 --warmup 5 > "$RES"/${R}_bench_driver.json 2> "$RES"/${R}_bench_driver.err
python bench.py --full > "$RES"/${R}_bench_65536x6.json 2>/dev/null
python bench.py --full --gpus 1 --chunk 20 --steps 3670100 --warmup 5 --coalesce 0 --no-cpu-baseline --no-evaluator > "$RES"/${R}_bench_driver_nocoalesce.json 2>/dev/null
python bench.py --full --players 9 --policy allin --no-cpu-baseline --no-evaluator > "$RES"/${R}_bench_65536x9_allin.json 2>/dev/null
python bench.py --full --tables 4096 --players 2 --no-cpu-baseline --no-evaluator > "$RES"/${R}_bench_4096x2.json 2>/dev/null
python bench.py --full --tables 1048576 --no-cpu-baseline --no-evaluator --samples 3 --steps 24576 > "$RES"/${R}_bench_1048576x6.json 2>/dev/null
python bench.py --full --unfused --steps 1536 --warmup 64 --no-cpu-baseline --no-evaluator --samples 3 > "$RES"/${R}_bench_65536x6_unfused.json 2>/dev/null
python bench.py --mode env --steps 200 --warmup 20 2>/dev/null | tail -1 > "$RES"/${R}_bench_env.json
python bench.py --mode env --steps 200 --warmup 20 --env-batches 4 2>/dev/null | tail -1 > "$RES"/${R}_bench_env_sync_batches4.json
python bench.py --mode env --steps 2000 --warmup 200 --env-async 8 2>/dev/null | tail -1 > "$RES"/${R}_bench_env_async8_batches1.json
python bench.py --mode env --steps 2000 --warmup 200 --env-async 8 --env-batches 4 2>/dev/null | tail -1 > "$RES"/${R}_bench_env_async8_batches4.json
python bench.py --mode env --steps 2000 --warmup 200 --env-async 8 --tables 524288 --env-inner-batches 3 2>/dev/null | tail -1 > "$RES"/${R}_bench_env_async8_inner3_524288.json
python tools/launch_overhead.py > "$RES"/${R}_launch_overhead.txt 2>&1
python tools/measure_api.py > "$RES"/${R}_measure_api.txt 2>&1
echo refreshed bench lines $R
