#!/bin/bash
# One visit to the GPU box: GPU test-suite (all failures reported), smoke, small bench.  Logs land in $GPU_CI_OUT (default ci_out/).
out="${GPU_CI_OUT:-ci_out}"
mkdir -p "$out"
export TMPDIR=/tmp
echo "== rocm-smi" > "$out/env.log"; rocm-smi --showproductname 2>&1 | head -20 >> "$out/env.log"; nproc >> "$out/env.log"
timeout 1500 python -m pytest tests -m gpu -q -rA -p no:cacheprovider 2>&1 | tail -150 > "$out/pytest_gpu.log"
echo "pytest exit: $?" >> "$out/pytest_gpu.log"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > "$out/smoke.log" 2>&1
echo "smoke exit: $?" >> "$out/smoke.log"
timeout 600 python bench.py --full --views ${BENCH_VIEWS:-20} --steps 2 --warmup 1 > "$out/bench_small.log" 2>&1
echo "bench exit: $?" >> "$out/bench_small.log"
tail -5 "$out/pytest_gpu.log"; tail -3 "$out/smoke.log"; tail -3 "$out/bench_small.log"
# the distributed code path of bench.py (RCCL init, view sharding, barrier, MAX all-reduce) in a world of one rank
F3R_BENCH_FORCE_DIST=1 timeout 600 python bench.py --full --views ${BENCH_VIEWS:-20} --steps 1 --warmup 1 --no-cpu-baseline > "$out/bench_forced_dist.log" 2>&1
echo "forced-dist bench exit: $?" >> "$out/bench_forced_dist.log"
tail -2 "$out/bench_forced_dist.log"
