#!/bin/bash
# GPU tests + forced-distributed bench path at world size 1 + the full bench; logs go to OUT_DIR; stops at the first failing step
O=${1:?usage: tools/gpu_check.sh OUT_DIR}
mkdir -p "$O"
timeout -k 10 400 python -m pytest tests -q -m gpu > "$O/pytest_gpu.log" 2>&1; rc=$?; echo "pytest rc=$rc"; tail -5 "$O/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
NERF_BENCH_FORCE_DIST=1 timeout -k 10 200 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 2 --warmup 1 --no-cpu-baseline > "$O/bench_dist1.json" 2> "$O/bench_dist1.err"; rc=$?; echo "dist bench rc=$rc"; tail -3 "$O/bench_dist1.err"; cut -c1-400 "$O/bench_dist1.json"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$O/bench_full.json" 2> "$O/bench_full.err"; rc=$?; echo "bench rc=$rc"; [ $rc -eq 0 ] || { tail -5 "$O/bench_full.err"; exit $rc; }
python3 -c "import sys,json; d=json.loads(open(sys.argv[1]).read()); print(d['value'], d['roofline']['frac'], d['roofline']['traffic'], d['cpu_baseline'])" "$O/bench_full.json"
