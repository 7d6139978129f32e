#!/bin/bash
# bench.py ms/step for the variants of the query-stationary scan (same box, alternating)
cd "$(dirname "$0")/.."
mkdir -p gpurun_out/${1:-sweep}
for rep in 1 2; do
for v in 1 3 0; do
  r=$(LYNSE_HIP_QS=$v python bench.py --gpus 1 --steps 30 --warmup 5 --no-configs --no-cpu-baseline --no-verify 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['roofline']['avg_launch_us'], d['rescored_per_query'], d['roofline']['plan']['stages'])")
  echo "QS=$v : ms/step, avg scan launch us, rescored/query, stages = $r"
done
done
