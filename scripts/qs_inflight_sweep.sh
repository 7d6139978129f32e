#!/bin/bash
cd "$(dirname "$0")/.."
for rep in 1 2; do
for n in 1 2 3 4; do
  r=$(LYNSE_HIP_CONTEXTS=4 python bench.py --gpus 1 --steps 40 --warmup 8 --in-flight $n --full --no-configs --no-cpu-baseline --no-verify 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['blocking_ms_per_batch'], d['config']['batches_in_flight'])")
  echo "in-flight=$n : ms/step, blocking ms/batch, in flight = $r"
done
done
