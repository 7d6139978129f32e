# round 6: the default bench line + a digest of its new keys
O=${OUT:-build/r6}
mkdir -p "$O"
T=${1:-bench_a}
python bench.py --full > $O/$T.json 2> $O/$T.err
tail -c 600 $O/$T.err
python - <<PY
import json
d = json.loads(open("$O/$T.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], json.dumps(d["roofline"])[:1000])
print(json.dumps(d.get("cpu_baseline"))[:1600])
for k, v in d.get("configs", {}).items():
    print(k, json.dumps(v)[:1500])
PY
