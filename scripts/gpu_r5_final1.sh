#!/bin/bash
# round 5: the whole GPU suite + smoke + the default bench line on one box
export O=${OUT:-build/final1}
mkdir -p "$O"
timeout 3000 python -m pytest tests -q -m gpu -x > $O/pytest.txt 2>&1; tail -5 $O/pytest.txt
timeout 600 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 1200 python bench.py --full 2>$O/bench.err | tail -1 > $O/bench.json; python - <<'PY'
import json, os
d=json.load(open(os.environ['O'] + '/bench.json'))
print({k:d[k] for k in ('value','ms_per_step','blocking_ms_per_batch','two_in_flight_ms_per_step','rescored_per_query')}, d['roofline'].get('frac'), d['roofline'].get('traffic_note','')[:80])
print('c3', d['configs']['c3'])
print('c1', d['configs']['c1'])
PY
