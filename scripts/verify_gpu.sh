#!/bin/bash
# smoke(), the whole -m gpu suite and the full bench.py line on an MI355X, from the repo root:  bash scripts/verify_gpu.sh <outdir>
OUT=${1:?usage: bash scripts/verify_gpu.sh <output directory>}
mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
python -m pytest tests -m gpu -x -q > "$OUT/tall.log" 2>&1; echo "tall rc=$?"; grep -E "passed|failed" "$OUT/tall.log" | tail -2
python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; OUT="$OUT" python - <<PY
import json, os
d=json.loads([l for l in open(os.path.join(os.environ["OUT"], "bench.json")) if l.startswith("{")][-1])
print(d["ms_per_step"], d["phase_ms_per_iter_1gpu"], d["roofline"]["frac"], d["k1_batched_jacobian"]["frac_sec8d"], d["k1_batched_jacobian"]["frac_moved"])
e=d["extras"]; print(e["north_star_1e6_pose3_1gpu"]["ms_per_iteration_device"], e["config4_pose2_1e6_landmarks_5e4_1gpu"]["ms_per_iteration_device"], e["config2_linear3_1e5"]["ms_per_iteration_device"])
PY
