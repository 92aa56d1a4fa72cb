#!/bin/bash
# One GPU-box call of a development session:  bash tools/gpu_session.sh <tag> [what...]
# what: tests | benchA | driverA | shard | trace | host | grad | gradbig     (default: tests benchA shard)
TAG=${1:-s}; shift
WHAT=${*:-tests benchA shard}
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$ROOT"; OUT=${OUT:-${TMPDIR:-/tmp}/gpu_session}; mkdir -p "$OUT"
for w in $WHAT; do case $w in
tests)
  timeout 1200 python -m pytest tests -m gpu -q > $OUT/${TAG}_pytest.log 2>&1; echo "pytest rc=$? $(tail -1 $OUT/${TAG}_pytest.log)"; grep -E "^FAILED|^ERROR" $OUT/${TAG}_pytest.log | head -20;;
testsx)
  timeout 1200 python -m pytest tests -m gpu -x -q > $OUT/${TAG}_pytest.log 2>&1; echo "pytest rc=$? $(tail -1 $OUT/${TAG}_pytest.log)";;
benchA)
  timeout 900 python bench.py --full > $OUT/${TAG}_bench_A.json 2> $OUT/${TAG}_bench_A.err; echo "benchA rc=$?"
  python - <<PY
import json
d=json.loads(open('$OUT/${TAG}_bench_A.json').read().strip().splitlines()[-1])
print('A', d['value'], 'evals/s median ms', d.get('ms_per_step_median'), 'kernel us', d['roofline']['kernel_us_per_eval'], 'frac', d['roofline']['frac'], 'scale_reads', d['roofline']['per_eval']['scale_reads'], 'lib', d.get('library_route') and d['library_route']['value'], 'shard', d.get('shard_point') and (d['shard_point']['ms_per_step'], d['shard_point']['ms_per_step_median']), 'cpu', d['cpu_baseline'] and d['cpu_baseline']['value'])
PY
  ;;
driverA)
  timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_bench_A_driver.json 2> $OUT/${TAG}_bench_A_driver.err; echo "driverA rc=$?"
  python - <<PY
import json
d=json.loads(open('$OUT/${TAG}_bench_A_driver.json').read().strip().splitlines()[-1])
print('A(driver cmdline)', d['value'], 'evals/s ms', d['ms_per_step'], 'median', d.get('ms_per_step_median'), 'kernel us', d['roofline']['kernel_us_per_eval'], 'traffic', d['roofline']['traffic'], 'shard', d.get('shard_point') and (d['shard_point']['ms_per_step'], d['shard_point']['ms_per_step_median']), 'move us', d.get('partial_update') and d['partial_update'].get('us_per_branch_move'))
PY
  ;;
shard)
  timeout 300 python bench.py --full --patterns 12500 --no-cpu-baseline --no-live-traffic > $OUT/${TAG}_bench_shard.json 2> $OUT/${TAG}_bench_shard.err; echo "shard rc=$?"
  python - <<PY
import json
d=json.loads(open('$OUT/${TAG}_bench_shard.json').read().strip().splitlines()[-1])
print('shard12500', d['value'], 'evals/s ms', d['ms_per_step'], 'median', d.get('ms_per_step_median'), 'kernel us', d['roofline']['kernel_us_per_eval'], 'lib', d.get('library_route') and d['library_route']['value'])
PY
  ;;
trace)
  (cd /tmp && export TMPDIR=/tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_trace" -o kt -- \
     python "$ROOT/bench.py" --patterns 12500 --steps 20 --warmup 3 --no-cpu-baseline --no-live-traffic --no-library-route --no-side-records > "$OUT/${TAG}_trace.json" 2> "$OUT/${TAG}_trace.err"; echo "trace rc=$?")
  find $OUT/${TAG}_trace -name "*.db" -delete 2>/dev/null
  python tools/timeline.py $OUT/${TAG}_trace 2>&1 | tail -40;;
host)
  BEAGLE_MI355_HOST_TIMING=1 timeout 200 python tools/step_profile.py 12500 2>&1 | tail -14;;
grad)
  timeout 300 python tools/gradient_bench.py --patterns 100000 > $OUT/${TAG}_gradient_1e5.json 2> $OUT/${TAG}_gradient_1e5.err; echo "grad rc=$?"; tail -3 $OUT/${TAG}_gradient_1e5.json | cut -c1-600
  timeout 300 python tools/gradient_bench.py > $OUT/${TAG}_gradient.json 2> $OUT/${TAG}_gradient.err; echo "grad20k rc=$?"; tail -3 $OUT/${TAG}_gradient.json | cut -c1-600;;
esac; done
