#!/bin/bash
# every bench config once, with every secondary measurement (--full); JSON lines into $OUT/s_bench_<config>.json
cd "$(dirname "$0")/.."
out=${OUT:-bench_out}; mkdir -p "$out"
for c in plane_b01 icp_b01 icp_b01_harness plane_b01_100k vplane_10m ndt_10m plane_100m; do
    python bench.py --full --config $c > "$out/s_bench_$c.json" 2> "$out/s_bench_$c.err"
    python - "$out/s_bench_$c.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["config"]["workload"], "value", d["value"], "ms/step", d["ms_per_step"], "[", d["ms_per_step_min"], d["ms_per_step_max"], "] noev", d["ms_per_step_events_off"],
      {k: v["avg_ms"] for k, v in d["kernels"].items()}, "frac", d["roofline"]["frac"], "traffic", d["roofline"]["traffic"], "cpu", d.get("cpu_baseline", {}).get("value"))
PY
done
