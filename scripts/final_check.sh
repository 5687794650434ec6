#!/bin/bash
# Round-end check on an MI355X: the full bench line (saved), then the randomised differential test, small and
# benchmark-sized cases.  usage: bash scripts/final_check.sh [fuzz seconds] [output dir]
secs=${1:-300}
out=${2:-final_check_out}
mkdir -p "$out"
python bench.py --full > "$out/bench_output.json" 2> "$out/bench_err.txt" || exit 1
python scripts/bench_fields.py "$out/bench_output.json"
python - "$out/bench_output.json" <<'PY'
import json, sys
r = json.load(open(sys.argv[1]))
print("frac", r["roofline"]["frac"], "traffic", r["roofline"]["traffic"], "step traffic / algorithmic", r["roofline"]["traffic_over_algorithmic_bytes_step"],
      "host calls ms", r.get("host_to_host_calls_ms"), "lib", r["library_sha16"])
PY
timeout -k 10 $((secs + 100)) python scripts/fuzz_parity.py $secs 61 > "$out/fuzz_small.txt" 2>&1; tail -1 "$out/fuzz_small.txt"
timeout -k 10 $((secs + 100)) python scripts/fuzz_parity.py $secs 62 --big > "$out/fuzz_big.txt" 2>&1; tail -1 "$out/fuzz_big.txt"
