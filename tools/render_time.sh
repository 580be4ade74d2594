#!/bin/bash
# rasteriser tests, then the render / preprocess kernels of tools/bench_side_paths.py at 1 M anchors under rocprofv3 --kernel-trace --stats
# Usage: tools/render_time.sh OUTDIR   (every GPU step under its own time limit; the script stops at the first failing step)
set -euo pipefail
OUT=$1
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests/test_gpu_rasterizer.py tests/test_gpu_rd_loop.py -x -q > "$OUT/tests.log" 2>&1 || { rc=$?; tail -20 "$OUT/tests.log"; exit $rc; }
tail -2 "$OUT/tests.log"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/ts" -o tr -- python3 tools/bench_side_paths.py 1000000 2>/dev/null | tail -1 > "$OUT/r05_side_c.json"
f=$(find "$OUT/ts" -name "*kernel_stats.csv" | head -1)
python3 -c "
import csv,sys,json
for r in csv.DictReader(open('$f')):
    n=r['Name']
    if 'k_render' in n or 'k_preprocess' in n: print(n[:40], r['Calls'], r['AverageNs'], r['Percentage'])
print(json.load(open('$OUT/r05_side_c.json'))['rd_loop'])
"
rm -rf "$OUT/ts"
