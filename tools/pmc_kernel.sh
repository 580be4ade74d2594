#!/bin/bash
# SQ counters of any kernel (substring match) over one bench step.  Usage: tools/pmc_kernel.sh OUTDIR SUBSTR
# (every GPU pass under its own time limit; the script stops at the first pass that fails)
set -euo pipefail
OUT=$1; K=$2
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
i=0
while read -r grp; do
  [ -z "$grp" ] && continue
  i=$((i+1))
  rc=0
  timeout -k 10 600 rocprofv3 --pmc $grp --output-format csv -d "$OUT/p$i" -o pmc -- python3 bench.py --steps 1 --warmup 0 --cpu-sample 0 --side-anchors 0 > "$OUT/p$i.log" 2>&1 || rc=$?
  echo "pass $i exit $rc"
  [ $rc -eq 0 ] || exit $rc
done <<'GROUPS'
SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_INSTS_VALU SQ_INSTS_SALU
SQ_INSTS_SMEM SQ_WAVES SQ_BUSY_CU_CYCLES SQ_INST_LEVEL_SMEM SQ_WAIT_INST_LDS SQ_ACTIVE_INST_MISC SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR
GRBM_GUI_ACTIVE
GROUPS
python3 tools/pmc_summary.py "$OUT" "$K"
rm -rf "$OUT"/p*/
