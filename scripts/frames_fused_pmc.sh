#!/bin/bash
# Hardware counters of k_verify_frames (hfv_verify_frames_fused) over the probe's 2^20 frames in
# 2 KiB slots: one rocprofv3 --pmc run per counter group, never combined with a tracing domain, each
# under its own time limit; the first failure ends the script.  Output: $1 (default
# profiles/frames/pmc_fused)/p<i>/ and summary.json (scripts/pmc_summary.py: every launch of the
# kernel but the first, averaged).  The extract kernel's counters for the same frames:
# scripts/frames_pmc.sh.
#   scripts/frames_fused_pmc.sh [outdir]
set -u
cd "$(dirname "$0")/.."
OUT=${1:-profiles/frames/pmc_fused}
mkdir -p "$OUT"
export TMPDIR=/tmp
groups=(
  "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE"
  "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS"
)
i=0
for g in "${groups[@]}"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $g --output-format csv -d "$OUT/p$i" -o run -- \
      python3 scripts/frames_probe.py --fused --extract-only --slots 2048 --warmup 1 --out "$OUT/probe_p$i.json" \
      > "$OUT/p$i.log" 2>&1 || { rc=$?; echo "pmc pass $i failed rc=$rc"; tail -5 "$OUT/p$i.log"; exit $rc; }
done
python3 scripts/pmc_summary.py "$OUT" 1048576 k_verify_frames
