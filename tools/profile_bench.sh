#!/bin/bash
# Run on the GPU box (via gpurun): kernel-trace stats + PMC passes (each in its own run: no tracing domains together with
# --pmc) of one command; outputs under gpurun_out/prof_<tag>/ for tools/summarize_profile.py.
#   profile_bench.sh <tag> [command ...]      default command: the primary bench config
# Every pass runs under its own time limit (PROFILE_PASS_TIMEOUT seconds, default 240: a pass of the default command takes
# well under a minute) and the passes are chained: after one that fails, faults or runs into its limit nothing more is started.
TAG=${1:-r03}
shift
OUT=/root/repo/gpurun_out/prof_$TAG
LIMIT=${PROFILE_PASS_TIMEOUT:-240}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
if [ $# -gt 0 ]; then CMD="$*"; else CMD="python /root/repo/bench.py --steps 50 --warmup 10 --no-cpu-baseline --no-secondary --no-strong"; fi
pass() {  # pass <name> <rocprofv3 options ...>
  local name=$1
  shift
  timeout -k 10 $LIMIT rocprofv3 "$@" --output-format csv -d $OUT/$name -o ac -- $CMD > $OUT/$name.log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "profile_bench: pass $name ended with status $rc (log: $OUT/$name.log); stopping" >&2; fi
  return $rc
}
pass trace --kernel-trace --stats &&
pass pmc_fetch --pmc FETCH_SIZE &&
pass pmc_write --pmc WRITE_SIZE &&
pass pmc_mfma --pmc SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA &&
pass pmc_wait --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS SQ_LDS_IDX_ACTIVE
rc=$?
find $OUT -name "*_kernel_stats.csv" | head -3
exit $rc
