#!/bin/bash
# rocprofv3 passes of one bench configuration (run on the GPU box via gpurun); raw output under gpurun_out/prof_<cfg>/,
# summaries are then written by tools/pmc_summary.py into profiles/.   usage: tools/prof.sh [cfg3] [extra bench args]
# Counters are collected in separate passes and never combined with a trace domain (profiles/README.md).
# Every pass runs under its own time limit; the first pass that fails or runs out of time ends the script.
set -e
CFG=${1:-cfg3}; shift || true
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/prof_$CFG; rm -rf $O; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
B="python3 $R/bench.py --config $CFG --no-cpu-baseline $*"
pass() {   # pass <name> <seconds> <rocprofv3 arguments>: one rocprofv3 run, its log in $O/<name>.log
    local name=$1 secs=$2; shift 2
    timeout -k 10 $secs rocprofv3 --output-format csv -d $O/$name "$@" > $O/$name.log 2>&1 || { echo "$name pass failed (exit $?)"; exit 1; }
    echo "$name done"
}
pass kt 240 --kernel-trace --stats -- $B --steps 2 --warmup 1
pass fetch 180 --pmc FETCH_SIZE -- $B --steps 1 --warmup 0
pass write 180 --pmc WRITE_SIZE -- $B --steps 1 --warmup 0
pass mfma 180 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE -- $B --steps 1 --warmup 0
pass tcc 180 --pmc TCC_HIT_sum TCC_MISS_sum -- $B --steps 1 --warmup 0
pass sq 180 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU SQ_VALU_MFMA_COEXEC_CYCLES -- $B --steps 1 --warmup 0
echo "all passes done"
