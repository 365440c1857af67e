#!/bin/bash
# Runs on the GPU box (via gpurun): the driver's bench command, then rocprofv3 kernel-trace stats and separate PMC passes of
# THE SAME command (--steps 20 --warmup 5, headline only), so that the per-kernel averages in kernel_stats.csv are averages
# over warm dispatches and can be held against the bench line's ms_per_step.  Output under gpurun_out/<tag>/ ; copy the
# summaries into profiles/.  Every GPU step runs under a time limit of its own (STEP_LIMIT seconds, default 240), and
# nothing is started after a step that fails or runs into it.
#   tools/profile_round.sh r03 [extra bench args]
TAG=${1:-r03}; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=gpurun_out/$TAG
mkdir -p $OUT
STEPS="--steps 20 --warmup 5"
LIMIT=${STEP_LIMIT:-240}
# step <stdout file> <command ...>: stderr goes to <stdout file>.err
step() {
  local log=$1; shift
  timeout -k 10 $LIMIT "$@" > $log 2> $log.err || { echo "profile_round: status $? from: $* (see $log.err); stopping" >&2; exit 1; }
}
step $OUT/bench.json python bench.py $STEPS --full "$@"
step $OUT/trace.log rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o bc7 -- python bench.py $STEPS --no-cpu --no-extra "$@"
# counters in their own runs (never together with --stats or a trace domain other than the kernel trace); the summary takes
# the LAST dispatch of every kernel -- 24 launches after start-up, clocks and caches warm -- and the mean over the timed ones
step $OUT/pmc_sq.log rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_SALU SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_sq -o bc7 -- python bench.py $STEPS --no-cpu --no-extra "$@"
step $OUT/pmc_fetch.log rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o bc7 -- python bench.py $STEPS --no-cpu --no-extra "$@"
step $OUT/pmc_write.log rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -o bc7 -- python bench.py $STEPS --no-cpu --no-extra "$@"
step $OUT/pmc_mix.log rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_CVT --kernel-trace --output-format csv -d $OUT/pmc_mix -o bc7 -- python bench.py $STEPS --no-cpu --no-extra "$@"
grep -o '{"metric.*' $OUT/bench.json | cut -c1-1500
cat $OUT/trace/bc7_kernel_stats.csv
python tools/summarize_pmc.py $OUT
