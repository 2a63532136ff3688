#!/bin/bash
# The one recipe for rocprofv3 passes over a command: a bench.py workload (any --config), examples/percall_bench, a probe.
#   usage: tools/gpu_rocprof_mdec.sh <out-dir> [seconds-per-pass] -- <command ...>
#   e.g.   tools/gpu_rocprof_mdec.sh <dir>/prof_a4 -- python bench.py --full --lanes 1 --steps 2 --warmup 1 \
#              --launches-per-step 16 --no-cpu-baseline --no-secondary
# The command runs from the repository root, once per pass: kernel-trace with --stats, then each counter group in a run of its own
# (MI355X_MICROARCH.md: FETCH_SIZE / WRITE_SIZE need their own passes; --pmc goes with --kernel-trace and nothing else).  Counter
# collection serialises the kernels, so give it a short run of the workload.  bench.py --lanes 1 makes every launch wait for the one
# before: a kernel's span in the trace is then its duration, the figure bench.py's roofline block measures live.
# Every pass has its own time limit (default 600 s), and the first pass that fails, faults or runs out of time ends the script:
# nothing more is started on the card.  <out-dir> receives <pass>.log, summary.txt and summary.json (tools/rocpd_summary.py);
# tools/make_profile_summary.py reads a directory named prof_<tag> (see its header for where).
set -uo pipefail
if [ $# -lt 3 ]; then echo "usage: $0 <out-dir> [seconds-per-pass] -- <command ...>" >&2; exit 2; fi
out=$(realpath -m "$1"); shift
limit=600
if [ "$1" != "--" ]; then limit=$1; shift; fi
if [ "${1:-}" != "--" ] || [ $# -lt 2 ]; then echo "usage: $0 <out-dir> [seconds-per-pass] -- <command ...>" >&2; exit 2; fi
shift
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
mkdir -p "$out"

pass() {      # pass <name> <rocprofv3 options ...>
    local name=$1; shift
    timeout -k 10 "$limit" rocprofv3 "$@" -d "$out/$name" -o r -- "${cmd[@]}" > "$out/$name.log" 2>&1 && return 0
    local rc=$?
    echo "pass $name ended with status $rc (see $out/$name.log): stopping" >&2
    return $rc
}
cmd=("$@")
pass kt --kernel-trace --stats &&
pass fetch --pmc FETCH_SIZE --kernel-trace &&
pass write --pmc WRITE_SIZE --kernel-trace &&
pass sq --pmc SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY --kernel-trace &&
pass sq2 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVES GRBM_GUI_ACTIVE TCC_HIT_sum TCC_MISS_sum --kernel-trace &&
pass sq3 --pmc SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_INSTS_FLAT SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA SQ_WAIT_INST_LDS SQ_INST_CYCLES_SALU --kernel-trace ||
exit $?
python tools/rocpd_summary.py --json "$out/summary.json" $(find "$out" -name "*.db" | sort) > "$out/summary.txt" 2>&1 || exit $?
find "$out" -name "*.db" -delete
grep "^{\"metric\"" "$out/kt.log" | tail -1 > "$out/bench_line.json" || true      # (a command that is not bench.py prints no such line)
cat "$out/summary.txt"
