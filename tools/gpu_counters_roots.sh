#!/bin/bash
# Per-kernel PMC counters of chosen roots (tools/run_roots.py), three passes:
# cycles / waits / HBM bytes, L2 hits and writes, and the instruction side
# (instructions issued per unit and the cycles the VALU / scalar units were
# busy -- whether a kernel is bound by instruction issue rather than by waits).
#   ROOTS="33465303" OPTS="--opt x=1" tools/gpu_counters_roots.sh
#   TREE=other/tree OUT_DIR=bench_out/parent ...   counters of another build of the project
#   (records go to $OUT_DIR, default bench_out/)
# Counters run in passes of their own (the kernel trace is the only tracing).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
TREE=${TREE:-.}
OUT=${OUT_DIR:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/cr1 $OUT/cr2 $OUT/cr3
run="python3 $TREE/tools/run_roots.py --scale ${SCALE:-26} --mode ${MODE:-do} --roots ${ROOTS} ${OPTS}"
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES FETCH_SIZE \
  -d $OUT/cr1 -o run --output-format csv -- $run > $OUT/cr1.log 2>&1 || { tail -30 $OUT/cr1.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum ${PMC2_EXTRA} \
  -d $OUT/cr2 -o run --output-format csv -- $run > $OUT/cr2.log 2>&1 || { tail -30 $OUT/cr2.log; exit 1; }
# instruction side: the candidates this machine lists (PMC3 overrides; PMC3=none skips the pass)
passes="$OUT/cr1 $OUT/cr2"
if [ "${PMC3}" != none ]; then
  if [ -z "${PMC3}" ]; then
    timeout -k 10 120 rocprofv3 --list-avail > $OUT/pmc_avail.txt 2>&1
    for c in SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_INST_CYCLES_SALU; do
      grep -qw $c $OUT/pmc_avail.txt && PMC3="$PMC3 $c"
    done
    echo "instruction counters listed: ${PMC3:-none}"
  fi
  if [ -n "${PMC3}" ]; then
    # (a set the hardware cannot collect in one pass: the first two passes' table is still written)
    if timeout -k 10 300 rocprofv3 --kernel-trace --pmc ${PMC3} \
      -d $OUT/cr3 -o run --output-format csv -- $run > $OUT/cr3.log 2>&1; then
      passes="$passes $OUT/cr3"
    else
      rc=$?
      tail -30 $OUT/cr3.log
      # a fault, abort or time limit: nothing more on the GPU
      case $rc in 124|134|137|139) exit $rc ;; esac
    fi
  fi
fi
: > $OUT/counters_roots.txt
for k in ${KERNELS:-td_expand update_kernel bu_hub}; do
  echo "== $k" >> $OUT/counters_roots.txt
  python3 tools/counter_dispatch.py --kernel $k --top ${TOP:-4} $passes >> $OUT/counters_roots.txt
done
find $OUT/cr1 $OUT/cr2 $OUT/cr3 -name "*.csv" -exec gzip -f {} \; 2> /dev/null
cat $OUT/counters_roots.txt
