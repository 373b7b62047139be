#!/bin/bash
# The driver's multi-GPU invocation (torch.distributed.run, one process per
# rank), rehearsed with 2 ranks sharing this box's one GPU (DBFS_DEVICE=0).
# Output goes to $OUT_DIR (default bench_out/).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
export DBFS_DEVICE=0
timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 \
  bench.py --gpus 2 --steps 8 --warmup 2 --full > $OUT/tr2.json 2> $OUT/tr2.err || { tail -30 $OUT/tr2.err; exit 1; }
grep -E "comm|validated" $OUT/tr2.err | head -6
tail -1 $OUT/tr2.json | cut -c1-700
