#!/usr/bin/env python3
"""Time of the batch's device check (run_batch(validate=True)) next to the
traversal it checks, on one GPU:

    python3 tools/batch_validate_time.py [--scales 20 22 24 26] [--reps 3] [--oracle-scales 20 22]

Per RMAT graph (edge factor 16): 64 roots from sample_roots(64, seed=5202611),
one warm-up, then `reps` batches with validate=True: `ms` (the traversal's
timed window) and `check_ms` (the check, after that window) of the same call,
medians.  The check reads one 64-B line of the level matrix per directed
adjacency entry, so its rate is given as entries x 64 B / check_ms.  For
--oracle-scales also the wall time of what the check replaces: cpu_bfs, the
sequential oracle the command line loops over a batch's roots, once per root
for the same roots; for --parents-scales the check with the parent form in
the same walk (the copy of the parents to the host included)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributed_cuda_bfs_amd as dbfs  # noqa: E402
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scales", type=int, nargs="*", default=[20, 22, 24, 26])
ap.add_argument("--oracle-scales", type=int, nargs="*", default=[20, 22])
ap.add_argument("--parents-scales", type=int, nargs="*", default=[20, 22])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--device", default="hip")
args = ap.parse_args()
rt = init_runtime(args.device)

print(f"# batch check vs traversal, {rt.backend.name}, 64 roots, medians of {args.reps}", flush=True)
print("graph  directed_entries  ms  check_ms  check_GB/s  parents_check_ms  oracle_loop_s", flush=True)
for s in args.scales:
    params = dbfs.rmat_params(s, 16, 1)
    bfs = dbfs.BFS(params, rt, mode="do")
    roots = bfs.sample_roots(64, seed=5202611)
    E = bfs.engine.global_directed_edges
    with_parents = s in args.parents_scales  # (k x n x 8 B of parents on the host)
    bfs.run_batch(roots, validate=True, parents=with_parents)  # warm-up
    ms, chk, both = [], [], []
    for _ in range(args.reps):
        r = bfs.run_batch(roots, validate=True)
        assert r.validated, [(roots[i], v) for i, v in enumerate(r.violations) if v != (0, 0, 0)]
        ms.append(r.ms)
        chk.append(r.check_ms)
        if with_parents:
            both.append(bfs.run_batch(roots, validate=True, parents=True).check_ms)
    c = statistics.median(chk)
    oracle = "-"
    if s in args.oracle_scales:
        csr = dbfs.host_csr_from_params(params)
        t0 = time.perf_counter()
        for v in roots:
            dbfs.cpu_bfs(csr, v)
        oracle = f"{time.perf_counter() - t0:.2f}"
        del csr
    print(f"rmat{s}_ef16 {E} {statistics.median(ms):.3f} {c:.3f} {E * 64 / (c * 1e6):.1f} "
          f"{f'{statistics.median(both):.3f}' if both else '-'} {oracle}", flush=True)
    del bfs
