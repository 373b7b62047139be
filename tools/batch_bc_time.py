#!/usr/bin/env python3
"""Time of a batch's path counts and betweenness accumulation
(run_batch(betweenness=True)) next to the traversal and the device check of
the same sources, on one GPU:

    python3 tools/batch_bc_time.py [--graphs rmat20 rmat22 d_rmat20 lj_uniform] [--reps 3]
                                   [--split 0 512] [--counts double wide auto] [--oracle rmat20]
                                   [--out profiles/ms_bfs_betweenness.txt]

Per graph: 64 roots from sample_roots(64, seed=5202611), one warm-up, then
`reps` batches each of run_batch(validate=True) -- `ms`, `check_ms` -- and of
run_batch(betweenness=True) for every --split value (engine option
bc_split_row: rows above it are walked by a workgroup of 16 waves, 0: every
row by one wave) -- `bc_ms` and its forward / backward parts; medians.  The
check walks every row once; the accumulation walks a row once per distinct
level its 64 sources put it on, in each direction: `walked` is that count
(BatchResult.bc_rows_walked), `rows x launches` what it would be without the
level skip, and bc_ms / check_ms the multiple to hold against walked / rows.
For --oracle graphs also the wall time of cpu_betweenness on the same sources.

--counts: the path counts' form (run_batch(wide_counts=...)), one line per
form and split: double (the default), wide (a mantissa and an exponent) or
auto (wide only for the passes that overflow); the last two columns name it
and give BatchResult.wide_count_passes.

gridN (an N x N grid): a grid whose path counts leave double's range --
C(dx + dy, dx) > 2^1024 once both offsets from a source pass about 516, so
grid1024 from almost every source -- makes run_batch raise with --counts
double, and so this tool; give it wide or auto only.  It is not among the
defaults."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributed_cuda_bfs_amd as dbfs  # noqa: E402
from distributed_cuda_bfs_amd.ops.graph import LJ_SIZED_POWER_LAW  # noqa: E402
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--graphs", nargs="*", default=["rmat20", "rmat22", "d_rmat20", "lj_uniform"])
ap.add_argument("--oracle", nargs="*", default=["rmat20"])
ap.add_argument("--split", type=int, nargs="*", default=[0, 512])
ap.add_argument("--counts", nargs="*", default=["double"], choices=["double", "wide", "auto"])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--device", default="hip")
ap.add_argument("--out", default=os.path.join("profiles", "ms_bfs_betweenness.txt"))
args = ap.parse_args()
WIDE = {"double": False, "wide": True, "auto": "auto"}
rt = init_runtime(args.device)


def graph(name):
    """(what BFS is built from, directed, the host CSR when one exists)"""
    if name.startswith("d_rmat"):
        p = dbfs.rmat_params(int(name[6:]), 16, 1)
        u, v = dbfs.generate_edges(p)
        csr = dbfs.build_csr(p.n, u, v, directed=True)
        return csr, True, csr
    if name.startswith("rmat"):
        return dbfs.rmat_params(int(name[4:]), 16, 1), False, None
    if name == "lj_uniform":
        return dbfs.uniform_params(LJ_SIZED_POWER_LAW[0], LJ_SIZED_POWER_LAW[1], 1), False, None
    if name.startswith("grid"):
        return dbfs.grid_params(int(name[4:]), int(name[4:])), False, None
    raise SystemExit(f"unknown graph {name}")


lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


emit(f"# batch betweenness vs traversal and check, {rt.backend.name}, 64 roots, medians of {args.reps}")
emit("graph split_above rows directed_entries depth ms check_ms bc_ms forward_ms backward_ms bc/check "
     "launches walked rows_x_launches walked/rows oracle_s counts wide_passes")
for name in args.graphs:
    g, directed, csr = graph(name)
    bfs = dbfs.BFS(g, rt, mode="td" if directed else "do", directed=directed)
    roots = bfs.sample_roots(64, seed=5202611)
    E = bfs.engine.global_directed_edges
    bfs.run_batch(roots, validate=True, betweenness=True, wide_counts=WIDE[args.counts[0]])  # warm-up
    ms, chk = [], []
    for _ in range(args.reps):
        r = bfs.run_batch(roots, validate=True)
        assert r.validated
        ms.append(r.ms)
        chk.append(r.check_ms)
    oracle = "-"
    if name in args.oracle:
        if csr is None:
            csr = dbfs.host_csr_from_params(g)
        t0 = time.perf_counter()
        dbfs.cpu_betweenness(csr, roots, directed, wide_counts="double" not in args.counts)
        oracle = f"{time.perf_counter() - t0:.2f}"
    del csr
    for above, counts in ((a, c) for a in args.split for c in args.counts):
        bfs.engine.set_option("bc_split_row", above)
        # (the long-row list of this threshold, and the form's buffers, are built here)
        bfs.run_batch(roots, betweenness=True, wide_counts=WIDE[counts])
        bc, fw, bw = [], [], []
        for _ in range(args.reps):
            r = bfs.run_batch(roots, betweenness=True, wide_counts=WIDE[counts])
            bc.append(r.bc_ms)
            fw.append(r.bc_forward_ms)
            bw.append(r.bc_backward_ms)
        c, m = statistics.median(chk), statistics.median(bc)
        emit(f"{name} {above} {bfs.n} {E} {max(r.depth)} {statistics.median(ms):.3f} {c:.3f} {m:.3f} "
             f"{statistics.median(fw):.3f} {statistics.median(bw):.3f} {m / c:.2f} {r.bc_launches} {r.bc_rows_walked} "
             f"{bfs.n * r.bc_launches} {r.bc_rows_walked / bfs.n:.2f} {oracle} {counts} {r.wide_count_passes}")
    del bfs
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
