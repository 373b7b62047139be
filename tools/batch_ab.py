#!/usr/bin/env python3
"""Same-process A/B of the concurrent multi-source BFS against 64 single
traversals, on one GPU:

    python3 tools/batch_ab.py [--scales 20 22 24 26] [--no-lj] [--no-grid] [--reps 5] [--directed]

Per graph: 64 roots from sample_roots(64, seed=5202611); after a warm-up of
both, run_many(roots) (sum of ms; the baseline) and run_batch(roots,
levels=False) alternate `reps` times; medians, spread and the ratio are
printed, and per-source reached / edges / depth of every timed batch are
asserted equal to run_many's.  That the batch's levels are right is the device
check's statement: one more run_batch(roots, validate=True) keeps the level
matrix and every source must come back clean (its time, check_ms, is printed
too).  Then one
forced-push and one forced-pull batch, level by level: a level's active set is
the same in both, so the table shows where each form is cheaper -- what the
direction constants (csrc/engine/batch.cpp) are chosen from.

--directed: the RMAT graphs of --scales as directed graphs instead (the
generator's pairs as u -> v, the CSR built on the host; no other graph), the
baseline run_many in mode td; the time of build_in_edges is printed first."""
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
ap.add_argument("--scales", type=int, nargs="*", default=[20, 22, 24, 26])
ap.add_argument("--no-lj", action="store_true")
ap.add_argument("--no-grid", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", default="hip")
ap.add_argument("--form-table-max-levels", type=int, default=24)
ap.add_argument("--directed", action="store_true")
args = ap.parse_args()
rt = init_runtime(args.device)

graphs = [(f"rmat{s}_ef16", dbfs.rmat_params(s, 16, 1)) for s in args.scales]
if args.directed:
    graphs = [(f"directed rmat{s}_ef16 (u -> v)", dbfs.rmat_params(s, 16, 1)) for s in args.scales]
elif not args.no_lj:
    n, m, _ = LJ_SIZED_POWER_LAW
    graphs.append((f"uniform_{n}_{m} (soc-LiveJournal1's size)", dbfs.uniform_params(n, m, 101)))
if not args.no_grid and not args.directed:
    graphs.append(("grid_1024x1024 (road-like)", dbfs.grid_params(1024, 1024)))


def spread(xs):
    return f"median {statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


print(f"# concurrent multi-source BFS vs run_many, {rt.backend.name}, {args.reps} alternating repetitions", flush=True)
for name, params in graphs:
    if args.directed:
        u, v = dbfs.generate_edges(params)
        bfs = dbfs.BFS(dbfs.build_csr(params.n, u, v, directed=True), rt, mode="td", directed=True)
        del u, v
        t0 = time.perf_counter()
        bfs.build_in_edges()
        print(f"\n{name}: build_in_edges {(time.perf_counter() - t0) * 1e3:.3f} ms", flush=True)
    else:
        bfs = dbfs.BFS(params, rt, mode="do")
    roots = bfs.sample_roots(64, seed=5202611)
    E = bfs.engine.global_directed_edges
    many = bfs.run_many(roots)  # warm-up of both
    batch = bfs.run_batch(roots, levels=False)
    t_many, t_batch = [], []
    for _ in range(args.reps):
        many = bfs.run_many(roots)
        t_many.append(sum(r.ms for r in many))
        batch = bfs.run_batch(roots, levels=False)
        t_batch.append(batch.ms)
        for i, r in enumerate(many):
            assert (r.reached, r.edges, r.depth) == (batch.reached[i], batch.edges[i], batch.depth[i]) or (
                # a directed run() counts the levels it expanded: one fewer than the batch's
                # levels when no vertex of the deepest level has an out-edge
                args.directed and (r.reached, r.edges, r.depth + 1) == (batch.reached[i], batch.edges[i], batch.depth[i])), \
                (name, roots[i], (r.reached, r.edges, r.depth), (batch.reached[i], batch.edges[i], batch.depth[i]))
    checked = bfs.run_batch(roots, validate=True)
    assert checked.validated, (name, [(roots[i], v) for i, v in enumerate(checked.violations) if v != (0, 0, 0)])
    mm, mb = statistics.median(t_many), statistics.median(t_batch)
    forms = "".join(l[2] for l in batch.levels)
    print(f"\n## {name}: n {bfs.n}, directed edges {E}, {len(roots)} roots, totals equal, every source validated on the device "
          f"(check {checked.check_ms:.3f} ms)", flush=True)
    print(f"run_many  sum  {spread(t_many)}")
    print(f"run_batch auto {spread(t_batch)}  forms {forms if len(forms) <= 40 else forms[:40] + '...'} "
          f"(P {forms.count('P')}, L {forms.count('L')})")
    print(f"ratio run_many / run_batch = {mm / mb:.2f}x  ({'batch faster' if mb < mm else 'batch SLOWER'}); "
          f"aggregate GTEPS {sum(batch.edges) / (mm * 1e6):.1f} -> {sum(batch.edges) / (mb * 1e6):.1f}", flush=True)
    # the two forms level by level (a level's active set does not depend on the form)
    push = bfs.run_batch(roots, direction="push", levels=False)
    push = bfs.run_batch(roots, direction="push", levels=False)
    pull = bfs.run_batch(roots, direction="pull", levels=False)
    pull = bfs.run_batch(roots, direction="pull", levels=False)
    print(f"forced push {push.ms:.3f} ms, forced pull {pull.ms:.3f} ms, auto {mb:.3f} ms")
    print("level  active  active_edges  E/active_edges  push_ms  pull_ms  auto_form")
    rows = list(zip(push.levels, pull.levels))
    for j, (a, b) in enumerate(rows[:args.form_table_max_levels]):
        assert a[3] == b[3] and a[4] == b[4]
        ratio = f"{E / a[4]:.1f}" if a[4] else "inf"
        print(f"{a[1]:5d} {a[3]:9d} {a[4]:12d} {ratio:>9s} {a[5]:9.4f} {b[5]:9.4f}  {forms[j] if j < len(forms) else '-'}")
    if len(rows) > args.form_table_max_levels:
        rest = rows[args.form_table_max_levels:]
        print(f"... {len(rest)} more levels: push {sum(a[5] for a, _ in rest):.3f} ms, pull {sum(b[5] for _, b in rest):.3f} ms")
    sys.stdout.flush()
    del bfs
