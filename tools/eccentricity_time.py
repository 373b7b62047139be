#!/usr/bin/env python3
"""Time of BFS.eccentricities() on one GPU, next to two yardsticks measured in
the same process on the same graph:

    python3 tools/eccentricity_time.py [--rows rmat20:diameter rmat20:all64 ...]
                                       [--reps 7] [--out profiles/eccentricity.txt]

A row is graph:form -- `diameter` (the largest component, target "diameter"),
`all` (the largest component, every vertex settled), `all64` (the same,
max_passes=64) or `whole64` (scope "all", max_passes=64).  Per row, after one
warm-up call: `reps` calls -- median, minimum and maximum of
EccentricityResult.ms and the medians of its bfs_ms (the batch passes),
bound_ms (ecc_update and ecc_totals) and select_ms (ecc_select and its copy)
parts (host clock around launches that end in a synchronise); passes,
sources, settled, exact and the values are those of the last call.
Yardsticks: (a) bfs_ms itself -- the new stages read at most one row of the
level matrix per live vertex where a pass walks edges, so bound + select
should be a small share of it; (b) check: the median check_ms of
run_batch(validate=True) on 64 roots sampled from the scope (one pass, the
existing device stage that walks every row's entries once), next to bound_ms
per pass.  `replaces` is what the feature stands in for, extrapolated, not
run: scope_size x the mean RunResult.ms of those 64 roots one at a time."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributed_cuda_bfs_amd as dbfs  # noqa: E402
from distributed_cuda_bfs_amd.ops.graph import LJ_SIZED_POWER_LAW  # noqa: E402
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime  # noqa: E402

GRAPHS = {
    "rmat20": lambda: dbfs.rmat_params(20, 16, 1),
    "rmat22": lambda: dbfs.rmat_params(22, 16, 1),
    "lj_uniform": lambda: dbfs.uniform_params(LJ_SIZED_POWER_LAW[0], LJ_SIZED_POWER_LAW[1], 1),
    "grid1024": lambda: dbfs.grid_params(1024, 1024),
    "uniform24": lambda: dbfs.uniform_params(1 << 24, 1 << 23, 1),
    "rmat13": lambda: dbfs.rmat_params(13, 16, 44),  # (rehearsals)
    "grid70x60": lambda: dbfs.grid_params(70, 60),
}
FORMS = {
    "diameter": dict(target="diameter", component="largest", max_passes=None),
    "all": dict(target="all", component="largest", max_passes=None),
    "all64": dict(target="all", component="largest", max_passes=64),
    "whole64": dict(target="all", component="all", max_passes=64),
}
DEFAULT_ROWS = ["rmat20:diameter", "rmat20:all64", "rmat22:diameter", "rmat22:all64", "lj_uniform:diameter",
                "grid1024:all", "uniform24:whole64"]


def spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", default=DEFAULT_ROWS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="hip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rt = init_runtime(args.device)
    lines = [f"# tools/eccentricity_time.py --reps {args.reps}   backend {rt.backend.name}",
             "# ms: median (min .. max) of EccentricityResult.ms over reps; bfs / bound / select: medians of its parts;",
             "# bound/pass: bound / passes; check: median check_ms of run_batch(validate=True), one pass of 64 roots of the",
             "# scope; run: mean ms of those roots one at a time; replaces: scope x run, extrapolated, in seconds",
             f"{'graph':<11} {'n':>9} {'nnz':>10} {'form':<9} {'scope':>9} {'passes':>6} {'sources':>7} {'settled':>9} "
             f"{'exact':>5} {'wide':>4} {'diam':>5} {'radius':>6} {'ms':>28} {'bfs':>9} {'bound':>8} {'select':>7} "
             f"{'bound/pass':>10} {'check':>7} {'run':>7} {'replaces s':>10}"]
    built = {}
    for row in args.rows:
        name, form = row.split(":")
        if name not in built:
            built.clear()  # (one graph resident at a time)
            print(f"# {name}: building", file=sys.stderr, flush=True)
            built[name] = dbfs.BFS(GRAPHS[name](), rt)
        bfs = built[name]
        kw = FORMS[form]
        bfs.eccentricities(**kw)  # warm-up (and components(), the first time)
        recs = []
        for _ in range(args.reps):
            recs.append(bfs.eccentricities(**kw))
            print(f"# {row}: {recs[-1].ms:.3f} ms, {recs[-1].passes} passes", file=sys.stderr, flush=True)
        res = recs[-1]
        roots = bfs.sample_roots(64, seed=5202611, component=None if kw["component"] == "all" else "largest")
        bfs.run_batch(roots, validate=True)  # warm-up
        check = statistics.median(bfs.run_batch(roots, validate=True).check_ms for _ in range(args.reps))
        bfs.run(roots[0])  # warm-up
        run = statistics.mean(bfs.run(r).ms for r in roots)
        m, lo, hi = spread([r.ms for r in recs])
        b, d, s = (statistics.median(getattr(r, k) for r in recs) for k in ("bfs_ms", "bound_ms", "select_ms"))
        lines.append(f"{name:<11} {bfs.n:>9} {int(bfs.graph.nnz):>10} {form:<9} {res.scope_size:>9} {res.passes:>6} "
                     f"{res.sources:>7} {res.settled:>9} {str(res.exact):>5} {str(res.wide_levels)[0]:>4} {res.diameter:>5} "
                     f"{res.radius:>6} {m:>9.3f} ({lo:>7.3f} ..{hi:>8.3f}) {b:>9.3f} {d:>8.3f} {s:>7.3f} "
                     f"{d / max(res.passes, 1):>10.4f} {check:>7.3f} {run:>7.3f} {res.scope_size * run / 1e3:>10.1f}")
        print(lines[-1], flush=True)
        if args.out:  # (kept current row by row: a later row that fails loses nothing)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if not args.out:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
