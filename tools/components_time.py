#!/usr/bin/env python3
"""Time of BFS.components() on one GPU, next to two yardsticks measured in
the same process on the same graph:

    python3 tools/components_time.py [--graphs rmat20 rmat22 rmat26 lj_uniform grid1024 uniform24]
                                     [--reps 7] [--roots 16] [--out profiles/components.txt]

Per graph, after one warm-up call of each form: `reps` calls of components()
(the engine's default cc_sample_entries: sample and skip) and `reps` of
components(sample_entries=0) (one pass over every entry), alternating -- median,
minimum and maximum of ComponentsResult.ms and the medians of its link_ms and
compress_ms parts (host clock around launches that end in a synchronise) --
and (a) the median RunResult.ms of one direction-optimising traversal from
each of `roots` vertices of the largest component (sample_roots(component=
"largest")): what naming ONE component costs with the traversal kernels.
`floor` is the time to stream the shard's col array once (nnz x 4 B) at 1.6
TB/s, the rate the late-switch bottom-up counters report: no full pass reads
less.  The labels of both forms are compared for equality on every graph."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import distributed_cuda_bfs_amd as dbfs  # noqa: E402
from distributed_cuda_bfs_amd.ops.graph import LJ_SIZED_POWER_LAW  # noqa: E402
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime  # noqa: E402

STREAM_BYTES_PER_MS = 1.6e9  # 1.6 TB/s

GRAPHS = {
    "rmat20": lambda: dbfs.rmat_params(20, 16, 1),
    "rmat22": lambda: dbfs.rmat_params(22, 16, 1),
    "rmat26": lambda: dbfs.rmat_params(26, 16, 1),
    "lj_powerlaw": lambda: dbfs.power_law_params(*LJ_SIZED_POWER_LAW, 1),
    "lj_uniform": lambda: dbfs.uniform_params(LJ_SIZED_POWER_LAW[0], LJ_SIZED_POWER_LAW[1], 1),
    "grid1024": lambda: dbfs.grid_params(1024, 1024),
    "uniform24": lambda: dbfs.uniform_params(1 << 24, 1 << 23, 1),
    "rmat13": lambda: dbfs.rmat_params(13, 16, 44),  # (rehearsals)
}


def spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="+", default=["rmat20", "rmat22", "rmat26", "lj_uniform", "grid1024", "uniform24"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--roots", type=int, default=16)
    ap.add_argument("--device", default="hip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rt = init_runtime(args.device)
    lines = [f"# tools/components_time.py --reps {args.reps} --roots {args.roots}   backend {rt.backend.name}",
             "# ms: median (min .. max) of ComponentsResult.ms over reps; link / compress: medians of its parts;",
             "# bfs: median RunResult.ms of one traversal per root of the largest component; floor: nnz x 4 B at 1.6 TB/s",
             f"{'graph':<12} {'n':>10} {'nnz':>11} {'comps':>9} {'largest':>9} {'form':<8} {'ms':>24} {'link':>8} "
             f"{'compress':>8} {'floor':>7} {'bfs ms':>22}"]
    for name in args.graphs:
        print(f"# {name}: building", file=sys.stderr, flush=True)
        bfs = dbfs.BFS(GRAPHS[name](), rt)
        print(f"# {name}: built", file=sys.stderr, flush=True)
        nnz = int(bfs.graph.nnz)
        forms = {"sampled": None, "full": 0}
        labels, recs = {}, {k: [] for k in forms}
        for k, s in forms.items():  # warm-up, and the equality check
            bfs.components(sample_entries=s)
            labels[k] = bfs.component_labels()
        if not np.array_equal(labels["sampled"], labels["full"]):
            raise SystemExit(f"{name}: the sampled and the full pass disagree")
        for _ in range(args.reps):
            for k, s in forms.items():
                recs[k].append(bfs.components(sample_entries=s))
                print(f"# {name}: {k} {recs[k][-1].ms:.3f} ms", file=sys.stderr, flush=True)
        res = recs["sampled"][-1]
        roots = bfs.sample_roots(args.roots, seed=5202611, component="largest")
        bfs.run(roots[0])  # warm-up
        runs = [bfs.run(r).ms for r in roots]
        bm, blo, bhi = spread(runs)
        for k in forms:
            m, lo, hi = spread([r.ms for r in recs[k]])
            link = statistics.median(r.link_ms for r in recs[k])
            comp = statistics.median(r.compress_ms for r in recs[k])
            assert recs[k][-1].sampled == (k == "sampled")
            lines.append(f"{name:<12} {bfs.n:>10} {nnz:>11} {res.components:>9} {res.largest_size:>9} {k:<8} "
                         f"{m:>8.3f} ({lo:>6.3f} ..{hi:>7.3f}) {link:>8.3f} {comp:>8.3f} {nnz * 4 / STREAM_BYTES_PER_MS:>7.3f} "
                         f"{bm:>7.3f} ({blo:.3f} .. {bhi:.3f})")
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)
        del bfs
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
