#!/usr/bin/env python3
"""Time of BFS.strong_components() on one GPU, next to two yardsticks measured
in the same process on the same engine:

    python3 tools/scc_time.py [--graphs d_rmat20 d_rmat22 d_lj_uniform] [--reps 7] [--out profiles/scc.txt]

Every graph is directed: the generator's pairs kept as u -> v edges
(build_csr(directed=True)).  Per graph, after one warm-up call of each form
(the first builds the in-edge shard): `reps` calls of strong_components() with
the defaults (trim to the fixed point, a pivot in the first round) and `reps`
with pivot=False, alternating -- median, minimum and maximum of
StrongComponentsResult.ms, the medians of its trim_ms and colour_ms parts (host
clock around launches that end in a counter read), and the rounds, sweeps and
trimmed vertices of the last call.  Yardsticks: (a) `cc`: the median ms of
components() (the weak components, one hook-and-compress pass) on the same
engine; (b) `2 x td`: twice the median RunResult.ms of a top-down traversal from
the pivot -- one forward and one backward reach of the giant component is the
least any forward-backward scheme does, and a traversal over the out-edges is
what the engine's own kernels take for one.  The labels of both forms are
compared for equality on every graph."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import distributed_cuda_bfs_amd as dbfs  # noqa: E402
from distributed_cuda_bfs_amd.ops.graph import LJ_SIZED_POWER_LAW  # noqa: E402
from distributed_cuda_bfs_amd.parallel.runtime import init_runtime  # noqa: E402

GRAPHS = {
    "d_rmat20": lambda: dbfs.rmat_params(20, 16, 1),
    "d_rmat22": lambda: dbfs.rmat_params(22, 16, 1),
    "d_lj_uniform": lambda: dbfs.uniform_params(LJ_SIZED_POWER_LAW[0], LJ_SIZED_POWER_LAW[1], 1),
    "d_rmat13": lambda: dbfs.rmat_params(13, 16, 44),  # (rehearsals)
}


def spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", nargs="+", default=["d_rmat20", "d_rmat22", "d_lj_uniform"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", default="hip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rt = init_runtime(args.device)
    lines = [f"# tools/scc_time.py --reps {args.reps}   backend {rt.backend.name}",
             "# ms: median (min .. max) of StrongComponentsResult.ms over reps; trim / colour: medians of its parts;",
             "# rounds / sweeps / trimmed: of the last call; cc: median ms of components() on the same engine;",
             "# 2 x td: twice the median ms of a top-down traversal from the pivot (reached: its vertices)",
             f"{'graph':<13} {'n':>9} {'nnz':>10} {'sccs':>9} {'largest':>9} {'form':<8} {'ms':>26} {'trim':>8} "
             f"{'colour':>8} {'rounds':>6} {'sweeps':>6} {'trimmed':>9} {'cc':>8} {'2 x td':>8} {'reached':>9}"]
    for name in args.graphs:
        print(f"# {name}: building", file=sys.stderr, flush=True)
        p = GRAPHS[name]()
        u, v = dbfs.generate_edges(p)
        csr = dbfs.build_csr(p.n, u, v, directed=True)
        del u, v
        bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
        del csr
        print(f"# {name}: built", file=sys.stderr, flush=True)
        nnz = int(bfs.graph.nnz)
        forms = {"pivot": True, "no-pivot": False}
        labels, recs = {}, {k: [] for k in forms}
        for k, pv in forms.items():  # warm-up, and the equality check
            bfs.strong_components(pivot=pv)
            labels[k] = bfs.strong_component_labels()
        if not np.array_equal(labels["pivot"], labels["no-pivot"]):
            raise SystemExit(f"{name}: the forms disagree")
        bfs.components()
        for _ in range(args.reps):
            for k, pv in forms.items():
                recs[k].append(bfs.strong_components(pivot=pv))
                print(f"# {name}: {k} {recs[k][-1].ms:.3f} ms", file=sys.stderr, flush=True)
        cc_ms = statistics.median(bfs.components().ms for _ in range(args.reps))
        res = recs["pivot"][-1]
        pivot = res.pivot if res.pivot >= 0 else bfs.sample_roots(1, strong_component="largest")[0]
        bfs.run(pivot)  # warm-up
        runs = [bfs.run(pivot) for _ in range(args.reps)]
        td = statistics.median(r.ms for r in runs)
        for k in forms:
            m, lo, hi = spread([r.ms for r in recs[k]])
            trim = statistics.median(r.trim_ms for r in recs[k])
            col = statistics.median(r.colour_ms for r in recs[k])
            last = recs[k][-1]
            lines.append(f"{name:<13} {bfs.n:>9} {nnz:>10} {res.components:>9} {res.largest_size:>9} {k:<8} "
                         f"{m:>9.3f} ({lo:>7.3f} ..{hi:>8.3f}) {trim:>8.3f} {col:>8.3f} {last.rounds:>6} {last.sweeps:>6} "
                         f"{last.trimmed:>9} {cc_ms:>8.3f} {2 * td:>8.3f} {runs[-1].reached:>9}")
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
