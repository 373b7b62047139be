#!/usr/bin/env python3
"""Headline benchmark: Graph500-style BFS GTEPS on RMAT-26 over N MI355X GPUs.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``.

* N > 1 under ``torch.distributed.run`` (RANK / LOCAL_RANK / WORLD_SIZE /
  MASTER_ADDR / MASTER_PORT in the environment): this process is one rank.
* N > 1 without a launcher (no WORLD_SIZE): the process starts N fresh child
  processes of itself (``subprocess``, never ``exec``), one per GPU, with the
  launcher's variables set, before it imports the native module or touches
  HIP; rank 0's JSON line is the output, the exit status is the worst child's.
  (The reference's 2-rank launch was ``mpirun -np 2 osu_bw``, README.md:18-23,
  bfs_mpi.cu:797-809.)

One *step* = one complete BFS traversal from a fresh random root (degree >= 1)
on the fixed RMAT-26 graph (strong scaling: the graph is 1D-partitioned over
the N GPUs).  W untimed warm-up traversals, then EXACTLY K traversals timed
between a barrier + device synchronisation on both sides, max over ranks;
rank 0 prints one JSON line.  value = total traversed input edges of the K
traversals / timed wall time (whole job, all GPUs).  The graph is generated on
the GPUs with the Graph500 Kronecker parameters (a=.57 b=.19 c=.19, edge
factor 16, scrambled vertex labels): synthetic by construction (no dataset).

A plain run does only that: build the graph, warm up, time the K traversals,
write them with ``--dump-outputs DIR`` and print the record.  Everything below
that takes traversals of its own (the int32-level pass, validation, held-out
roots, secondary graphs, the per-level profile, ``--per-level``,
``--baseline-live``, ``--allow-fallback``) runs only with ``--full``; without
it those fields are null.

Honesty fields (``--full``):
  * ``level_state_dtype``: the engine keeps one-byte levels during a traversal
    (widened to the reference's int32 when read, outside the timer);
    ``value_int32_levels`` is a second timed pass of the same K roots with
    32-bit levels written by every kernel (``narrow_levels=0``).
  * ``validated_roots``: after the timed windows every timed root is traversed
    again, checked by the device Graph500 validator, and its reached vertices,
    traversed edges and depth must equal the timed traversal's.
  * a traversal that fails validation makes the exit status 4; with
    ``--allow-fallback`` a peer-transport failure is re-measured on RCCL and the
    primary transport's failure kept in ``primary``.
  * ``vs_baseline``: value / the reference algorithm's GTEPS (``--mode ref``, a
    HIP re-implementation of bfs.cu:134-165).  With ``--baseline-live`` it is
    measured in this process on the same graph; otherwise the number measured
    on MI355X in round 1 is used for the 1-GPU RMAT-26
    configuration and vs_baseline is null elsewhere.
  * ``comm`` / ``comm_ranks`` / ``devices`` / ``comm_topology``: the
    communicator the ranks formed (N > 1 GPUs: ``peer+tcp``, peer-memory
    collective kernels over xGMI whose setup agreements go over TCP -- no
    library collective on the path; ``rccl`` only if the peer self-test fails),
    each rank's HIP device, and what the peer transport saw at setup: every
    rank's PCI bus id, the hipDeviceCanAccessPeer matrix (2 = same GPU), its
    self-test verdict and whether collectives ran fused.
  * ``heldout``: a second root sample from a seed no tuning used (the
    round-4 held-out seed 20261017 chose alpha and is a tuning seed now).

The K timed traversals run back to back in native code (``BFS.run_many``;
``--python-loop`` times one ``bfs.run`` call per root instead); each one is
complete before the next one's initialisation runs (stream order).
"""
from __future__ import annotations

import argparse
import json
import os
import resource
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

METRIC = "GTEPS (traversed edges/sec) on RMAT-26 + soc-LiveJournal1 at 1/2/4/8 MI355X"

# The reference publishes no number.  Its algorithm, re-implemented
# in HIP (`--mode ref`), measured on MI355X in round 1: (scale, n_gpus) -> GTEPS.
MEASURED_REF_GTEPS = {(26, 1): 0.8088}


def log(msg: str) -> None:
    print(f"[bench r{os.environ.get('RANK', '0')}] {msg}", file=sys.stderr, flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graph", default=None, metavar="PATH",
                    help="real graph instead of RMAT: edge list / .mtx / binary .csr cache (e.g. soc-LiveJournal1; "
                         "no dataset ships with the repo and the GPU pool has no network)")
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--uniform", default=None, metavar="N:M",
                    help="uniform-random graph of N vertices and M input edges generated on the device "
                         "(e.g. 4847571:68993773, soc-LiveJournal1's size) instead of RMAT")
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--weak", action="store_true",
                    help="weak scaling: RMAT scale = --scale + log2(N) (per-GPU shard size fixed)")
    ap.add_argument("--mode", default="do", choices=["ref", "td", "bu", "do", "simple", "scan"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--root-seed", type=int, default=12345)
    ap.add_argument("--alpha", type=float, default=40.0,
                    help="Beamer alpha (TD -> BU when m_f > m_u / alpha); the engine / CLI default, 40: chosen over "
                         "24 / 32 / 48 / 64 on the 64-root tuning sample of seed 20261017 (profiles/"
                         "r4_final_alpha_sweep.txt) -- that seed is a tuning seed now, not a held-out one")
    ap.add_argument("--beta", type=float, default=384.0)
    ap.add_argument("--bu-lane-limit", type=int, default=16)
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="engine tuning option (see Engine.get_options()), repeatable")
    ap.add_argument("--no-hubs", action="store_true", help="bottom-up without the LDS hub frontier")
    ap.add_argument("--max-hubs", type=int, default=None)
    ap.add_argument("--no-id-order", action="store_true",
                    help="keep the top-down adjacency in hub-first order (not neighbour-id order)")
    ap.add_argument("--device", default="hip", choices=["hip", "cpu"])
    ap.add_argument("--no-validate", action="store_true")
    ap.add_argument("--no-int32-pass", action="store_true",
                    help="skip the second timed pass with 32-bit level arrays")
    ap.add_argument("--baseline-gteps", type=float, default=None)
    ap.add_argument("--baseline-live", action="store_true",
                    help="measure the reference algorithm (--mode ref) on the same graph in this process")
    ap.add_argument("--baseline-roots", type=int, default=2)
    ap.add_argument("--per-level", action="store_true", help="print per-level records of the first timed run")
    ap.add_argument("--python-loop", action="store_true",
                    help="time one bfs.run() call per root instead of one native run_many()")
    ap.add_argument("--allow-fallback", action="store_true",
                    help="if the timed traversals fail validation on the peer-memory transport, measure again on "
                         "the RCCL communicator it wraps (the failure is kept in the record; exit status 4)")
    ap.add_argument("--heldout-roots", type=int, default=128,
                    help="after the headline pass, time this many roots drawn with --heldout-seed (a root sample "
                         "no tuning saw), every one validated; 0 skips")
    # (20261017 was round 4's held-out seed; alpha 40 was picked on it, so it
    # is a tuning seed now.  5202611 was drawn fresh in round 5 and no sweep
    # or A/B has used it.)
    ap.add_argument("--heldout-seed", type=int, default=5202611)
    ap.add_argument("--secondary", default="auto", metavar="N:M",
                    help="the metric's second graph, separately timed in the same record: a uniform random graph "
                         "and a power-law (Chung-Lu) graph of N vertices and M input edges, each in td (the "
                         "reference's algorithm class) and do modes; 'auto' = soc-LiveJournal1's size, "
                         "4847571:68993773 (the dataset is not on the pool), on GPUs and none on the CPU backend; "
                         "'none' skips")
    ap.add_argument("--secondary-roots", type=int, default=16)
    ap.add_argument("--spawn-timeout", type=float, default=1500.0,
                    help="self-spawned ranks: seconds before the children are killed")
    ap.add_argument("--full", action="store_true",
                    help="after the headline pass also run everything else the record can hold: the int32-level "
                         "pass, validation of every timed root, the held-out roots, the secondary graphs, the "
                         "per-level profile (and --per-level / --baseline-live / --allow-fallback); without it "
                         "those fields are null")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed traversal computed as DIR/<name>.npy: "
                         "levels.npy (float32 per-vertex levels, -1 = unreached; a fixed seeded sample of the "
                         "vertices, their ids in level_vertices.npy, when the graph is too large) and "
                         "last_step.npy (float64: source, reached vertices, traversed edges, depth)")
    return ap.parse_args(argv)


# ---- self-spawn (no launcher) -------------------------------------------------

def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, argv, timeout_s: float) -> int:
    """Start n child processes of this script, one rank each (RANK = LOCAL_RANK
    = i, WORLD_SIZE = n, MASTER_* = 127.0.0.1 and a free port).  The parent
    never touches the GPU.  If a child fails the others are given 30 s to
    notice (their collectives time out or see the closed peer) and are then
    killed; the exit status is the first failing child's (0 if all succeed)."""
    port = _free_port()
    boot_port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DBFS_BOOTSTRAP_PORT=str(boot_port), DBFS_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    t0 = time.time()
    rc = 0
    failed_at = None
    while True:
        codes = [p.poll() for p in procs]
        bad = [c for c in codes if c not in (None, 0)]
        if bad and failed_at is None:
            failed_at = time.time()
            rc = bad[0]
            log(f"a rank exited with status {rc}; waiting 30 s for the others")
        if all(c is not None for c in codes):
            break
        now = time.time()
        if (failed_at is not None and now - failed_at > 30) or now - t0 > timeout_s:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            for p in procs:
                p.wait()
            return rc or 124
        time.sleep(0.05)
    return rc


# ---- measurement ---------------------------------------------------------------

PYTHON_LOOP = False


def timed_pass(bfs, rt, roots):
    rt.barrier()
    rt.backend.synchronize()
    t_start = time.perf_counter()
    # back to back in native code (--python-loop: one bfs.run per root)
    results = [bfs.run(r) for r in roots] if PYTHON_LOOP else bfs.run_many(roots)
    rt.backend.synchronize()
    rt.barrier()
    wall_ms = (time.perf_counter() - t_start) * 1e3
    return results, rt.comm.max_host(wall_ms)


DUMP_MAX_LEVELS = 4 << 20  # levels written at most: 16 MiB of float32 (+ 32 MiB of vertex ids as float64)


def dump_outputs(out_dir: str, bfs, rank: int, last):
    """--dump-outputs: what a caller of the timed path holds after its last
    step -- the per-vertex levels of that traversal (collective gather; rank 0
    writes) and its totals.  Graph, roots and the vertex sample depend only on
    the arguments, so two builds run with the same arguments write comparable
    files."""
    import numpy as np

    from distributed_cuda_bfs_amd import UNREACHED

    levels = bfs.levels()
    if rank != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    if levels.size > DUMP_MAX_LEVELS:
        idx = np.sort(np.random.default_rng(20260101).integers(0, levels.size, size=DUMP_MAX_LEVELS))
        np.save(os.path.join(out_dir, "level_vertices.npy"), idx.astype(np.float64))
        levels = levels[idx]
    lv = levels.astype(np.float32)
    lv[levels == UNREACHED] = -1.0
    np.save(os.path.join(out_dir, "levels.npy"), lv)
    np.save(os.path.join(out_dir, "last_step.npy"),
            np.array([last.source, last.reached, last.edges, last.depth], dtype=np.float64))


def validated_pass(bfs, rt, roots):
    """Time `roots` back to back (timed_pass), then re-run and validate every
    one (device Graph500 validator + totals equal to the timed run's).
    Returns (GTEPS, ms per root, validated count, per-root results)."""
    results, wall = timed_pass(bfs, rt, roots)
    ok = 0
    for r, tr in zip(roots, results):
        res = bfs.run(r)
        valid = bfs.validate(r)
        same = (res.reached, res.edges, res.depth) == (tr.reached, tr.edges, tr.depth)
        if not (valid and same):
            log(f"root {r} FAILED: validator {'ok' if valid else 'REJECTED the levels'}; timed run (reached, edges, "
                f"depth) {(tr.reached, tr.edges, tr.depth)} rerun {(res.reached, res.edges, res.depth)}; "
                f"chains timed {[c[:3] for c in tr.chains]} rerun {[c[:3] for c in res.chains]}")
        ok += int(valid and same)
    return sum(r.edges for r in results) / (wall * 1e6), wall / len(roots), ok, results


def comm_topology(rt):
    """What the peer transport saw at setup (None on other transports)."""
    c = rt.comm
    if not hasattr(c, "peer_access"):
        return None
    return {"bus_ids": list(c.bus_ids), "peer_access": [list(r) for r in c.peer_access],
            "shared_device": bool(c.shared_device), "split_waits": bool(c.split_waits), "fused": bool(c.fused),
            "direct": bool(c.direct_on), "frontier_push": bool(c.frontier_on), "self_test": c.self_test_verdict,
            "inner": c.name.partition("+")[2]}


def secondary_block(dbfs, rt, params, graph: str, nroots: int, seed: int, args):
    """One of the metric's second-graph stand-ins (soc-LiveJournal1-sized, or
    the high-diameter road-like grid; generated on the device) in td and do
    modes: 2 warm-up roots, then `nroots` timed and validated, per mode --
    with the mean depth and the time per level (the per-level latency a
    high-diameter traversal is made of)."""
    t0 = time.time()
    g = dbfs.BFS(params, rt, mode="td", alpha=args.alpha, beta=args.beta, bu_lane_limit=args.bu_lane_limit)
    for kv in args.opt:  # (the primary engine's --opt settings apply here too)
        name, _, val = kv.partition("=")
        g.engine.set_option(name, float(val))
    rt.barrier()
    gen_s = time.time() - t0
    roots = g.sample_roots(nroots + 2, seed=seed + 1)
    out = {"graph": graph, "generate_s": round(gen_s, 3), "roots": len(roots) - 2, "opts": list(args.opt)}
    for mode in ("td", "do"):
        g.mode = mode
        for r in roots[:2]:
            g.run(r)
        gteps, ms, ok, res = validated_pass(g, rt, roots[2:])
        depth = sum(x.depth for x in res) / len(res)
        out[mode] = {"value": round(gteps, 4), "ms_per_step": round(ms, 4),
                     "harmonic_mean_gteps": round(len(res) / sum(1.0 / max(x.gteps, 1e-12) for x in res), 4),
                     "depth_mean": round(depth, 1), "us_per_level": round(1e3 * ms / max(depth, 1.0), 3),
                     "validated_roots": f"{ok}/{len(res)}"}
        log(f"secondary {graph} {mode}: {gteps:.2f} GTEPS ({ms:.4f} ms/root, depth {depth:.0f}, "
            f"{1e3 * ms / max(depth, 1.0):.2f} us/level), validated {ok}/{len(res)}")
    del g
    return out


def main(argv=None) -> int:
    args = parse_args(argv)
    global PYTHON_LOOP
    PYTHON_LOOP = args.python_loop
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args.gpus, sys.argv[1:] if argv is None else argv, args.spawn_timeout)
    if world != args.gpus:
        log(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size wins")

    import distributed_cuda_bfs_amd as dbfs
    from distributed_cuda_bfs_amd.parallel.runtime import init_runtime
    from distributed_cuda_bfs_amd.utils.metrics import harmonic_mean

    rt = init_runtime(args.device)
    rank, nranks = rt.rank, rt.world
    devices = rt.comm.allgather_host_i64(int(rt.backend.device_id))
    log(f"backend {rt.backend.name}, comm {rt.comm.name}, ranks {nranks}, devices {devices}")

    scale = args.scale
    if args.weak and not args.graph:
        lg = nranks.bit_length() - 1
        if 1 << lg != nranks:
            log("--weak needs a power-of-two number of ranks")
            return 2
        scale += lg
    if args.graph:
        # sharded: every rank parses only its byte range (or its rows of a
        # binary cache) and builds its shard on its GPU
        params = args.graph
        graph_name = os.path.basename(args.graph)
    elif args.uniform:
        un, _, um = args.uniform.partition(":")
        params = dbfs.uniform_params(int(un), int(um), args.seed)
        graph_name = f"uniform random {int(un)} V / {int(um)} E"
        n_vertices, n_input_edges = params.n, params.m
    else:
        params = dbfs.rmat_params(scale, args.edge_factor, args.seed)
        graph_name = (f"RMAT-{scale} (Graph500 Kronecker a=.57 b=.19 c=.19, "
                      f"edge factor {args.edge_factor})")
        n_vertices, n_input_edges = params.n, params.m
    t0 = time.time()
    bfs = dbfs.BFS(params, rt, mode=args.mode, alpha=args.alpha, beta=args.beta,
                   bu_lane_limit=args.bu_lane_limit, hubs=not args.no_hubs, max_hubs=args.max_hubs,
                   id_order=not args.no_id_order)
    for kv in args.opt:
        name, _, val = kv.partition("=")
        bfs.engine.set_option(name, float(val))
    rt.backend.synchronize()
    rt.barrier()
    gen_s = time.time() - t0
    if args.graph:
        n_vertices, n_input_edges = bfs.n, bfs.graph.input_edges
    log(f"built {graph_name} shard: rows {bfs.graph.rows} nnz {bfs.graph.nnz} in {gen_s:.2f}s")

    roots = bfs.sample_roots(args.warmup + args.steps, seed=args.root_seed)
    if len(roots) < args.warmup + args.steps:
        log("could not sample enough roots")
        return 3
    warm, timed = roots[:args.warmup], roots[args.warmup:]

    def measure():
        for r in warm:
            res = bfs.run(r)
            log(f"warmup root {r}: {res.ms:.3f} ms, {res.gteps:.2f} GTEPS, depth {res.depth}")
        results, wall_ms = timed_pass(bfs, rt, timed)
        if args.dump_outputs:
            # before anything else traverses: the engine holds the last timed step's levels
            dump_outputs(args.dump_outputs, bfs, rank, results[-1])
        # Second timed pass: the same roots with 32-bit levels written by the kernels.
        narrow = bool(dict(bfs.engine.get_options()).get("narrow_levels", 0)) and args.mode in ("td", "bu", "do")
        value_i32 = None
        if args.full and narrow and not args.no_int32_pass:
            bfs.engine.set_option("narrow_levels", 0)
            bfs.run(warm[0] if warm else timed[0])
            res32, wall32 = timed_pass(bfs, rt, timed)
            value_i32 = sum(r.edges for r in res32) / (wall32 * 1e6)
            bfs.engine.set_option("narrow_levels", 1)
            log(f"int32-level pass: {value_i32:.2f} GTEPS ({wall32 / len(timed):.4f} ms/step)")
        # Validation of every timed root: re-traversed after the timed windows,
        # checked by the device Graph500 validator, and its totals must equal
        # the timed traversal's (reached vertices, traversed edges, depth) --
        # so the validated traversal is the one that was timed.
        validated, n_valid = None, 0
        if args.full and not args.no_validate:
            for r, tr in zip(timed, results):
                res = bfs.run(r)
                ok = bfs.validate(r)
                same = (res.reached, res.edges, res.depth) == (tr.reached, tr.edges, tr.depth)
                if not same:
                    log(f"root {r}: timed traversal reached {tr.reached} / {tr.edges} edges / depth {tr.depth}, "
                        f"validated rerun {res.reached} / {res.edges} / {res.depth}")
                n_valid += int(ok and same)
                if not ok:
                    log(f"validation of root {r}: FAILED")
            validated = n_valid == len(timed)
            log(f"validated {n_valid}/{len(timed)} timed roots (device validator + totals equal to the timed run)")
        return results, wall_ms, narrow, value_i32, validated, n_valid

    comm_note = None
    primary = None
    results, wall_ms, narrow, value_i32, validated, n_valid = measure()
    if validated is False and args.allow_fallback and getattr(rt, "fallback_comm", None) is not None:
        # --allow-fallback: a wrong traversal on the peer-memory transport is
        # measured again on the communicator it wraps (RCCL); the primary
        # transport's failure stays in the record ("primary") and the exit
        # status is still non-zero
        primary = {"comm": rt.comm.name, "validated": False, "validated_roots": f"{n_valid}/{len(timed)}",
                   "value": round(sum(r.edges for r in results) / (wall_ms * 1e6), 4)}
        comm_note = f"{rt.comm.name} FAILED validation ({n_valid}/{len(timed)}); re-measured on {rt.fallback_comm.name}"
        log(comm_note)
        bfs.use_comm(rt.fallback_comm)
        results, wall_ms, narrow, value_i32, validated, n_valid = measure()

    if rank == 0:
        for r in results:
            dirs = "".join(lv["dir"] for lv in r.levels)
            log(f"timed root {r.source}: {r.ms:.3f} ms {r.gteps:.1f} GTEPS levels {dirs} "
                f"frontier-edges {[lv['frontier_edges'] for lv in r.levels]} "
                f"level-us {[round(lv['ms'] * 1e3, 1) for lv in r.levels]}")
    edges = sum(r.edges for r in results)
    bfs_ms = sum(r.ms for r in results)
    value = edges / (wall_ms * 1e6)

    if args.full and args.per_level:
        order = sorted(results, key=lambda r: r.ms)
        bfs.engine.phase_timing = True
        profs = [bfs.run(order[0].source), bfs.run(order[-1].source)]
        bfs.engine.phase_timing = False
        for prof in profs:
            if rank != 0:
                break
            log(f"per-level profile of root {prof.source} ({prof.ms:.3f} ms incl. event overhead):")
            for lv in prof.levels:
                log(f"  level {lv['level']} {lv['dir']} frontier {lv['frontier']} edges {lv['frontier_edges']}"
                    f" new {lv['discovered']} {lv['ms']:.3f} ms (collectives {lv.get('comm_ms', 0.0):.3f} ms)")
    # A held-out root sample (another seed, never used for tuning): timed the
    # same way, every root validated.  Reported next to the headline, which is
    # the driver's K roots.
    heldout = None
    fast_mode = args.mode in ("td", "bu", "do")  # (ref / simple / scan take seconds per root)
    if args.full and args.heldout_roots > 0 and fast_mode:
        hroots = bfs.sample_roots(args.heldout_roots, seed=args.heldout_seed)
        if hroots:
            hv, hms, hok, hres = validated_pass(bfs, rt, hroots)
            heldout = {"value": round(hv, 4), "ms_per_step": round(hms, 4), "roots": len(hroots),
                       "mispredicted_levels": sum(r.mispredicts for r in hres),
                       "seed": args.heldout_seed, "validated_roots": f"{hok}/{len(hroots)}"}
            log(f"held-out roots (seed {args.heldout_seed}): {hv:.2f} GTEPS, validated {hok}/{len(hroots)}")
            if hok != len(hroots):
                validated = False
    secondary = None
    if not args.full:
        args.secondary = "none"
    elif args.secondary == "auto":
        args.secondary = "4847571:68993773" if rt.is_gpu else "none"
    if args.secondary and args.secondary != "none" and not args.graph and fast_mode:
        un, _, um = args.secondary.partition(":")
        n2, m2 = int(un), int(um)
        lj = (n2, m2) == (4847571, 68993773)
        secondary = {}
        # uniform random at that size, and the power-law (Chung-Lu) stand-in
        # with soc-LiveJournal1's largest degree: its heavy tail is what the
        # real graph's top-down levels see (parity with the dataset unpinned)
        secondary["lj_sized"] = secondary_block(
            dbfs, rt, dbfs.uniform_params(n2, m2, args.seed + 100),
            f"uniform random {n2} V / {m2} E " + ("(soc-LiveJournal1's size; synthetic)" if lj else "(synthetic)"),
            args.secondary_roots, args.seed + 100, args)
        dmax = dbfs.ops.graph.LJ_SIZED_POWER_LAW[2] if lj else max(64, int(20 * 2 * m2 / max(n2, 1)))
        secondary["lj_power_law"] = secondary_block(
            dbfs, rt, dbfs.power_law_params(n2, m2, dmax, args.seed + 200),
            f"power-law (Chung-Lu, degree tail exponent 2.5, max expected degree {dmax}) {n2} V / {m2} E "
            + ("(soc-LiveJournal1's size and largest degree; synthetic)" if lj else "(synthetic)"),
            args.secondary_roots, args.seed + 200, args)
        if lj:
            # the high-diameter case: a 1024 x 1024 road-like
            # grid, ~1000-2000 levels of a few hundred vertices each
            secondary["road_grid"] = secondary_block(
                dbfs, rt, dbfs.grid_params(1024, 1024),
                "2-D grid 1024 x 1024 (road-like: degree <= 4, diameter 2046; synthetic)",
                max(4, args.secondary_roots // 4), args.seed + 300, args)
        for blk in secondary.values():
            for m in ("td", "do"):
                ok, tot = blk[m]["validated_roots"].split("/")
                if ok != tot:
                    validated = False
    # One extra (untimed) traversal of the median timed root with per-level
    # device events: where the time goes (collectives vs kernels) at this N.
    med = sorted(results, key=lambda r: r.ms)[len(results) // 2]
    prof, level_profile = None, None
    if args.full:
        bfs.engine.phase_timing = True
        prof = bfs.run(med.source)
        bfs.engine.phase_timing = False
        level_profile = {"root": med.source, "columns": ["dir", "ms", "comm_ms"],
                         "levels": [[lv["dir"], round(lv["ms"], 4), round(lv.get("comm_ms", 0.0), 4)]
                                    for lv in prof.levels]}

    baseline = args.baseline_gteps
    baseline_src = "--baseline-gteps" if baseline else None
    if args.full and args.baseline_live and args.mode != "ref":
        mode = bfs.mode
        bfs.mode = "ref"
        ref_roots = timed[:max(1, args.baseline_roots)]
        bfs.run(ref_roots[0])
        ref_res, ref_wall = timed_pass(bfs, rt, ref_roots)
        bfs.mode = mode
        baseline = sum(r.edges for r in ref_res) / (ref_wall * 1e6)
        baseline_src = f"reference algorithm (--mode ref) measured live, {len(ref_roots)} roots, same graph"
        log(f"live baseline: {baseline:.4f} GTEPS")
    if baseline is None and not args.graph and not args.uniform and args.edge_factor == 16 and args.mode != "ref":
        baseline = MEASURED_REF_GTEPS.get((scale, nranks))
        if baseline:
            baseline_src = "reference algorithm (--mode ref) on MI355X, measured round 1 (BASELINE.md)"
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": round(value, 4),
            "unit": "GTEPS",
            "n_gpus": nranks,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(wall_ms / args.steps, 4),
            "higher_is_better": True,
            "full": args.full,
            "scaling": "weak" if args.weak else "strong",
            "vs_baseline": (round(value / baseline, 2) if baseline else None),
            "baseline": baseline_src,
            "baseline_gteps": (round(baseline, 4) if baseline else None),
            # what the timed kernels wrote: one-byte levels (widened to the
            # reference's int32 when read, outside the timer) or int32 levels;
            # value_int32_levels is the same roots timed with int32 levels
            "dtype": "uint8 levels (int32 on read)" if narrow else "int32",
            "level_state_dtype": "uint8" if narrow else "int32",
            "value_int32_levels": (round(value_i32, 4) if value_i32 is not None else None),
            "data": (f"file {graph_name}, random roots" if args.graph
                     else "synthetic (uniform random graph generated on device, random roots)" if args.uniform
                     else "synthetic (Graph500 RMAT generated on device, random roots)"),
            "config": {
                "model": graph_name,
                "global_batch": 1,
                "seq_len": None,
                "parallelism": f"1d-vertex-partition x{nranks}",
                "mode": args.mode,
                "alpha": args.alpha,
                "beta": args.beta,
                "opts": list(args.opt),
                "vertices": n_vertices,
                "input_edges": n_input_edges,
                "directed_edges": bfs.engine.global_directed_edges,
            },
            "comm": rt.comm.name,
            # peer transport: the kernels exchange owner lists and level ends
            # themselves (its self-test passed on every rank)
            "comm_direct": bool(getattr(rt.comm, "direct_on", False)),
            "comm_note": comm_note,
            "primary": primary,
            "comm_ranks": rt.comm.size,
            "comm_topology": comm_topology(rt),
            # peer transport: collectives through the IPC windows / handed to
            # the wrapped communicator (RCCL) -- every payload size goes
            # through the windows in slot-sized rounds, so 0 is expected
            "comm_peer_ops": getattr(rt.comm, "peer_ops", None),
            "comm_inner_ops": getattr(rt.comm, "inner_ops", None),
            # chains of the profiled traversal whose frontier the producing
            # kernels pushed into the peers' windows (direct_frontier)
            "pushed_chains": (sum(1 for c in prof.chains if len(c) > 4 and c[4]) if prof else None),
            # ... and its bottom-up chains with the hub cut's launches
            "cut_chains": (sum(1 for c in prof.chains if len(c) > 7 and c[7]) if prof else None),
            "heldout": heldout,
            "secondary": secondary,
            "devices": [f"{'hip' if rt.is_gpu else 'cpu'}:{d}" for d in devices],
            "bfs_ms_mean": round(bfs_ms / len(results), 4),
            "harmonic_mean_gteps": round(harmonic_mean([r.gteps for r in results]), 4),
            "traversed_edges_mean": edges // len(results),
            "depth_mean": sum(r.depth for r in results) / len(results),
            "mispredicted_levels": sum(r.mispredicts for r in results),
            # timed traversals that ended at the all-reached stop (every vertex
            # with an edge reached: the last frontier was not expanded, so its
            # last level record discovered vertices)
            "all_reached_stops": sum(1 for r in results if r.levels and r.levels[-1]["discovered"] > 0),
            "validated": validated,
            "validated_roots": (f"{n_valid}/{len(timed)}" if validated is not None else None),
            "generate_s": round(gen_s, 3),
            # peak resident host memory of rank 0's process (graph build included)
            "host_peak_rss_gb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20, 3),
            "level_profile": level_profile,
            # the timed traversal of the same root, from the device clock the
            # kernels stamp (device loop only): level time and the idle gap
            # before its first kernel
            "level_clock": {"levels": [[lv["dir"], round(lv["ms"], 4), round(lv.get("gap_ms", -1.0), 4)]
                                       for lv in med.levels],
                            "columns": ["dir", "ms", "gap_ms"]},
        }
        print(json.dumps(out), flush=True)
    return 0 if validated in (None, True) and primary is None else 4


if __name__ == "__main__":
    sys.exit(main())
