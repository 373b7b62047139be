"""Graphs and checks shared by the large analytics tests (test_large_analytics.py
on the CPU backend, test_large_analytics_gpu.py on the GPU): connected
components, strongly connected components and eccentricities on graphs past
the grid caps of cc_kernels.hip, scc_kernels.hip and ecc_kernels.hip, where
every grid-stride loop takes a second trip and the "slots, then one workgroup"
reductions merge slots that accumulated over several trips.  Every comparison
is np.array_equal or an integer literal.

CAPS pins the constants the graphs are sized by; caps_match_the_sources()
reads them back from the sources and checks every graph against the cap it is
there for, so a changed cap fails instead of turning these into one-trip tests.

Graph facts and run literals (identical on every backend; the host times are
those of the references on the CPU the cases were written on):

  cc_1m           n = 4096 * 256 + 4097 = 1 052 673, 840 199 stored pairs; hub 123 457 with 140 000
                  leaves; a 200-vertex path inside the last 4097 ids; 251 497 components, the largest
                  labelled 2 with 550 812 vertices, 196 514 singletons.  cpu_components 0.2 s, the
                  numpy propagation 0.6 s.  Scoped to the path's label: diameter 199, radius 100,
                  centre 2, periphery 2, 2 passes, 70 sources
  cc_two_largest  the same n; two 5000-vertex paths with smallest ids 300 000 and 600 000, 200 000
                  single edges; 842 675 components, the largest labelled 300 000 with 5000 vertices,
                  642 673 singletons.  References 0.03 s and 0.4 s
  cc_star_out     directed, n = 140 065: 70 000 -> each of the 140 000 other vertices below 140 001, 64
                  isolated; 65 components, the largest labelled 0 with 140 001 vertices.  References
                  0.01 s and 0.1 s
  scc_528k        n = 2048 * 256 + 4097 = 528 385, 1 360 000 arcs; hubs 1000 and 400 000 with 40 000
                  out- and 40 000 in-arcs each, every other out-degree at most 14 and in-degree at most
                  13; 114 166 strongly connected components, the largest labelled 0 with 414 220
                  vertices, 114 165 singletons; 1 round and 114 165 trimmed with the defaults, pivot
                  1000; 6 rounds forced.  cpu_strong_components 0.1 s, the numpy peeling 0.4 s
  scc_528k_high   the same with hubs 200 000 and 400 000 (the ids between the first hubs shift by one):
                  the same totals, pivot 200 000, whose slot of scc_pivot is not among the first 256
  tree270k        random recursive tree, n = 270 001: diameter 52, radius 26, centre 1, periphery 2;
                  "all": 3 passes, 192 sources; "diameter": 2 passes, 128 sources.  Double sweep 0.1 s,
                  the numpy bounding loop 7 s and 6 s
  deep140k        a 300-vertex spine, then random attachment, n = 140 001: diameter 321, radius 161,
                  centre 2, periphery 4, 16-bit levels; "all": 3 passes, 192 sources; "diameter": 2
                  passes, 128 sources.  Double sweep 0.02 s, the numpy bounding loop 9 s and 7 s
"""
import os
import re

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks
from distributed_cuda_bfs_amd.utils.validate import (component_labels_reference, eccentricity_bounding_reference,
                                                     strong_component_labels_reference)

import components_cases as cc
import directed_cases as dc
import eccentricity_cases as ec
import scc_cases as sc

CSRC = os.path.join(cc.REPO, "csrc")
# constant -> (value, file under csrc/)
CAPS = {
    "kCcBlock": (256, "kernels/cc_kernels.hip"),
    "kCcGrid": (4096, "kernels/cc_kernels.hip"),
    "kCcLongGrid": (512, "kernels/cc_kernels.hip"),
    "kCcLane": (32, "kernels/cc_kernels.hip"),
    "kCcWave": (1024, "kernels/cc_kernels.hip"),
    "kCcSizeGrid": (1024, "include/dbfs/backend.hpp"),
    "kSccBlock": (256, "kernels/scc_kernels.hip"),
    "kSccGrid": (2048, "kernels/scc_kernels.hip"),
    "kSccLane": (32, "kernels/scc_kernels.hip"),
    "kSccPivotGrid": (1024, "include/dbfs/backend.hpp"),
    "kEccBlock": (256, "kernels/ecc_kernels.hip"),
    "kEccGrid": (4096, "kernels/ecc_kernels.hip"),
    "kEccSelGrid": (256, "include/dbfs/backend.hpp"),
    "kEccSelHi": (32, "include/dbfs/backend.hpp"),
    "kEccTotalsGrid": (1024, "include/dbfs/backend.hpp"),
    "kMsSources": (64, "include/dbfs/backend.hpp"),
}

CC_N = 4096 * 256 + 4097
CC_HUB, CC_LEAVES, CC_PATH, CC_TAIL = 123457, 140000, 200, 4097
TWO_LOW, TWO_HIGH, TWO_LEN = 300000, 600000, 5000
STAR_N, STAR_HUB, STAR_LEAVES = 140065, 70000, 140000
SCC_N = 2048 * 256 + 4097
SCC_HUB_ARCS = 40000
# the two hubs of one degree product: the pivot is the first.  scc_528k_high: the same arcs with the
# first hub's id past the 256 slots scc_pivot_finish's threads read on their first trip
SCC_HUBS = {"scc_528k": (1000, 400000), "scc_528k_high": (200000, 400000)}
TREES = {"tree270k": (270001, 1, 35), "deep140k": (140001, 300, 32)}  # name -> (n, spine, seed)

# literal facts of the oracles' labels: (components, largest size, its label, singletons)
CC_FACTS = {"cc_1m": (251497, 550812, 2, 196514), "cc_two_largest": (842675, 5000, 300000, 642673),
            "cc_star_out": (65, 140001, 0, 64)}
# (scc_528k_high is scc_528k with the ids between the two first hubs shifted by one: the same totals)
SCC_FACTS = {"scc_528k": (114166, 414220, 0, 114165), "scc_528k_high": (114166, 414220, 0, 114165)}
# name -> (rounds, trimmed) with the defaults, rounds of the forced form
SCC_RUN = {"scc_528k": (1, 114165, 6), "scc_528k_high": (1, 114165, 6)}
SCC_MAX_OTHER = {"scc_528k": (14, 13), "scc_528k_high": (14, 13)}  # the largest out- and in-degree but the hubs'
# name -> (diameter, radius, centre, periphery), and target -> (passes, sources)
TREE_FACTS = {"tree270k": (52, 26, 1, 2), "deep140k": (321, 161, 2, 4)}
TREE_RUN = {"tree270k": {"all": (3, 192), "diameter": (2, 128)}, "deep140k": {"all": (3, 192), "diameter": (2, 128)}}
WIDE = ("deep140k",)
PATH_RUN = (2, 70)  # passes and sources of the scope "the planted path" on cc_1m

_graphs = {}
_oracles = {}
_references = {}
_engines = {}


# ---- generators ----------------------------------------------------------------------------

def _cc_1m():
    """700 000 random pairs over the vertices that are not named; the hub's
    star (its leaves below the tail); a path on 200 shuffled ids of the last
    4097.  No named vertex is in the pool, so the hub is not in the giant
    component, whose rows the sampled form skips."""
    rng = np.random.default_rng(101)
    path = rng.permutation(np.arange(CC_N - CC_TAIL, CC_N))[:CC_PATH]
    leaves = rng.choice(np.setdiff1d(np.arange(CC_N - CC_TAIL), [CC_HUB]), CC_LEAVES, replace=False)
    named = np.zeros(CC_N, dtype=bool)
    named[CC_HUB] = named[leaves] = named[path] = True
    pool = np.nonzero(~named)[0]
    pu, pv = pool[rng.integers(0, pool.size, 700000)], pool[rng.integers(0, pool.size, 700000)]
    csr = dbfs.build_csr(CC_N, np.concatenate([pu, np.full(CC_LEAVES, CC_HUB), path[:-1]]),
                         np.concatenate([pv, leaves, path[1:]]))
    return csr, dict(path=path, leaves=leaves)


def _cc_two_largest():
    """Two paths of 5000 vertices each, on shuffled ids of [300 000, 600 000)
    and of [600 000, n) that include the range's first; 200 000 disjoint single
    edges over the rest; the remaining vertices are isolated."""
    rng = np.random.default_rng(102)
    low = np.concatenate([[TWO_LOW], TWO_LOW + 1 + rng.choice(TWO_HIGH - TWO_LOW - 1, TWO_LEN - 1, replace=False)])
    high = np.concatenate([[TWO_HIGH], TWO_HIGH + 1 + rng.choice(CC_N - TWO_HIGH - 1, TWO_LEN - 1, replace=False)])
    low, high = rng.permutation(low), rng.permutation(high)
    taken = np.zeros(CC_N, dtype=bool)
    taken[low] = taken[high] = True
    ends = rng.permutation(np.nonzero(~taken)[0])[:400000]
    csr = dbfs.build_csr(CC_N, np.concatenate([low[:-1], high[:-1], ends[:200000]]),
                         np.concatenate([low[1:], high[1:], ends[200000:]]))
    return csr, dict(low=low, high=high)


def _cc_star_out():
    """Directed: 70 000 -> every other vertex below 140 001, in shuffled order,
    and 64 isolated vertices.  An undirected graph stores each edge in both
    rows, so a hook cc_link_long leaves out is made from the leaf's row: only
    a directed row tells whether every entry of a long row was walked."""
    leaves = np.random.default_rng(104).permutation(np.setdiff1d(np.arange(STAR_LEAVES + 1), [STAR_HUB]))
    return dc._csr(STAR_N, np.full(STAR_LEAVES, STAR_HUB), leaves), dict(leaves=leaves)


def _scc_528k(name):
    """1 200 000 random arcs over the vertices that are not hubs; each hub has
    40 000 out-arcs and 40 000 in-arcs, to 80 000 distinct vertices."""
    rng = np.random.default_rng(103)
    pool = np.setdiff1d(np.arange(SCC_N), SCC_HUBS[name])
    u, v = [pool[rng.integers(0, pool.size, 1200000)]], [pool[rng.integers(0, pool.size, 1200000)]]
    for hub in SCC_HUBS[name]:
        ends = rng.choice(pool, 2 * SCC_HUB_ARCS, replace=False)
        h = np.full(SCC_HUB_ARCS, hub)
        u += [h, ends[SCC_HUB_ARCS:]]
        v += [ends[:SCC_HUB_ARCS], h]
    return dc._csr(SCC_N, np.concatenate(u), np.concatenate(v)), {}


def _tree(name):
    """A random recursive tree on shuffled ids: vertex c hangs under c - 1
    below `spine`, under floor(U * c) from there on."""
    n, spine, seed = TREES[name]
    rng = np.random.default_rng(seed)
    child = np.arange(1, n)
    parent = np.where(child < spine, child - 1, np.floor(rng.random(n - 1) * child).astype(np.int64))
    perm = rng.permutation(n)
    return dbfs.build_csr(n, perm[child], perm[parent]), {}


BUILDERS = {"cc_1m": _cc_1m, "cc_two_largest": _cc_two_largest, "cc_star_out": _cc_star_out,
            "scc_528k": lambda: _scc_528k("scc_528k"), "scc_528k_high": lambda: _scc_528k("scc_528k_high"),
            "tree270k": lambda: _tree("tree270k"), "deep140k": lambda: _tree("deep140k")}
DIRECTED = tuple(SCC_HUBS) + ("cc_star_out",)


def graph(name):
    """(host CSR, the generator's named vertices), built once."""
    if name not in _graphs:
        _graphs[name] = BUILDERS[name]()
    return _graphs[name]


def host_csr(name):
    return graph(name)[0]


def degrees(csr):
    """(out-degree, in-degree) of every vertex, stored entries."""
    return np.diff(np.asarray(csr.row_off)), np.bincount(np.asarray(csr.col), minlength=csr.n)


def engine(name, rt, hub_sort=True):
    """One BFS per graph and runtime: the tests of a graph share its shard."""
    key = (name, hub_sort, id(rt))
    if key not in _engines:
        kw = dict(mode="td", directed=True) if name in DIRECTED else {}
        _engines[key] = dbfs.BFS(host_csr(name), rt, hub_sort=hub_sort, **kw)
    return _engines[key]


# ---- 0. the caps ---------------------------------------------------------------------------

def source_constants():
    """Every `constexpr int kName = <integer>;` of the files CAPS names."""
    found = {}
    for path in sorted({f for _, f in CAPS.values()}):
        with open(os.path.join(CSRC, path)) as f:
            for name, value in re.findall(r"^\s*constexpr int (k\w+) = (\d+);", f.read(), flags=re.M):
                found[(name, path)] = int(value)
    return found


def update_rows(level_bytes):
    """Rows per workgroup and step of ecc_update_kernel<L>, sizeof(L) = level_bytes."""
    c = {k: v for k, (v, _) in CAPS.items()}
    return c["kEccBlock"] // (c["kMsSources"] * level_bytes // 16)


def trip_and_slot(v, grid, block):
    """The trip of a grid-stride loop over vertices that takes v, and the workgroup."""
    return v // (grid * block), v % (grid * block) // block


def caps_match_the_sources():
    found = source_constants()
    for name, (value, path) in CAPS.items():
        assert found.get((name, path)) == value, f"{name} in {path}: {found.get((name, path))}, the tests assume {value}"
    c = {k: v for k, (v, _) in CAPS.items()}
    # ---- connected components
    cc_span = c["kCcGrid"] * c["kCcBlock"]
    size_span = c["kCcSizeGrid"] * c["kCcBlock"]
    assert CC_N > cc_span and CC_N > size_span and CC_N > c["kEccGrid"] * c["kEccBlock"]
    csr, parts = graph("cc_1m")
    deg = np.diff(np.asarray(csr.row_off))
    assert deg[CC_HUB] == CC_LEAVES and CC_LEAVES - 2 > c["kCcLongGrid"] * c["kCcBlock"]  # a second stride, sampled or not
    assert deg[CC_HUB] > c["kCcWave"] and np.sort(deg)[-2] <= c["kCcLane"]  # the one queued row
    assert parts["path"].size == CC_PATH and parts["path"].min() >= cc_span  # wholly in the second trip
    assert CC_N * 4 <= (64 << 20) // 2  # two ranks: one piece of all n labels per peer, past cc_link_pairs' cap
    star = host_csr("cc_star_out")
    assert np.array_equal(np.nonzero(np.diff(np.asarray(star.row_off)))[0], [STAR_HUB])  # out-arcs only, one row
    assert np.asarray(star.col).size == STAR_LEAVES > c["kCcLongGrid"] * c["kCcBlock"]
    _, two = graph("cc_two_largest")
    assert (int(two["low"].min()), int(two["high"].min())) == (TWO_LOW, TWO_HIGH)
    (trip_a, slot_a), (trip_b, slot_b) = (trip_and_slot(v, c["kCcSizeGrid"], c["kCcBlock"]) for v in (TWO_LOW, TWO_HIGH))
    assert trip_a != trip_b and slot_a != slot_b and trip_a >= 1
    tiers = np.diff(np.asarray(cc.host_csr("cc_tiers").row_off))[cc.TIER_CENTRE:cc.TIER_CENTRE + len(cc.TIER_LENGTHS)]
    for cap in (c["kCcLane"], c["kCcWave"]):
        for first in cc.SAMPLE_SETTINGS:
            assert {cap - 1, cap, cap + 1} <= {int(d) - first for d in tiers}
    # ---- strongly connected components
    assert SCC_N > c["kSccGrid"] * c["kSccBlock"] and SCC_N > c["kSccPivotGrid"] * c["kSccBlock"]
    for name, hubs in SCC_HUBS.items():
        (trip_a, slot_a), (trip_b, slot_b) = (trip_and_slot(v, c["kSccPivotGrid"], c["kSccBlock"]) for v in hubs)
        assert trip_a != trip_b and slot_a != slot_b and hubs[0] < hubs[1]
        # the finish reads the slots kSccBlock at a time: the pivot's is in its first trip or not
        assert (slot_a >= c["kSccBlock"]) == (name == "scc_528k_high") and slot_b >= c["kSccBlock"]
    assert SCC_HUB_ARCS > c["kSccLane"]
    lane, step = c["kSccLane"], 64
    assert sc.TIER_LENGTHS == (lane, lane + 1, lane + step, lane + step + 1, lane + 2 * step)
    # ---- eccentricities
    n270, n140 = TREES["tree270k"][0], TREES["deep140k"][0]
    assert (n270 + c["kEccSelGrid"] * c["kEccBlock"] - 1) // (c["kEccSelGrid"] * c["kEccBlock"]) == 5
    assert n270 > c["kEccGrid"] * update_rows(1) and n270 > c["kEccTotalsGrid"] * c["kEccBlock"]
    assert n140 > c["kEccGrid"] * update_rows(2) and n140 > c["kEccSelGrid"] * c["kEccBlock"]
    assert TREE_FACTS["deep140k"][0] > 254 >= TREE_FACTS["tree270k"][0]  # 16-bit and one-byte levels
    assert update_rows(1) == 64 and update_rows(2) == 32


# ---- 1. connected components -----------------------------------------------------------------

def cc_oracle(name):
    """The labels both references agree on (checked once; read-only)."""
    if ("cc", name) not in _oracles:
        csr = host_csr(name)
        lab = np.asarray(dbfs.cpu_components(csr))
        assert lab.dtype == np.int64 and lab.shape == (csr.n,)
        assert np.array_equal(lab, component_labels_reference(csr)), f"{name}: the two references differ"
        lab.setflags(write=False)
        _oracles[("cc", name)] = lab
    return _oracles[("cc", name)]


def cc_references_state_the_facts(name):
    lab = cc_oracle(name)
    comps, largest, label, single, sz = cc.totals(lab)
    assert lab.size == (STAR_N if name == "cc_star_out" else CC_N)
    assert (comps, largest, label, single) == CC_FACTS[name]
    assert np.array_equal(lab[lab], lab) and np.all(lab <= np.arange(lab.size))
    csr, parts = graph(name)
    if name == "cc_1m":
        path = parts["path"]
        assert np.all(lab[path] == path.min()) and sz[path.min()] == CC_PATH
        assert np.all(lab[parts["leaves"]] == min(CC_HUB, parts["leaves"].min())) and sz[lab[CC_HUB]] == CC_LEAVES + 1
    elif name == "cc_star_out":
        assert np.all(lab[parts["leaves"]] == 0) and lab[STAR_HUB] == 0 and np.all(sz[STAR_LEAVES + 1:] == 1)
    else:
        assert sz[TWO_LOW] == sz[TWO_HIGH] == TWO_LEN and np.all(lab[parts["high"]] == TWO_HIGH)
        assert np.count_nonzero(sz == 2) == 200000 and np.count_nonzero(sz > 2) == 2


def cc_check(name, res, lab, sizes, sampled):
    ref = cc_oracle(name)
    assert lab.dtype == np.int64 and lab.shape == ref.shape
    bad = np.nonzero(lab != ref)[0]
    assert np.array_equal(lab, ref), (f"{name}: {bad.size} labels differ, first " +
                                      ", ".join(f"[{int(v)}] {int(lab[v])} vs {int(ref[v])}" for v in bad[:6]))
    comps, largest, label, single, sz = cc.totals(ref)
    assert sizes.dtype == np.int64 and np.array_equal(sizes, sz[ref])
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == (comps, largest, label, single)
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == CC_FACTS[name]
    assert res.sampled == sampled


def cc_matches_references(rt, name, hub_sort=True):
    """Both settings of cc_sample_entries on one engine (a directed graph is never sampled)."""
    bfs = engine(name, rt, hub_sort)
    for sample in (2, 0):
        res = bfs.components(sample_entries=sample)
        cc_check(name, res, bfs.component_labels(), bfs.component_sizes(), sample != 0 and name not in DIRECTED)


def cc_two_ranks(name, device):
    """Two virtual ranks with the default piece size: each exchange is one piece
    of n vertices per peer, past cc_link_pairs' cap."""
    assert "DBFS_CC_PIECE_VERTICES" not in os.environ
    csr = host_csr(name)

    def body(rt):
        bfs = dbfs.BFS(csr, rt)
        res = bfs.components()
        return res, bfs.component_labels(), bfs.component_sizes()

    for res, lab, sizes in run_virtual_ranks(2, body, device=device):
        cc_check(name, res, lab, sizes, False)


# ---- 2. strongly connected components -------------------------------------------------------------

def scc_oracle(name):
    """The labels both references agree on (checked once; read-only)."""
    if ("scc", name) not in _oracles:
        csr = host_csr(name)
        lab = np.asarray(dbfs.cpu_strong_components(csr))
        assert lab.dtype == np.int64 and lab.shape == (csr.n,)
        assert np.array_equal(lab, strong_component_labels_reference(csr)), f"{name}: the two references differ"
        lab.setflags(write=False)
        _oracles[("scc", name)] = lab
    return _oracles[("scc", name)]


def scc_references_state_the_facts(name):
    csr = host_csr(name)
    out, in_ = degrees(csr)
    for hub in SCC_HUBS[name]:
        assert (out[hub], in_[hub]) == (SCC_HUB_ARCS, SCC_HUB_ARCS)
    other = np.ones(SCC_N, dtype=bool)
    other[list(SCC_HUBS[name])] = False
    assert (int(out[other].max()), int(in_[other].max())) == SCC_MAX_OTHER[name]
    lab = scc_oracle(name)
    comps, largest, label, single, sz = sc.totals(lab)
    assert lab.size == SCC_N and (comps, largest, label, single) == SCC_FACTS[name]
    assert np.array_equal(lab[lab], lab) and np.all(lab <= np.arange(lab.size))
    assert all(lab[hub] == label for hub in SCC_HUBS[name])  # either pivot settles the giant component


def scc_check(name, res, lab, sizes):
    ref = scc_oracle(name)
    assert lab.dtype == np.int64 and lab.shape == ref.shape
    bad = np.nonzero(lab != ref)[0]
    assert np.array_equal(lab, ref), (f"{name}: {bad.size} labels differ, first " +
                                      ", ".join(f"[{int(v)}] {int(lab[v])} vs {int(ref[v])}" for v in bad[:6]))
    comps, largest, label, single, sz = sc.totals(ref)
    assert sizes.dtype == np.int64 and np.array_equal(sizes, sz[ref])
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == (comps, largest, label, single)
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == SCC_FACTS[name]
    assert res.sweeps >= 1  # (stale reads may change the count between backends: not asserted)


def scc_defaults(rt, name, in_edges=False):
    """Trim to the fixed point, the pivot in the first round: the smaller id
    of the two hubs.  in_edges: the in-edge shard this first call builds is
    the numpy transpose."""
    bfs = engine(name, rt)
    res = bfs.strong_components()
    scc_check(name, res, bfs.strong_component_labels(), bfs.strong_component_sizes())
    assert res.pivot == SCC_HUBS[name][0] and res.pivot_size == SCC_FACTS[name][1]
    assert (res.rounds, res.trimmed) == SCC_RUN[name][:2]
    assert bfs.graph.has_in_edges
    if in_edges:
        h = bfs.graph.in_edges_to_host()
        dc.in_edge_shards_are_the_transpose(host_csr(name), [(np.asarray(h.row_off), np.asarray(h.col))])


def scc_forced(rt, name="scc_528k"):
    """No trim, no pivot: whole-row minima and closures over several rounds."""
    bfs = engine(name, rt)
    res = bfs.strong_components(**sc.FORCED)
    scc_check(name, res, bfs.strong_component_labels(), bfs.strong_component_sizes())
    assert (res.rounds, res.trimmed, res.pivot, res.pivot_size) == (SCC_RUN[name][2], 0, -1, 0)


def scc_two_ranks(device, name="scc_528k"):
    csr = host_csr(name)

    def body(rt):
        bfs = dbfs.BFS(csr, rt, mode="td", directed=True)
        res = bfs.strong_components()
        return res, bfs.strong_component_labels(), bfs.strong_component_sizes()

    for res, lab, sizes in run_virtual_ranks(2, body, device=device):
        scc_check(name, res, lab, sizes)
        assert (res.pivot, res.rounds, res.trimmed) == (SCC_HUBS[name][0],) + SCC_RUN[name][:2]


def scc_tier_positions(rt):
    """scc_tiers unsorted: the shard read back states where each row's one live
    entry is, then the defaults and the forced form give every pair its label."""
    name = "scc_tiers"
    bfs = sc.make_bfs(name, rt, hub_sort=False)
    res = bfs.strong_components()
    lab = sc.check_result(name, bfs, res)
    out = bfs.graph.to_host()
    in_ = bfs.graph.in_edges_to_host()
    expected = np.arange(lab.size)
    at = []
    for kind, x, p, others in sc.tier_rows():
        h = out if kind == "out" else in_
        ro, col = np.asarray(h.row_off), np.asarray(h.col)
        row = col[ro[x]:ro[x + 1]]
        assert row.size == others.size + 1 and np.count_nonzero(row == p) == 1
        at.append((kind, int(np.nonzero(row == p)[0][0])))
        expected[x] = p
    assert at == [(k, i) for k in ("out", "in") for i in (31, 32, 95, 96, 159)]
    assert np.array_equal(lab, expected)
    sc.check_result(name, bfs, bfs.strong_components(**sc.FORCED))
    assert np.array_equal(bfs.strong_component_labels(), expected)


# ---- 3. eccentricities -----------------------------------------------------------------------------

def tree_oracle(name):
    """ecc(v) = max(d(v, a), d(v, b)) for the ends a, b of a longest path of the
    tree: three traversals, no bounding."""
    if ("ecc", name) not in _oracles:
        csr = host_csr(name)
        assert np.asarray(csr.col).size == 2 * (csr.n - 1)
        d0 = np.asarray(dbfs.cpu_bfs(csr, 0)[0])
        assert np.all(d0 != dbfs.UNREACHED)  # n - 1 edges and connected: a tree
        da = np.asarray(dbfs.cpu_bfs(csr, int(np.argmax(d0)))[0])
        db = np.asarray(dbfs.cpu_bfs(csr, int(np.argmax(da)))[0])
        ecc = np.maximum(da, db).astype(np.int32)
        ecc.setflags(write=False)
        _oracles[("ecc", name)] = ecc
    return _oracles[("ecc", name)]


def tree_totals(name):
    e = tree_oracle(name)
    d, r = int(e.max()), int(e.min())
    return d, r, int(np.count_nonzero(e == r)), int(np.count_nonzero(e == d))


def tree_reference(name, target):
    """eccentricity_bounding_reference over the whole tree, once per session."""
    if (name, target) not in _references:
        csr = host_csr(name)
        out = eccentricity_bounding_reference(csr, np.ones(csr.n, dtype=bool), target)
        for a in out[:3]:
            a.setflags(write=False)
        _references[(name, target)] = out
    return _references[(name, target)]


def tree_references_state_the_facts(name):
    assert tree_totals(name) == TREE_FACTS[name]
    for target, run in TREE_RUN[name].items():
        lo, hi, settled, passes, used = tree_reference(name, target)
        assert (passes, used) == run
        ecc = tree_oracle(name)
        assert np.all(lo <= ecc) and np.all(ecc <= hi) and np.array_equal(lo[settled], ecc[settled])
        assert target != "all" or settled.all()


def tree_all(rt, name):
    bfs = engine(name, rt)
    res = bfs.eccentricities(component="all")
    ecc = tree_oracle(name)
    e = bfs.eccentricity()
    assert e.dtype == np.int32 and np.array_equal(e, ecc), f"{name}: {np.count_nonzero(e != ecc)} values differ"
    assert (res.diameter, res.radius, res.centre, res.periphery) == tree_totals(name) == TREE_FACTS[name]
    assert res.exact and res.settled == res.scope_size == ecc.size
    lo, hi = bfs.eccentricity_bounds()
    assert np.array_equal(lo, ecc) and np.array_equal(hi, ecc)
    ec.equals_bounding_reference(tree_reference(name, "all"), bfs, res, f"{name} all")
    assert (res.passes, res.sources) == TREE_RUN[name]["all"]
    assert res.wide_levels == (name in WIDE)


def tree_diameter(rt, name):
    """The promised value, exact settled values, valid bounds, the reference's run."""
    bfs = engine(name, rt)
    res = bfs.eccentricities(target="diameter", component="all")
    ecc = tree_oracle(name)
    assert res.exact and res.diameter == TREE_FACTS[name][0] and res.scope_size == ecc.size
    e = bfs.eccentricity()
    assert np.array_equal(e[e >= 0], ecc[e >= 0])
    lo, hi = bfs.eccentricity_bounds()
    assert lo.dtype == np.int32 and hi.dtype == np.int32
    assert np.all(lo <= ecc) and np.all(ecc <= hi)
    assert np.all(lo[e < 0] < hi[e < 0])  # no unsettled vertex reads as settled
    ec.equals_bounding_reference(tree_reference(name, "diameter"), bfs, res, f"{name} diameter")
    assert (res.passes, res.sources) == TREE_RUN[name]["diameter"]
    assert res.wide_levels == (name in WIDE)


def tree_two_ranks(name, device):
    csr = host_csr(name)

    def body(rt):
        bfs = dbfs.BFS(csr, rt)
        res = bfs.eccentricities(component="all")
        lo, hi = bfs.eccentricity_bounds()
        return res, bfs.eccentricity(), lo, hi

    ecc = tree_oracle(name)
    rlo, rhi, settled, passes, used = tree_reference(name, "all")
    for r, (res, e, lo, hi) in enumerate(run_virtual_ranks(2, body, device=device)):
        assert np.array_equal(e, ecc), f"rank {r}/2"
        assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi)
        assert (res.passes, res.sources, res.settled) == (passes, used, ecc.size)
        assert (res.diameter, res.radius, res.centre, res.periphery) == TREE_FACTS[name]
        assert res.exact and res.wide_levels == (name in WIDE)


def path_scope(rt):
    """cc_1m scoped to the planted path's label: 200 in-scope vertices, all in
    the second trip of ecc_init and ecc_degrees, 1 052 473 out of scope."""
    bfs = engine("cc_1m", rt)
    path = graph("cc_1m")[1]["path"]
    label = int(path.min())
    bfs.components()
    assert bfs.component_labels()[label] == label
    res = bfs.eccentricities(component=label)
    expected = np.full(CC_N, -1, dtype=np.int32)
    i = np.arange(CC_PATH)
    expected[path] = np.maximum(i, CC_PATH - 1 - i)
    e = bfs.eccentricity()
    assert e.dtype == np.int32 and np.array_equal(e, expected), f"{np.count_nonzero(e != expected)} values differ"
    assert (res.diameter, res.radius, res.centre, res.periphery) == (199, 100, 2, 2)
    assert res.exact and res.settled == res.scope_size == CC_PATH and not res.wide_levels
    lo, hi = bfs.eccentricity_bounds()
    assert np.array_equal(lo, expected) and np.array_equal(hi, expected)
    assert (res.passes, res.sources) == PATH_RUN
