"""Cases shared by the binned-settle tests (test_binned_settle.py on the CPU
backend, test_binned_settle_gpu.py on the GPU).

A binned top-down level ends in its apply kernel: the workgroup that claimed a
bin's targets in LDS also writes the new vertices' levels, its units'
statistics and its totals, and the last workgroup finishes the level (totals,
decision, stamp, the folded unit scan).  No update and no scan follow it.  The
cases are the smallest shapes where that can go wrong; every one forces the
binned form for the levels past a tiny seed (td_bin_edges = 1,
td_bin_min_rows = 0, a small td_sparse_edges) and checks, per root,

  * the levels element-wise against the sequential CPU oracle,
  * every per-level record (frontier vertices, their degree sum, newly
    discovered) against counts derived from the oracle, with
    test_gpu_shard_sizes.check_totals_and_records (a directed graph: by the
    rule the kernels follow, a vertex counts only when its row is non-empty),
  * the same engine with device_loop = 0 (the host loop, which has no binned
    form): equal levels, records and totals,
  * validate(),
  * form X among the chains.

Everything is an integer: no tolerance.
"""
import numpy as np

import distributed_cuda_bfs_amd as dbfs
from test_gpu_shard_sizes import check_totals_and_records

N = dbfs.native
UNIT = N.UNIT_VERTICES

OPTIONS = {"td_bin_edges": 1, "td_bin_min_rows": 0, "td_sparse_edges": 64}
MODES = ("td", "do")
NARROW = (1, 0)


def _star():
    """Centre 0, leaves 1 .. 70000: one row spans many edge blocks and names
    every bin in id order.  A separate pair keeps a vertex with an edge
    unreached, so the level after the leaves runs (binned) and discovers 0:
    its own finish ends the traversal."""
    leaves = np.arange(1, 70001, dtype=np.uint32)
    u = np.concatenate([np.zeros_like(leaves), np.asarray([70001], dtype=np.uint32)])
    v = np.concatenate([leaves, np.asarray([70002], dtype=np.uint32)])
    return dbfs.build_csr(70003, u, v)


def _bipartite():
    """Root 0 joined to A = 1 .. 64; every vertex of A joined to every vertex
    of B = 65 .. 5064: 64 frontier rows name the same 5000 targets (and the
    visited root).  A separate pair as in the star."""
    a = np.arange(1, 65, dtype=np.uint32)
    b = np.arange(65, 5065, dtype=np.uint32)
    u = np.concatenate([np.zeros_like(a), np.repeat(a, b.size), np.asarray([5065], dtype=np.uint32)])
    v = np.concatenate([a, np.tile(b, a.size), np.asarray([5066], dtype=np.uint32)])
    return dbfs.build_csr(5067, u, v)


def _directed_sinks():
    """Directed: 0 -> 100 mids, every mid -> 700 leaves of its own; every third
    leaf -> one vertex of a last layer, the other leaves and the last layer
    have no out-edges (sinks: reached, a level, a frontier bit -- but no count,
    no degree, no work-list entry)."""
    mids = np.arange(1, 101, dtype=np.uint32)
    leaves = np.arange(101, 101 + 70000, dtype=np.uint32)
    last0 = 101 + 70000
    third = leaves[::3]
    u = np.concatenate([np.zeros_like(mids), np.repeat(mids, 700), third])
    v = np.concatenate([mids, leaves, (last0 + (third % 1000)).astype(np.uint32)])
    return dbfs.build_csr(last0 + 1000 + 5, u, v, directed=True)


# The star's and the bipartite graph's large levels hold most of the graph's
# edges: under the default alpha a `do` run expands them bottom-up and no level
# is binned.  alpha = 0.5 there keeps them top-down (the switch needs a frontier
# with twice the unvisited edges); the finish still runs mode do's decision.
KEEP_TOP_DOWN = {"alpha": 0.5}

# name: (graph maker -> GenParams or HostCSR, directed, roots (None: the
# maximum-degree vertex and one sampled root), modes, further options)
CASES = {
    # bin shift 12, 41 bins: a partial last bin, unit and word; every
    # workgroup reaches the ticket, the short last bin's included
    "partial_last_bin": (lambda: dbfs.uniform_params(UNIT * 40 + 77, 3 * (UNIT * 40 + 77), 11), False, None, MODES, {}),
    # bin shift 13: two units per workgroup; in td mode a compaction reads
    # their statistics back
    "units_per_bin": (lambda: dbfs.uniform_params(UNIT * 300 + 77, 3 * (UNIT * 300 + 77), 12), False, None, MODES, {}),
    "star": (_star, False, (0, 4097), MODES, KEEP_TOP_DOWN),
    "bipartite_duplicates": (_bipartite, False, (0,), MODES, KEEP_TOP_DOWN),
    # (a directed graph runs top-down modes only)
    "directed_sinks": (_directed_sinks, True, (0,), ("td",), {}),
    # several consecutive binned levels whose statistics scan_units / compact
    # consume, with the folded scan (16 units).  The unfolded scan (more than
    # FOLD_SCAN_UNITS units) needs 2^25 vertices: the GPU file runs it on
    # test_gpu_shard_sizes' graph C, at that graph's own size.
    "rmat16": (lambda: dbfs.rmat_params(16, 16, 7), False, None, ("td",), {}),
}

_graphs = {}  # (runtime, case) -> Graph


class Graph:
    """A case's graph on one runtime: the engine, and per root the oracle's
    levels with the per-level counts derived from them (the interface
    check_totals_and_records reads)."""

    def __init__(self, name, rt):
        make, self.directed, roots, self.modes, self.options = CASES[name]
        self.name = name
        g = make()
        csr = g if isinstance(g, N.HostCSR) else dbfs.host_csr_from_params(g)
        self.deg = np.diff(np.asarray(csr.row_off)).astype(np.int64)
        kw = dict(mode="td", directed=True) if self.directed else dict(mode="do")
        self.bfs = dbfs.BFS(g, rt, **kw)
        self.base = dict(self.bfs.engine.get_options())
        if roots is None:
            hub = int(np.argmax(self.deg))
            lv = np.asarray(dbfs.cpu_bfs(csr, hub)[0])
            roots = [hub] + [int(s) for s in self.bfs.sample_roots(16, seed=4)
                             if s != hub and lv[s] != dbfs.UNREACHED][:1]
        self.roots = list(roots)
        self.exp, self.cnt, self.dsum = {}, {}, {}
        for s in self.roots:
            lv = np.asarray(dbfs.cpu_bfs(csr, s)[0])
            ok = lv != dbfs.UNREACHED
            # the kernels' rule: a vertex counts only when its row is non-empty
            # (undirected: every reached vertex but an isolated root)
            counted = ok & (self.deg > 0) if self.directed else ok
            self.exp[s] = lv
            self.all_cnt = np.bincount(lv[ok]).astype(np.int64)
            self.cnt[s] = np.bincount(lv[counted], minlength=self.all_cnt.size).astype(np.int64)
            self.dsum[s] = np.bincount(lv[ok], weights=self.deg[ok]).astype(np.int64)  # (exact below 2^53)
            lv.setflags(write=False)

    def depth(self, s):
        return int(self.cnt[s].size)

    def reached(self, s):
        return int(self.cnt[s].sum())

    def edges(self, s):
        return int(self.dsum[s].sum()) // 2

    def restore(self):
        for k, v in self.base.items():
            self.bfs.engine.set_option(k, v)


def graph(rt, name):
    if (id(rt), name) not in _graphs:
        _graphs[(id(rt), name)] = Graph(name, rt)
    return _graphs[(id(rt), name)]


def strip(res):
    return [(l["dir"], l["frontier"], l["frontier_edges"], l["discovered"]) for l in res.levels]


def forms(res):
    return "".join(c[1] for c in res.chains)


def check_directed_records(g, src, res):
    """A directed graph's records: per level the frontier vertices with
    out-edges, their out-degree sum and the newly reached vertices with
    out-edges.  The traversal ends when a level reaches none (sinks get their
    levels all the same: the element-wise comparison covers them)."""
    cnt, dsum = g.cnt[src], g.dsum[src]
    exp = g.exp[src]
    ok = exp != dbfs.UNREACHED
    assert res.reached == int(np.count_nonzero(ok)), (g.name, src)
    assert res.edges == int(g.deg[ok].sum()), (g.name, src)
    assert len(res.levels) >= 1
    for i, rec in enumerate(res.levels):
        assert rec["level"] == i
        want = (int(cnt[i]), int(dsum[i]), int(cnt[i + 1]) if i + 1 < cnt.size else 0)
        got = (rec["frontier"], rec["frontier_edges"], rec["discovered"])
        assert got == want, f"{g.name} root {src} level {i}: {got}, oracle {want}; chains {forms(res)}"
    # (it ran until a level reached no vertex with out-edges)
    last = len(res.levels) - 1
    assert all(cnt[k] > 0 for k in range(last + 1)) and (last + 1 >= cnt.size or cnt[last + 1] == 0)


def check_run(g, bfs, src, want_x=True):
    """One root on the device loop under the options already set, then on the
    host loop of the same engine."""
    res = bfs.run(src)
    got = bfs.levels().copy()
    exp = g.exp[src]
    assert np.array_equal(got, exp), (g.name, src, forms(res), np.nonzero(got != exp)[0][:8])
    if g.directed:
        check_directed_records(g, src, res)
    else:
        check_totals_and_records(g, src, res)
    assert bfs.validate(src), (g.name, src)
    if want_x:
        assert "X" in forms(res), (g.name, src, forms(res))
    bfs.engine.set_option("device_loop", 0)
    try:
        host = bfs.run(src)
        assert not host.chains
        assert np.array_equal(bfs.levels(), got), (g.name, src)
        assert strip(host) == strip(res), (g.name, src, forms(res))
        assert (host.reached, host.edges, host.depth) == (res.reached, res.edges, res.depth), (g.name, src)
    finally:
        bfs.engine.set_option("device_loop", 1)
    return res


def check_case(rt, name, mode, narrow):
    g = graph(rt, name)
    bfs = g.bfs
    try:
        bfs.mode = mode
        for k, v in dict(OPTIONS, narrow_levels=narrow, **g.options).items():
            bfs.engine.set_option(k, v)
        assert dict(bfs.engine.get_options())["device_loop"] == 1.0
        return [check_run(g, bfs, s) for s in g.roots]
    finally:
        g.restore()
        bfs.mode = "td" if g.directed else "do"


def params():
    """(case, mode, narrow) of every run."""
    return [(name, mode, narrow) for name, spec in CASES.items() for mode in spec[3] for narrow in NARROW]
