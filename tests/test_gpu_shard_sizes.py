"""The kernels at the shard sizes the benchmark runs them at.

The launchers pick template instantiations, grid shapes and finish paths by
the number of 4096-vertex bitmap units on a rank; the headline shard (RMAT-26
on one rank) holds 16 384 of them.  Three sparse graphs cross every such
threshold (host oracle time, not GPU time, is what a larger graph costs):

  A  uniform, 1101 units: more than one scan workgroup (chunk totals handed
     to the last arriver, non-zero chunk prefixes in the compaction), the
     4-words-per-wave bottom-up form and the fused update finish looping
     over more units than their persistent grids hold.
  B  uniform, 4201 units: compact_kernel<false> / update_unit<1> (a unit per
     wave) instead of the split variants, the 16-words-per-wave bottom-up
     form with a looping persistent grid, the from-bitmap sparse level with
     several units per wave, a bin shift of 13.
  C  power law, 8301 units, n >= 2^25: no folded scan (a scan_units launch
     between levels), whole units per wave by default with a partial second
     pass, split top-down levels in 2 x td_split_parts parts, hubs.

(B and C are also the first graphs in the suite with top-down levels of
2^24 frontier edges, where the hub filter starts: in the bitmap form such a
level used to lose its hubs, see test_td_hub_filter_bitmap_levels_gpu.)

n = 4096 U + 77, so the last unit and the last word are partial.  Every case
checks the levels element-wise against the sequential CPU oracle, the
totals, every per-level record (frontier vertices, their degree sum, newly
discovered vertices -- what the scans and per-unit statistics compute and
the direction switch reads) against counts derived from the oracle, and the
device-side validation.  Everything is an integer: no tolerance.
"""
import numpy as np
import pytest

import chain_plans
import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks
from test_gpu_engine import _describe

pytestmark = pytest.mark.gpu

N = dbfs.native
UNIT = N.UNIT_VERTICES


def _n(units):
    return UNIT * units + 77


SPECS = {
    # name: (params, sampled roots (next to the maximum-degree vertex), keep the CSR for the parent check)
    "A": (lambda: dbfs.uniform_params(_n(1100), 3 * _n(1100), 5), 1, True),
    "B": (lambda: dbfs.uniform_params(_n(4200), 3 * _n(4200), 5), 2, False),
    "C": (lambda: dbfs.power_law_params(_n(8300), 2 * _n(8300), 20000, 9), 1, True),
}


class Shard:
    """One graph: its device copy, and per root the oracle's levels with the
    per-level vertex counts and degree sums derived from them."""

    def __init__(self, name, rt):
        make, sampled, keep = SPECS[name]
        self.name, self.rt = name, rt
        self.params = make()
        self.n = int(self.params.n)
        self.units = -(-self.n // UNIT)
        csr = dbfs.host_csr_from_params(self.params)
        ro = np.asarray(csr.row_off)
        self.deg = np.diff(ro).astype(np.int64)
        self._bfs = {}
        bfs = self.bfs()
        # the maximum-degree vertex, and sampled roots of its component (C has
        # millions of isolated pairs: a root there is a two-level traversal)
        hub = int(np.argmax(self.deg))
        self.roots = [hub]
        self.exp, self.cnt, self.dsum = {}, {}, {}
        for s in [hub] + [int(s) for s in bfs.sample_roots(16, seed=4)]:
            if s != hub and (len(self.roots) > sampled or self.exp[hub][s] == dbfs.UNREACHED):
                continue
            if s != hub:
                self.roots.append(s)
            lv = np.asarray(dbfs.cpu_bfs(csr, s)[0])
            ok = lv != dbfs.UNREACHED
            self.exp[s] = lv
            self.cnt[s] = np.bincount(lv[ok]).astype(np.int64)
            # (float64 sums of integers below 2^53: exact)
            self.dsum[s] = np.bincount(lv[ok], weights=self.deg[ok]).astype(np.int64)
            lv.setflags(write=False)
        self.row_off, self.col = (ro, np.asarray(csr.col)) if keep else (None, None)

    def bfs(self, max_hubs=None):
        """The device graph, built once per max_hubs, with its engine's
        options as they were after construction."""
        if max_hubs not in self._bfs:
            b = dbfs.BFS(self.params, self.rt, mode="do", max_hubs=max_hubs)
            self._bfs[max_hubs] = (b, dict(b.engine.get_options()))
        return self._bfs[max_hubs][0]

    def restore(self):
        for b, base in self._bfs.values():
            for k, v in base.items():
                b.engine.set_option(k, v)
            b.mode = "do"

    def depth(self, s):
        return int(self.cnt[s].size)

    def reached(self, s):
        return int(self.cnt[s].sum())

    def edges(self, s):
        return int(self.dsum[s].sum()) // 2


_shards = {}


@pytest.fixture(scope="module")
def shards(gpu_runtime):
    """name -> Shard, each built on first use and kept for the module."""
    def get(name):
        if name not in _shards:
            _shards[name] = Shard(name, gpu_runtime)
        return _shards[name]

    yield get
    _shards.clear()


def check_totals_and_records(g, src, res):
    """reached / edges / depth and every level record against the oracle's
    per-level counts.  The device loop may stop once every vertex with an
    edge is reached, without expanding the last frontier: the records that
    are present are compared, and at least depth - 1 must be."""
    cnt, dsum, depth = g.cnt[src], g.dsum[src], g.depth(src)
    assert (res.reached, res.edges, res.depth) == (g.reached(src), g.edges(src), depth), (g.name, src)
    recs = res.levels
    assert depth - 1 <= len(recs) <= depth, (g.name, src, len(recs), depth)
    for i, rec in enumerate(recs):
        k = rec["level"]
        assert k == i
        want = (int(cnt[k]), int(dsum[k]), int(cnt[k + 1]) if k + 1 < depth else 0)
        got = (rec["frontier"], rec["frontier_edges"], rec["discovered"])
        assert got == want, (f"{g.name} root {src} level {k} ({rec['dir']}): frontier, frontier_edges, discovered = "
                             f"{got}, oracle {want}; chains {' '.join(f'{c[0]}{c[1]}' for c in res.chains)}")


def check_run(g, bfs, src):
    res = bfs.run(src)
    got = bfs.levels()
    exp = g.exp[src]
    assert np.array_equal(got, exp), g.name + " " + _describe(src, res, got, exp)
    check_totals_and_records(g, src, res)
    assert bfs.validate(src), (g.name, src)
    return res


def run_case(g, mode, options, roots=None, max_hubs=None):
    """Both roots under `options` in `mode`; the options are put back after."""
    bfs = g.bfs(max_hubs)
    try:
        bfs.mode = mode
        for k, v in options.items():
            bfs.engine.set_option(k, v)
        res = [check_run(g, bfs, s) for s in (roots or g.roots[:2])]
        chain_plans.check("gpu", chain_plans.key("shard", g.name, mode, options, roots or "-", max_hubs), res)
        return res
    finally:
        g.restore()


def forms(results):
    return "|".join("".join(c[1] for c in r.chains) for r in results)


# ---- the thresholds each graph is there for ---------------------------------------


def test_thresholds_crossed(gpu_runtime, shards):
    """A changed constant or another CU count must fail here instead of
    leaving the cases below to cover nothing."""
    cus = gpu_runtime.backend.compute_units
    assert cus > 0
    a, b, c = SPECS["A"][0]().n, SPECS["B"][0]().n, SPECS["C"][0]().n
    ua, ub, uc = (-(-int(x) // UNIT) for x in (a, b, c))
    for n in (a, b, c):
        assert n % UNIT != 0 and n % 64 != 0  # (a partial last unit and last word)
    # A: several scan workgroups; persistent bottom-up workgroups (two per CU,
    # a unit each at 4 words per wave) and the fused update finish's grid
    # (a unit per workgroup below the split bound) loop
    assert ua > N.SCAN_CHUNK and ua > 2 * cus
    assert ua > N.MAX_FUSED_GRID // 8 and ua < N.UPDATE_SPLIT_UNITS
    assert ua * 4 < 2 * cus * 16  # (4 words per wave by default: too few units for the wave slots at 16)
    # B: the unsplit update / compaction; 16 words per wave (4 units per
    # workgroup), more than one pass
    assert ub >= N.UPDATE_SPLIT_UNITS and ub / 4 > 2 * cus
    assert ub > 8 * cus and ub < 2 * cus * 16 and ub <= N.FOLD_SCAN_UNITS
    # C: no folded scan; whole units per wave (16 per workgroup), a second pass
    assert uc > N.FOLD_SCAN_UNITS and uc / 16 > 2 * cus and c >= 1 << 25
    assert uc >= 2 * cus * 16
    # the several-rank cases: C's shard on 2 ranks keeps the unsplit update, on 3 it does not
    assert N.Partition(int(c), 2).slice_words() // 64 >= N.UPDATE_SPLIT_UNITS
    assert N.Partition(int(c), 3).slice_words() // 64 < N.UPDATE_SPLIT_UNITS
    assert shards("A").units == ua


# ---- defaults, device loop and host loop ----------------------------------------------


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("mode", ["td", "bu", "do"])
@pytest.mark.parametrize("graph", ["A", "B", "C"])
def test_defaults_device_loop(shards, graph, mode, narrow):
    run_case(shards(graph), mode, {"narrow_levels": narrow})


@pytest.mark.parametrize("mode", ["td", "do"])
@pytest.mark.parametrize("graph", ["A", "B", "C"])
def test_host_loop(shards, graph, mode):
    """scan_units with its finish and a compaction on every level."""
    res = run_case(shards(graph), mode, {"device_loop": 0})
    assert all(not r.chains for r in res)


# ---- top-down forms ---------------------------------------------------------------------

TD_FORMS = {
    "dense": {"td_sparse_edges": 0},  # every level dense and compacted
    "bytes_default": {},
    "bytes_all": {"td_byte_edges": 0},
    "direct_all": {"td_direct_edges": 0},
    "direct_never": {"td_direct_edges": float(1 << 40)},
    "binned": {"td_bin_edges": 1, "td_bin_min_rows": 0},
}


@pytest.mark.parametrize("form", list(TD_FORMS))
@pytest.mark.parametrize("mode", ["td", "do"])
@pytest.mark.parametrize("graph", ["B", "C"])
def test_top_down_forms(shards, graph, mode, form):
    res = run_case(shards(graph), mode, TD_FORMS[form])
    if form == "dense":
        assert "S" not in forms(res)
    if form == "binned" and mode == "td":  # (bin shift 13 on B, 14 on C)
        assert "X" in forms(res)


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("graph", ["B", "C"])
def test_forced_unvisited_filter(shards, graph, narrow):
    res = run_case(shards(graph), "td", {"td_unvis_edges": 1, "td_unvis_vis_frac": 0.0, "td_unvis_max_density": 1.0,
                                         "narrow_levels": narrow})
    assert any(c[5] for r in res for c in r.chains)


@pytest.mark.parametrize("bits", [1, 0])
@pytest.mark.parametrize("graph", ["B", "C"])
def test_sparse_level_from_bitmap(shards, graph, bits):
    """The sparse level after a bottom-up one: from the output bitmap (above
    the grid cap: several units per wave) or from a compacted list."""
    res = run_case(shards(graph), "do", {"td_sparse_bits": bits})
    assert "BS" in forms(res)


@pytest.mark.parametrize("bitmap", [False, True])
@pytest.mark.parametrize("mode", ["td", "do"])
@pytest.mark.parametrize("graph", ["B", "C"])
def test_split_levels(shards, graph, mode, bitmap):
    """Every direct top-down level split: 4 parts, and on a graph of >= 2^25
    vertices 8 for levels of >= 16 x td_split_edges frontier edges."""
    opts = {"td_split_edges": 1, "td_split_parts": 4, "td_sparse_edges": 0}
    opts.update({"td_direct_edges": float(1 << 40)} if bitmap else {"td_byte_edges": 0})
    res = run_case(shards(graph), mode, opts)
    parts = [c[6] for r in res for c in r.chains]
    if graph == "C":
        assert 8 in parts
    else:
        assert max(parts) <= 4 and 4 in parts


# ---- bottom-up forms ----------------------------------------------------------------------


@pytest.mark.parametrize("whole,small", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
@pytest.mark.parametrize("mode", ["bu", "do"])
@pytest.mark.parametrize("graph", ["A", "B", "C"])
def test_bottom_up_forms(shards, graph, mode, whole, small):
    """Whole units per wave forced and forbidden, 4 words per wave on first
    levels forced and forbidden: every form at every size."""
    run_case(shards(graph), mode, {"bu_whole_units": whole, "bu_small_waves": small})


@pytest.mark.parametrize("mode", ["bu", "do"])
@pytest.mark.parametrize("graph", ["A", "B", "C"])
def test_bottom_up_lane_limit_1(shards, graph, mode):
    run_case(shards(graph), mode, {"bu_lane_limit": 1})


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("cut", [1 << 40, 0])
@pytest.mark.parametrize("mode", ["bu", "do"])
def test_hub_cut(shards, mode, cut, narrow):
    """C's hubs: the hub-cut first bottom-up level on, whatever its frontier's
    edges, and off; 32-bit levels keep the claims in bytes of their own."""
    g = shards("C")
    assert g.bfs().graph.nhubs > 0
    res = run_case(g, mode, {"bu_cut_edges": float(cut), "narrow_levels": narrow})
    cuts = [c[7] for r in res for c in r.chains]
    if cut == 0:
        assert not any(cuts)
    elif mode == "bu":  # (level 0 is a first bottom-up level of a few frontier edges)
        assert any(cuts)


# ---- back-to-back runs, several ranks, parents --------------------------------------------


@pytest.mark.parametrize("mode", ["td", "do"])
def test_run_many_twice(shards, mode):
    """Three roots back to back and the same three again: narrow epochs and
    the clean-frontier shortcut across runs."""
    g = shards("B")
    bfs = g.bfs()
    try:
        bfs.mode = mode
        for _ in range(2):
            res = bfs.run_many(g.roots)
            for r, s in zip(res, g.roots):
                assert r.source == s
                check_totals_and_records(g, s, r)
            last = g.roots[-1]
            got = bfs.levels()
            assert np.array_equal(got, g.exp[last]), _describe(last, res[-1], got, g.exp[last])
            assert bfs.validate(last)
    finally:
        g.restore()


@pytest.mark.parametrize("P", [2, 3])
def test_virtual_ranks(shards, P):
    """C on 2 ranks (4151 units each: the unsplit update with the several-rank
    arguments) and on 3 (2767: the split one), gathered levels exact."""
    g = shards("C")
    srcs = g.roots[:2]

    def body(rt):
        b = dbfs.BFS(g.params, rt, mode="do")
        out = []
        for s in srcs:
            r = b.run(s)
            lv = b.levels()  # (collective)
            out.append((r.reached, r.edges, r.depth, lv if rt.rank == 0 else None, b.validate(s)))
        return out

    outs = run_virtual_ranks(P, body, device="hip")
    for rank_out in outs:
        for (reached, edges, depth, lv, valid), s in zip(rank_out, srcs):
            assert (reached, edges, depth) == (g.reached(s), g.edges(s), g.depth(s))
            assert valid
            if lv is not None:
                assert np.array_equal(lv, g.exp[s]), _describe(s, None, lv, g.exp[s])


@pytest.mark.parametrize("graph", ["A", "C"])
def test_parents(shards, graph):
    """The root its own parent, -1 for unreached vertices, every other
    vertex's parent one level closer -- and, for a seeded sample of 100 000
    reached vertices, in the vertex's row."""
    g = shards(graph)
    bfs = g.bfs()
    for src in g.roots[:2]:
        bfs.run(src)
        par = np.asarray(bfs.parents(src))
        lv = g.exp[src]
        ok = lv != dbfs.UNREACHED
        assert par[src] == src
        assert np.all(par[~ok] == -1)
        ok[src] = False
        v = np.nonzero(ok)[0]
        assert np.all((par[v] >= 0) & (par[v] < g.n))
        assert np.array_equal(lv[par[v]], lv[v] - 1)
        s = np.random.default_rng(11).choice(v, size=min(100000, v.size), replace=False)
        d = g.deg[s]
        owner = np.repeat(np.arange(s.size), d)
        first = np.cumsum(d) - d
        idx = np.repeat(g.row_off[s], d) + (np.arange(int(d.sum())) - np.repeat(first, d))
        hit = np.zeros(s.size, dtype=bool)
        hit[owner[g.col[idx] == par[s][owner]]] = True
        assert hit.all(), (graph, src, s[~hit][:8])
