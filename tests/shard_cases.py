"""Graphs and checks shared by the shard table tests (test_shard_tables.py on the
CPU backend, test_shard_tables_gpu.py on the GPU): what the build leaves on a
rank -- the sorted adjacency copies, the hub tables, the row heads, the
non-empty-row view -- against the numpy definitions of
distributed_cuda_bfs_amd.utils.shard_reference, every table with
np.array_equal; the device generator and from_edges against build_csr, every
row; the exclusive scan against np.cumsum."""
import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.utils import shard_reference as sr

import directed_cases as dc

N = dbfs.native
LADDER_LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 5000)


def _ladder():
    """16 centres 6000 + k with exactly L distinct leaves among 0..5999 each, L
    around every boundary of the row sorts (one entry / wave sort at 2..64 /
    LDS sort at 65..4096, whose padding to a power of two is exercised by 65,
    127, 129, 255, 257, 4095 / long rows), then five isolated vertices: n =
    6021, no multiple of 64.  The leaves' degrees are 0..7: many key ties."""
    rng = np.random.default_rng(7)
    u, v = [], []
    for k, length in enumerate(LADDER_LENGTHS):
        u.append(np.full(length, 6000 + k))
        v.append(rng.choice(6000, length, replace=False))
    csr = dbfs.build_csr(6021, np.concatenate(u), np.concatenate(v))
    deg = np.diff(np.asarray(csr.row_off))
    assert [int(d) for d in deg[6000:6016]] == list(LADDER_LENGTHS)
    assert set(np.unique(deg[:6000])) == set(range(8)) and np.count_nonzero(deg == 0) == 29
    return csr


# name -> (generator parameters | builder of a HostCSR, directed)
GRAPHS = {
    "ladder": (_ladder, False),
    "rmat13": (dbfs.rmat_params(13, 16, 44), False),
    "rmat17": (dbfs.rmat_params(17, 16, 21), False),
    "powerlaw": (dbfs.power_law_params(20011, 300000, 6000, 3), False),
    "n4097": (dbfs.uniform_params(4097, 10000, 5), False),
    "uniform5000": (dbfs.uniform_params(5000, 12000, 9), False),
    "tiny5": (lambda: dc.host_csr("tiny5"), True),
    "empty3": (lambda: dc.host_csr("empty3"), True),
    "d_rmat10": (lambda: dc.host_csr("d_rmat10"), True),
}
# (graph, max_hubs): every graph at the default cap, the ladder also at 100 (42
# hubs: ties at the threshold are left out), 7 and 0 (no hub at all)
TABLE_CASES = [("ladder", None), ("ladder", 100), ("ladder", 7), ("ladder", 0), ("rmat13", None), ("rmat17", None),
               ("powerlaw", None), ("n4097", None), ("d_rmat10", None)]
RANK_CASES = [("ladder", None), ("ladder", 100), ("rmat13", None), ("n4097", None)]
TINY_CASES = [("tiny5", 4), ("tiny5", 2), ("empty3", 4), ("empty3", 2)]
GENERATED = ("rmat13", "powerlaw", "uniform5000")
_csr_cache = {}
_expected_cache = {}


def generated(name):
    return isinstance(GRAPHS[name][0], N.GenParams)


def host_csr(name):
    if name not in _csr_cache:
        g = GRAPHS[name][0]
        _csr_cache[name] = dbfs.host_csr_from_params(g) if generated(name) else g()
    return _csr_cache[name]


def make_bfs(name, rt, max_hubs=None, hub_sort=True):
    """The BFS as the benchmark builds it: a generated graph on the device, a
    host CSR through from_host."""
    g, directed = GRAPHS[name]
    kw = dict(mode="td", directed=True) if directed else {}
    return dbfs.BFS(g if generated(name) else host_csr(name), rt, max_hubs=max_hubs, hub_sort=hub_sort, **kw)


def expected(name, max_hubs, part, rank):
    key = (name, max_hubs, part.nranks, rank)
    if key not in _expected_cache:
        _expected_cache[key] = sr.expected_shard(host_csr(name), part.lo(rank), part.count(rank), max_hubs,
                                                 part.nranks * part.part)
    return _expected_cache[key]


def snapshot(bfs):
    """One rank's shard and tables, copied to the host."""
    g = bfs.graph
    h = g.to_host()
    return dict(rank=g.rank, lo=g.lo, rows=g.rows, nnz=g.nnz, nhubs=g.nhubs, col_by_id=g.col_by_id,
                hub_sorted=g.hub_sorted, td_hub_share=g.td_hub_share, row_off=np.asarray(h.row_off).copy(),
                col=np.asarray(h.col).copy(), tables=g.debug_tables())


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype, f"{what}: dtype {got.dtype}, expected {exp.dtype}"
    assert got.shape == exp.shape, f"{what}: {got.shape[0]} entries, expected {exp.shape[0]}"
    bad = np.nonzero(got != exp)[0]
    assert np.array_equal(got, exp), (f"{what}: {bad.size} of {got.size} entries differ, first " +
                                      ", ".join(f"[{int(i)}] {int(got[i])} vs {int(exp[i])}" for i in bad[:6]))


def _same_rows(ro, got, exp_sorted, what):
    """Every row holds the multiset of the reference's row (given sorted by id)."""
    _same(sr.sort_rows(ro, np.asarray(got)), exp_sorted, what + " (as multisets per row)")


def check_tables(name, max_hubs, part, s):
    """One rank's snapshot against the definitions."""
    exp = expected(name, max_hubs, part, s["rank"])
    t = s["tables"]
    ro, long_e = exp["row_off"], exp["long_entry"]
    from_host = not generated(name)
    assert (s["lo"], s["rows"], s["nnz"]) == (part.lo(s["rank"]), part.count(s["rank"]), exp["nnz"])
    assert s["hub_sorted"]
    _same(s["row_off"], ro, "row_off")
    hubs = exp["hub_vertex"]
    # ---- the hub set
    assert s["nhubs"] == hubs.size
    _same(t["hub_vertex"], hubs, "hub_vertex")
    _same(t["hub_deg"], exp["hub_deg"], "hub_deg")
    _same(t["hub_bits"], exp["hub_bits"], "hub_bits")
    # ---- hub_col: hub-first, hub-encoded; long rows as the source has them
    hub_col = np.asarray(t["hub_col"])
    assert hub_col.shape == (exp["nnz"],)
    _same(hub_col[~long_e], exp["hub_col"][~long_e], "hub_col, rows up to SORTED_ROW_MAX")
    if from_host:
        _same(hub_col, exp["hub_col"], "hub_col")
    _same_rows(ro, sr.decode(hub_col, hubs), exp["sorted_src"], "hub_col decoded")
    # ---- col: id order with hubs, else the degree order
    assert s["col_by_id"] == exp["col_by_id"]
    col = s["col"]
    _same(col[~long_e], exp["col"][~long_e], "col, rows up to SORTED_ROW_MAX")
    _same_rows(ro, col, exp["sorted_src"], "col")
    if exp["col_by_id"]:
        key = (col >> sr.id_shift(part.n)).astype(np.int64)
        same_row = np.diff(sr.row_index(ro)) == 0
        assert np.all(np.diff(key)[same_row] >= 0), "col: id >> shift is not non-decreasing along a row"
    elif from_host:
        _same(col, exp["col"], "col")
    # ---- td_col: the rank's own col, the top-down hubs encoded
    assert t["td_nhubs"] == exp["td_nhubs"]
    _same(t["td_hub_vertex"], exp["td_hub_vertex"], "td_hub_vertex")
    assert s["td_hub_share"] == exp["td_hub_share"]
    if exp["td_nhubs"]:
        _same(t["td_col"], sr.encode(col, exp["td_hub_vertex"], part.nranks * part.part), "td_col")
    else:
        assert np.asarray(t["td_col"]).size == 0
    # ---- heads: the first entry of every non-empty row of hub_col
    nz, head = sr.heads(ro, hub_col)
    _same(nz, exp["nz_rows"], "non-empty rows")
    got_head = np.asarray(t["head"])
    assert got_head.shape == (s["rows"],) and got_head.dtype == np.uint32
    _same(got_head[nz], head, "head")
    # ---- the non-empty-row view and its records
    _same(t["nz_pref"], exp["nz_pref"], "nz_pref")
    _same(t["nz_row_off"], exp["nz_row_off"], "nz_row_off")
    _same(t["nz_head"], head, "nz_head")
    _same(t["unit_base"], exp["unit_base"], "unit_base")
    _same(t["nz_rec_off"], exp["nz_rec_off"], "nz_rec.off")
    _same(t["nz_rec_head"], head, "nz_rec.head")
    _same(t["nz_loc"], exp["nz_loc"], "nz_loc")
    return exp


def check_graph_facts(name, max_hubs, exp):
    """What the graphs were chosen for (one rank)."""
    length = np.diff(exp["row_off"])
    if name == "ladder":
        assert {None: 5992, 100: 42, 7: 7, 0: 0}[max_hubs] == exp["hub_vertex"].size
    if name == "rmat13":
        assert np.count_nonzero((length >= 2) & (length <= 64)) == 4472
        assert np.count_nonzero((length >= 65) & (length <= 4096)) == 998
        assert length.max() == 7410 and np.count_nonzero(length > 4096) == 1
        assert {63, 64, 65} <= set(length.tolist()) and np.count_nonzero(length == 0) == 1716
    if name == "rmat17":
        assert np.count_nonzero(length) == 90259 > sr.TD_MAX_HUBS and np.count_nonzero(length > 4096) == 19
        assert exp["td_nhubs"] < exp["hub_vertex"].size  # td_col and hub_col encode differently
    if name == "powerlaw":
        assert np.count_nonzero(length == 0) == 0 and np.count_nonzero(length > 4096) == 2
    if name == "d_rmat10":
        # neighbours without out-edges sort last: every row's zero-degree entries are its tail
        deg = sr.padded_degrees(host_csr(name), exp["padded_n"])
        zero = deg[sr.decode(exp["hub_col"], exp["hub_vertex"]).astype(np.int64)] == 0
        assert zero.any()
        same_row = np.diff(sr.row_index(exp["row_off"])) == 0
        assert not np.any(zero[:-1] & ~zero[1:] & same_row)


def tables_one_rank(rt, name, max_hubs):
    bfs = make_bfs(name, rt, max_hubs)
    exp = check_tables(name, max_hubs, bfs.partition, snapshot(bfs))
    check_graph_facts(name, max_hubs, exp)


def ranks_body(name, max_hubs=None, hub_sort=True):
    def body(rt):
        bfs = make_bfs(name, rt, max_hubs, hub_sort)
        return snapshot(bfs)
    return body


def check_ranks(name, max_hubs, P, shots):
    part = N.Partition(host_csr(name).n, P)
    assert [s["rank"] for s in shots] == list(range(P))
    for s in shots:
        check_tables(name, max_hubs, part, s)
        for k in ("hub_vertex", "hub_bits", "hub_deg"):  # the hub set is identical on every rank
            _same(s["tables"][k], shots[0]["tables"][k], f"rank {s['rank']}: {k} against rank 0's")


def check_tiny(name, P, shots):
    """Ranks of one row or none, nnz 0: every table absent or trivial."""
    csr = host_csr(name)
    part = N.Partition(csr.n, P)
    for s in shots:
        check_tables(name, None, part, s)
        t = s["tables"]
        if s["rows"] == 0:
            for k in ("head", "nz_head", "nz_rec_off", "nz_rec_head", "nz_loc", "unit_base", "hub_col", "td_col"):
                assert np.asarray(t[k]).size == 0, k
            assert np.array_equal(t["nz_pref"], [0, 0]) and np.array_equal(t["nz_row_off"], [0])
    if name == "empty3":
        assert all(s["nnz"] == 0 and s["nhubs"] == 0 and not s["col_by_id"] for s in shots)


# ---- construction ----------------------------------------------------------------------


def check_generated(name, part, s):
    """The device generator's shard, unsorted: build_csr's rows, every one as a multiset."""
    ro, src = sr.shard_slice(host_csr(name), part.lo(s["rank"]), part.count(s["rank"]))
    assert not s["hub_sorted"]
    _same(s["row_off"], ro, "row_off")
    _same_rows(ro, s["col"], sr.sort_rows(ro, src), "col")


def edge_list():
    """3000 edges on 700 vertices with duplicates and self-loops, n no multiple of 64."""
    rng = np.random.default_rng(11)
    u, v = rng.integers(0, 700, 3000), rng.integers(0, 700, 3000)
    u[:40], v[:40] = u[100:140], v[100:140]  # duplicates
    v[40:60] = u[40:60]  # self-loops
    return 700, u.astype(np.uint32), v.astype(np.uint32)


def from_edges_body(split):
    n, u, v = edge_list()

    def body(rt):
        part = N.Partition(n, rt.world)
        if split == "rank0":
            mine = slice(0, u.size) if rt.rank == 0 else slice(0, 0)
        else:
            mine = slice(rt.rank, u.size, rt.world)
        g = N.DeviceGraph.from_edges(rt.backend, rt.comm, part, rt.rank, u.size, u[mine], v[mine])
        h = g.to_host()
        return dict(rank=g.rank, lo=g.lo, rows=g.rows, nnz=g.nnz, row_off=np.asarray(h.row_off).copy(),
                    col=np.asarray(h.col).copy())
    return body


def check_from_edges(P, shots):
    n, u, v = edge_list()
    csr = dbfs.build_csr(n, u, v)
    part = N.Partition(n, P)
    assert sum(s["nnz"] for s in shots) == 2 * u.size
    for s in shots:
        ro, src = sr.shard_slice(csr, part.lo(s["rank"]), part.count(s["rank"]))
        assert (s["lo"], s["rows"]) == (part.lo(s["rank"]), part.count(s["rank"]))
        _same(s["row_off"], ro, "row_off")
        _same_rows(ro, s["col"], sr.sort_rows(ro, src), "col")


# ---- scan ------------------------------------------------------------------------------

SCAN_SIZES = [1, 4095, 4096, 4097, 8193, 4096 * 4096, 4096 * 4096 + 1]


def check_scan(backend, n):
    """Backend::exclusive_scan against np.cumsum; the values' sums cross 32
    bits within a few elements.  One 4096-element tile up to 4096, two levels
    up to 4096^2, three above."""
    x = np.random.default_rng(n).integers(0, 1 << 33, n, dtype=np.int64)
    got = backend.debug_exclusive_scan(x)
    assert got.dtype == np.int64 and got.shape == (n + 1,)
    assert got[0] == 0
    assert np.array_equal(got[1:], np.cumsum(x))
