"""Checks shared by the single-traversal validator tests (test_validator.py on
the CPU backend, test_validator_gpu.py on the GPU): Engine.validate -- the
check behind the benchmark's validated_roots -- must count planted gaps, cross
edges and orphans exactly as the numpy references count them
(batch_levels_violations, on a directed graph directed_levels_violations), and
parents() must keep the first match in the device's own row order."""
import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.utils.validate import batch_levels_violations, directed_levels_violations

import batch_cases as bc
import directed_cases as dc

UNREACHED = dbfs.UNREACHED
GRAPHS = ("rmat13", "star5000", "path300", "d_rmat10")
_cache = {}


def directed(name):
    return name.startswith("d_")


def host_csr(name):
    return dc.host_csr(name) if directed(name) else bc.host_csr(name)


def make_bfs(name, rt):
    if directed(name):
        return dbfs.BFS(host_csr(name), rt, mode="td", directed=True)
    return dbfs.BFS(host_csr(name), rt)


def reference(name, levels, src):
    fn = directed_levels_violations if directed(name) else batch_levels_violations
    return tuple(int(x) for x in fn(host_csr(name), levels, src))


def check_rows(name):
    """The rows the check walks, as a whole-graph (row_off, col, length): the
    adjacency, or on a directed graph its transpose (the in-edges)."""
    if name not in _cache:
        csr = host_csr(name)
        ro = np.asarray(csr.row_off).astype(np.int64)
        col = np.asarray(csr.col).astype(np.int64)
        if directed(name):
            src = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(ro))
            order = np.lexsort((src, col))
            ro = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=csr.n))])
            col = src[order]
        _cache[name] = (ro, col, np.diff(ro))
    return _cache[name]


def root(name):
    """A root that is not the highest-degree vertex, reaches level >= 2 and, where
    the graph has more than one component, leaves vertices unreached."""
    csr = host_csr(name)
    deg = np.diff(np.asarray(csr.row_off))
    if name == "star5000":
        return 5003  # the tail's end: the centre at level 4, its leaves at 5
    if name == "path300":
        return 0
    low = np.nonzero(deg == deg[deg > 0].min())[0]
    for s in low:
        lv = np.asarray(dbfs.cpu_bfs(csr, int(s))[0])
        if lv[lv != UNREACHED].max() >= 3:
            return int(s)
    raise AssertionError("no root of depth >= 3")


def sole_parent(name, levels, lowest=0):
    """(p, child): p >= lowest at level >= 2 is the only vertex one level closer
    in child's row, so child is an orphan once p moves."""
    ro, col, _ = check_rows(name)
    lv = levels.astype(np.int64)
    rows = np.repeat(np.arange(lv.size, dtype=np.int64), np.diff(ro))
    m = (lv[rows] != UNREACHED) & (lv[col] == lv[rows] - 1) & (lv[rows] >= 3)
    pairs = np.unique(rows[m] * lv.size + col[m])
    child, parent = pairs // lv.size, pairs % lv.size
    once = np.bincount(child, minlength=lv.size) == 1
    ok = once[child] & (parent >= lowest)
    assert ok.any(), "no vertex with a single parent"
    i = int(np.nonzero(ok)[0][0])
    return int(parent[i]), int(child[i])


def plantings(name, levels, src, device_rows=None, lowest=0):
    """label -> [(vertex, level)] (level < 0: unreached); vertices >= lowest
    where the planting names one vertex."""
    _, _, length = check_rows(name)
    lv = levels.astype(np.int64)
    reached = lv != UNREACHED
    own = np.arange(lv.size) >= lowest
    p, _ = sole_parent(name, levels, lowest)
    plan = {"1 two deeper": [(p, int(lv[p]) + 2)]}
    near = np.nonzero(reached & (lv == 1) & own)[0]
    v2 = int(near[0]) if near.size else int(np.nonzero(reached & own & (lv > 0))[0][0])
    plan["2 reached to unreached"] = [(v2, -1)]
    lost = np.nonzero(~reached & own)[0]
    if lost.size:
        with_edges = lost[length[lost] > 0]
        plan["3 unreached to level 3"] = [(int(with_edges[0] if with_edges.size else lost[0]), 3)]
    plan["4 source to level 1"] = [(src, 1)]
    hub = int(np.argmax(np.where(own & reached, length, -1)))
    assert hub != src and reached[hub]
    plan["5a hub two deeper"] = [(hub, int(lv[hub]) + 2)]
    plan["5b hub to unreached"] = [(hub, -1)]
    if device_rows is not None:
        ro, col = device_rows
        # (a directed graph: the in-row's last reached entry -- an unreached in-neighbour is legal there)
        row = col[ro[hub]:ro[hub + 1]]
        last = int(row[np.nonzero(reached[row] & (row != src))[0][-1]])
        assert directed(name) or last == row[-1]
        plan["6 last entry of the hub's row to unreached"] = [(last, -1)]
    if name == "rmat13" and lowest == 0:
        # the first two reached vertices with rows above 64 entries that share a wave (64 consecutive rows)
        big = np.nonzero((length > 64) & reached & (np.arange(lv.size) != src))[0]
        pair = np.nonzero(np.diff(big >> 6) == 0)[0]
        a, b = int(big[pair[0]]), int(big[pair[0] + 1])
        assert a >> 6 == b >> 6 and length[a] > 64 and length[b] > 64
        plan["7 two long rows of one wave"] = [(a, int(lv[a]) + 2), (b, -1)]
    return plan


def first_parents(device_rows, levels, src):
    """parent[v] = the first u of v's row, in the device's order, with
    level[u] == level[v] - 1; src for src; -1 without one or unreached."""
    ro, col = device_rows
    lv = levels.astype(np.int64)
    n = lv.size
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    m = (lv[rows] != UNREACHED) & (lv[col] == lv[rows] - 1)
    first = np.full(n, col.size, dtype=np.int64)
    np.minimum.at(first, rows[m], np.nonzero(m)[0])
    par = np.full(n, -1, dtype=np.int64)
    has = first < col.size
    par[has] = col[first[has]]
    par[src] = src
    return par


def device_rows(bfs, name):
    """The rows validate() and parents() walk on the device, one rank."""
    if directed(name):
        bfs.build_in_edges()
        h = bfs.graph.in_edges_to_host()
    else:
        h = bfs.graph.to_host()
    return np.asarray(h.row_off).astype(np.int64), np.asarray(h.col).astype(np.int64)


def clean_run(bfs, name):
    src = root(name)
    bfs.run(src)
    levels = np.asarray(bfs.levels()).copy()
    assert np.array_equal(levels, np.asarray(dbfs.cpu_bfs(host_csr(name), src)[0]))
    assert levels[levels != UNREACHED].max() >= 2
    clean = tuple(bfs.engine.validate(src))
    assert clean == (0, 0, 0) == reference(name, levels, src)
    return src, levels


def run_plantings(bfs, name, src, levels, plan):
    """Every planting alone: validate() is the reference's triple on the
    modified levels and not clean; the old values go back.  Returns the triples."""
    seen = {}
    for label, writes in plan.items():
        mod = levels.copy()
        for v, level in writes:
            bfs.engine.debug_set_level(v, level)
            mod[v] = UNREACHED if level < 0 else level
        assert np.array_equal(bfs.levels(), mod), label
        got = tuple(bfs.engine.validate(src))
        exp = reference(name, mod, src)
        print(f"{name} {label}: validate {got}, reference {exp}")
        for v, _ in writes:
            bfs.engine.debug_set_level(v, -1 if levels[v] == UNREACHED else int(levels[v]))
        assert got == exp, f"{label}: validate {got}, reference {exp}"
        assert got != (0, 0, 0), label
        seen[label] = got
    assert np.array_equal(bfs.levels(), levels)
    assert tuple(bfs.engine.validate(src)) == (0, 0, 0)
    return seen


def planted_one_rank(rt, name):
    bfs = make_bfs(name, rt)
    src, levels = clean_run(bfs, name)
    rows = device_rows(bfs, name)
    plan = plantings(name, levels, src, rows)
    if name in ("rmat13", "d_rmat10"):
        assert "3 unreached to level 3" in plan
    if name in ("rmat13", "star5000"):
        hub = plan["5a hub two deeper"][0][0]
        assert rows[0][hub + 1] - rows[0][hub] > 64 * 2  # the wave's walk takes several steps
    seen = run_plantings(bfs, name, src, levels, plan)
    total = np.sum(np.array(list(seen.values())), axis=0)
    assert total[0] > 0 and total[1] > 0 and total[2] > 0, f"gap, cross, orphan over all plantings: {total}"
    return seen


def ranks_body(name, P):
    csr = host_csr(name)
    lowest = dbfs.native.Partition(csr.n, P).lo(1)

    def body(rt):
        bfs = make_bfs(name, rt)
        src, levels = clean_run(bfs, name)
        plan = plantings(name, levels, src, None, lowest)
        plan = {k: w for k, w in plan.items() if k[0] in "125"}
        assert all(bfs.partition.owner(v) > 0 for w in plan.values() for v, _ in w)
        return run_plantings(bfs, name, src, levels, plan)
    return body


def check_ranks(results):
    assert all(r == results[0] for r in results) and len(results[0]) == 4


def parents_first_match(rt, name):
    """The kernel's documented first-match rule on every vertex, then after
    planting 1 the child left without a parent."""
    bfs = make_bfs(name, rt)
    src, levels = clean_run(bfs, name)
    rows = device_rows(bfs, name)
    par = np.asarray(bfs.parents(src))
    exp = first_parents(rows, levels, src)
    reached = levels != UNREACHED
    assert np.all(par[~reached] == -1) and np.all(par[reached] >= 0)
    assert np.array_equal(par, exp)
    p, child = sole_parent(name, levels)
    bfs.engine.debug_set_level(p, int(levels[p]) + 2)
    mod = levels.copy()
    mod[p] += 2
    par = np.asarray(bfs.parents(src))
    assert par[child] == -1
    assert np.array_equal(par, first_parents(rows, mod, src))
    bfs.engine.debug_set_level(p, int(levels[p]))
    assert np.array_equal(np.asarray(bfs.parents(src)), exp)


def argument_errors(rt, pytest):
    bfs = make_bfs("path300", rt)
    bfs.run(0)
    for v, level in ((-1, 0), (300, 0), (0, UNREACHED)):
        with pytest.raises(Exception, match="debug_set_level"):
            bfs.engine.debug_set_level(v, level)
