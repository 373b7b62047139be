"""Host-side BFS result checks.

``check_levels_against_oracle`` is the reference's ``checkOutput``
(bfs.cu:374-384): element-wise level equality against the CPU oracle, reporting
the first mismatch.  ``levels_are_consistent`` is the Graph500 level test on the
host (the device version is ``Engine.validate``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

UNREACHED = np.iinfo(np.int32).max


def check_levels_against_oracle(got, expected) -> Optional[Tuple[int, int, int]]:
    got = np.asarray(got)
    expected = np.asarray(expected)
    if got.shape != expected.shape:
        return (-1, int(got.size), int(expected.size))
    bad = np.nonzero(got != expected)[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (i, int(got[i]), int(expected[i]))


def levels_are_consistent(csr, levels, src: int) -> bool:
    lv = np.asarray(levels, dtype=np.int64)
    ro = np.asarray(csr.row_off)
    col = np.asarray(csr.col)
    if lv[src] != 0:
        return False
    rows = np.repeat(np.arange(csr.n), np.diff(ro))
    lu, lw = lv[rows], lv[col]
    ru, rw = lu != UNREACHED, lw != UNREACHED
    if np.any(ru != rw):
        return False
    both = ru & rw
    if np.any(np.abs(lu[both] - lw[both]) > 1):
        return False
    has_parent = np.zeros(csr.n, dtype=bool)
    m = both & (lw == lu - 1)
    has_parent[rows[m]] = True
    reached = lv != UNREACHED
    reached[src] = False
    return bool(np.all(has_parent[reached]))


def batch_levels_violations(csr, levels_row, src: int) -> Tuple[int, int, int]:
    """(gap, cross, orphan) of one source's levels (a row of
    ``BFS.batch_levels()``), counted exactly as the device check of
    ``run_batch(validate=True)`` counts them -- its host reference.  Over the
    directed adjacency entries (u, w) as stored, self-loops and duplicates
    included: gap = both ends reached and more than one level apart; cross =
    exactly one end reached; orphan = reached vertices other than ``src``
    without a neighbour one level closer, plus one if ``src`` is not at level
    0 (unreached included)."""
    lv = np.asarray(levels_row, dtype=np.int64)
    ro = np.asarray(csr.row_off)
    col = np.asarray(csr.col).astype(np.int64)
    n = lv.size
    rows = np.repeat(np.arange(n), np.diff(ro))
    lu, lw = lv[rows], lv[col]
    ru, rw = lu != UNREACHED, lw != UNREACHED
    both = ru & rw
    cross = int(np.count_nonzero(ru != rw))
    gap = int(np.count_nonzero(both & (np.abs(lu - lw) > 1)))
    has_parent = np.zeros(n, dtype=bool)
    has_parent[rows[both & (lw == lu - 1)]] = True
    lone = (lv != UNREACHED) & ~has_parent
    lone[src] = lv[src] != 0
    return gap, cross, int(np.count_nonzero(lone))


def directed_levels_violations(csr, levels_row, src: int) -> Tuple[int, int, int]:
    """(gap, cross, orphan) of one source's levels on a directed CSR (out-edges
    only), counted exactly as the device check counts them on a directed
    engine.  Over every stored entry u -> w, duplicates and self-loops
    included: cross = u reached and w unreached (the reverse is legal); gap =
    both reached and level[w] > level[u] + 1 (a back edge is legal); orphan =
    reached vertices v other than ``src`` without an entry u -> v with
    level[u] == level[v] - 1, plus one if ``src`` is not at level 0 (unreached
    included).  All zero exactly when the levels are the BFS distances."""
    lv = np.asarray(levels_row, dtype=np.int64)
    ro = np.asarray(csr.row_off)
    w = np.asarray(csr.col).astype(np.int64)
    n = lv.size
    u = np.repeat(np.arange(n), np.diff(ro))
    lu, lw = lv[u], lv[w]
    ru, rw = lu != UNREACHED, lw != UNREACHED
    both = ru & rw
    cross = int(np.count_nonzero(ru & ~rw))
    gap = int(np.count_nonzero(both & (lw > lu + 1)))
    has_parent = np.zeros(n, dtype=bool)
    has_parent[w[both & (lu == lw - 1)]] = True
    lone = (lv != UNREACHED) & ~has_parent
    lone[src] = lv[src] != 0
    return gap, cross, int(np.count_nonzero(lone))


def directed_first_parents(csr, levels_row, src: int) -> np.ndarray:
    """The parent tree the device derives from one source's levels on a directed
    CSR, int64[n]: parent[v] = the smallest u with a stored entry u -> v and
    level[u] == level[v] - 1, parent[src] = src, -1 for unreached vertices (and
    for a reached one without such an entry)."""
    lv = np.asarray(levels_row, dtype=np.int64)
    ro = np.asarray(csr.row_off)
    w = np.asarray(csr.col).astype(np.int64)
    n = lv.size
    u = np.repeat(np.arange(n), np.diff(ro))
    lu, lw = lv[u], lv[w]
    m = (lu != UNREACHED) & (lw != UNREACHED) & (lu == lw - 1)
    par = np.full(n, n, dtype=np.int64)
    np.minimum.at(par, w[m], u[m])
    par[par == n] = -1
    par[lv == UNREACHED] = -1
    par[src] = src
    return par


def parents_are_valid(csr, levels, parents, src: int) -> bool:
    """Graph500 parent-tree check: every reached v != src has an edge to
    parent[v] and level[parent[v]] == level[v] - 1; unreached have -1."""
    lv = np.asarray(levels, dtype=np.int64)
    par = np.asarray(parents, dtype=np.int64)
    ro = np.asarray(csr.row_off)
    col = np.asarray(csr.col)
    if par[src] != src:
        return False
    for v in range(csr.n):
        if v == src:
            continue
        if lv[v] == UNREACHED:
            if par[v] != -1:
                return False
            continue
        p = par[v]
        if p < 0 or lv[p] != lv[v] - 1:
            return False
        if p not in col[ro[v]:ro[v + 1]]:
            return False
    return True


def component_labels_reference(csr) -> np.ndarray:
    """Connected-component labels by numpy min-label propagation, int64[n]:
    label[v] = the smallest vertex id of v's component, every stored entry
    u -> w joining u and w (a directed CSR: weak connectivity).  Each round
    gives both ends of every entry the smaller of their labels and then jumps
    every pointer to its label's label until nothing moves; labels only fall,
    so the fixed point is the component minimum.  O(log n) rounds on the
    graphs of the tests; independent of cpu_components and of the backends."""
    ro = np.asarray(csr.row_off)
    w = np.asarray(csr.col).astype(np.int64)
    n = int(csr.n)
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    label = np.arange(n, dtype=np.int64)
    while True:
        low = np.minimum(label[u], label[w])
        new = label.copy()
        # hook the labels themselves (the roots), not only the two vertices
        np.minimum.at(new, label[u], low)
        np.minimum.at(new, label[w], low)
        while True:
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            return label
        label = new


def strong_component_labels_reference(csr) -> np.ndarray:
    """Strongly-connected-component labels by numpy peeling, int64[n]:
    label[v] = the smallest vertex id of v's strongly connected component over
    the stored entries u -> w (self-loops ignored).  Among the entries whose
    two ends are still unlabelled: vertices without an in- or an out-entry are
    peeled as their own components until none is left; then the smallest
    unlabelled vertex p is taken, its forward and its backward reachability
    closures are grown with np.minimum.at until they stop growing, and their
    intersection is p's component, labelled p (nothing smaller is unlabelled).
    One closure pair per component of two or more vertices, each step a pass
    over all remaining entries: slow, for tests only; independent of
    cpu_strong_components and of the backends."""
    ro = np.asarray(csr.row_off)
    n = int(csr.n)
    w = np.asarray(csr.col).astype(np.int64)
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    keep = u != w
    u, w = u[keep], w[keep]
    label = np.full(n, -1, dtype=np.int64)

    def closure(start, src, dst):
        far = np.ones(n, dtype=np.int64)  # 0: reached
        far[start] = 0
        while True:
            before = int(far.sum())
            np.minimum.at(far, dst, far[src])
            if int(far.sum()) == before:
                return far == 0

    while True:
        while True:
            live = (label[u] < 0) & (label[w] < 0)
            u, w = u[live], w[live]
            alone = (label < 0) & ((np.bincount(u, minlength=n) == 0) | (np.bincount(w, minlength=n) == 0))
            if not alone.any():
                break
            label[alone] = np.nonzero(alone)[0]
        rest = np.nonzero(label < 0)[0]
        if rest.size == 0:
            return label
        p = int(rest[0])
        label[closure(p, u, w) & closure(p, w, u)] = p


def _batch_levels_reference(ro, col, n, src) -> np.ndarray:
    """Levels from up to 64 sources at once, int32 [n, k] (-1 unreached): one
    bit per source in a word per vertex, every level one OR-reduction of the
    neighbours' frontier words over each row (np.bitwise_or.reduceat)."""
    k = len(src)
    shifts = np.arange(k, dtype=np.uint64)
    seen = np.zeros(n, dtype=np.uint64)
    seen[src] = np.uint64(1) << shifts  # (distinct sources)
    dist = np.full((n, k), -1, dtype=np.int32)
    dist[src, np.arange(k)] = 0
    has = np.diff(ro) > 0
    starts = ro[:-1][has]
    front = seen.copy()
    level = 0
    while col.size and front.any():
        level += 1
        acc = np.zeros(n, dtype=np.uint64)
        # (rows without entries take no part: the starts of the others delimit exactly their entries)
        acc[has] = np.bitwise_or.reduceat(front[col], starts)
        new = acc & ~seen
        idx = np.nonzero(new)[0]
        if idx.size == 0:
            break
        bits = ((new[idx, None] >> shifts[None, :]) & np.uint64(1)).astype(bool)
        sub = dist[idx]
        sub[bits] = level
        dist[idx] = sub
        seen |= new
        front = new
    return dist


def eccentricity_bounding_reference(csr, scope_mask, target: str = "all", max_passes: Optional[int] = None):
    """Eccentricity bounding (Takes and Kosters) as BFS.eccentricities runs it,
    in numpy: ``(lo, hi, settled, passes, sources_used)`` -- int32 [n] bounds
    ((-1, -1) out of scope, hi = INT32_MAX where no source reached), the bool
    [n] mask of settled vertices, the passes of at most 64 sources and the
    traversals in them.  In scope: lo = 0, hi = INT32_MAX and live; a row
    without entries is settled at 0.  Every pass first drops the live vertices
    the target no longer needs (``"diameter"``: hi <= max lo over the scope,
    ``"radius"``: lo >= min hi), then takes its sources among the live ones --
    first pass: the 64 of largest stored row length, ties to the smaller id;
    later: the 32 of largest hi (ties to the smaller id), then of the rest
    those of smallest lo (ties to the smaller id) up to 64 in all -- traverses
    from all of them and, for every live v and source s at distance d with
    eccentricity e, sets lo[v] = max(lo[v], d, e - d), hi[v] = min(hi[v], e +
    d); bounds that meet settle v.  Ends when nothing is live or after
    ``max_passes``.  Independent of cpu_eccentricities and of the backends."""
    if target not in ("all", "diameter", "radius"):
        raise ValueError('target must be "all", "diameter" or "radius"')
    ro = np.asarray(csr.row_off).astype(np.int64)
    col = np.asarray(csr.col).astype(np.int64)
    n = int(csr.n)
    inf = np.iinfo(np.int32).max
    deg = np.diff(ro)
    scope = np.asarray(scope_mask, dtype=bool)
    lo = np.where(scope, 0, -1).astype(np.int64)
    hi = np.where(scope, np.where(deg == 0, 0, inf), -1).astype(np.int64)
    settled = scope & (deg == 0)
    live = scope & (deg > 0)
    passes = sources_used = 0
    while True:
        if scope.any() and target == "diameter":
            live &= ~(hi <= lo[scope].max())
        if scope.any() and target == "radius":
            live &= ~(lo >= hi[scope].min())
        if max_passes is not None and passes >= max_passes:
            break
        cand = np.nonzero(live)[0]
        if cand.size == 0:
            break
        if passes == 0:
            src = cand[np.lexsort((cand, -deg[cand]))[:64]]
        else:
            first = cand[np.lexsort((cand, -hi[cand]))[:32]]
            rest = np.setdiff1d(cand, first)
            src = np.concatenate([first, rest[np.lexsort((rest, lo[rest]))[:64 - first.size]]])
        dist = _batch_levels_reference(ro, col, n, src).astype(np.int64)
        ecc = dist.max(axis=0)
        d = dist[live]
        reached = d >= 0
        lo[live] = np.maximum(lo[live], np.where(reached, np.maximum(d, ecc[None, :] - d), 0).max(axis=1))
        hi[live] = np.minimum(hi[live], np.where(reached, ecc[None, :] + d, inf).min(axis=1))
        met = live & (lo >= hi)
        settled |= met
        live &= ~met
        passes += 1
        sources_used += int(src.size)
    return lo.astype(np.int32), hi.astype(np.int32), settled, passes, sources_used
