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
