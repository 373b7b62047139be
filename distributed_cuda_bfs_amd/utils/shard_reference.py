"""numpy definitions of a rank's built shard and its derived tables.

What ``DeviceGraph.sort_neighbors_by_degree`` leaves on a rank (``to_host()``
and ``debug_tables()``), written from the definitions and not from the build's
kernels: the hub threshold and hub set, the hub-first hub-encoded adjacency
``hub_col``, the id-ordered ``col``, the top-down encoding ``td_col``, the row
heads and the non-empty-row view.  Integer-only and exact; the tests compare
with ``np.array_equal``.

``deg`` is every vertex's global degree (a directed graph: its out-degree) over
the padded vertex range ``P * part``; vertices >= n have degree 0.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np

from .._native import N

SORTED_ROW_MAX = int(N.SORTED_ROW_MAX)
HUB_FLAG = int(N.HUB_FLAG)
TD_MAX_HUBS = int(N.TD_MAX_HUBS)
MAX_HUBS = int(N.MAX_HUBS)
UNIT = int(N.UNIT_VERTICES)


def padded_degrees(csr, padded_n: int) -> np.ndarray:
    deg = np.zeros(int(padded_n), dtype=np.int64)
    deg[:csr.n] = np.diff(np.asarray(csr.row_off))
    return deg


def hub_threshold(deg: np.ndarray, cap: int) -> Optional[int]:
    """The smallest d >= 1 with |{v : deg[v] >= d}| <= cap, None if there is
    none.  (|{v : deg[v] >= max(deg) + 1}| = 0, so one exists for every cap
    >= 0; ties at the threshold are left out, so fewer than cap vertices may
    qualify -- none at all with cap 0.)"""
    if cap < 0:
        return None
    hist = np.bincount(deg)
    at_least = np.cumsum(hist[::-1])[::-1]  # at_least[d] = |{v : deg[v] >= d}|
    ok = np.nonzero(at_least[1:] <= cap)[0]
    return int(ok[0]) + 1 if ok.size else int(hist.size)


def hub_set(deg: np.ndarray, cap: int) -> np.ndarray:
    """Ascending ids of the vertices of degree >= hub_threshold(deg, cap)."""
    d = hub_threshold(deg, cap)
    if d is None:
        return np.zeros(0, dtype=np.uint32)
    return np.nonzero(deg >= d)[0].astype(np.uint32)


def encode(ids: np.ndarray, hubs: np.ndarray, padded_n: int) -> np.ndarray:
    """enc(v) = HUB_FLAG | index for a hub (index: its position in the
    ascending hub list), v otherwise."""
    idx = np.full(int(padded_n), -1, dtype=np.int64)
    idx[hubs] = np.arange(hubs.size)
    v = np.asarray(ids).astype(np.int64)
    k = idx[v]
    return np.where(k >= 0, HUB_FLAG | k, v).astype(np.uint32)


def decode(enc: np.ndarray, hubs: np.ndarray) -> np.ndarray:
    e = np.asarray(enc).astype(np.int64)
    is_hub = (e & HUB_FLAG) != 0
    out = e.copy()
    if hubs.size:
        out[is_hub] = hubs[np.minimum(e[is_hub] & (HUB_FLAG - 1), hubs.size - 1)]
    assert not np.any(is_hub & ((e & (HUB_FLAG - 1)) >= hubs.size)), "a hub index past the hub list"
    return out.astype(np.uint32)


def bitmap(ids: np.ndarray, words: int) -> np.ndarray:
    bits = np.zeros(int(words), dtype=np.uint64)
    v = np.asarray(ids).astype(np.int64)
    np.bitwise_or.at(bits, v >> 6, np.uint64(1) << (v & 63).astype(np.uint64))
    return bits


def id_shift(n: int) -> int:
    """Long rows of an id-ordered ``col`` are ordered by id >> id_shift(n)."""
    bits = 0
    while (1 << bits) < n:
        bits += 1
    return max(0, bits - 12)


def shard_slice(csr, lo: int, rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """(row_off relative to the slice, col) of rows [lo, lo + rows) of a whole-graph CSR."""
    ro = np.asarray(csr.row_off)[lo:lo + rows + 1].astype(np.int64)
    col = np.asarray(csr.col)[ro[0]:ro[-1]] if rows > 0 else np.zeros(0, dtype=np.uint32)
    return ro - (ro[0] if ro.size else 0), col.astype(np.uint32)


def row_index(row_off: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(row_off.size - 1, dtype=np.int64), np.diff(row_off))


def sort_rows(row_off: np.ndarray, col: np.ndarray, deg: Optional[np.ndarray] = None) -> np.ndarray:
    """Every row of ``col`` sorted by id, or with ``deg`` by (deg descending, id
    ascending).  One sort of (row, rank of the neighbour in that order) pairs
    packed into 64 bits; the ranks are a permutation of the ids."""
    ids = np.asarray(col).astype(np.int64)
    if deg is None:
        rank = vertex = None
    else:
        vertex = np.lexsort((np.arange(deg.size), -deg))  # vertex[k]: the k-th vertex in the order
        rank = np.empty(deg.size, dtype=np.int64)
        rank[vertex] = np.arange(deg.size)
    key = np.sort((row_index(row_off) << 32) | (ids if rank is None else rank[ids]))
    low = key & 0xFFFFFFFF
    return (low if vertex is None else vertex[low]).astype(np.uint32)


def expected_shard(csr, lo: int, rows: int, max_hubs: Optional[int], padded_n: int) -> Dict[str, Any]:
    """The tables of rows [lo, lo + rows) of ``csr`` after a degree sort with
    hubs, id order and top-down hubs (the defaults).  Entries of rows above
    SORTED_ROW_MAX (``long_entry``) are given in the source row's order, which
    a shard loaded from the host keeps; a shard built on the device holds the
    same multiset there.  Heads are not here: they are the first entries of
    the shard's own rows (``heads``)."""
    cap = MAX_HUBS if max_hubs is None else int(max_hubs)
    deg = padded_degrees(csr, padded_n)
    ro, src = shard_slice(csr, lo, rows)
    nnz = int(ro[-1]) if ro.size else 0
    length = np.diff(ro)
    long_entry = np.repeat(length > SORTED_ROW_MAX, length)
    out: Dict[str, Any] = {"row_off": ro, "src_col": src, "long_entry": long_entry, "nnz": nnz,
                           "padded_n": int(padded_n)}

    hubs = hub_set(deg, cap)
    out["min_deg"] = hub_threshold(deg, cap)
    out["hub_vertex"] = hubs
    out["hub_deg"] = deg[hubs].astype(np.uint32)
    out["hub_bits"] = bitmap(hubs, padded_n // 64) if hubs.size else np.zeros(0, dtype=np.uint64)

    by_deg = sort_rows(ro, src, deg)
    by_deg[long_entry] = src[long_entry]
    out["hub_col"] = encode(by_deg, hubs, padded_n)
    out["col_by_id"] = bool(hubs.size > 0)
    out["sorted_src"] = sort_rows(ro, src)  # every row as a sorted multiset
    if out["col_by_id"]:
        by_id = out["sorted_src"].copy()
        by_id[long_entry] = src[long_entry]
        out["col"] = by_id
    else:
        out["col"] = by_deg

    td = hub_set(deg, min(TD_MAX_HUBS, cap)) if hubs.size else np.zeros(0, dtype=np.uint32)
    out["td_hub_vertex"] = td
    out["td_nhubs"] = int(td.size)
    total = int(deg.sum())
    # (both sums are integers below 2^53 and there is one division: exact in a double)
    out["td_hub_share"] = float(int(deg[td].sum())) / float(total) if td.size and total else 0.0

    nz = np.nonzero(length > 0)[0]
    words = max((rows + 63) // 64, 1)
    per_word = np.bincount(nz >> 6, minlength=words)[:words]
    out["nz_rows"] = nz
    out["nz_pref"] = np.concatenate([[0], np.cumsum(per_word)]).astype(np.int64)
    out["nz_row_off"] = np.concatenate([ro[nz], [nnz]]).astype(np.int64)
    if rows > 0:
        units = (rows + UNIT - 1) // UNIT
        base = ro[np.minimum(np.arange(units + 1, dtype=np.int64) * UNIT, rows)]
        out["unit_base"] = base.astype(np.int64)
        out["nz_rec_off"] = (ro[nz] - base[nz // UNIT]).astype(np.uint32)
        out["nz_loc"] = (nz % UNIT).astype(np.uint16)
    else:
        out["unit_base"] = np.zeros(0, dtype=np.int64)
        out["nz_rec_off"] = np.zeros(0, dtype=np.uint32)
        out["nz_loc"] = np.zeros(0, dtype=np.uint16)
    return out


def heads(row_off: np.ndarray, first_table: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(non-empty rows, their heads): head[r] is the first entry of row r in
    ``first_table`` -- the shard's ``hub_col``, or its ``col`` without one."""
    nz = np.nonzero(np.diff(row_off) > 0)[0]
    return nz, np.asarray(first_table)[row_off[nz]].astype(np.uint32)
