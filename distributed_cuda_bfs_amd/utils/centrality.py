"""Betweenness centrality scores from the raw dependency sums of
``BFS.batch_betweenness()`` (Brandes 2001; sampled sources: Brandes & Pich 2007).
"""
from __future__ import annotations

import numpy as np


def betweenness_scores(dep, n: int, k: int, directed: bool, normalized: bool = False,
                       rescale: bool = True) -> np.ndarray:
    """``dep``: float64 [n], the sum over k source slots of each source's
    dependency on every vertex, as the batch returns it.

    * An undirected graph counts every pair {s, t} from both ends: x 1/2.
    * ``rescale`` and k < n: the k sources are a sample of the n vertices, the
      sum is extrapolated x n / k.
    * ``normalized``: divided by the number of pairs a vertex can lie between
      -- (n - 1)(n - 2) ordered pairs on a directed graph, (n - 1)(n - 2) / 2
      unordered ones on an undirected graph (after the halving), so a score
      is the mean fraction of shortest paths through the vertex, in [0, 1].
    """
    n, k = int(n), int(k)
    if k < 1:
        raise ValueError("betweenness_scores: k must be >= 1")
    out = np.array(dep, dtype=np.float64, copy=True)
    if out.shape != (n,):
        raise ValueError(f"betweenness_scores: expected {n} values, got shape {out.shape}")
    if not directed:
        out *= 0.5
    if rescale and k < n:
        out *= n / k
    if normalized and n > 2:
        pairs = (n - 1) * (n - 2)
        out /= pairs if directed else pairs / 2
    return out
