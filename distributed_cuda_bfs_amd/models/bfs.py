"""High-level distributed BFS.

Reference entry points: ``main`` -> ``runCudaQueueBfs`` (bfs.cu:783-823,
542-629) and the MPI variant (bfs_mpi.cu:797-856).  One ``BFS`` object holds
this rank's CSR shard on its device and a native engine; ``run(src)`` is one
level-synchronous traversal (all ranks call it collectively).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Union

import numpy as np

from .._native import N
from ..parallel.runtime import Runtime, init_runtime

MODES = ("ref", "td", "bu", "do", "simple", "scan")
BATCH_DIRECTIONS = ("auto", "push", "pull", "alternate")


class BFSResult:
    """One traversal: totals, plus per-level records (list of dicts with level,
    dir, frontier, frontier_edges, discovered, ms, comm_ms, gap_ms) converted
    from the native record on first access."""

    __slots__ = ("source", "ms", "reached", "edges", "depth", "gteps", "mispredicts", "_native", "_levels")

    def __init__(self, source: int, ms: float, reached: int, edges: int, depth: int, gteps: float,
                 levels: Optional[List[Dict[str, Any]]] = None, mispredicts: int = 0, native: Any = None):
        self.source, self.ms, self.reached, self.edges = source, ms, reached, edges
        self.depth, self.gteps, self.mispredicts = depth, gteps, mispredicts
        self._native, self._levels = native, levels

    @property
    def chains(self) -> List[Any]:
        """Device loop: every level chain enqueued, in order, as an 8-tuple
        (level, form, cap, gathered, pushed, unvisited filter, parts, hub cut)
        -- form T (dense top-down) / S (sparse top-down) / X (binned top-down)
        / B (bottom-up), mispredicted chains included; cap (index 2): the
        frontier edges a sparse chain stays live for (0: any);
        parts > 1 (index 6): a split top-down level (Options td_split_edges /
        td_split_parts); hub cut (index 7): a first bottom-up level enqueued
        with the hub cut (Options bu_cut_edges)."""
        return list(self._native.chains) if self._native is not None else []

    @property
    def levels(self) -> List[Dict[str, Any]]:
        if self._levels is None:
            self._levels = list(self._native.level_dicts()) if self._native is not None else []
        return self._levels

    def __repr__(self) -> str:
        return (f"BFSResult(source={self.source}, ms={self.ms:.4f}, reached={self.reached}, edges={self.edges}, "
                f"depth={self.depth}, gteps={self.gteps:.2f})")

    @classmethod
    def from_native(cls, r: Any) -> "BFSResult":
        if isinstance(r, dict):
            return cls(r["source"], r["ms"], r["reached"], r["edges"], r["depth"], r["gteps"],
                       levels=list(r["levels"]), mispredicts=int(r.get("mispredicts", 0)))
        return cls(r.source, r.ms, r.reached, r.edges, r.depth, r.gteps, mispredicts=r.mispredicts, native=r)


class BatchResult:
    """One concurrent traversal from k sources (``BFS.run_batch``), 64 sources
    per pass.  Per source, in the order given: ``reached``, ``edges`` (degree
    sum of the reached // 2; on a directed graph their out-degree sum, not
    halved), ``depth`` (max level + 1; on a directed graph ``run().depth`` is
    one lower when no vertex of the deepest level has an out-edge, since a
    single traversal counts the levels it expanded), ``depth`` (levels), ``dist_sum`` (sum of levels
    over the reached) and ``discovered[s][L]`` (vertices source s found at
    level L).  ``levels``: per level of each pass a tuple (pass, level, form,
    active vertices, their edges, host ms), form 'P' push or 'L' pull.  ``wide_levels``:
    the levels are 16-bit (a pass deeper than 254 levels, in this batch or an
    earlier one, was rerun).

    With ``run_batch(validate=True)``: ``violations``, per source a tuple
    (gap, cross, orphan) of the device check's counts over the directed
    adjacency entries -- both ends reached and more than one level apart, one
    end reached and the other not, a reached vertex other than the source
    without a neighbour one level closer (or the source not at level 0); on a
    directed graph, over every stored entry u -> w: both reached and
    level[w] > level[u] + 1, u reached and w not, a reached vertex without an
    in-neighbour one level closer (``utils.validate.directed_levels_violations``)
    -- and ``validated``, True when every count is zero; both None when the check was
    not asked for.  ``check_ms``: wall time of the per-pass checks (validation
    and parents), which ``ms`` never includes; 0.0 without them.

    With ``run_batch(betweenness=True)`` or ``path_counts=True``: ``bc_ms``,
    the wall time of the per-pass path counts and dependency accumulation
    (never part of ``ms`` or ``check_ms``), its ``bc_forward_ms`` /
    ``bc_backward_ms`` parts, ``bc_launches`` (one per level and direction)
    and ``bc_rows_walked`` (the rows those launches walked on this rank: the
    ones with a source on the launch's level); zeros without them.
    ``wide_count_passes``: the passes whose counts ran in the extended-range
    form (``run_batch(wide_counts=True)``: all; ``"auto"``: those redone)."""

    __slots__ = ("sources", "ms", "gteps", "passes", "wide_levels", "reached", "edges", "depth", "dist_sum",
                 "discovered", "levels", "violations", "validated", "check_ms", "bc_ms", "bc_forward_ms",
                 "bc_backward_ms", "bc_launches", "bc_rows_walked", "wide_count_passes")

    def __init__(self, r: Any, validate: bool = False):
        self.violations = [tuple(int(x) for x in v) for v in r.violations] if validate else None
        self.validated = all(v == (0, 0, 0) for v in self.violations) if validate else None
        self.check_ms = float(r.check_ms)
        self.bc_ms, self.bc_forward_ms, self.bc_backward_ms = float(r.bc_ms), float(r.bc_forward_ms), float(r.bc_backward_ms)
        self.bc_launches, self.bc_rows_walked = int(r.bc_launches), int(r.bc_rows_walked)
        self.wide_count_passes = int(r.wide_count_passes)
        self.sources, self.ms, self.gteps, self.passes = list(r.sources), r.ms, r.gteps, r.passes
        self.wide_levels = bool(r.wide_levels)
        self.reached, self.edges, self.depth = list(r.reached), list(r.edges), list(r.depth)
        self.dist_sum, self.discovered, self.levels = list(r.dist_sum), [list(d) for d in r.discovered], list(r.levels)

    def __repr__(self) -> str:
        return (f"BatchResult(sources={len(self.sources)}, passes={self.passes}, ms={self.ms:.4f}, "
                f"gteps={self.gteps:.2f})")


class ComponentsResult:
    """Connected components of the whole graph (``BFS.components``):
    ``components`` (how many), ``largest_label`` / ``largest_size`` (the
    largest one: its smallest vertex id and its vertex count; the smaller
    label on a tie), ``singletons`` (components of one vertex: no entries, or
    only self-loops), ``ms`` (wall time, max over ranks) with its ``link_ms``
    (hook launches; several ranks: the label exchange too) and ``compress_ms``
    (pointer jumping) parts, and ``sampled``: the sample-and-skip form ran
    (one rank, undirected, a non-zero ``sample_entries``)."""

    __slots__ = ("components", "largest_label", "largest_size", "singletons", "ms", "link_ms", "compress_ms", "sampled")

    def __init__(self, r: Any):
        self.components, self.singletons = int(r.components), int(r.singletons)
        self.largest_label, self.largest_size = int(r.largest_label), int(r.largest_size)
        self.ms, self.link_ms, self.compress_ms = float(r.ms), float(r.link_ms), float(r.compress_ms)
        self.sampled = bool(r.sampled)

    def __repr__(self) -> str:
        return (f"ComponentsResult(components={self.components}, largest_label={self.largest_label}, "
                f"largest_size={self.largest_size}, singletons={self.singletons}, ms={self.ms:.4f}, "
                f"sampled={self.sampled})")


class StrongComponentsResult:
    """Strongly connected components of the whole graph
    (``BFS.strong_components``): ``components`` (how many), ``largest_label``
    / ``largest_size`` (the largest one: its smallest vertex id and its vertex
    count; the smaller label on a tie), ``singletons`` (components of one
    vertex), ``trimmed`` (vertices the trim settled), ``rounds`` (rounds of
    trim, colouring and closure), ``sweeps`` (sweep launches of all steps),
    ``pivot`` / ``pivot_size`` (the first round's pivot vertex, -1 when none,
    and the size of its component), ``ms`` (wall time, max over ranks) with
    its ``trim_ms`` and ``colour_ms`` parts."""

    __slots__ = ("components", "largest_label", "largest_size", "singletons", "trimmed", "rounds", "sweeps", "pivot",
                 "pivot_size", "ms", "trim_ms", "colour_ms")

    def __init__(self, r: Any):
        for name in self.__slots__[:9]:
            setattr(self, name, int(getattr(r, name)))
        self.ms, self.trim_ms, self.colour_ms = float(r.ms), float(r.trim_ms), float(r.colour_ms)

    def __repr__(self) -> str:
        return (f"StrongComponentsResult(components={self.components}, largest_label={self.largest_label}, "
                f"largest_size={self.largest_size}, singletons={self.singletons}, trimmed={self.trimmed}, "
                f"rounds={self.rounds}, sweeps={self.sweeps}, pivot={self.pivot}, ms={self.ms:.4f})")


class EccentricityResult:
    """Eccentricities by bounding (``BFS.eccentricities``): ``diameter`` (the
    largest lower bound over the scope) and ``radius`` (the smallest upper
    bound) -- with target ``"all"`` and ``exact`` the scope's diameter and
    radius; target ``"diameter"`` promises ``diameter`` only (``radius`` is then
    an upper bound) and ``"radius"`` the reverse; ``centre`` / ``periphery``
    (settled vertices whose eccentricity equals ``radius`` / ``diameter``),
    ``passes`` (batch passes run) and ``sources`` (traversals in them),
    ``settled`` of ``scope_size`` in-scope vertices, ``exact`` (the loop ended
    by itself, not by ``max_passes``), ``wide_levels`` (a pass needed 16-bit
    levels), ``ms`` (wall time, max over ranks) with its ``bfs_ms`` (the
    passes), ``bound_ms`` (bound updates and totals) and ``select_ms`` (source
    selection) parts."""

    __slots__ = ("diameter", "radius", "centre", "periphery", "passes", "sources", "settled", "scope_size", "exact",
                 "wide_levels", "ms", "bfs_ms", "bound_ms", "select_ms")

    def __init__(self, r: Any):
        for name in self.__slots__[:8]:
            setattr(self, name, int(getattr(r, name)))
        self.exact, self.wide_levels = bool(r.exact), bool(r.wide_levels)
        self.ms, self.bfs_ms, self.bound_ms, self.select_ms = float(r.ms), float(r.bfs_ms), float(r.bound_ms), float(r.select_ms)

    def __repr__(self) -> str:
        return (f"EccentricityResult(diameter={self.diameter}, radius={self.radius}, centre={self.centre}, "
                f"periphery={self.periphery}, settled={self.settled}/{self.scope_size}, passes={self.passes}, "
                f"sources={self.sources}, exact={self.exact}, ms={self.ms:.4f})")


class BFS:
    """Distributed BFS over a graph given as a HostCSR, generator params, or a file path."""

    def __init__(self, graph: Union[str, Any], runtime: Optional[Runtime] = None, mode: str = "do",
                 alpha: float = 40.0, beta: float = 384.0, bu_lane_limit: int = 16, phase_timing: bool = False,
                 hub_sort: bool = True, force_exchange: bool = False, hubs: bool = True,
                 max_hubs: Optional[int] = None, directed: bool = False, sharded: bool = True,
                 read_threads: int = 0, id_order: bool = True):
        """``hub_sort`` reorders every adjacency row by neighbour degree (descending)
        once, before any traversal: levels are unchanged, bottom-up probes find a
        frontier parent sooner (see csrc/kernels/graph_sort.hip).  ``hubs`` also
        indexes the highest-degree vertices so that bottom-up probes of them test
        an LDS-resident copy of their frontier bits (needs ``hub_sort``); with
        hubs and ``id_order`` the top-down copy of the adjacency is then put in
        neighbour-id order (bottom-up keeps the hub-first order).

        A file path is read in shards (``sharded``, the default for undirected
        files): every rank parses only its byte range of an edge list /
        MatrixMarket file with ``read_threads`` host threads and the CSR shard
        is built on its GPU (edges routed to their owners by an all-to-all-v),
        or reads only its rows of a binary CSR cache.  ``sharded=False`` reads
        the whole file on every rank (the reference's bfs_mpi.cu:815 pattern).

        ``directed=True`` keeps the pairs as u -> v edges.  ``run`` then needs a
        top-down mode (``bu`` and ``do`` raise); ``run_batch``, ``validate``
        and ``parents`` work on the graph's in-edge shard, which the first of
        them builds on the device (``build_in_edges`` pays for it up front).  A
        directed file is read whole on every rank."""
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        self.rt = runtime or init_runtime()
        if directed and mode in ("bu", "do"):
            raise ValueError("directed graphs need a top-down mode (td, ref, simple, scan)")
        if isinstance(graph, str) and not (sharded and not directed and graph != "-"):
            graph = N.read_graph(graph, False, directed)
        if isinstance(graph, str):
            self.graph = N.DeviceGraph.from_file(self.rt.backend, self.rt.comm, graph, int(read_threads))
            self.n = self.graph.n
            self.partition = self.graph.partition
        elif isinstance(graph, N.GenParams):
            self.n = graph.n
            self.partition = N.Partition(graph.n, self.rt.world)
            self.graph = N.DeviceGraph.generate(self.rt.backend, graph, self.partition, self.rt.rank)
        elif isinstance(graph, N.HostCSR):
            self.n = graph.n
            self.partition = N.Partition(graph.n, self.rt.world)
            self.graph = N.DeviceGraph.from_host(self.rt.backend, graph, self.partition, self.rt.rank)
        else:
            raise TypeError("graph must be a path, HostCSR or GenParams")
        if hub_sort:
            cap = N.MAX_HUBS if max_hubs is None else int(max_hubs)
            self.graph.sort_neighbors_by_degree(self.rt.comm, hubs, cap, id_order)
        self.engine = N.Engine(self.graph, self.rt.comm, mode=mode, alpha=alpha, beta=beta,
                               bu_lane_limit=bu_lane_limit, phase_timing=phase_timing,
                               force_exchange=force_exchange)
        if directed:  # the CSR holds out-edges only (see build_csr / read_graph)
            self.engine.set_option("directed", 1)

    def build_in_edges(self) -> None:
        """Directed graphs: build the in-edge shard now (collective, one time;
        4 bytes per stored entry + 8 per vertex on the device) instead of in
        the first run_batch / validate / parents call.  Nothing happens, and
        nothing is allocated, on an undirected graph."""
        self.engine.build_in_edges()

    def use_comm(self, comm) -> None:
        """Rebuild the engine on another communicator (same shard, same
        options): e.g. the RCCL communicator a peer-memory one wraps."""
        opts = dict(self.engine.get_options())
        mode = self.engine.mode
        self.rt.comm = comm
        comm.bind_backend(self.rt.backend)
        self.engine = N.Engine(self.graph, comm, mode=mode, alpha=opts["alpha"], beta=opts["beta"],
                               bu_lane_limit=int(opts["bu_lane_limit"]), phase_timing=bool(opts["phase_timing"]),
                               force_exchange=bool(opts["force_exchange"]))
        for k, v in opts.items():
            self.engine.set_option(k, v)

    @property
    def mode(self) -> str:
        return self.engine.mode

    @mode.setter
    def mode(self, m: str) -> None:
        if m not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        self.engine.mode = m

    def run(self, source: int) -> BFSResult:
        return BFSResult.from_native(self.engine.run(int(source)))

    def run_many(self, sources) -> List[BFSResult]:
        """One complete traversal per source, back to back in native code (no
        return to Python between them: the host gap between two traversals is
        the engine's own).  Collective like run()."""
        return [BFSResult.from_native(r) for r in self.engine.run_many([int(s) for s in sources])]

    def run_batch(self, sources, direction: str = "auto", levels: bool = True, validate: bool = False,
                  parents: bool = False, betweenness: bool = False, path_counts: bool = False,
                  wide_counts=False) -> BatchResult:
        """One concurrent traversal from all ``sources`` (64 per pass, one bit
        per source in a 64-bit word per vertex); collective like run().
        ``direction``: "auto" picks push or pull per level (one rank; several
        ranks always pull), "push" / "pull" / "alternate" force a form.  On a
        directed graph a push follows out-edges and a pull searches the
        in-edge shard (build_in_edges; built here on first use, untimed).
        ``levels=False`` keeps no level matrix (64 bytes per vertex on the
        device): the totals are the same, batch_levels() then raises.  The
        single-source state of run() is left alone.

        ``validate=True`` checks every pass's level matrix on the device
        against every edge, for all its sources at once (Graph500's level
        rules, as validate() for one source): ``BatchResult.violations`` /
        ``validated``.  ``parents=True`` also keeps every source's parent tree
        for batch_parents().  Both read the level matrix (``levels=True``) and
        run after each pass's timed window: ``BatchResult.check_ms``, never
        ``ms``.

        ``betweenness=True`` computes, after each pass, the number of shortest
        paths from each of its sources and Brandes' dependencies on the device
        (one launch per level outwards and one per level back, over the level
        matrix) and sums them over all sources for batch_betweenness().
        ``path_counts=True`` keeps the path counts for batch_path_counts().
        Both read the level matrix (``levels=True``) and are timed on their
        own: ``BatchResult.bc_ms``.  512 + 8 bytes per owned vertex on the
        device.  Several ranks use a simple replicated form: correct, not fast.
        The counts are doubles: when a source has more than 2**1024 shortest
        paths to some vertex the call raises (on every rank, naming the source)
        and leaves no result; it never returns a non-finite value.

        ``wide_counts=True`` keeps counts and coefficients as a mantissa and
        an exponent instead (768 + 8 bytes per owned vertex): no count is out
        of range, nothing raises for it, and every rounding is the one the
        doubles would make -- where all counts fit a double the results are
        the same bits.  ``wide_counts="auto"`` runs each pass in doubles and
        redoes only a pass that overflowed in the wide form:
        ``BatchResult.wide_count_passes``.  batch_betweenness() stays float64
        and finite (a single source's share below 2**-1074 counts as 0);
        the counts are read with batch_path_counts_wide()."""
        if isinstance(wide_counts, (bool, np.bool_)):
            counts = "wide" if wide_counts else "double"
        elif isinstance(wide_counts, str) and wide_counts == "auto":
            counts = "auto"
        else:
            raise ValueError('wide_counts must be False, True or "auto"')
        if direction not in BATCH_DIRECTIONS:
            raise ValueError(f"direction must be one of {BATCH_DIRECTIONS}")
        if (validate or parents) and not levels:
            raise ValueError("validate and parents read the level matrix: levels=True")
        if (betweenness or path_counts) and not levels:
            raise ValueError("betweenness and path_counts read the level matrix (keep_levels): levels=True")
        return BatchResult(self.engine.run_batch([int(s) for s in sources], direction, bool(levels), bool(validate),
                                                 bool(parents), bool(betweenness), bool(path_counts), counts),
                           validate=bool(validate))

    def batch_betweenness(self) -> np.ndarray:
        """Dependency sums of the last run_batch(betweenness=True) as float64 [n]:
        dep[v] = the sum, over the source slots i with v != sources[i], of
        Brandes' dependency of sources[i] on v, where parallel (duplicate)
        entries are distinct paths and a source listed twice counts twice.
        Raw: not halved on an undirected graph, not rescaled for sampled
        sources, not normalised -- ``utils.centrality.betweenness_scores`` does
        that.  Collective; raises when the last batch did not ask for it."""
        return self.engine.gather_betweenness()

    def batch_path_counts(self) -> np.ndarray:
        """Shortest-path counts of the last run_batch(path_counts=True) as
        float64 [k, n]: row i holds the number of shortest paths from
        sources[i] to every vertex (1 for the source itself, 0 where it does
        not reach), exact while below 2**53, rounded above (run_batch raises
        where one would pass 2**1024).  k x n x 8 bytes on the host.  After a
        batch with ``wide_counts``: the same doubles when every count fits
        one; otherwise it raises, naming batch_path_counts_wide -- never a
        non-finite value."""
        return self.engine.gather_batch_path_counts()

    def batch_path_counts_wide(self):
        """The same counts as ``(mant float64 [k, n], exp int32 [k, n])`` with
        count == mant * 2.0**exp, in frexp's convention: mant in [0.5, 1), and
        (0.0, 0) for a zero count.  After any run_batch(path_counts=True),
        whatever its ``wide_counts``."""
        return self.engine.gather_batch_path_counts_wide()

    def batch_levels(self) -> np.ndarray:
        """Levels of the last run_batch as int32 [k, n] (UNREACHED where a
        source does not reach); collective."""
        return self.engine.gather_batch_levels()

    def batch_parents(self) -> np.ndarray:
        """Parent trees of the last run_batch(parents=True) as int64 [k, n]:
        row i is source i's tree with the convention of parents() (a neighbour
        one level closer, the first in the stored row; parent[source] = source;
        -1 unreached; a directed graph: the smallest in-neighbour one level
        closer); collective.  k x n x 8 bytes on the host."""
        return self.engine.gather_batch_parents()

    def levels(self) -> np.ndarray:
        """Full per-vertex level array of the last run (collective)."""
        return self.engine.gather_levels()

    def local_levels(self) -> np.ndarray:
        return self.engine.levels_local()

    def parents(self, source: int) -> np.ndarray:
        """Graph500 parent tree of the last run from ``source`` (collective).

        parent[v] is a neighbour one level closer to the source (global vertex
        id; on a directed graph the smallest u with an edge u -> v one level
        closer), parent[source] = source, -1 for unreached vertices.  The reference
        records edge indices as parents and never gathers them (bfs.cu:147,439).
        """
        return self.engine.gather_parents(int(source))

    def validate(self, source: int) -> bool:
        """Graph500-style level validation of the last run on the device
        (collective); a directed graph is checked by the directed rules
        (``utils.validate.directed_levels_violations``)."""
        gap, cross, orphan = self.engine.validate(int(source))
        return gap == 0 and cross == 0 and orphan == 0

    def degree(self, v: int) -> int:
        """Degree of global vertex v (collective: the owner contributes)."""
        own = self.partition.owner(int(v))
        d = 0
        if own == self.rt.rank:
            d = self.graph.degrees_of([int(v) - self.partition.lo(own)])[0]
        return int(self.rt.comm.sum_host(int(d))) if self.rt.world > 1 else int(d)

    def components(self, sample_entries: Optional[int] = None) -> ComponentsResult:
        """Connected components of the whole graph on the device (collective):
        label[v] = the smallest vertex id of v's component; on a directed
        graph the weakly connected components.  A hook-and-compress forest
        over the adjacency (one pass over the entries, then pointer jumping),
        not a traversal per component.  ``sample_entries`` (default: the
        engine option ``cc_sample_entries``, 2): on one rank of an undirected
        graph only that many entries of every row are hooked first, and the
        rows of the component most of a vertex sample then lies in are skipped
        in the pass over the rest; 0 links every entry in one pass, which
        directed graphs and several ranks always do.  The labels are the same
        either way.  Several ranks exchange whole label arrays: correct, not
        fast.  8 bytes per vertex of the whole graph on the device, kept; the
        state of run / run_batch / validate is left alone."""
        return ComponentsResult(self.engine.components(-1 if sample_entries is None else int(sample_entries)))

    def component_labels(self) -> np.ndarray:
        """Labels of the last components() as int64 [n]."""
        return self.engine.gather_components()

    def component_sizes(self) -> np.ndarray:
        """int64 [n]: entry v is the number of vertices in v's component (last components())."""
        return self.engine.gather_component_sizes()

    def strong_components(self, trim_rounds: Optional[int] = None, pivot: Optional[bool] = None) -> StrongComponentsResult:
        """Strongly connected components of the whole graph on the device
        (collective): label[v] = the smallest vertex id of v's strongly
        connected component; on an undirected graph the connected components.
        Rounds of trim (a vertex without a live in- or out-neighbour of its
        class is its own component), forward colouring (the smallest id that
        reaches each vertex, pulled over the in-edges) and backward closure
        (the vertices of a colour that reach its root), each swept until
        nothing changes; no traversal per component.  ``trim_rounds`` (default:
        the engine option ``scc_trim_rounds``, -1): trim sweeps per round at
        most, -1 to the fixed point, 0 none.  ``pivot`` (default: the engine
        option ``scc_pivot``, on): the first round colours only the live vertex
        with the largest in-degree x out-degree, which settles a giant
        component in two reaches.  The labels are the same whatever the
        options.  A directed graph's in-edge shard is built by the first call.
        Several ranks all-gather the state after every sweep: correct, not
        fast.  16 bytes per vertex of the whole graph on the device, kept; the
        state of run / run_batch / validate / components is left alone."""
        return StrongComponentsResult(self.engine.strong_components(
            -2 if trim_rounds is None else int(trim_rounds), -1 if pivot is None else int(bool(pivot))))

    def strong_component_labels(self) -> np.ndarray:
        """Labels of the last strong_components() as int64 [n]."""
        return self.engine.gather_strong_components()

    def strong_component_sizes(self) -> np.ndarray:
        """int64 [n]: entry v is the number of vertices in v's strongly connected component (last strong_components())."""
        return self.engine.gather_strong_component_sizes()

    def eccentricities(self, target: str = "all", component="largest",
                       max_passes: Optional[int] = None) -> EccentricityResult:
        """Exact eccentricities, diameter and radius by eccentricity bounding
        (Takes and Kosters) over 64-source batch passes (collective;
        undirected graphs only -- a directed engine raises).  ecc(v) is the
        largest distance from v within its connected component: 0 for a vertex
        without neighbours, stored duplicates and self-loops change nothing.
        ``component`` is the scope the call answers for: ``"largest"`` the
        largest component, an int the component with that label, ``"all"``
        every vertex (components() runs first if the first two need it).
        ``diameter`` / ``radius`` are the max / min of ecc over the scope: with
        ``"all"`` and a vertex without neighbours the radius is 0.  ``target``:
        ``"all"`` runs until every in-scope vertex is settled; ``"diameter"``
        drops a vertex once its upper bound is no larger than the largest
        lower bound and returns that bound, ``"radius"`` drops one once its
        lower bound is no smaller than the smallest upper bound -- dropped
        vertices stay unsettled with valid bounds.  Every pass picks the 64
        live vertices with the widest bounds (first pass: the largest
        degrees), traverses from all at once and tightens every live vertex's
        bounds from the level matrix; it settles at least its own sources, so
        the loop ends -- a cycle needs a traversal per vertex, n / 64 passes.
        ``max_passes`` ends it early: ``exact`` is then False and the bounds
        stand as they are, nothing raises.  Several ranks hold and update all
        n bounds each, from the all-gathered level matrix: correct, not fast.
        16 bytes per vertex of the whole graph on the device, kept.  run /
        levels(), components() and a later run_batch are left alone; the
        call's passes replace the resident batch pass (validate_batch_pass
        needs a new run_batch)."""
        if isinstance(component, str):
            if component not in ("largest", "all"):
                raise ValueError('component must be "largest", "all" or a component label')
            scope = -2 if component == "largest" else -1
        else:
            scope = int(component)
            if scope < 0:
                raise ValueError('component must be "largest", "all" or a component label')
        if target not in ("all", "diameter", "radius"):
            raise ValueError('target must be "all", "diameter" or "radius"')
        return EccentricityResult(self.engine.eccentricities(
            target, scope, -1 if max_passes is None else max(0, int(max_passes))))

    def eccentricity(self) -> np.ndarray:
        """int32 [n]: the last eccentricities() call's values, -1 where out of scope or unsettled."""
        return self.engine.gather_eccentricities()

    def eccentricity_bounds(self):
        """(lo, hi), int32 [n] each: the last eccentricities() call's bounds;
        (-1, -1) out of scope, hi = INT32_MAX where no source has reached the vertex."""
        return self.engine.gather_eccentricity_bounds()

    def _component_roots(self, k: int, seed: int, component, strong: bool = False) -> List[int]:
        what = "strong_component" if strong else "component"
        if strong and not self.engine.has_strong_components:
            self.strong_components()
        if not strong and not self.engine.has_components:
            self.components()
        if isinstance(component, str):
            if component != "largest":
                raise ValueError(f'{what} must be None, "largest" or a component label')
            last = self.engine.last_strong_components() if strong else self.engine.last_components()
            label = int(last.largest_label)
        else:
            label = int(component)
        labels = self.strong_component_labels() if strong else self.component_labels()
        members = np.nonzero(labels == label)[0]
        roots: List[int] = []
        if members.size >= k:
            for v in np.random.default_rng(seed).permutation(members):
                if len(roots) == k:
                    break
                if self.degree(int(v)) > 0:
                    roots.append(int(v))
        if len(roots) < k:
            raise ValueError(f"{what.replace('_', ' ')} {label} has fewer than {k} vertices of degree >= 1")
        return roots

    def sample_roots(self, k: int, seed: int = 1, component=None, strong_component=None) -> List[int]:
        """Graph500 root sampling: k distinct random vertices of degree >= 1 (collective).
        ``component="largest"`` samples them from the largest connected
        component (running components() first if it has not run), an int from
        the component with that label; raises ValueError when the component
        has fewer than k vertices of degree >= 1.  ``strong_component`` does
        the same over the strongly connected components (strong_components());
        giving both is a ValueError."""
        if component is not None and strong_component is not None:
            raise ValueError("sample_roots takes component or strong_component, not both")
        if strong_component is not None:
            return self._component_roots(int(k), seed, strong_component, strong=True)
        if component is not None:
            return self._component_roots(int(k), seed, component)
        rng = np.random.default_rng(seed)
        roots: List[int] = []
        seen = set()
        tries = 0
        while len(roots) < k and tries < 64 * k + 64:
            tries += 1
            v = int(rng.integers(0, self.n))
            if v in seen:
                continue
            seen.add(v)
            if self.degree(v) > 0:
                roots.append(v)
        return roots
