"""Graphs and checks shared by the connected-components tests
(test_components.py on the CPU backend, test_components_gpu.py on the GPU):
BFS.components / component_labels / component_sizes against two independent
references -- the sequential union-find oracle cpu_components and the numpy
label propagation utils.validate.component_labels_reference -- always with
np.array_equal: label[v] is the smallest vertex id of v's component, so the
answer is unique and nothing is compared up to renaming.

FACTS are properties of the graphs (computed once with scipy.sparse.csgraph on
the generators' host CSRs), asserted as literals; where a graph has none the
totals come from the oracle's labels."""
import json
import os
import socket
import subprocess

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks
from distributed_cuda_bfs_amd.utils.validate import component_labels_reference

import directed_cases as dc
import shard_cases as sc

N = dbfs.native
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "data")
SAMPLE_SETTINGS = (0, 2)


def _path(order):
    """The path on 3000 vertices whose k-th vertex has id order[k]."""
    order = np.asarray(order)
    return dbfs.build_csr(order.size, order[:-1], order[1:])


def _zigzag(n):
    """0, n - 1, 1, n - 2, ...: every edge joins a low id and a high one."""
    z = np.empty(n, dtype=np.int64)
    z[0::2] = np.arange((n + 1) // 2)
    z[1::2] = n - 1 - np.arange(n // 2)
    return z


def _max_id_star():
    """Vertex n - 1 joined to all of 0..4998: every hook contends on one root,
    which is then re-rooted under ever smaller ids."""
    return dbfs.build_csr(5000, np.full(4999, 4999), np.arange(4999))


def planted_edge_list():
    """shard_cases.edge_list() (700 vertices, duplicates, self-loops) and two
    more vertices: 700 has only a self-loop (two stored entries, its own component), 701
    has no entry at all."""
    n, u, v = sc.edge_list()
    return n + 2, np.concatenate([u, [700]]).astype(np.uint32), np.concatenate([v, [700]]).astype(np.uint32)


def _edge_list_csr():
    n, u, v = planted_edge_list()
    return dbfs.build_csr(n, u, v)


TIER_LENGTHS = (31, 32, 33, 34, 35, 1023, 1024, 1025, 1026, 1027)
TIER_CENTRE = 7990  # centre k has id TIER_CENTRE + k
TIER_DECOY = 2000


def _tiers(directed=False):
    """Ten stars whose centres 7990 + k have exactly L leaves: L and, with the
    sampled form's first 2 entries gone, L - 2 lie on both sides of cc_link's
    lane tier (a range of up to 32 entries) and wave tier (up to 1024).  Every
    star has leaves of its own among the shuffled ids 0..5289, so no centre is
    in the largest component, whose rows the sampled form skips: that is a
    path on the 2000 shuffled ids 5290..7289.  The rest is isolated: n = 8005.
    Undirected, every edge is also stored in its leaf's row, which hooks it
    whatever the centre's walk leaves out; directed (centre -> leaf only, never
    sampled) an entry the walk of its row skips is hooked nowhere."""
    rng = np.random.default_rng(11)
    leaves = rng.permutation(sum(TIER_LENGTHS))
    ends = np.cumsum(TIER_LENGTHS)
    u = [np.full(length, TIER_CENTRE + k) for k, length in enumerate(TIER_LENGTHS)]
    v = [leaves[e - length:e] for e, length in zip(ends, TIER_LENGTHS)]
    decoy = leaves.size + rng.permutation(TIER_DECOY)
    assert decoy.max() < TIER_CENTRE
    csr = dbfs.build_csr(8005, np.concatenate(u + [decoy[:-1]]).astype(np.uint32),
                         np.concatenate(v + [decoy[1:]]).astype(np.uint32), directed=directed)
    deg = np.diff(np.asarray(csr.row_off))
    assert [int(d) for d in deg[TIER_CENTRE:TIER_CENTRE + len(TIER_LENGTHS)]] == list(TIER_LENGTHS)
    back = 0 if directed else 1  # entries of the edges' other ends
    assert np.all(deg[:leaves.size] == back) and deg[leaves.size:TIER_CENTRE].max() == 1 + back
    return csr


# name -> (generator parameters | builder of a HostCSR | file path, directed)
GRAPHS = {
    "rmat13": (dbfs.rmat_params(13, 16, 44), False),
    "rmat10": (dbfs.rmat_params(10, 16, 3), False),
    "sparse20000": (dbfs.uniform_params(20000, 9000, 3), False),
    "partial20000": (dbfs.uniform_params(20000, 11000, 3), False),
    "n4097": (dbfs.uniform_params(4097, 10000, 5), False),
    "ladder": (sc._ladder, False),
    "cc_tiers": (_tiers, False),
    "grid70x60": (dbfs.grid_params(70, 60), False),
    "path_desc": (lambda: _path(np.arange(3000)[::-1]), False),
    "path_asc": (lambda: _path(np.arange(3000)), False),
    "path_zigzag": (lambda: _path(_zigzag(3000)), False),
    "max_id_star": (_max_id_star, False),
    "edge_list": (_edge_list_csr, False),
    "two_components": (os.path.join(DATA, "two_components.txt"), False),
    "chain8": (os.path.join(DATA, "chain8.txt"), False),
    "tiny5": (lambda: dc.host_csr("tiny5"), True),
    "empty3": (lambda: dc.host_csr("empty3"), True),
    "d_rmat10": (lambda: dc.host_csr("d_rmat10"), True),
    "one_way_bridge": (lambda: dc.host_csr("one_way_bridge"), True),
    "star_in5000": (lambda: dc.host_csr("star_in5000"), True),
    "star_out5000": (lambda: dc.host_csr("star_out5000"), True),
    "back_edge10": (lambda: dc.host_csr("back_edge10"), True),
    "cc_tiers_out": (lambda: _tiers(directed=True), True),
}
# graph facts: n, components, largest (size), label (of the largest), singletons, pairs (components of size 2),
# multi (components of size >= 2)
FACTS = {
    "rmat13": dict(n=8192, components=1718, largest=6474, label=2, singletons=1716, pairs=1),
    "rmat10": dict(n=1024, components=130, largest=895, label=0, singletons=129),
    "sparse20000": dict(n=20000, components=11000, largest=153, label=57, singletons=8141, multi=2859),
    "partial20000": dict(n=20000, components=9016, largest=3573, label=0),
    "n4097": dict(n=4097, components=33, largest=4064),
    "ladder": dict(n=6021),
    "cc_tiers": dict(n=8005, components=716, largest=2000, label=5290, singletons=705, multi=11),
    "cc_tiers_out": dict(n=8005, components=716, largest=2000, label=5290, singletons=705, multi=11),
    "grid70x60": dict(n=4200, components=1, largest=4200, label=0, singletons=0),
    "path_desc": dict(n=3000, components=1, label=0),
    "path_asc": dict(n=3000, components=1, label=0),
    "path_zigzag": dict(n=3000, components=1, label=0),
    "max_id_star": dict(n=5000, components=1, label=0),
    "empty3": dict(n=3, components=3, largest=1, label=0, singletons=3),
}
UNDIRECTED = [g for g, (_, d) in GRAPHS.items() if not d]
DIRECTED = [g for g, (_, d) in GRAPHS.items() if d]
HUB_SORT_BOTH = ("rmat13", "rmat10", "ladder", "cc_tiers", "cc_tiers_out")
# (graph, hub_sort): every graph as the BFS builds it, the RMAT, ladder and tier graphs also unsorted
CASES = [(g, True) for g in GRAPHS] + [(g, False) for g in HUB_SORT_BOTH]
RANK_CASES = ["rmat13", "sparse20000", "n4097", "ladder", "cc_tiers", "cc_tiers_out", "one_way_bridge",
              "path_desc"]
TINY_RANK_CASES = ["tiny5", "empty3"]

_csr_cache = {}
_oracle_cache = {}
_bfs_cache = {}


def host_csr(name):
    if name not in _csr_cache:
        g, directed = GRAPHS[name]
        if isinstance(g, N.GenParams):
            _csr_cache[name] = dbfs.host_csr_from_params(g)
        elif isinstance(g, str):
            _csr_cache[name] = dbfs.read_graph(g)
        else:
            _csr_cache[name] = g()
    return _csr_cache[name]


def symmetrised(csr):
    ro = np.asarray(csr.row_off)
    u = np.repeat(np.arange(csr.n), np.diff(ro)).astype(np.uint32)
    return dbfs.build_csr(csr.n, u, np.asarray(csr.col).astype(np.uint32))


def oracle(name):
    """The labels both references agree on (checked once; read-only): cpu_components
    and the numpy propagation; a directed graph: also those of its symmetrised CSR."""
    if name not in _oracle_cache:
        csr = host_csr(name)
        lab = np.asarray(dbfs.cpu_components(csr))
        assert lab.dtype == np.int64 and lab.shape == (csr.n,)
        assert np.array_equal(lab, component_labels_reference(csr)), f"{name}: the two references differ"
        if GRAPHS[name][1]:
            assert np.array_equal(lab, dbfs.cpu_components(symmetrised(csr)))
        lab.setflags(write=False)
        _oracle_cache[name] = lab
    return _oracle_cache[name]


def totals(labels):
    """(components, largest size, its label -- the smaller on a tie --, singletons, sizes per label)."""
    sz = np.bincount(labels, minlength=labels.size)
    return int(np.count_nonzero(sz)), int(sz.max()), int(np.argmax(sz)), int(np.count_nonzero(sz == 1)), sz


def references_state_the_facts(name):
    """The oracle itself against the literal graph facts."""
    lab = oracle(name)
    f = FACTS.get(name, {})
    comps, largest, label, single, sz = totals(lab)
    assert lab.size == f.get("n", lab.size)
    assert comps == f.get("components", comps) and largest == f.get("largest", largest)
    assert label == f.get("label", label) and single == f.get("singletons", single)
    if "pairs" in f:
        assert int(np.count_nonzero(sz == 2)) == f["pairs"]
    if "multi" in f:
        assert int(np.count_nonzero(sz >= 2)) == f["multi"]
    assert np.array_equal(lab[lab], lab) and np.all(lab <= np.arange(lab.size))


def bfs_input(name):
    g = GRAPHS[name][0]
    return g if isinstance(g, (N.GenParams, str)) else host_csr(name)


def make_bfs(name, rt, hub_sort=True, fresh=False):
    key = (name, hub_sort, id(rt))
    if fresh or key not in _bfs_cache:
        kw = dict(mode="td", directed=True) if GRAPHS[name][1] else {}
        bfs = dbfs.BFS(bfs_input(name), rt, hub_sort=hub_sort, **kw)
        if fresh:
            return bfs
        _bfs_cache[key] = bfs
    return _bfs_cache[key]


def check_result(name, bfs, res, sample, world=1):
    lab = bfs.component_labels()
    ref = oracle(name)
    assert lab.dtype == np.int64 and lab.shape == ref.shape
    bad = np.nonzero(lab != ref)[0]
    assert np.array_equal(lab, ref), (f"{name}: {bad.size} labels differ, first " +
                                      ", ".join(f"[{int(v)}] {int(lab[v])} vs {int(ref[v])}" for v in bad[:6]))
    assert np.array_equal(lab, component_labels_reference(host_csr(name)))
    assert np.array_equal(lab[lab], lab) and np.all(lab <= np.arange(lab.size))
    comps, largest, label, single, sz = totals(ref)
    sizes = bfs.component_sizes()
    assert sizes.dtype == np.int64 and np.array_equal(sizes, np.bincount(lab, minlength=lab.size)[lab])
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == (comps, largest, label, single)
    f = FACTS.get(name, {})
    assert res.components == f.get("components", comps) and res.largest_size == f.get("largest", largest)
    assert res.largest_label == f.get("label", label) and res.singletons == f.get("singletons", single)
    assert res.sampled == (world == 1 and not GRAPHS[name][1] and sample != 0)
    assert res.ms > 0.0 and res.link_ms > 0.0 and res.compress_ms > 0.0 and res.ms >= res.link_ms
    return lab


def matches_references(rt, name, hub_sort):
    """Both settings of cc_sample_entries on one engine, the second call after
    the first: identical labels, sizes and totals."""
    bfs = make_bfs(name, rt, hub_sort)
    for sample in SAMPLE_SETTINGS:
        check_result(name, bfs, bfs.components(sample_entries=sample), sample)
    # the default is the engine option
    assert dict(bfs.engine.get_options())["cc_sample_entries"] == 2.0
    assert bfs.components().sampled == (not GRAPHS[name][1])


def edge_list_from_edges(rt):
    """The planted edge list through DeviceGraph.from_edges: a vertex with only
    self-loops is a singleton of degree > 0."""
    n, u, v = planted_edge_list()
    ref = oracle("edge_list")
    deg = np.diff(np.asarray(host_csr("edge_list").row_off))
    assert deg[700] == 2 and deg[701] == 0
    g = N.DeviceGraph.from_edges(rt.backend, rt.comm, N.Partition(n, 1), 0, u.size, u, v)
    eng = N.Engine(g, rt.comm)
    for sample in SAMPLE_SETTINGS:
        res = eng.components(sample)
        assert np.array_equal(eng.gather_components(), ref)
        assert res.singletons == totals(ref)[3] > np.count_nonzero(deg == 0)
        assert res.sampled == (sample != 0)


def virtual_ranks(name, P, device, piece=None, monkeypatch=None):
    """Every rank's full label array equals the oracle's; the skip never runs."""
    if piece is not None:
        monkeypatch.setenv("DBFS_CC_PIECE_VERTICES", str(piece))
    directed = GRAPHS[name][1]
    g = bfs_input(name)
    kw = dict(mode="td", directed=True) if directed else {}

    def body(rt):
        bfs = dbfs.BFS(g, rt, **kw)
        out = []
        for sample in SAMPLE_SETTINGS:
            res = bfs.components(sample_entries=sample)
            out.append((res, bfs.component_labels(), bfs.component_sizes()))
        return out

    ref = oracle(name)
    comps, largest, label, single, sz = totals(ref)
    for r, out in enumerate(run_virtual_ranks(P, body, device=device)):
        for res, lab, sizes in out:
            assert np.array_equal(lab, ref), f"rank {r}/{P}"
            assert np.array_equal(sizes, sz[ref])
            assert (res.components, res.largest_size, res.largest_label, res.singletons) == (comps, largest, label, single)
            assert not res.sampled


# ---- ties to the rest of the engine ------------------------------------------------

def _batch_totals(res):
    return (res.reached, res.edges, res.depth, res.dist_sum, res.discovered, res.violations, res.validated)


def ties_to_traversals(rt, name):
    """reached == the component's size, the finite levels are exactly the
    component, and a validated batch is the same before and after."""
    bfs = make_bfs(name, rt, fresh=True)
    roots = bfs.sample_roots(8, seed=5)
    before = _batch_totals(bfs.run_batch(roots, validate=True))
    assert before[-1]
    bfs.run(roots[0])
    lv0 = bfs.levels().copy()
    bfs.components()
    assert np.array_equal(bfs.levels(), lv0)  # the single-source state is left alone
    lab, sizes = bfs.component_labels(), bfs.component_sizes()
    for s in roots:
        res = bfs.run(s)
        assert res.reached == sizes[s]
        assert np.array_equal(bfs.levels() != dbfs.UNREACHED, lab == lab[s])
        assert bfs.validate(s)
    assert _batch_totals(bfs.run_batch(roots, validate=True)) == before
    assert np.array_equal(bfs.component_labels(), lab)  # ... and the other way round


# ---- sample_roots ------------------------------------------------------------------------

# BFS.sample_roots(8, seed) on sparse20000 as the parent commit returns it
PINNED_ROOTS = {1: [9463, 10236, 15103, 19009, 697, 2883, 16458, 4984],
                2: [16751, 9025, 1838, 12002, 16263, 19857, 17604, 5499],
                3: [16230, 1712, 4736, 17384, 11643, 787, 1882, 6644]}


def sample_roots(rt, pytest):
    bfs = make_bfs("sparse20000", rt, fresh=True)
    for seed, roots in PINNED_ROOTS.items():
        assert bfs.sample_roots(8, seed=seed) == roots
    assert bfs.sample_roots(4) == PINNED_ROOTS[1][:4]
    assert not bfs.engine.has_components
    ref = oracle("sparse20000")
    roots = bfs.sample_roots(16, seed=3, component="largest")  # (runs components() itself)
    assert bfs.engine.has_components
    assert len(set(roots)) == 16 and all(ref[r] == 57 for r in roots)
    assert bfs.sample_roots(16, seed=3, component="largest") == roots
    assert bfs.sample_roots(16, seed=4, component="largest") != roots
    other = int(ref[PINNED_ROOTS[1][0]])
    k = int(np.count_nonzero(ref == other))
    assert sorted(bfs.sample_roots(k, component=other)) == [int(v) for v in np.nonzero(ref == other)[0]]
    with pytest.raises(ValueError, match="fewer than 200"):
        bfs.sample_roots(200, component="largest")  # 153 vertices
    isolated = int(np.nonzero(np.bincount(ref, minlength=ref.size)[ref] == 1)[0][0])
    if np.diff(np.asarray(host_csr("sparse20000").row_off))[isolated] == 0:
        with pytest.raises(ValueError, match="fewer than 1"):
            bfs.sample_roots(1, component=isolated)  # one vertex, of degree 0
    with pytest.raises(ValueError, match="largest"):
        bfs.sample_roots(1, component="biggest")


# ---- determinism ---------------------------------------------------------------------------

def deterministic(rt, name="rmat13", calls=10):
    """The race-order property: the labels do not depend on which hook won."""
    ref = oracle(name)
    a, b = make_bfs(name, rt, fresh=True), make_bfs(name, rt, hub_sort=False, fresh=True)
    for i in range(calls):
        bfs = a if i % 2 == 0 else b
        bfs.components(sample_entries=SAMPLE_SETTINGS[(i // 2) % 2])
        assert np.array_equal(bfs.component_labels(), ref), f"call {i}"


def needs_a_call(rt, pytest):
    bfs = make_bfs("rmat10", rt, fresh=True)
    with pytest.raises(Exception, match="components\\(\\) has not run"):
        bfs.component_labels()
    with pytest.raises(Exception, match="components\\(\\) has not run"):
        bfs.component_sizes()


# ---- fault injection ----------------------------------------------------------------------

def injected_violation_fails(rt, monkeypatch, pytest):
    """DBFS_FAULT_INJECT kind cc_device records violation 99 during the link:
    that call fails and leaves no result, a traversal is not disturbed, the
    next clean engine passes."""
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=cc_device")
    bfs = make_bfs("rmat10", rt, fresh=True)
    bfs.run(bfs.sample_roots(1)[0])  # not the link's
    with pytest.raises(Exception, match="device check failed on rank 0: code 99"):
        bfs.components()
    with pytest.raises(Exception, match="components\\(\\) has not run"):
        bfs.component_labels()
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    bfs = make_bfs("rmat10", rt, fresh=True)
    check_result("rmat10", bfs, bfs.components(), 2)


# ---- CLI -------------------------------------------------------------------------------------

LINE = "components {c} largest label {l} size {s} singletons {i} ms "


def run_cli(bfs_bin, flags, env=None):
    return subprocess.run([bfs_bin] + flags, capture_output=True, text=True, timeout=120, env=env)


def _expected_line(ref):
    comps, largest, label, single, _ = totals(ref)
    return LINE.format(c=comps, l=label, s=largest, i=single)


def cli_components(bfs_bin, flags, tmp_dir, expect_sampled):
    """The line, the JSON fields, the labels file, and the reference's stdout
    for source 3 after it, unchanged."""
    path = os.path.join(DATA, "two_components.txt")
    ref = oracle("two_components")
    out_file = os.path.join(str(tmp_dir), "labels.txt")
    plain = run_cli(bfs_bin, ["3", path] + flags)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    out = run_cli(bfs_bin, ["3", path, "--components", "--components-out", out_file, "--json"] + flags)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("components ")]
    assert len(at) == 1 and lines[at[0]].startswith(_expected_line(ref)), out.stdout
    assert lines[at[0] + 1] == "Components OK!" and "Wrong output!" not in out.stdout
    rec = json.loads(lines[at[0] + 2])
    comps, largest, label, single, _ = totals(ref)
    assert (rec["components"], rec["largest_label"], rec["largest_size"], rec["singletons"]) == (comps, label, largest, single)
    assert rec["ms"] > 0 and rec["cc_link_ms"] > 0 and rec["cc_compress_ms"] > 0 and rec["cc_sampled"] is expect_sampled
    with open(out_file) as f:
        assert [int(x) for x in f.read().split()] == [int(x) for x in ref]
    # without the three lines and the run's JSON line, the stdout of the plain call (times aside)
    rest = [l for i, l in enumerate(lines) if i not in (at[0], at[0] + 1, at[0] + 2) and not l.startswith("{")]

    def untimed(ls):
        return [l for l in ls if not l.startswith("Elapsed time in milliseconds")]
    assert untimed(rest) == untimed(plain.stdout.splitlines())
    assert "Output OK!" in out.stdout
    # the option: a full pass gives the same line
    out = run_cli(bfs_bin, ["3", path, "--components", "--cc-sample-entries", "0", "--json", "--no-oracle"] + flags)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("components ")]
    assert lines[at[0]].startswith(_expected_line(ref)) and "Components OK!" not in out.stdout
    assert json.loads(lines[at[0] + 1])["cc_sampled"] is False


def cli_usage(bfs_bin):
    path = os.path.join(DATA, "chain8.txt")
    out = run_cli(bfs_bin, ["0", path, "--cpu", "--components-out", "x"])
    assert out.returncode == 2 and "--components-out needs --components" in out.stderr


def cli_generated(bfs_bin, flags):
    out = run_cli(bfs_bin, ["--rmat", "13", "--seed", "44", "--components", "--quiet"] + flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "components 1718 largest label 2 size 6474 singletons 1716 ms " in out.stdout, out.stdout


def cli_checked_reports(bfs_checked):
    flags = ["--rmat", "13", "--seed", "44", "--components"]
    out = run_cli(bfs_checked, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "components 1718 largest label 2 size 6474 singletons 1716 ms " in out.stdout and "Components OK!" in out.stdout
    out = run_cli(bfs_checked, flags, env=dict(os.environ, DBFS_FAULT_INJECT="rank=0,kind=cc_device"))
    assert out.returncode != 0, out.stdout
    assert "device check failed on rank 0: code 99" in out.stderr, out.stderr[-2000:]
    assert "file cc_kernels" in out.stderr, out.stderr[-2000:]
    assert "components 1718" not in out.stdout


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def cli_two_processes(bfs_bin, tmp_dir):
    """One process per rank on the CPU backend over TCP: the leader's line,
    check and labels file."""
    path = os.path.join(DATA, "two_components.txt")
    ref = oracle("two_components")
    out_file = os.path.join(str(tmp_dir), "labels2.txt")
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port - 1), DBFS_BOOTSTRAP_PORT=str(port), DBFS_COMM_TIMEOUT_S="30")
        procs.append(subprocess.Popen([bfs_bin, "3", path, "--cpu", "--components", "--components-out", out_file],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=120) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs
    assert _expected_line(ref) in outs[0][0] and "Components OK!" in outs[0][0] and "Output OK!" in outs[0][0]
    assert "components " not in outs[1][0]
    with open(out_file) as f:
        assert [int(x) for x in f.read().split()] == [int(x) for x in ref]
