"""Graphs and checks shared by the strongly-connected-components tests
(test_scc.py on the CPU backend, test_scc_gpu.py on the GPU):
BFS.strong_components / strong_component_labels / strong_component_sizes
against two independent references -- the sequential Tarjan oracle
cpu_strong_components and the numpy peeling
utils.validate.strong_component_labels_reference -- always with np.array_equal:
label[v] is the smallest vertex id of v's strongly connected component, so the
answer is unique and nothing is compared up to renaming.

FACTS are properties of the graphs (computed once with
scipy.sparse.csgraph.connected_components(connection="strong") on the host
CSRs), asserted as literals."""
import json
import os
import subprocess

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks
from distributed_cuda_bfs_amd.utils.validate import strong_component_labels_reference

import components_cases as cc
import directed_cases as dc

N = dbfs.native
DATA = cc.DATA
FORCED = dict(trim_rounds=0, pivot=False)  # pure colouring: no trim, every vertex coloured in every round


def _cycle_desc():
    """One directed cycle 2999 -> 2998 -> ... -> 0 -> 2999: the colour 0 crosses
    it one vertex per sweep in the worst order, and so does the closure."""
    k = 3000
    return dc._csr(k, np.arange(k), (np.arange(k) - 1) % k)


def _cycle_chain(ascending):
    """40 cycles of length 3, cycle j joined to cycle j + 1 by the one edge
    base_j + 1 -> base_{j + 1} + 2.  Ids ascending along the chain: every
    vertex gets the colour of the first cycle, and a round settles one cycle
    (40 rounds without the trim).  Descending: every cycle keeps a colour of
    its own and one round settles them all."""
    k = 40
    base = 3 * (np.arange(k) if ascending else np.arange(k)[::-1])
    u = np.concatenate([base, base + 1, base + 2, base[:-1] + 1])
    v = np.concatenate([base + 1, base + 2, base, base[1:] + 2])
    return dc._csr(3 * k, u, v)


def _hub_cycle():
    """0 -> i and i -> 0 for i = 1..5000: both rows of vertex 0 are walked by a wave."""
    k = 5000
    i = np.arange(1, k + 1)
    g = dc._csr(k + 1, np.concatenate([np.zeros(k, dtype=np.int64), i]), np.concatenate([i, np.zeros(k, dtype=np.int64)]))
    assert np.diff(np.asarray(g.row_off))[0] == k
    return g


def _bowtie():
    """A chain 0..199 into a 1000-vertex cycle on shuffled ids 200..1199, a
    chain 1200..1399 leaving it, 1400 with a duplicated self-loop only, 1401
    with one edge into the core, 1402 with no entry, and a duplicated chain edge."""
    core = 200 + np.random.default_rng(12).permutation(1000)
    tail = np.arange(1200, 1400)
    u = np.concatenate([np.arange(0, 199), [199], core, [core[500]], tail[:-1], [1400, 1400], [1401], [57]])
    v = np.concatenate([np.arange(1, 200), [core[0]], np.roll(core, -1), [1200], tail[1:], [1400, 1400], [core[7]], [58]])
    return dc._csr(1403, u, v)


TIER_LENGTHS = (32, 33, 96, 97, 160)


def tier_rows():
    """scc_tiers' ten rows as (kind, vertex, partner, others): kind "out": the
    vertex's out-row holds len(others) sinks and the partner; kind "in": its
    in-row holds len(others) sources and the partner.  The other direction of
    the pair is one arc, so {partner, vertex} is a cycle.  Ids ascend within a
    block: others < partner < vertex."""
    rows, at = [], 0
    for kind in ("out", "in"):
        for length in TIER_LENGTHS:
            others = np.arange(at, at + length - 1)
            rows.append((kind, at + length, at + length - 1, others))
            at += length + 1
    return rows


def _tiers():
    """Rows on scc_row_any's tiers (the first kSccLane = 32 entries by the
    lane, the rest in 64-entry steps by the wave): out-rows and in-rows of 32,
    33, 96, 97 and 160 entries of which all but the last, the partner's, lead
    to sinks (from sources) that the first trim sweep settles.  Unsorted, the
    partner -- the largest id of its row -- is entry 31, 32, 95, 96 and 159:
    the lane's last, the wave's first, the last of a full step, the first of a
    partial one, the last of all.  A walk that misses it trims half of a
    2-cycle.  The partner's id is below the vertex's, so the closure too
    reaches its root only through that entry."""
    u, v = [], []
    for kind, x, p, others in tier_rows():
        a, b = np.full(others.size, x), others
        u += [a if kind == "out" else b, [x], [p]]
        v += [b if kind == "out" else a, [p], [x]]
    g = dc._csr(tier_rows()[-1][1] + 1, np.concatenate(u), np.concatenate(v))
    deg = np.diff(np.asarray(g.row_off))
    assert [int(deg[x]) for kind, x, _, _ in tier_rows() if kind == "out"] == list(TIER_LENGTHS)
    return g


_NEW = {"scc_tiers": _tiers, "cycle3000_desc": _cycle_desc, "cycle_chain_asc": lambda: _cycle_chain(True),
        "cycle_chain_desc": lambda: _cycle_chain(False), "hub_cycle5000": _hub_cycle, "bowtie": _bowtie}
DIRECTED = [g for g in dc.GRAPHS if g != "file_d6"] + ["dup_in6000"] + list(_NEW)
UNDIRECTED = ["rmat13"]  # components_cases': the labels are the connected components'
GRAPHS = DIRECTED + UNDIRECTED
# graph facts: n, strongly connected components, largest (size), label (of the largest), singletons, multi (size >= 2)
FACTS = {
    "d_rmat10": dict(n=1024, components=317, largest=708, label=1, singletons=316, multi=1),
    "d_rmat13": dict(n=8192, components=3281, largest=4912, label=2, singletons=3280, multi=1),
    "d_n4097": dict(n=4097, components=903, largest=3195, label=0, singletons=902, multi=1),
    "one_way_bridge": dict(n=8192, components=126, largest=4038, label=0, singletons=124, multi=2),
    "star_out5000": dict(n=5004, components=5004, largest=1, label=0, singletons=5004, multi=0),
    "star_in5000": dict(n=5004, components=5004, largest=1, label=0, singletons=5004, multi=0),
    "d_path300": dict(n=300, components=300, largest=1, label=0, singletons=300, multi=0),
    "dup_in6000": dict(n=701, components=701, largest=1, label=0, singletons=701, multi=0),
    "back_edge10": dict(n=10, components=1, largest=10, label=0, singletons=0, multi=1),
    "tiny5": dict(n=5, components=4, largest=2, label=0, singletons=3, multi=1),
    "empty3": dict(n=3, components=3, largest=1, label=0, singletons=3, multi=0),
    "cycle3000_desc": dict(n=3000, components=1, largest=3000, label=0, singletons=0, multi=1),
    "cycle_chain_asc": dict(n=120, components=40, largest=3, label=0, singletons=0, multi=40),
    "cycle_chain_desc": dict(n=120, components=40, largest=3, label=0, singletons=0, multi=40),
    "hub_cycle5000": dict(n=5001, components=1, largest=5001, label=0, singletons=0, multi=1),
    "bowtie": dict(n=1403, components=404, largest=1000, label=200, singletons=403, multi=1),
    "scc_tiers": dict(n=846, components=836, largest=2, label=31, singletons=826, multi=10),
    # (the undirected graph: components_cases.FACTS["rmat13"])
    "rmat13": dict(n=8192, components=1718, largest=6474, label=2, singletons=1716, multi=2),
}
ACYCLIC = ("star_out5000", "star_in5000", "d_path300", "dup_in6000", "empty3")
HUB_SORT_BOTH = ("d_rmat10", "d_rmat13", "scc_tiers")
CASES = [(g, True) for g in GRAPHS] + [(g, False) for g in HUB_SORT_BOTH]
# pure colouring needs about 243 000 sweeps on bowtie and 45 000 on d_path300: not run there
FORCED_CASES = ["d_rmat10", "d_rmat13", "d_n4097", "star_out5000", "star_in5000", "one_way_bridge", "back_edge10",
                "tiny5", "empty3", "cycle_chain_asc", "cycle_chain_desc", "hub_cycle5000", "cycle3000_desc", "scc_tiers"]
RANK_CASES = ["d_rmat13", "one_way_bridge", "d_n4097", "cycle_chain_asc", "hub_cycle5000", "scc_tiers"]
TINY_RANK_CASES = ["tiny5", "empty3"]

_csr_cache = {}
_oracle_cache = {}
_bfs_cache = {}


def is_directed(name):
    return name not in UNDIRECTED


def host_csr(name):
    if name not in _csr_cache:
        if name in _NEW:
            _csr_cache[name] = _NEW[name]()
        elif is_directed(name):
            _csr_cache[name] = dc.host_csr(name)
        else:
            _csr_cache[name] = cc.host_csr(name)
    return _csr_cache[name]


def oracle(name):
    """The labels both references agree on (checked once; read-only); the
    undirected graph: also the connected-components oracle's."""
    if name not in _oracle_cache:
        csr = host_csr(name)
        lab = np.asarray(dbfs.cpu_strong_components(csr))
        assert lab.dtype == np.int64 and lab.shape == (csr.n,)
        assert np.array_equal(lab, strong_component_labels_reference(csr)), f"{name}: the two references differ"
        if not is_directed(name):
            assert np.array_equal(lab, cc.oracle(name))
        lab.setflags(write=False)
        _oracle_cache[name] = lab
    return _oracle_cache[name]


totals = cc.totals


def references_state_the_facts(name):
    """The oracle itself against the literal graph facts."""
    lab = oracle(name)
    f = FACTS[name]
    comps, largest, label, single, sz = totals(lab)
    assert (lab.size, comps, largest, label, single) == (f["n"], f["components"], f["largest"], f["label"], f["singletons"])
    assert int(np.count_nonzero(sz >= 2)) == f["multi"]
    assert np.array_equal(lab[lab], lab) and np.all(lab <= np.arange(lab.size))


def make_bfs(name, rt, hub_sort=True, fresh=False):
    key = (name, hub_sort, id(rt))
    if fresh or key not in _bfs_cache:
        kw = dict(mode="td", directed=True) if is_directed(name) else {}
        bfs = dbfs.BFS(host_csr(name), rt, hub_sort=hub_sort, **kw)
        if fresh:
            return bfs
        _bfs_cache[key] = bfs
    return _bfs_cache[key]


def check_result(name, bfs, res):
    lab = bfs.strong_component_labels()
    ref = oracle(name)
    n = ref.size
    assert lab.dtype == np.int64 and lab.shape == ref.shape
    bad = np.nonzero(lab != ref)[0]
    assert np.array_equal(lab, ref), (f"{name}: {bad.size} labels differ, first " +
                                      ", ".join(f"[{int(v)}] {int(lab[v])} vs {int(ref[v])}" for v in bad[:6]))
    assert np.array_equal(lab, strong_component_labels_reference(host_csr(name)))
    assert np.array_equal(lab[lab], lab) and np.all(lab <= np.arange(n))
    comps, largest, label, single, sz = totals(ref)
    sizes = bfs.strong_component_sizes()
    assert sizes.dtype == np.int64 and np.array_equal(sizes, sz[ref])
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == (comps, largest, label, single)
    f = FACTS[name]
    assert (res.components, res.largest_size, res.largest_label, res.singletons) == (
        f["components"], f["largest"], f["label"], f["singletons"])
    assert 1 <= res.rounds <= n and res.sweeps >= 1
    assert 0 <= res.trimmed <= res.singletons
    assert res.ms > 0.0 and res.ms >= res.trim_ms >= 0.0 and res.ms >= res.colour_ms >= 0.0
    if res.pivot >= 0:
        assert res.pivot_size == sz[ref[res.pivot]]
    return lab


def matches_references(rt, name, hub_sort):
    """The defaults (trim to the fixed point, a pivot in the first round)."""
    bfs = make_bfs(name, rt, hub_sort)
    res = bfs.strong_components()
    check_result(name, bfs, res)
    if name in ACYCLIC:
        assert res.trimmed == FACTS[name]["n"] and res.pivot == -1 and res.rounds == 1
    opts = dict(bfs.engine.get_options())
    assert opts["scc_trim_rounds"] == -1.0 and opts["scc_pivot"] == 1.0


def forced_form(rt, name):
    """No trim and no pivot: the colouring alone, after a default call on the same engine."""
    bfs = make_bfs(name, rt)
    res = bfs.strong_components(**FORCED)
    check_result(name, bfs, res)
    assert res.trimmed == 0 and res.pivot == -1 and res.pivot_size == 0


def early_trim_stop(rt):
    """One trim sweep per round on star_out5000 settles what one sweep can; the colouring does the rest."""
    bfs = make_bfs("star_out5000", rt)
    full = bfs.strong_components()
    res = bfs.strong_components(trim_rounds=1)
    check_result("star_out5000", bfs, res)
    assert full.trimmed == 5004 and res.trimmed <= 5004
    bfs.engine.set_option("scc_trim_rounds", 1)
    try:
        assert dict(bfs.engine.get_options())["scc_trim_rounds"] == 1.0
        check_result("star_out5000", bfs, bfs.strong_components())
    finally:
        bfs.engine.set_option("scc_trim_rounds", -1)


def virtual_ranks(name, P, device):
    """Every rank's full label array, sizes and totals equal the oracle's, with the defaults and forced."""
    csr = host_csr(name)
    kw = dict(mode="td", directed=True) if is_directed(name) else {}

    def body(rt):
        bfs = dbfs.BFS(csr, rt, **kw)
        out = []
        for opts in ({}, FORCED):
            res = bfs.strong_components(**opts)
            out.append((res, bfs.strong_component_labels(), bfs.strong_component_sizes()))
        return out

    ref = oracle(name)
    comps, largest, label, single, sz = totals(ref)
    for r, out in enumerate(run_virtual_ranks(P, body, device=device)):
        for res, lab, sizes in out:
            assert np.array_equal(lab, ref), f"rank {r}/{P}"
            assert np.array_equal(sizes, sz[ref])
            assert (res.components, res.largest_size, res.largest_label, res.singletons) == (comps, largest, label, single)
            assert 1 <= res.rounds <= ref.size
        assert out[1][0].trimmed == 0 and out[1][0].pivot == -1


# ---- ties to the rest of the engine ------------------------------------------------

def ties_to_traversals(rt):
    """A root of the largest SCC reaches at least that SCC; run / run_batch /
    validate state and components() are left alone, and the other way round."""
    name = "d_rmat13"
    bfs = make_bfs(name, rt, fresh=True)
    ref = oracle(name)
    plain = bfs.sample_roots(8, seed=5)
    before = cc._batch_totals(bfs.run_batch(plain, validate=True))
    assert before[-1]
    bfs.run(plain[0])
    lv0 = bfs.levels().copy()
    cres = bfs.components()
    weak = bfs.component_labels().copy()
    assert not bfs.engine.has_strong_components
    roots = bfs.sample_roots(8, strong_component="largest")  # (runs strong_components() itself)
    assert bfs.engine.has_strong_components
    res = bfs.engine.last_strong_components()
    assert np.array_equal(bfs.levels(), lv0)  # the single-source state is left alone
    assert np.array_equal(bfs.component_labels(), weak)  # ... and the weak components
    lab = bfs.strong_component_labels()
    assert np.array_equal(lab, ref)
    assert len(set(roots)) == 8 and all(ref[r] == FACTS[name]["label"] for r in roots)
    assert bfs.sample_roots(8, strong_component="largest") == roots
    assert bfs.sample_roots(8, strong_component=FACTS[name]["label"]) == roots
    for s in roots:
        run = bfs.run(s)
        assert run.reached >= res.largest_size == FACTS[name]["largest"]
        assert np.all(bfs.levels()[ref == ref[s]] != dbfs.UNREACHED)
    assert cc._batch_totals(bfs.run_batch(plain, validate=True)) == before
    assert np.array_equal(bfs.strong_component_labels(), lab)
    again = bfs.components()
    assert (again.components, again.largest_size) == (cres.components, cres.largest_size)
    assert np.array_equal(bfs.component_labels(), weak) and np.array_equal(bfs.strong_component_labels(), lab)


def sample_roots(rt, pytest):
    bfs = make_bfs("star_in5000", rt, fresh=True)
    # every SCC is one vertex: the largest is the one labelled 0, whose only vertex has an out-edge
    assert bfs.sample_roots(1, strong_component="largest") == [0]
    assert bfs.sample_roots(1, strong_component=17) == [17]
    with pytest.raises(ValueError, match="fewer than 2"):
        bfs.sample_roots(2, strong_component="largest")
    with pytest.raises(ValueError, match="fewer than 1"):
        bfs.sample_roots(1, strong_component=5003)  # the tail's end: no out-edge
    with pytest.raises(ValueError, match="largest"):
        bfs.sample_roots(1, strong_component="biggest")
    with pytest.raises(ValueError, match="not both"):
        bfs.sample_roots(1, component="largest", strong_component="largest")
    # the weak component of vertex 0 holds every vertex: component= is what it was
    assert not bfs.engine.has_components
    weak = bfs.sample_roots(4, seed=2, component="largest")
    assert len(weak) == 4 and bfs.engine.has_components


def deterministic(rt, calls=10):
    """Ten calls alternating hub_sort and the forced form: one array."""
    ref = oracle("d_rmat13")
    a, b = make_bfs("d_rmat13", rt, fresh=True), make_bfs("d_rmat13", rt, hub_sort=False, fresh=True)
    for i in range(calls):
        bfs = a if i % 2 == 0 else b
        bfs.strong_components(**(FORCED if (i // 2) % 2 else {}))
        assert np.array_equal(bfs.strong_component_labels(), ref), f"call {i}"


def needs_a_call(rt, pytest):
    bfs = make_bfs("d_rmat10", rt, fresh=True)
    with pytest.raises(Exception, match="strong_components\\(\\) has not run"):
        bfs.strong_component_labels()
    with pytest.raises(Exception, match="strong_components\\(\\) has not run"):
        bfs.strong_component_sizes()
    bfs.components()  # (the weak components are not the strong ones' result)
    with pytest.raises(Exception, match="strong_components\\(\\) has not run"):
        bfs.strong_component_labels()


# ---- fault injection ----------------------------------------------------------------------

def injected_violation_fails(rt, monkeypatch, pytest):
    """DBFS_FAULT_INJECT kind scc_device records violation 99 in scc_kernels'
    word during the first trim: that call fails and leaves no result, a
    traversal is not disturbed, the next clean engine passes."""
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=scc_device")
    bfs = make_bfs("d_rmat10", rt, fresh=True)
    src = bfs.sample_roots(1)[0]
    bfs.run(src)  # not the trim's
    lv = bfs.levels().copy()
    with pytest.raises(Exception, match="device check failed on rank 0: code 99, detail 0, file scc_kernels"):
        bfs.strong_components()
    with pytest.raises(Exception, match="strong_components\\(\\) has not run"):
        bfs.strong_component_labels()
    assert not bfs.engine.has_strong_components
    assert np.array_equal(bfs.levels(), lv) and np.array_equal(lv, dc.oracle("d_rmat10", src))
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=scc_device,file=td_kernels")
    with pytest.raises(Exception, match="file applies to kind=device only"):
        make_bfs("d_rmat10", rt, fresh=True)
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    bfs = make_bfs("d_rmat10", rt, fresh=True)
    check_result("d_rmat10", bfs, bfs.strong_components())


# ---- CLI -------------------------------------------------------------------------------------

LINE = "strong components {c} largest label {l} size {s} singletons {i} trimmed "


def run_cli(bfs_bin, flags, env=None):
    return subprocess.run([bfs_bin] + flags, capture_output=True, text=True, timeout=120, env=env)


def _expected_line(ref):
    comps, largest, label, single, _ = totals(ref)
    return LINE.format(c=comps, l=label, s=largest, i=single)


def _file_oracle(path, directed):
    csr = dbfs.read_graph(path, directed=True) if directed else dbfs.read_graph(path)
    lab = np.asarray(dbfs.cpu_strong_components(csr))
    assert np.array_equal(lab, strong_component_labels_reference(csr))
    return lab


def cli_strong_components(bfs_bin, path, directed, flags, tmp_dir):
    """The line, the check, the JSON fields and the labels file; with the
    feature's lines removed, the stdout of the plain call."""
    ref = _file_oracle(path, directed)
    base = ["3", path] + (["--directed"] if directed else []) + flags
    out_file = os.path.join(str(tmp_dir), "scc_labels.txt")
    plain = run_cli(bfs_bin, base)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    out = run_cli(bfs_bin, base + ["--strong-components", "--strong-components-out", out_file, "--json"])
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("strong components ")]
    assert len(at) == 1 and lines[at[0]].startswith(_expected_line(ref)), out.stdout
    words = lines[at[0]].split()
    assert words[-6:-1:2] == ["trimmed", "rounds", "ms"] and float(words[-1]) > 0
    assert lines[at[0] + 1] == "Strong components OK!" and "Wrong output!" not in out.stdout
    rec = json.loads(lines[at[0] + 2])
    comps, largest, label, single, _ = totals(ref)
    assert (rec["strong_components"], rec["largest_label"], rec["largest_size"], rec["singletons"]) == (
        comps, label, largest, single)
    assert rec["trimmed"] == int(words[-5]) <= single and 1 <= rec["rounds"] == int(words[-3]) <= ref.size
    assert rec["ms"] > 0 and rec["scc_trim_ms"] >= 0 and rec["scc_colour_ms"] >= 0 and rec["scc_sweeps"] >= 1
    assert rec["scc_pivot"] == -1 or ref[rec["scc_pivot"]] >= 0
    with open(out_file) as f:
        assert [int(x) for x in f.read().split()] == [int(x) for x in ref]
    rest = [l for i, l in enumerate(lines) if i not in (at[0], at[0] + 1, at[0] + 2) and not l.startswith("{")]

    def untimed(ls):
        return [l for l in ls if not l.startswith("Elapsed time in milliseconds")]
    assert untimed(rest) == untimed(plain.stdout.splitlines())
    assert "Output OK!" in out.stdout
    # the options, and both kinds of components in one call: the same counts
    out = run_cli(bfs_bin, base + ["--strong-components", "--components", "--scc-trim-rounds", "0", "--no-scc-pivot",
                                   "--json", "--no-oracle"])
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("strong components ")]
    assert lines[at[0]].startswith(_expected_line(ref) + "0 rounds ") and "Strong components OK!" not in out.stdout
    assert json.loads(lines[at[0] + 1])["scc_pivot"] == -1
    assert any(l.startswith("components ") for l in lines[:at[0]])


def cli_usage(bfs_bin):
    path = os.path.join(DATA, "chain8.txt")
    out = run_cli(bfs_bin, ["0", path, "--cpu", "--strong-components-out", "x"])
    assert out.returncode == 2 and "--strong-components-out needs --strong-components" in out.stderr
    out = run_cli(bfs_bin, ["--help"])
    assert "--strong-components" in out.stderr and "--scc-trim-rounds" in out.stderr and "--no-scc-pivot" in out.stderr


def cli_checked_reports(bfs_checked, path):
    """bin/bfs_checked runs --directed --strong-components clean with every
    DBFS_DCHECK of scc_kernels.hip live, and fails on the recorded violation."""
    ref = _file_oracle(path, True)
    flags = ["0", path, "--directed", "--strong-components", "--json"]
    out = run_cli(bfs_checked, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert _expected_line(ref) in out.stdout and "Strong components OK!" in out.stdout
    runs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{") and '"source"' in l]
    assert runs and all(r["backend"].endswith("+checked") for r in runs), out.stdout
    out = run_cli(bfs_checked, flags, env=dict(os.environ, DBFS_FAULT_INJECT="rank=0,kind=scc_device"))
    assert out.returncode != 0, out.stdout
    assert "device check failed on rank 0: code 99, detail 0, file scc_kernels" in out.stderr, out.stderr[-2000:]
    assert "strong components " not in out.stdout


def cli_two_processes(bfs_bin, tmp_dir):
    """One process per rank on the CPU backend over TCP: the leader's line, check and labels file."""
    path = os.path.join(DATA, "two_components.txt")
    ref = _file_oracle(path, True)
    out_file = os.path.join(str(tmp_dir), "scc_labels2.txt")
    port = cc._free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port - 1), DBFS_BOOTSTRAP_PORT=str(port), DBFS_COMM_TIMEOUT_S="30")
        procs.append(subprocess.Popen([bfs_bin, "3", path, "--cpu", "--directed", "--strong-components",
                                       "--strong-components-out", out_file],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=120) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs
    assert _expected_line(ref) in outs[0][0] and "Strong components OK!" in outs[0][0] and "Output OK!" in outs[0][0]
    assert "strong components " not in outs[1][0]
    with open(out_file) as f:
        assert [int(x) for x in f.read().split()] == [int(x) for x in ref]
