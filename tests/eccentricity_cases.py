"""Graphs and checks shared by the eccentricity tests (test_eccentricity.py
on the CPU backend, test_eccentricity_gpu.py on the GPU): BFS.eccentricities /
eccentricity / eccentricity_bounds against two independent references -- the
sequential oracle cpu_eccentricities (one traversal per vertex) for the
values, always with np.array_equal, and the numpy loop
utils.validate.eccentricity_bounding_reference for the bounds, the settled
set, the pass counts and the sources used.

Why each graph: k < 64 and a scope smaller than one pass (chain8,
two_components); zero passes, every value 0 (isolated3); depth 128 in one-byte
levels (grid70x60); depth 2999, the 16-bit matrix (path_zigzag); one pass
(max_id_star); n = 64 * 64 + 1, the last partial group of rows, and 35
selections over a shrinking live set (n4097); rows on every tier boundary
(ladder); duplicates, self-loops, a self-loop-only vertex and one without
entries (edge_list); skewed degrees (rmat10, rmat13); thousands of small
components, 129 and 141 passes with scope "all", and a widest component that
is not the largest (partial20000, sparse20000); a traversal per vertex
(cycle2000); a second pass with one source (path65)."""
import json
import os
import re
import subprocess

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks
from distributed_cuda_bfs_amd.utils.validate import eccentricity_bounding_reference

import components_cases as cc

REPO = cc.REPO
DATA = cc.DATA
INF = np.iinfo(np.int32).max


def _cycle(n):
    v = np.arange(n)
    return dbfs.build_csr(n, v, (v + 1) % n)


def _isolated(n):
    return dbfs.build_csr(n, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))


BUILDERS = {
    "cycle2000": lambda: _cycle(2000),
    "path65": lambda: cc._path(np.arange(65)),
    "isolated3": lambda: _isolated(3),
}
FROM_COMPONENTS = ["chain8", "two_components", "grid70x60", "path_zigzag", "max_id_star", "n4097", "ladder",
                   "edge_list", "rmat10", "rmat13", "partial20000", "sparse20000"]
GRAPHS = FROM_COMPONENTS + list(BUILDERS)
SCOPES = ("largest", "all")
CASES = [(g, s) for g in GRAPHS for s in SCOPES]
# name -> (diameter, radius) of the largest component, and passes with target "all"
LITERALS = {"grid70x60": (128, 65), "path_zigzag": (2999, 1500), "max_id_star": (2, 1), "chain8": (7, 4),
            "cycle2000": (1000, 1000), "isolated3": (0, 0), "path65": (64, 32)}
PASSES = {"grid70x60": 2, "path_zigzag": 2, "max_id_star": 1, "chain8": 1, "cycle2000": 32, "isolated3": 0}
WIDE = ("path_zigzag", "cycle2000")  # deeper than one-byte levels hold
TARGET_GRAPHS = ["chain8", "grid70x60", "path_zigzag", "n4097", "ladder", "edge_list", "rmat13", "partial20000",
                 "sparse20000", "cycle2000", "path65", "isolated3"]
RANK_CASES = [("rmat13", "largest"), ("n4097", "largest"), ("path_zigzag", "largest"), ("sparse20000", "all")]
TINY_RANK_CASES = ["chain8", "isolated3"]

_csr = {}
_oracle = {}
_reference = {}
_bfs = {}


def host_csr(name):
    if name in BUILDERS:
        if name not in _csr:
            _csr[name] = BUILDERS[name]()
        return _csr[name]
    return cc.host_csr(name)


def bfs_input(name):
    return host_csr(name) if name in BUILDERS else cc.bfs_input(name)


def oracle(name):
    """cpu_eccentricities and cpu_components' labels, once per graph, read-only."""
    if name not in _oracle:
        csr = host_csr(name)
        ecc = np.asarray(dbfs.cpu_eccentricities(csr))
        assert ecc.dtype == np.int32 and ecc.shape == (csr.n,)
        lab = np.asarray(dbfs.cpu_components(csr))
        ecc.setflags(write=False)
        lab.setflags(write=False)
        _oracle[name] = (ecc, lab)
    return _oracle[name]


def scope_mask(name, scope):
    ecc, lab = oracle(name)
    if scope == "all":
        return np.ones(lab.size, dtype=bool)
    label = cc.totals(lab)[2] if scope == "largest" else int(scope)
    return lab == label


def reference(name, scope, target="all", max_passes=None):
    key = (name, scope, target, max_passes)
    if key not in _reference:
        out = eccentricity_bounding_reference(host_csr(name), scope_mask(name, scope), target, max_passes)
        for a in out[:3]:
            a.setflags(write=False)
        _reference[key] = out
    return _reference[key]


def make_bfs(name, rt, hub_sort=True, fresh=False):
    key = (name, hub_sort, id(rt))
    if fresh:
        return dbfs.BFS(bfs_input(name), rt, hub_sort=hub_sort)
    if key not in _bfs:
        _bfs[key] = dbfs.BFS(bfs_input(name), rt, hub_sort=hub_sort)
    return _bfs[key]


def oracle_totals(name, scope):
    ecc, _ = oracle(name)
    e = ecc[scope_mask(name, scope)]
    d, r = int(e.max()), int(e.min())
    return d, r, int(np.count_nonzero(e == r)), int(np.count_nonzero(e == d))


def check_bounds(name, scope, lo, hi):
    """Out of scope (-1, -1); in scope lo <= ecc <= hi."""
    ecc, _ = oracle(name)
    m = scope_mask(name, scope)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and lo.shape == hi.shape == ecc.shape
    assert np.all(lo[~m] == -1) and np.all(hi[~m] == -1)
    assert np.all(lo[m] <= ecc[m]) and np.all(ecc[m] <= hi[m])


def check_against_reference(name, scope, target, bfs, res, max_passes=None):
    """Bounds, settled set, passes and sources equal the numpy loop's."""
    equals_bounding_reference(reference(name, scope, target, max_passes), bfs, res, f"{name} {scope} {target}")


def equals_bounding_reference(ref, bfs, res, what):
    """... `ref` being eccentricity_bounding_reference's tuple for the call that gave `res`."""
    lo, hi, settled, passes, used = ref
    got_lo, got_hi = bfs.eccentricity_bounds()
    e = bfs.eccentricity()
    assert (res.passes, res.sources) == (passes, used), what
    assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi)
    assert np.array_equal(e >= 0, settled) and res.settled == int(settled.sum())
    assert np.array_equal(e[settled], lo[settled])


def exact_all(rt, name, scope):
    """Check 1 and 3: target "all"."""
    bfs = make_bfs(name, rt)
    res = bfs.eccentricities(component=scope)
    ecc, _ = oracle(name)
    m = scope_mask(name, scope)
    e = bfs.eccentricity()
    assert e.dtype == np.int32 and np.array_equal(e[m], ecc[m]) and np.all(e[~m] == -1), \
        f"{name} {scope}: {np.count_nonzero(e[m] != ecc[m])} values differ"
    assert (res.diameter, res.radius, res.centre, res.periphery) == oracle_totals(name, scope)
    assert res.exact and res.settled == res.scope_size == int(m.sum())
    lo, hi = bfs.eccentricity_bounds()
    check_bounds(name, scope, lo, hi)
    assert np.array_equal(lo[m], ecc[m]) and np.array_equal(hi[m], ecc[m])
    check_against_reference(name, scope, "all", bfs, res)
    if scope == "largest" and name in LITERALS:
        assert (res.diameter, res.radius) == LITERALS[name]
    if name in PASSES:
        assert res.passes == PASSES[name]
    assert res.wide_levels == (name in WIDE)
    assert res.ms >= 0.0 and res.ms >= res.bfs_ms and (res.passes == 0 or (res.bfs_ms > 0.0 and res.bound_ms > 0.0))
    # capped at the reference's own count: the same result, still exact
    capped = bfs.eccentricities(component=scope, max_passes=res.passes)
    assert capped.exact and (capped.passes, capped.sources, capped.settled) == (res.passes, res.sources, res.settled)
    assert np.array_equal(bfs.eccentricity(), e)
    return res


def by_label(rt):
    """A label as the scope: sparse20000's widest component is not its largest."""
    name = "sparse20000"
    ecc, lab = oracle(name)
    widest = int(lab[int(np.argmax(ecc))])
    assert widest != cc.totals(lab)[2] and int(ecc.max()) == 36 and oracle_totals(name, "largest")[0] == 32
    bfs = make_bfs(name, rt)
    res = bfs.eccentricities(component=widest)
    m = lab == widest
    e = bfs.eccentricity()
    assert res.exact and res.diameter == 36 and res.scope_size == int(m.sum())
    assert np.array_equal(e[m], ecc[m]) and np.all(e[~m] == -1)
    check_against_reference(name, widest, "all", bfs, res)


def targets(rt, name, scope, target):
    """Check 2: the promised value, exact settled values, valid bounds, no more passes than "all"."""
    bfs = make_bfs(name, rt)
    res = bfs.eccentricities(target=target, component=scope)
    ecc, _ = oracle(name)
    m = scope_mask(name, scope)
    d, r, _, _ = oracle_totals(name, scope)
    assert res.exact
    assert (res.diameter if target == "diameter" else res.radius) == (d if target == "diameter" else r)
    e = bfs.eccentricity()
    assert np.all(e[~m] == -1) and np.array_equal(e[e >= 0], ecc[e >= 0])
    lo, hi = bfs.eccentricity_bounds()
    check_bounds(name, scope, lo, hi)
    open_ = m & (e < 0)
    assert np.all(lo[open_] < hi[open_])  # no unsettled vertex reads as settled
    check_against_reference(name, scope, target, bfs, res)
    assert res.passes <= reference(name, scope, "all")[3]
    if name == "cycle2000" and target == "diameter":
        assert res.passes == 32
    return res


def capped_cycle(rt):
    """Check 4: three passes of a cycle settle their 192 sources and nothing else."""
    name = "cycle2000"
    bfs = make_bfs(name, rt)
    res = bfs.eccentricities(max_passes=3)
    assert not res.exact and res.passes == 3 and res.sources == 192 and res.settled == 192 and res.scope_size == 2000
    e = bfs.eccentricity()
    lo, hi = bfs.eccentricity_bounds()
    check_bounds(name, "largest", lo, hi)
    assert np.count_nonzero(e >= 0) == 192 and np.all(e[e >= 0] == 1000)
    assert np.all(lo[e < 0] < hi[e < 0])
    check_against_reference(name, "largest", "all", bfs, res, max_passes=3)
    assert res.diameter == 1000 and res.radius >= 1000  # (bounds: the largest lo, the smallest hi)
    none = bfs.eccentricities(max_passes=0)
    assert not none.exact and none.passes == 0 and none.settled == 0
    lo, hi = bfs.eccentricity_bounds()
    assert np.all(lo == 0) and np.all(hi == INF)


def virtual_ranks(name, scope, P, device):
    """Check 5: every rank's arrays and pass counts are those of one rank."""
    g = bfs_input(name)

    def body(rt):
        bfs = dbfs.BFS(g, rt)
        res = bfs.eccentricities(component=scope)
        lo, hi = bfs.eccentricity_bounds()
        return res, bfs.eccentricity(), lo, hi

    ecc, _ = oracle(name)
    m = scope_mask(name, scope)
    rlo, rhi, settled, passes, used = reference(name, scope, "all")
    for r, (res, e, lo, hi) in enumerate(run_virtual_ranks(P, body, device=device)):
        assert np.array_equal(e[m], ecc[m]) and np.all(e[~m] == -1), f"rank {r}/{P}"
        assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi)
        assert (res.passes, res.sources, res.settled) == (passes, used, int(settled.sum()))
        assert (res.diameter, res.radius, res.centre, res.periphery) == oracle_totals(name, scope)
        assert res.exact and res.wide_levels == (name in WIDE)


def hub_sort_and_repeats(rt):
    """Check 6."""
    for name in ("rmat13", "ladder"):
        ecc, _ = oracle(name)
        m = scope_mask(name, "largest")
        passes = reference(name, "largest")[3]
        for hub_sort in (True, False):
            bfs = make_bfs(name, rt, hub_sort=hub_sort, fresh=True)
            for call in range(5 if name == "rmat13" else 1):
                res = bfs.eccentricities()
                assert res.passes == passes and np.array_equal(bfs.eccentricity()[m], ecc[m]), f"{name} call {call}"


def ties_to_traversals(rt, name="rmat13"):
    """Check 7: run(v).depth - 1 == ecc[v]; run / levels, run_batch / batch_levels
    and components() are the same before and after."""
    bfs = make_bfs(name, rt, fresh=True)
    csr = host_csr(name)
    roots = bfs.sample_roots(8, seed=5)
    before = cc._batch_totals(bfs.run_batch(roots, validate=True))
    bfs.run(roots[0])
    lv0 = bfs.levels().copy()
    comp = bfs.components()
    lab0 = bfs.component_labels().copy()
    res = bfs.eccentricities()
    assert res.exact
    assert np.array_equal(bfs.levels(), lv0)  # the single-source state is left alone
    assert np.array_equal(bfs.component_labels(), lab0)
    # the batch before the call: its levels were collected before the passes took the matrix
    got = bfs.batch_levels()
    for i, s in enumerate(roots):
        assert np.array_equal(got[i], dbfs.cpu_bfs(csr, s)[0])
    e = bfs.eccentricity()
    inside = np.nonzero(e >= 0)[0]
    for v in np.random.default_rng(7).choice(inside, 16, replace=False):
        assert bfs.run(int(v)).depth - 1 == e[v]
        assert np.array_equal(bfs.levels(), dbfs.cpu_bfs(csr, int(v))[0])
    assert cc._batch_totals(bfs.run_batch(roots, validate=True)) == before
    got = bfs.batch_levels()
    for i, s in enumerate(roots):
        assert np.array_equal(got[i], dbfs.cpu_bfs(csr, s)[0])
    again = bfs.components()
    assert (again.components, again.largest_label) == (comp.components, comp.largest_label)
    assert np.array_equal(bfs.component_labels(), cc.oracle(name))
    assert np.array_equal(bfs.eccentricity(), e)  # ... and the other way round


def refusals(rt, pytest):
    """Check 8."""
    bfs = make_bfs("rmat10", rt, fresh=True)
    with pytest.raises(Exception, match="eccentricities\\(\\) has not run"):
        bfs.eccentricity()
    with pytest.raises(Exception, match="eccentricities\\(\\) has not run"):
        bfs.eccentricity_bounds()
    with pytest.raises(Exception, match="eccentricities\\(\\) has not run"):
        bfs.engine.gather_eccentricities()
    with pytest.raises(Exception, match="eccentricities\\(\\) has not run"):
        bfs.engine.last_eccentricities()
    with pytest.raises(ValueError, match="target"):
        bfs.eccentricities(target="width")
    with pytest.raises(Exception, match="target"):
        bfs.engine.eccentricities("width")
    with pytest.raises(ValueError, match="component"):
        bfs.eccentricities(component="biggest")
    _, lab = oracle("rmat10")
    not_a_label = int(np.nonzero(lab != np.arange(lab.size))[0][0])
    for bad in (not_a_label, lab.size, lab.size + 5):
        with pytest.raises(Exception, match="no component with label"):
            bfs.eccentricities(component=bad)
    assert not bfs.engine.has_eccentricities
    p = dbfs.rmat_params(10, 16, 3)
    u, v = dbfs.generate_edges(p)
    directed = dbfs.BFS(dbfs.build_csr(p.n, u, v, directed=True), rt, mode="td", directed=True)
    with pytest.raises(Exception, match="undirected graphs only"):
        directed.eccentricities()
    assert bfs.eccentricities().exact and bfs.engine.has_eccentricities


def injected_violation_fails(rt, monkeypatch, pytest):
    """DBFS_FAULT_INJECT kind ecc_device records violation 99 after the first
    bound update: the call fails naming ecc_kernels and leaves no result, a
    traversal and components() are not disturbed, the next clean engine passes."""
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=ecc_device")
    bfs = make_bfs("rmat10", rt, fresh=True)
    bfs.run(bfs.sample_roots(1)[0])
    bfs.components()
    with pytest.raises(Exception, match="device check failed on rank 0: code 99, detail 0, file ecc_kernels$"):
        bfs.eccentricities()
    with pytest.raises(Exception, match="eccentricities\\(\\) has not run"):
        bfs.eccentricity()
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=ecc_device,file=td_kernels")
    with pytest.raises(Exception, match="DBFS_FAULT_INJECT: file"):
        make_bfs("rmat10", rt, fresh=True)
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    bfs = make_bfs("rmat10", rt, fresh=True)
    assert bfs.eccentricities().exact


def injected_violation_fails_checked(bfs_checked, flags):
    """The same through the checked build (on the device: the build whose
    kernels compile their check sites): the call fails naming rank and file,
    also on the second of two ranks; file= is refused with this kind; without
    the injection the same run is clean."""
    base = ["--rmat", "10", "--seed", "3", "--eccentricities", "--ecc-component", "all"] + flags

    def run(inject, more=()):
        return run_cli(bfs_checked, base + list(more), env=dict(os.environ, DBFS_FAULT_INJECT=inject))

    out = run("rank=0,kind=ecc_device")
    assert out.returncode != 0 and "eccentricities diameter" not in out.stdout, out.stdout
    assert "device check failed on rank 0: code 99, detail 0, file ecc_kernels" in out.stderr, out.stderr[-2000:]
    out = run("rank=1,kind=ecc_device", ["--virtual-ranks", "2"])
    assert out.returncode != 0 and "eccentricities diameter" not in out.stdout, out.stdout
    # (virtual ranks share the device's word: whichever rank reads it first reports it)
    assert re.search(r"device check failed on rank [01]: code 99, detail 0, file ecc_kernels", out.stderr), \
        out.stderr[-2000:]
    out = run("rank=0,kind=ecc_device,file=td_kernels")
    assert out.returncode != 0 and "DBFS_FAULT_INJECT: file" in out.stderr, out.stderr[-2000:]
    out = run_cli(bfs_checked, base)
    assert out.returncode == 0 and _line("rmat10", "all") in out.stdout and "Eccentricities OK!" in out.stdout, \
        out.stdout + out.stderr


# ---- CLI -------------------------------------------------------------------------------------

LINE ="eccentricities diameter {d} radius {r} centre {c} periphery {q} settled {s} of {t} passes {p} sources {k} exact {e} ms "


def run_cli(bfs_bin, flags, env=None):
    return subprocess.run([bfs_bin] + flags, capture_output=True, text=True, timeout=120, env=env)


def _line(name, scope, target="all"):
    d, r, c, q = oracle_totals(name, scope)
    _, _, settled, passes, used = reference(name, scope, target)
    return LINE.format(d=d, r=r, c=c, q=q, s=int(settled.sum()), t=int(scope_mask(name, scope).sum()), p=passes, k=used, e=1)


def cli_eccentricities(bfs_bin, flags, tmp_dir):
    """The line, the check's line, the JSON fields and the values file."""
    path = os.path.join(DATA, "two_components.txt")
    name = "two_components"
    ecc, _ = oracle(name)
    for scope in SCOPES:
        out_file = os.path.join(str(tmp_dir), f"ecc_{scope}.txt")
        out = run_cli(bfs_bin, ["3", path, "--components", "--eccentricities", "--ecc-component", scope,
                                "--eccentricities-out", out_file, "--json"] + flags)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        at = [i for i, l in enumerate(lines) if l.startswith("eccentricities ")]
        assert len(at) == 1 and lines[at[0]].startswith(_line(name, scope)), out.stdout
        assert lines[at[0] + 1] == "Eccentricities OK!" and "Wrong output!" not in out.stdout
        assert at[0] > [i for i, l in enumerate(lines) if l.startswith("components ")][0]
        rec = json.loads(lines[at[0] + 2])
        d, r, c, q = oracle_totals(name, scope)
        m = scope_mask(name, scope)
        assert (rec["diameter"], rec["radius"], rec["centre"], rec["periphery"]) == (d, r, c, q)
        assert rec["settled"] == rec["scope_size"] == int(m.sum()) and rec["exact"] is True
        assert rec["passes"] == 1 and rec["sources"] == reference(name, scope)[4] and rec["wide_levels"] is False
        assert rec["ecc_target"] == "all" and rec["ms"] > 0 and rec["bfs_ms"] > 0 and rec["bound_ms"] > 0
        assert rec["select_ms"] > 0
        with open(out_file) as f:
            assert [int(x) for x in f.read().split()] == [int(x) if k else -1 for x, k in zip(ecc, m)]
        assert "Output OK!" in out.stdout  # the traversal from <src> after it
    # a label, a target and a cap
    out = run_cli(bfs_bin, ["3", path, "--eccentricities", "--ecc-component", "0", "--ecc-target", "diameter"] + flags)
    assert out.returncode == 0 and "Eccentricities OK!" in out.stdout, out.stdout + out.stderr
    out = run_cli(bfs_bin, ["3", path, "--eccentricities", "--ecc-max-passes", "0", "--no-oracle"] + flags)
    assert out.returncode == 0 and " passes 0 sources 0 exact 0 ms " in out.stdout, out.stdout + out.stderr
    assert "Eccentricities OK!" not in out.stdout


def cli_generated(bfs_bin, flags):
    """rmat13 whole and, with the threshold lowered, the sampled check."""
    base = ["--rmat", "13", "--seed", "44", "--eccentricities"] + flags
    out = run_cli(bfs_bin, base)
    assert out.returncode == 0, out.stdout + out.stderr
    assert _line("rmat13", "largest") in out.stdout and "Eccentricities OK!\n" in out.stdout, out.stdout
    out = run_cli(bfs_bin, base + ["--ecc-target", "diameter"], env=dict(os.environ, DBFS_ECC_ORACLE_LIMIT="1000"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "eccentricities diameter 6 " in out.stdout and "Eccentricities OK! (16 sampled)" in out.stdout, out.stdout


def cli_usage(bfs_bin):
    path = os.path.join(DATA, "chain8.txt")
    for flags, msg in ((["--directed", "--eccentricities"], "--eccentricities needs an undirected graph"),
                       (["--eccentricities-out", "x"], "--eccentricities-out needs --eccentricities"),
                       (["--eccentricities", "--ecc-target", "width"], "--ecc-target must be"),
                       (["--eccentricities", "--ecc-component", "biggest"], "--ecc-component must be")):
        out = run_cli(bfs_bin, ["0", path, "--cpu"] + flags)
        assert out.returncode == 2 and msg in out.stderr, out.stderr[:300]
    out = run_cli(bfs_bin, ["0", path, "--cpu", "--eccentricities", "--ecc-component", "3"])
    assert out.returncode != 0 and "no component with label 3" in out.stderr, out.stderr[-500:]


def cli_checked_reports(bfs_checked, flags):
    """bin/bfs_checked runs --eccentricities clean, and the injected violation
    fails it naming the file."""
    base = ["--rmat", "13", "--seed", "44", "--eccentricities", "--json"] + flags
    out = run_cli(bfs_checked, base)
    assert out.returncode == 0, out.stdout + out.stderr
    assert _line("rmat13", "largest") in out.stdout and "Eccentricities OK!" in out.stdout
    runs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{") and '"backend"' in l]
    assert runs and all(r["backend"].endswith("+checked") for r in runs) or flags == ["--cpu"], out.stdout
    out = run_cli(bfs_checked, base, env=dict(os.environ, DBFS_FAULT_INJECT="rank=0,kind=ecc_device"))
    assert out.returncode != 0, out.stdout
    assert "device check failed on rank 0: code 99" in out.stderr, out.stderr[-2000:]
    assert "file ecc_kernels" in out.stderr, out.stderr[-2000:]
    assert "eccentricities diameter" not in out.stdout
