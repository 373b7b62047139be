"""Checks shared by the batch validation tests (test_batch_validate.py on the
CPU backend, test_batch_validate_gpu.py on the GPU): the device check of
run_batch(validate=True) against the numpy reference batch_levels_violations,
the parent trees of run_batch(parents=True), and the planted violations."""
import json
import subprocess

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.utils.validate import batch_levels_violations

import batch_cases as bc

# graph, source set: what each pins is in the table of the two test files' docstrings
CASES = [
    ("star5000", "k64"),
    ("n4097", "k130"),
    ("rmat13", "k63"),
    ("rmat13", "k64dup"),
    ("two_components", "k64"),
    ("path300", "k64"),
    ("file_chain8", "k1"),
    ("fans300", "k1"),
    ("fans300", "k64"),
    ("fans", "k64"),
]
_edge_codes = {}
_reference = {}


def edge_codes(name, csr=None):
    """Every adjacency entry (v, w) of the graph as v * n + w."""
    if name not in _edge_codes:
        csr = csr or bc.host_csr(name)
        ro = np.asarray(csr.row_off)
        rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(ro))
        _edge_codes[name] = np.unique(rows * csr.n + np.asarray(csr.col).astype(np.int64))
    return _edge_codes[name]


def reference(name, kind, src, levels):
    """batch_levels_violations per source, computed once per (graph, source
    set): the levels do not depend on the direction, which is asserted."""
    key = (name, kind)
    if key not in _reference:
        lv = np.array(levels, copy=True)
        lv.setflags(write=False)
        _reference[key] = (lv, [batch_levels_violations(bc.host_csr(name), lv[i], s) for i, s in enumerate(src)])
    lv, ref = _reference[key]
    assert np.array_equal(levels, lv)
    return ref


def check_parent_trees(name, src, levels, par, csr=None):
    """Graph500's parent-tree rules for all k trees at once."""
    k, n = levels.shape
    assert par.shape == (k, n) and par.dtype == np.int64
    idx = np.arange(k)
    s = np.asarray(src, dtype=np.int64)
    assert np.array_equal(par[idx, s], s), "parent[src] == src"
    reached = levels != dbfs.UNREACHED
    assert np.all(par[~reached] == -1), "unreached vertices have -1"
    need = reached.copy()
    need[idx, s] = False
    ki, v = np.nonzero(need)
    p = par[ki, v]
    assert np.all((p >= 0) & (p < n)), "every reached vertex has a parent"
    assert np.array_equal(levels[ki, p], levels[ki, v] - 1), "the parent is one level closer"
    assert np.all(np.isin(v.astype(np.int64) * n + p, edge_codes(name, csr))), "(v, parent[v]) is an adjacency entry"


def check_clean(name, kind, src, res, levels, par):
    assert res.validated is True
    assert res.violations == [(0, 0, 0)] * len(src)
    assert res.violations == reference(name, kind, src, levels)
    check_parent_trees(name, src, levels, par)
    assert res.check_ms > 0  # (reported apart from res.ms; no timing comparison)


def positive(bfs, name, kind, direction):
    src = bc.sources(name, kind)
    res = bfs.run_batch(src, direction=direction, validate=True, parents=True)
    levels = bfs.batch_levels()
    bc.check_batch(name, src, res, levels)
    check_clean(name, kind, src, res, levels, bfs.batch_parents())
    assert res.wide_levels == (name in ("path300", "fans300"))


# parents without validate: the parent form alone, which leaves a row once every reached lane has
# its parent -- the 5000-entry row, the 16-bit form, skewed rows with k < 64, three passes with masked lanes
PARENTS_ONLY_CASES = [("star5000", "k64"), ("path300", "k64"), ("rmat13", "k63"), ("n4097", "k130"),
                      ("fans300", "k1"), ("fans300", "k64"), ("fans", "k64")]


def parents_only(bfs, name, kind):
    """run_batch(parents=True) gives the trees of run_batch(validate=True,
    parents=True): both keep the first parent in stored row order."""
    src = bc.sources(name, kind)
    bfs.run_batch(src, validate=True, parents=True)
    both = bfs.batch_parents().copy()
    res = bfs.run_batch(src, parents=True)
    assert res.violations is None and res.validated is None
    assert res.check_ms > 0
    par = bfs.batch_parents()
    check_parent_trees(name, src, bfs.batch_levels(), par)
    assert np.array_equal(par, both)


def parents_chunked(make_bfs):
    """131072 owned rows: the parents come back to the host 65536 rows at a
    time, so two full chunks; three sources, the rest of the lanes masked."""
    name = "rmat17"
    if name not in _reference:
        csr = dbfs.host_csr_from_params(dbfs.rmat_params(17, 16, 48))
        some = np.nonzero(np.diff(np.asarray(csr.row_off)))[0]
        src = [int(some[0]), int(some[some.size // 2]), int(some[-1])]
        _reference[name] = (csr, src, np.stack([np.asarray(dbfs.cpu_bfs(csr, s)[0]) for s in src]))
    csr, src, exp = _reference[name]
    bfs = make_bfs(csr)
    res = bfs.run_batch(src, validate=True, parents=True)
    levels = bfs.batch_levels()
    assert np.array_equal(levels, exp)
    assert res.validated is True
    par = bfs.batch_parents()
    check_parent_trees(name, src, levels, par, csr)
    assert bfs.run_batch(src, parents=True).violations is None and np.array_equal(bfs.batch_parents(), par)


def swapped(src, i, j):
    out = list(src)
    out[i], out[j] = out[j], out[i]
    return out


def as_tuples(a):
    return [tuple(int(x) for x in row) for row in np.asarray(a)]


def negative_swapped(bfs, name="rmat10"):
    src = bc.sources(name, "k64")
    assert src[3] != src[7]
    bfs.run_batch(src)
    levels = bfs.batch_levels()
    sw = swapped(src, 3, 7)
    got = as_tuples(bfs.engine.validate_batch_pass(sw))
    assert got == [batch_levels_violations(bc.host_csr(name), levels[i], s) for i, s in enumerate(sw)]
    # each of the two lanes: its true source has no parent, its claimed one is not at level 0
    assert got == [(0, 0, 2) if i in (3, 7) else (0, 0, 0) for i in range(64)]
    assert as_tuples(bfs.engine.validate_batch_pass(src)) == [(0, 0, 0)] * 64


def negative_planted(bfs, level):
    """path300, source 0 on slot 0: vertex 150's level overwritten (level < 0: unreached)."""
    name = "path300"
    src = bc.sources(name, "k64")
    assert src[0] == 0
    bfs.run_batch(src)
    levels = bfs.batch_levels().copy()
    bfs.engine.debug_set_batch_level(0, 150, level)
    got = as_tuples(bfs.engine.validate_batch_pass(src))
    levels[0, 150] = dbfs.UNREACHED if level < 0 else level
    exp = batch_levels_violations(bc.host_csr(name), levels[0], src[0])
    assert got[0] == exp
    assert got[1:] == [(0, 0, 0)] * 63
    if level < 0:
        assert exp[1] > 0 and exp[2] > 0 and exp[0] == 0
    else:
        assert exp[0] > 0
    return exp


def ranks_body(name):
    """One virtual rank's part of the several-rank test."""
    src = bc.sources(name, "k130")
    csr = bc.host_csr(name)

    def body(rt):
        bfs = dbfs.BFS(csr, rt)
        res = bfs.run_batch(src, validate=True, parents=True)
        levels = bfs.batch_levels()
        par = bfs.batch_parents()
        alone = bfs.run_batch(src, parents=True)  # the parent form alone: the same trees
        assert alone.violations is None and np.array_equal(bfs.batch_parents(), par)
        # the negative: two of the first 64 sources swapped, distinct vertices on different ranks
        own = [bfs.partition.owner(int(s)) for s in src[:64]]
        i, j = next((i, j) for i in range(64) for j in range(i + 1, 64) if own[i] != own[j])
        bfs.run_batch(src[:64])
        sw = swapped(src[:64], i, j)
        return res, levels, par, sw, as_tuples(bfs.engine.validate_batch_pass(sw))

    return src, body


def check_ranks(name, src, results):
    csr = bc.host_csr(name)
    for res, levels, par, sw, got in results:
        bc.check_batch(name, src, res, levels)
        check_clean(name, "k130", src, res, levels, par)
        assert np.array_equal(par, results[0][2])
        exp = [batch_levels_violations(csr, levels[i], s) for i, s in enumerate(sw)]
        assert got == exp and sum(e[2] for e in exp) == 4 and sw == results[0][3]


def argument_errors(bfs, pytest):
    src = bc.sources("rmat10", "k64")
    with pytest.raises(Exception, match="level"):
        bfs.run_batch(src, levels=False, validate=True)
    with pytest.raises(Exception, match="level"):
        bfs.engine.run_batch(src, "auto", False, False, True)
    plain = bfs.run_batch(src)
    assert plain.violations is None and plain.validated is None and plain.check_ms == 0.0
    with pytest.raises(Exception, match="keep_parents"):
        bfs.batch_parents()
    with pytest.raises(Exception, match="as many sources"):
        bfs.engine.validate_batch_pass(src[:63])
    bfs.run_batch(src, levels=False)
    with pytest.raises(Exception, match="keep_levels"):
        bfs.engine.validate_batch_pass(src)


CLI_BATCH = ["--uniform", "5000:12000", "--roots", "70", "--batch"]
CLEAN_LINE = "batch validation 70/70 sources clean gap 0 cross 0 orphan 0"


def cli(bfs_bin, flags):
    out = subprocess.run([bfs_bin] + flags, capture_output=True, text=True, timeout=120)
    lines = [l for l in out.stdout.splitlines() if l.startswith("batch validation")]
    return out, lines


def check_cli(bfs_bin, device_flags):
    for extra in ([], ["--virtual-ranks", "3"]):
        out, lines = cli(bfs_bin, device_flags + CLI_BATCH + ["--validate"] + extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert lines == [CLEAN_LINE], out.stdout
        assert "Wrong output!" not in out.stdout
        # the device check is the only one left
        out, lines = cli(bfs_bin, device_flags + CLI_BATCH + ["--validate", "--no-oracle", "--json"] + extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert lines == [CLEAN_LINE], out.stdout
        rec = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{") and '"batch":true' in l]
        assert len(rec) == 1 and rec[0]["validated_sources"] == "70/70" and rec[0]["check_ms"] > 0
    out, lines = cli(bfs_bin, device_flags + CLI_BATCH)
    assert out.returncode == 0 and lines == [] and "validated_sources" not in out.stdout
