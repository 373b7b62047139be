"""Cases and checks shared by the batch betweenness tests (test_betweenness.py
on the CPU backend, test_betweenness_gpu.py on the GPU): run_batch(betweenness /
path_counts) against the sequential Brandes oracle cpu_betweenness and against
hand-derived values.  Graphs and source sets are batch_cases' and
directed_cases'.

Comparison rule for the dependency sums: relative error 1e-9, an exact 0.0
wherever the oracle has one, every value finite.  Every operation adds,
multiplies or divides non-negative doubles, so nothing cancels: a result's
relative error is at most (roundings on its dependency chain) x 2^-53, and the
chain is shorter than 8 (nnz + n) ~ 2.2e6 on the largest graph here (rmat13,
262144 entries): 2.4e-10 per side.  Path counts are compared for equality:
sums of integers below 2^53 are exact in any order.  Counts at and above 2^53,
up to the range contract at 2^1024, are betweenness_exact_cases.py's, against
an exact reference."""
import json
import os
import subprocess

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks
from distributed_cuda_bfs_amd.utils.centrality import betweenness_scores

import batch_cases as bc
import directed_cases as dc

RTOL = 1e-9

# (graph, source set): undirected from batch_cases, directed from directed_cases
UNDIRECTED = [("star5000", "k64"), ("n4097", "k130"), ("rmat13", "k63"), ("rmat13", "k64dup"), ("rmat10", "all"),
              ("two_components", "k64"), ("path300", "k64"), ("file_chain8", "k1"),
              ("fans300", "k1"), ("fans300", "k64"), ("fans", "k64")]
# exact path counts (path_counts): the fans graphs' rows end on every boundary of the row walk
PATH_COUNT_CASES = [("rmat10", "k64dup", False), ("d_rmat10", "k64", True),
                    ("fans300", "k1", False), ("fans300", "k64", False), ("fans", "k64", False)]
DIRECTED = [("d_rmat13", "k64dup"), ("star_in5000", "k64"), ("star_out5000", "k64"), ("one_way_bridge", "k64"),
            ("tiny5", "k64"), ("empty3", "k64")]
CASES = [(g, k, False) for g, k in UNDIRECTED] + [(g, k, True) for g, k in DIRECTED]
RANK_CASES = [("rmat10", False), ("n4097", False), ("d_rmat10", True)]

_oracle_cache = {}
_bfs_cache = {}


def host_csr(name, directed):
    return dc.host_csr(name) if directed else bc.host_csr(name)


def sources(name, kind, directed):
    if kind == "all":
        return list(range(host_csr(name, directed).n))
    return dc.sources(name, kind) if directed else bc.sources(name, kind)


def oracle(name, kind, directed, counts=False):
    """cpu_betweenness of the case: (dep, sigma or None), computed once, never written to."""
    key = (name, kind, directed, counts)
    if key not in _oracle_cache:
        dep, sigma = dbfs.cpu_betweenness(host_csr(name, directed), sources(name, kind, directed), directed, counts)
        for a in (dep, sigma):
            if a is not None:
                a.setflags(write=False)
        _oracle_cache[key] = (dep, sigma)
    return _oracle_cache[key]


def make_bfs(name, directed, rt):
    """One BFS per graph and runtime, shared by the tests of a module."""
    key = (name, directed, id(rt))
    if key not in _bfs_cache:
        if directed:
            _bfs_cache[key] = dbfs.BFS(dc.host_csr(name), rt, mode="td", directed=True)
        else:
            _bfs_cache[key] = dbfs.BFS(bc.bfs_input(name), rt)
    return _bfs_cache[key]


def assert_close(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.all(np.isfinite(got))
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0), f"{np.count_nonzero(got[zero])} values where the oracle has 0.0"
    bad = np.nonzero(~np.isclose(got, ref, rtol=RTOL, atol=0.0))[0]
    assert bad.size == 0, (f"{bad.size} vertices differ, first " +
                           ", ".join(f"{int(v)}: {got[v]!r} vs {ref[v]!r}" for v in bad[:6]))
    assert np.allclose(got, ref, rtol=RTOL, atol=0.0)


def matches_oracle(rt, name, kind, directed, **kw):
    src = sources(name, kind, directed)
    bfs = make_bfs(name, directed, rt)
    res = bfs.run_batch(src, betweenness=True, **kw)
    assert_close(bfs.batch_betweenness(), oracle(name, kind, directed)[0])
    n = host_csr(name, directed).n
    assert bfs.batch_betweenness().shape == (n,)
    assert res.bc_ms > 0.0 and res.check_ms == 0.0
    assert res.bc_ms >= res.bc_forward_ms and res.bc_ms >= res.bc_backward_ms
    # one launch per level out (1 .. depth - 1) and back (depth - 1 .. 1) of every pass
    depth = np.asarray(res.depth)
    launches = sum(2 * (int(depth[p:p + 64].max()) - 1) for p in range(0, len(src), 64))
    assert res.bc_launches == launches
    assert 0 <= res.bc_rows_walked <= launches * n
    assert res.wide_levels == (name in ("path300", "d_path300", "fans300"))
    return res


def path_counts(rt, name, kind, directed):
    src = sources(name, kind, directed)
    dep_ref, sig_ref = oracle(name, kind, directed, counts=True)
    assert sig_ref.max() < 2.0 ** 53  # (a finding if not: the counts would no longer be exact)
    bfs = make_bfs(name, directed, rt)
    bfs.run_batch(src, betweenness=True, path_counts=True)
    got = bfs.batch_path_counts()
    assert got.dtype == np.float64 and got.shape == (len(src), host_csr(name, directed).n)
    assert np.array_equal(got, sig_ref)
    if kind == "k64dup":
        assert src[5] == src[9] and np.array_equal(got[5], got[9])
    assert_close(bfs.batch_betweenness(), dep_ref)
    # counts alone: the same, and no dependency vector
    bfs.run_batch(src, path_counts=True)
    assert np.array_equal(bfs.batch_path_counts(), sig_ref)
    with np.testing.assert_raises(Exception):
        bfs.batch_betweenness()


# ---- hand-derived values (they check the oracle too) -----------------------------

def _both(rt, csr, directed, src, **kw):
    bfs = dbfs.BFS(csr, rt, mode="td" if directed else "do", directed=directed)
    res = bfs.run_batch(src, betweenness=True, **kw)
    return bfs, res, bfs.batch_betweenness(), dbfs.cpu_betweenness(csr, src, directed)[0]


def hand_path300(rt):
    """Undirected path, every vertex a source: i (299 - i) pairs pass through i, each from both ends."""
    i = np.arange(300, dtype=np.float64)
    bfs, res, got, ref = _both(rt, bc.host_csr("path300"), False, list(range(300)))
    assert res.passes == 5 and res.wide_levels
    assert np.array_equal(ref, 2 * i * (299 - i)) and np.array_equal(got, 2 * i * (299 - i))
    assert np.array_equal(betweenness_scores(got, 300, 300, False, normalized=False), i * (299 - i))


def hand_d_path300(rt):
    i = np.arange(300, dtype=np.float64)
    _, _, got, ref = _both(rt, dc.host_csr("d_path300"), True, list(range(300)))
    assert np.array_equal(ref, i * (299 - i)) and np.array_equal(got, i * (299 - i))


def hand_back_edge10(rt):
    """A directed 10-cycle: from every source the 8 inner vertices at distance d carry 9 - d."""
    _, _, got, ref = _both(rt, dc.host_csr("back_edge10"), True, list(range(10)))
    assert np.array_equal(ref, np.full(10, 36.0)) and np.array_equal(got, np.full(10, 36.0))


def hand_doubled_square(rt):
    """The square 0-1-2-3-0 with edge 0-1 doubled: duplicates are parallel edges."""
    csr = dbfs.build_csr(4, np.array([0, 0, 1, 2, 3], dtype=np.uint32), np.array([1, 1, 2, 3, 0], dtype=np.uint32))
    bfs, _, got, ref = _both(rt, csr, False, [0, 1, 2, 3], path_counts=True)
    exp = np.array([4 / 3, 4 / 3, 2 / 3, 2 / 3])
    assert np.allclose(ref, exp, rtol=RTOL, atol=0.0) and np.allclose(got, exp, rtol=RTOL, atol=0.0)
    assert list(bfs.batch_path_counts()[0]) == [1.0, 2.0, 3.0, 1.0]
    assert list(dbfs.cpu_betweenness(csr, [0, 1, 2, 3], False, True)[1][0]) == [1.0, 2.0, 3.0, 1.0]


def hand_fans300(rt):
    """From source 0 every fan vertex has one shortest path per entry of its row."""
    csr = bc.host_csr("fans300")
    bfs = dbfs.BFS(csr, rt)
    bfs.run_batch([0], path_counts=True)
    got = bfs.batch_path_counts()[0]
    ref = dbfs.cpu_betweenness(csr, [0], False, True)[1][0]
    for d in bc.FAN_SIZES:
        assert got[bc.fan_vertex(d)] == d and ref[bc.fan_vertex(d)] == d
    assert np.array_equal(got, ref)


HAND = {"path300": hand_path300, "fans300": hand_fans300, "d_path300": hand_d_path300, "back_edge10": hand_back_edge10,
        "doubled_square": hand_doubled_square}


def scores():
    dep = np.array([0.0, 6.0, 8.0, 6.0, 0.0])
    assert np.array_equal(betweenness_scores(dep, 5, 5, False), dep / 2)
    assert np.array_equal(betweenness_scores(dep, 5, 5, True), dep)
    assert np.array_equal(betweenness_scores(dep, 5, 2, True), dep * 2.5)
    assert np.array_equal(betweenness_scores(dep, 5, 2, True, rescale=False), dep)
    assert np.array_equal(betweenness_scores(dep, 5, 5, True, normalized=True), dep / 12)
    assert np.array_equal(betweenness_scores(dep, 5, 5, False, normalized=True), dep / 2 / 6)
    assert dep[2] == 8.0  # (the input is left alone)


# ---- other properties --------------------------------------------------------------

def deterministic(rt):
    src = sources("rmat13", "k130", False)
    bfs = make_bfs("rmat13", False, rt)
    bfs.run_batch(src, betweenness=True)
    first = bfs.batch_betweenness().copy()
    bfs.run_batch(src, betweenness=True)
    assert np.array_equal(first.view(np.uint64), bfs.batch_betweenness().view(np.uint64))
    assert_close(first, oracle("rmat13", "k130", False)[0])


def split_threshold(rt, name, directed, above):
    """Engine option bc_split_row: rows of more than `above` entries go to the
    workgroup-per-row launch (0: none do); the default is crossed by the stars'
    5000-entry rows only, so a low one sends many rows of an RMAT graph there."""
    bfs = dbfs.BFS(host_csr(name, directed), rt, mode="td" if directed else "do", directed=directed)
    bfs.engine.set_option("bc_split_row", above)
    src = sources(name, "k64dup", directed)
    bfs.run_batch(src, betweenness=True, path_counts=True)
    dep_ref, sig_ref = oracle(name, "k64dup", directed, counts=True)
    assert_close(bfs.batch_betweenness(), dep_ref)
    assert np.array_equal(bfs.batch_path_counts(), sig_ref)
    first = bfs.batch_betweenness().copy()
    bfs.run_batch(src, betweenness=True)
    assert np.array_equal(first.view(np.uint64), bfs.batch_betweenness().view(np.uint64))


def direction_independent(rt, direction):
    matches_oracle(rt, "rmat10", "k64", False, direction=direction)


def with_validate_and_parents(rt):
    """The check and the accumulation after one pass each leave the other's result alone."""
    src = sources("n4097", "k130", False)
    bfs = make_bfs("n4097", False, rt)
    res = bfs.run_batch(src, validate=True, parents=True, betweenness=True)
    assert res.validated is True and res.check_ms > 0.0 and res.bc_ms > 0.0
    assert_close(bfs.batch_betweenness(), oracle("n4097", "k130", False)[0])
    bc.check_batch("n4097", src, res, bfs.batch_levels())


def virtual_ranks(name, directed, P, device):
    src = sources(name, "k130", directed)
    csr = host_csr(name, directed)

    def body(rt):
        bfs = dbfs.BFS(csr, rt, mode="td" if directed else "do", directed=directed)
        bfs.run_batch(src, betweenness=True, path_counts=True)
        return bfs.batch_betweenness(), bfs.batch_path_counts()

    dep_ref, sig_ref = oracle(name, "k130", directed, counts=True)
    for dep, sig in run_virtual_ranks(P, body, device=device):
        assert_close(dep, dep_ref)
        assert np.array_equal(sig, sig_ref)


def argument_errors(rt, pytest):
    bfs = dbfs.BFS(bc.host_csr("rmat10"), rt)
    src = sources("rmat10", "k64", False)
    with pytest.raises(Exception, match="keep_levels"):
        bfs.run_batch(src, betweenness=True, levels=False)
    with pytest.raises(Exception, match="keep_levels"):
        bfs.engine.run_batch(src, "auto", False, False, False, True, False)
    with pytest.raises(Exception, match="no batch has run with betweenness"):
        bfs.batch_betweenness()
    with pytest.raises(Exception, match="no batch has run with keep_path_counts"):
        bfs.batch_path_counts()
    bfs.run_batch(src)  # a batch without the flags leaves none either
    with pytest.raises(Exception, match="no batch has run with betweenness"):
        bfs.batch_betweenness()


def injected_violation_fails(rt, monkeypatch, pytest):
    """DBFS_FAULT_INJECT kind bc_device records violation 99 during the
    accumulation: that call fails, the next clean one passes."""
    csr = bc.host_csr("rmat10")
    src = sources("rmat10", "k64", False)
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,kind=bc_device")
    bfs = dbfs.BFS(csr, rt)
    bfs.run_batch(src, validate=True)  # not the accumulation's
    with pytest.raises(Exception, match="device check failed on rank 0: code 99"):
        bfs.run_batch(src, betweenness=True)
    with pytest.raises(Exception, match="no batch has run with betweenness"):
        bfs.batch_betweenness()
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    bfs = dbfs.BFS(csr, rt)
    bfs.run_batch(src, betweenness=True)
    assert_close(bfs.batch_betweenness(), oracle("rmat10", "k64", False)[0])


# ---- CLI ---------------------------------------------------------------------------

LINE = "batch betweenness sources 70 bc_ms "


def _line(out):
    lines = [l for l in out.stdout.splitlines() if l.startswith("batch betweenness")]
    assert len(lines) == 1 and lines[0].startswith(LINE), out.stdout + out.stderr
    w = lines[0].split()
    assert w[6:8] == ["max", "vertex"] and w[9] == "score"
    return int(w[8]), float(w[10])


def cli_betweenness(bfs_bin, path, flags):
    base = ["0", path, "--roots", "70", "--batch", "--betweenness"] + flags
    out = dc.run_cli(bfs_bin, base)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Betweenness OK!" in out.stdout and "Output OK!" in out.stdout and "Wrong output!" not in out.stdout
    _line(out)
    out = dc.run_cli(bfs_bin, base + ["--no-oracle", "--json"])
    assert out.returncode == 0 and "Betweenness OK!" not in out.stdout
    _line(out)
    assert any(l.startswith("{") and '"batch":true' in l and '"bc_ms":' in l for l in out.stdout.splitlines())


def cli_out_file(bfs_bin, path, tmp_dir, rt, cpu, directed):
    """--betweenness-out holds one value per vertex: the printed top vertex and
    score are the file's, and the file is what the API gives for the same
    roots (the K single runs of `--roots K --json` without --batch name them)."""
    dest = os.path.join(str(tmp_dir), "bc_out_%d.txt" % int(directed))
    extra = (["--directed"] if directed else []) + (["--cpu"] if cpu else [])
    out = dc.run_cli(bfs_bin, ["0", path, "--roots", "70", "--batch", "--betweenness", "--betweenness-out", dest] + extra)
    assert out.returncode == 0 and "Betweenness OK!" in out.stdout, out.stdout + out.stderr
    with open(dest) as f:
        vals = np.array([float(x) for x in f.read().split()])
    top, score = _line(out)
    csr = dbfs.read_graph(path, directed=directed)
    assert vals.shape == (csr.n,) and int(np.argmax(vals)) == top and vals[top] == score
    out = dc.run_cli(bfs_bin, ["0", path, "--roots", "70", "--json", "--no-oracle", "--cpu"] + (["--directed"] if directed else []))
    assert out.returncode == 0, out.stdout + out.stderr
    roots = [json.loads(l)["source"] for l in out.stdout.splitlines() if l.startswith("{") and '"source"' in l][1:]
    assert len(roots) == 70
    bfs = dbfs.BFS(csr, rt, mode="td" if directed else "do", directed=directed)
    bfs.run_batch(roots, betweenness=True)
    assert_close(vals, bfs.batch_betweenness())
    assert_close(vals, dbfs.cpu_betweenness(csr, roots, directed)[0])


def cli_usage(bfs_bin, path):
    for flags in (["--betweenness"], ["--roots", "70", "--betweenness"], ["--batch", "--betweenness"],
                  ["--roots", "70", "--batch", "--betweenness-out", "x"]):
        out = dc.run_cli(bfs_bin, ["0", path, "--cpu"] + flags)
        assert out.returncode == 2 and "--betweenness" in out.stderr, (flags, out.stdout, out.stderr)


def cli_checked_reports(bfs_checked, path):
    flags = ["0", path, "--roots", "70", "--batch", "--betweenness"]
    env = dict(os.environ, DBFS_FAULT_INJECT="rank=0,kind=bc_device")
    out = subprocess.run([bfs_checked] + flags, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0, out.stdout
    assert "device check failed on rank 0: code 99" in out.stderr, out.stderr[-2000:]
    assert "file ms_bc_kernels" in out.stderr, out.stderr[-2000:]
    assert "batch betweenness" not in out.stdout
    out = dc.run_cli(bfs_checked, flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Betweenness OK!" in out.stdout and "Wrong output!" not in out.stdout
