"""Cases and checks shared by test_betweenness_exact.py (CPU backend and the
oracle cpu_betweenness) and test_betweenness_exact_gpu.py (ms_bc_kernels.hip):
path counts and dependency sums against an exact reference, where the counts
no longer fit 53 bits, and the range contract above 2^1024.

The reference (exact) is sequential Brandes over a HostCSR's row_off / col in
Python integers (sigma) and fractions.Fraction (delta): no double anywhere.
Duplicate entries are parallel edges, the source takes no share, a directed
graph is followed along its stored out-rows.

Tolerances, derived and not tuned.  Every operation adds, multiplies or
divides non-negative doubles, so nothing cancels.  With u = 2^-53, r the
longest walked row and a vertex on level L: its count is a sum of at most r
counts of level L - 1, so it carries at most L (r - 1) u, in whatever order the
terms meet (the 16 partial sums of a long row in wave order included).  The
backward sweep repeats that per level and adds a few roundings for the divide,
the multiply and the 1 +.  With depth = max(res.depth):
  counts        relative error <= 1.01 depth (r - 1) u; equal where the exact
                count is below 2^53
  dependencies  relative error <= 4 depth (r + 2) u; an exact 0.0 where the
                exact value is 0; every value finite
For the graphs here the bounds lie between 1e-13 and 2.2e-11.  Errors are
computed exactly (Fraction(float) - reference), and the largest one of every
check is printed (`exact-error ...`; profiles/ms_bfs_bc_exact.txt has them).

Range contract: a batch in which some source has more than DBL_MAX shortest
paths to a vertex raises, names the source and leaves no result; it never
returns a non-finite value."""
import os
from fractions import Fraction

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks

import directed_cases as dc

U = Fraction(1, 2 ** 53)
OVERFLOW = "exceed the range of a double"


# ---- graphs ------------------------------------------------------------------------

def _csr(n, u, v, directed):
    return dbfs.build_csr(int(n), np.asarray(u, dtype=np.uint32), np.asarray(v, dtype=np.uint32), directed=directed)


def _multi_path_edges(mults):
    u = np.repeat(np.arange(len(mults), dtype=np.int64), np.asarray(mults, dtype=np.int64))
    return u, u + 1


def multi_path(mults, directed=False):
    """Vertex i joined to i + 1 by mults[i] parallel edges (directed: i -> i + 1)."""
    u, v = _multi_path_edges(mults)
    return _csr(len(mults) + 1, u, v, directed)


def thick_tail(mult, plen, m, L, directed=False):
    """multi_path([mult] * plen), its last vertex joined to all of layer 0, and
    L layers of m vertices each completely joined to the next."""
    u, v = _multi_path_edges([mult] * plen)
    first = plen + 1  # layer l holds first + l * m .. first + (l + 1) * m - 1
    us, vs = [u, np.full(m, plen, dtype=np.int64)], [v, first + np.arange(m, dtype=np.int64)]
    for l in range(L - 1):
        a = first + l * m + np.arange(m, dtype=np.int64)
        us.append(np.repeat(a, m))
        vs.append(np.tile(a + m, m))
    return _csr(first + L * m, np.concatenate(us), np.concatenate(vs), directed)


def grid(w, h, directed=False):
    """dbfs.grid_params(w, h); directed: its edges from the lower to the higher vertex id."""
    g = dbfs.host_csr_from_params(dbfs.grid_params(w, h))
    if not directed:
        return g
    row_off, col = np.asarray(g.row_off), np.asarray(g.col).astype(np.int64)
    u = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(row_off))
    return _csr(g.n, u[u < col], col[u < col], True)


def _grid40_sources():
    return [0, 820, 1599] + [int(x) for x in np.random.default_rng(40).integers(0, 1600, 61)]


def _tail_n(plen, m, L):
    return plen + 1 + m * L


# name -> (builder(directed), sources); every graph has both forms
GRAPHS = {
    "grid40x40": (lambda d: grid(40, 40, d), _grid40_sources()),
    "grid20x300": (lambda d: grid(20, 300, d), [0, 3010]),
    "doubled1023": (lambda d: multi_path([2] * 1023, d), [0, 511, 1023]),
    "tripled646": (lambda d: multi_path([3] * 646, d), [0, 323, 646]),
    "mult2357": (lambda d: multi_path([2, 3, 5, 7] * 130, d), [0, 100, 520]),
    "tail40x8": (lambda d: thick_tail(7, 340, 40, 8, d), [0, 170, _tail_n(340, 40, 8) - 1]),
    "tail70x6": (lambda d: thick_tail(7, 340, 70, 6, d), [0, 170, _tail_n(340, 70, 6) - 1]),
    # the range contract's
    "doubled1024": (lambda d: multi_path([2] * 1024, d), [0]),
    "tripled647": (lambda d: multi_path([3] * 647, d), [0]),
    "tail40x8_long": (lambda d: thick_tail(7, 362, 40, 8, d), [0]),
}

# (graph, directed) of part A, by what they are there for
IN_RANGE = [("grid40x40", False), ("grid20x300", False)]
EXACT_TOP = [("doubled1023", False), ("doubled1023", True)]
ROUNDED_TOP = [("tripled646", False), ("mult2357", False)]
LONG_ROWS = [("tail40x8", False), ("tail70x6", False), ("tail40x8", True), ("tail70x6", True)]
ORACLE_CASES = IN_RANGE + EXACT_TOP + ROUNDED_TOP + LONG_ROWS
RANK_CASES = [("tail40x8", False), ("grid20x300", False)]
OVERFLOWING = [("doubled1024", False), ("tripled647", False), ("doubled1024", True)]

_csr_cache = {}
_exact_cache = {}


def host_csr(name, directed):
    key = (name, directed)
    if key not in _csr_cache:
        _csr_cache[key] = GRAPHS[name][0](directed)
    return _csr_cache[key]


def sources(name):
    return list(GRAPHS[name][1])


# ---- the exact reference -------------------------------------------------------------

class Exact:
    """dep[v]: Fraction; sigma[i][v]: int; depth: levels of the deepest source;
    max_row: the longest row either sweep walks."""
    __slots__ = ("dep", "sigma", "depth", "max_row")


def exact_brandes(csr, srcs, directed):
    row_off, col = np.asarray(csr.row_off).tolist(), np.asarray(csr.col).tolist()
    n = csr.n
    ex = Exact()
    ex.dep, ex.sigma, ex.depth = [Fraction(0)] * n, [], 0
    deg = np.diff(np.asarray(csr.row_off))
    ex.max_row = int(deg.max()) if n else 0
    if directed and len(col):  # (the forward sweep walks the rows of in-edges)
        ex.max_row = max(ex.max_row, int(np.bincount(np.asarray(csr.col), minlength=n).max()))
    for s in srcs:
        dist, sigma, order = [-1] * n, [0] * n, [s]
        dist[s], sigma[s] = 0, 1
        for u in order:  # (grows while read: the queue)
            du, su = dist[u] + 1, sigma[u]
            for e in range(row_off[u], row_off[u + 1]):
                w = col[e]
                if dist[w] < 0:
                    dist[w] = du
                    order.append(w)
                if dist[w] == du:
                    sigma[w] += su  # (u's count is final: every vertex one level closer came before it)
        # coef[w] = (1 + delta[w]) / sigma[w]; delta[v] = sigma[v] * the sum of coef over v's successors
        coef = [None] * n
        for v in reversed(order):
            dv, acc = dist[v] + 1, Fraction(0)
            for e in range(row_off[v], row_off[v + 1]):
                if dist[col[e]] == dv:
                    acc += coef[col[e]]
            delta = sigma[v] * acc
            coef[v] = (1 + delta) / sigma[v]
            if v != s:
                ex.dep[v] += delta
        ex.sigma.append(sigma)
        ex.depth = max(ex.depth, dist[order[-1]] + 1)
    return ex


def exact(name, directed, srcs=None):
    """The reference of a case, computed once per module run and never written to."""
    srcs = sources(name) if srcs is None else list(srcs)
    key = (name, directed, tuple(srcs))
    if key not in _exact_cache:
        _exact_cache[key] = exact_brandes(host_csr(name, directed), srcs, directed)
    return _exact_cache[key]


# ---- the comparison --------------------------------------------------------------------

def _rel(got, ref):
    return abs(Fraction(float(got)) - ref) / ref


def check_counts(label, got, ex):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == (len(ex.sigma), len(ex.dep))
    assert np.all(np.isfinite(got)), f"{label}: {np.count_nonzero(~np.isfinite(got))} counts are not finite"
    bound = Fraction(101, 100) * ex.depth * (ex.max_row - 1) * U
    worst = Fraction(0)
    for i, ref in enumerate(ex.sigma):
        row = got[i].tolist()
        for v, s in enumerate(ref):
            if s < 2 ** 53:
                assert row[v] == s, f"{label}: count [{i}][{v}] is {row[v]!r}, exactly {s}"
            else:
                worst = max(worst, _rel(row[v], s))
    print(f"exact-error {label} counts {float(worst):.3g} bound {float(bound):.3g}")
    assert worst <= bound, f"{label}: counts off by {float(worst):.3g} relative, bound {float(bound):.3g}"


def check_dep(label, got, ex):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == (len(ex.dep),)
    assert np.all(np.isfinite(got)), f"{label}: {np.count_nonzero(~np.isfinite(got))} dependency sums are not finite"
    bound = 4 * ex.depth * (ex.max_row + 2) * U
    worst = Fraction(0)
    for v, (g, ref) in enumerate(zip(got.tolist(), ex.dep)):
        if ref == 0:
            assert g == 0.0, f"{label}: dependency of {v} is {g!r}, exactly 0"
        else:
            worst = max(worst, _rel(g, ref))
    print(f"exact-error {label} dependencies {float(worst):.3g} bound {float(bound):.3g}")
    assert worst <= bound, f"{label}: dependencies off by {float(worst):.3g} relative, bound {float(bound):.3g}"


def _label(rt, name, directed, extra=""):
    return f"{rt.backend.name.split()[0]} {name}{' directed' if directed else ''}{extra}"


def make_bfs(rt, name, directed, split=None):
    bfs = dbfs.BFS(host_csr(name, directed), rt, mode="td" if directed else "do", directed=directed)
    if split is not None:
        bfs.engine.set_option("bc_split_row", split)
    return bfs


def run_exact(rt, name, directed, split=None, bfs=None, srcs=None):
    """run_batch(betweenness, path_counts) of the case against the reference; -> (dep, counts)."""
    srcs = sources(name) if srcs is None else srcs
    ex = exact(name, directed, srcs)
    bfs = bfs or make_bfs(rt, name, directed, split)
    res = bfs.run_batch(srcs, betweenness=True, path_counts=True)
    assert max(res.depth) == ex.depth
    label = _label(rt, name, directed, "" if split is None else f" split {split}")
    dep, sig = bfs.batch_betweenness(), bfs.batch_path_counts()
    check_counts(label, sig, ex)
    check_dep(label, dep, ex)
    return res, dep, sig


def in_range_grid40(rt):
    """Counts up to C(78, 39) ~ 2^75 on 8-bit levels, a full pass of 64 lanes with different level sets."""
    res, _, sig = run_exact(rt, "grid40x40", False)
    assert len(sources("grid40x40")) == 64 and res.passes == 1 and not res.wide_levels
    assert sig.max() > 2.0 ** 70


def in_range_grid300(rt):
    """Counts up to ~2^101 on 16-bit levels."""
    res, _, sig = run_exact(rt, "grid20x300", False)
    assert res.wide_levels and sig.max() > 2.0 ** 90


def exact_top(rt, directed):
    """Doubled path: every operation is exact in binary, so every bit is the reference's."""
    name = "doubled1023"
    ex = exact(name, directed)
    _, dep, sig = run_exact(rt, name, directed)
    assert sig[0].tolist() == [2.0 ** k for k in range(1024)] and sig[0][1023] == 2.0 ** 1023
    assert dep.tolist() == [float(d) for d in ex.dep] and all(Fraction(float(d)) == d for d in ex.dep)
    # from source 0 alone: n - 1 - v (the source takes no share)
    bfs = make_bfs(rt, name, directed)
    bfs.run_batch([0], betweenness=True)
    want = np.arange(1023, -1, -1, dtype=np.float64)
    want[0] = 0.0
    assert np.array_equal(bfs.batch_betweenness(), want)


def rounded_top(rt, name):
    """Rounded counts up to 3^646 ~ 2^1023.9, where the deepest vertices'
    coefficients 1 / sigma are subnormal, and up to 210^130 ~ 2^1003."""
    ex = exact(name, False)
    assert max(ex.sigma[0]) > 2 ** 1000
    if name == "tripled646":
        assert Fraction(1, max(ex.sigma[0])) < Fraction(1, 2 ** 1022)
    run_exact(rt, name, False)


def long_rows(rt, name, directed, split):
    """Counts near 2^990 through rows of 80 / 140 entries (directed: 40 / 70),
    by the workgroup-per-row launch (split 16) and by one wave (0)."""
    ex = exact(name, directed)
    assert 2 ** 980 < max(ex.sigma[0]) < 2 ** 1024
    run_exact(rt, name, directed, split=split)


def deterministic(rt, name, split):
    bfs = make_bfs(rt, name, False, split)
    _, dep, sig = run_exact(rt, name, False, split=split, bfs=bfs)
    dep, sig = dep.copy(), sig.copy()
    bfs.run_batch(sources(name), betweenness=True, path_counts=True)
    assert np.array_equal(dep.view(np.uint64), bfs.batch_betweenness().view(np.uint64))
    assert np.array_equal(sig.view(np.uint64), bfs.batch_path_counts().view(np.uint64))


def virtual_ranks(name, directed, P, device):
    srcs, csr, ex = sources(name), host_csr(name, directed), exact(name, directed)

    def body(rt):
        bfs = dbfs.BFS(csr, rt, mode="td" if directed else "do", directed=directed)
        bfs.run_batch(srcs, betweenness=True, path_counts=True)
        return bfs.batch_betweenness(), bfs.batch_path_counts()

    for r, (dep, sig) in enumerate(run_virtual_ranks(P, body, device=device)):
        check_counts(f"{device} {name} rank {r}/{P}", sig, ex)
        check_dep(f"{device} {name} rank {r}/{P}", dep, ex)


def oracle_matches_exact(name, directed):
    """cpu_betweenness, which the other betweenness tests lean on, under the same bounds."""
    ex = exact(name, directed)
    dep, sig = dbfs.cpu_betweenness(host_csr(name, directed), sources(name), directed, True)
    label = f"oracle {name}{' directed' if directed else ''}"
    check_counts(label, sig, ex)
    check_dep(label, dep, ex)


# ---- the range contract ----------------------------------------------------------------

def _no_result(bfs, pytest):
    with pytest.raises(Exception, match="no batch has run with betweenness"):
        bfs.batch_betweenness()
    with pytest.raises(Exception, match="no batch has run with keep_path_counts"):
        bfs.batch_path_counts()


def overflow_raises(rt, pytest, name, directed):
    """One vertex past cases 3 and 4 (2^1024, 3^647): the call fails, names the
    source, leaves nothing, and the same BFS then runs an in-range set."""
    assert max(exact(name, directed).sigma[0]) > 2 ** 1024 - 2 ** 970  # (what DBL_MAX rounds down from)
    bfs = make_bfs(rt, name, directed)
    n = host_csr(name, directed).n
    for kw in ({"betweenness": True}, {"betweenness": True, "path_counts": True}, {"path_counts": True}):
        with pytest.raises(Exception, match=f"run_batch: the shortest-path counts from source 0 {OVERFLOW}"):
            bfs.run_batch([0], **kw)
        _no_result(bfs, pytest)
    run_exact(rt, name, directed, bfs=bfs, srcs=[n // 2, 1])


def oracle_overflow_raises(pytest, name, directed):
    csr = host_csr(name, directed)
    for counts in (False, True):
        with pytest.raises(Exception, match=f"cpu_betweenness: the shortest-path counts from source 0 {OVERFLOW}"):
            dbfs.cpu_betweenness(csr, [5, 0], directed, counts)


def middle_source_succeeds(rt):
    """From the middle of the 1025-vertex doubled path no count passes 2^512."""
    _, dep, sig = run_exact(rt, "doubled1024", False, srcs=[512])
    assert sig[0].tolist() == [2.0 ** abs(v - 512) for v in range(1025)]
    assert dep.tolist() == [float(d) for d in exact("doubled1024", False, [512]).dep]


def one_lane_overflows(rt, pytest):
    """A full pass in which only the source in slot 37 overflows."""
    srcs = list(range(1, 38)) + [0] + list(range(500, 526))
    assert len(srcs) == 64 and srcs[37] == 0
    bfs = make_bfs(rt, "doubled1024", False)
    with pytest.raises(Exception, match=f"from source 0 {OVERFLOW}"):
        bfs.run_batch(srcs, betweenness=True)
    _no_result(bfs, pytest)
    srcs[37] = 38
    run_exact(rt, "doubled1024", False, bfs=bfs, srcs=srcs)


def third_pass_overflows(rt, pytest):
    """130 sources, the overflowing one in the third pass: the two finished passes leave no result."""
    srcs = list(range(1, 129)) + [512, 1024]
    bfs = make_bfs(rt, "doubled1024", False)
    with pytest.raises(Exception, match=f"from source 1024 {OVERFLOW}"):
        bfs.run_batch(srcs, betweenness=True, path_counts=True)
    _no_result(bfs, pytest)


def long_row_overflows(rt, pytest):
    """7^362 ~ 2^1016 at the end of the path, x 40 in layer 1, x 40^2 > 2^1024 in
    layer 2: the first non-finite sum is a long row's (80 entries, bc_split_row
    16), and so is every later one."""
    name = "tail40x8_long"
    ex = exact(name, False)
    sig, first = ex.sigma[0], 363
    assert max(sig[:first + 80]) < 2 ** 1024 - 2 ** 970 < sig[first + 80]
    deg = np.diff(np.asarray(host_csr(name, False).row_off))
    assert deg[:first - 1].max() <= 16 and deg[first:].min() > 16  # (the path's last vertex: 7 + 40, still finite)
    bfs = make_bfs(rt, name, False, split=16)
    with pytest.raises(Exception, match=f"from source 0 {OVERFLOW}"):
        bfs.run_batch([0], betweenness=True)
    _no_result(bfs, pytest)
    run_exact(rt, name, False, bfs=bfs, srcs=[181])


def ranks_overflow(pytest, device):
    """Three ranks: the overflowing count is rank 2's, every rank raises, none waits in a collective."""
    csr = host_csr("doubled1024", False)

    def body(rt):
        bfs = dbfs.BFS(csr, rt)
        try:
            bfs.run_batch([0, 512], betweenness=True, path_counts=True)
        except Exception as e:  # noqa: BLE001 - the message is the result
            first = str(e)
        else:
            first = "no error"
        _no_result(bfs, pytest)
        bfs.run_batch([512], betweenness=True, path_counts=True)  # (the ranks are still in step)
        return first, bfs.batch_betweenness(), bfs.batch_path_counts()

    ex = exact("doubled1024", False, [512])
    for r, (first, dep, sig) in enumerate(run_virtual_ranks(3, body, device=device)):
        assert f"from source 0 {OVERFLOW}" in first, (r, first)
        check_counts(f"{device} doubled1024 after overflow rank {r}/3", sig, ex)
        check_dep(f"{device} doubled1024 after overflow rank {r}/3", dep, ex)


# ---- CLI -------------------------------------------------------------------------------

def cli_file(tmp_dir):
    """A doubled path of 2100 vertices: every source is 1024 edges or more from an end."""
    path = os.path.join(str(tmp_dir), "doubled_path2100.txt")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write("2100 4198\n" + "".join(f"{i} {i + 1}\n{i} {i + 1}\n" for i in range(2099)))
    return path


def cli_overflow(bfs_bin, tmp_dir, flags):
    """The error on stderr, a non-zero status, no result line and no --betweenness-out file."""
    dest = os.path.join(str(tmp_dir), "bc_overflow_out.txt")
    for extra in ([], ["--no-oracle"]):
        out = dc.run_cli(bfs_bin, ["0", cli_file(tmp_dir), "--roots", "3", "--batch", "--betweenness",
                                   "--betweenness-out", dest] + flags + extra)
        assert out.returncode == 1, out.stdout + out.stderr
        assert OVERFLOW in out.stderr and "shortest-path counts from source" in out.stderr, out.stderr[-2000:]
        assert "batch betweenness" not in out.stdout and "nan" not in out.stdout.lower(), out.stdout
        assert not os.path.exists(dest)
