"""Cases and checks shared by test_betweenness_wide.py (CPU backend and the
oracle cpu_betweenness) and test_betweenness_wide_gpu.py (the wide forms of
ms_bc_kernels.hip): extended-range path counts -- a mantissa and an exponent
per vertex and source (csrc/include/dbfs/wide.hpp) -- past 2^1024, against the
exact reference of betweenness_exact_cases (Python integers and Fractions).

Contract.  With u = 2^-53, r the longest walked row, depth as in that file and
k sources:
  counts        Fraction(mant) * 2**exp within relative error 1.01 depth (r - 1) u
                of the exact integer, equal where that is below 2^53; mant in
                [0.5, 1), or (0.0, 0) for a zero count.  The bound is the double
                path's: the wide add aligns by an exact power of two and rounds
                once, as a double add does.
  dependencies  |got - exact| <= 4 depth (r + 2) u exact + k 2^-1074: the double
                path's bound, and one new term -- delta = sigma * acc leaves the
                wide form as a double, so one source's share below double's
                smallest subnormal counts as 0.  An exact 0 is 0.0, every value
                is finite.
  same bits     where all counts fit a double and no coefficient is subnormal,
                wide and double results are the same bits, and so are two runs.
Errors are computed exactly, in integers; the largest one of every check is
printed (`wide-error ...`)."""
import math
import os
from fractions import Fraction

import numpy as np

import distributed_cuda_bfs_amd as dbfs
from distributed_cuda_bfs_amd.parallel.runtime import run_virtual_ranks

import betweenness_exact_cases as bx
import directed_cases as dc

U = bx.U
TINY = Fraction(1, 2 ** 1074)
NAMES_WIDE = "batch_path_counts_wide"


# ---- graphs ------------------------------------------------------------------------

CHAIN = 1500


def two_chains(directed=False):
    """Vertex 0 joined to t by two chains of CHAIN hops, one of doubled edges
    (vertices 1 .. CHAIN - 1) and one of single edges (CHAIN .. 2 CHAIN - 2),
    then a tail of 3 vertices behind t = 2 CHAIN - 1: sigma_0(t) = 2^CHAIN + 1."""
    t = 2 * CHAIN - 1
    a = [0] + list(range(1, CHAIN)) + [t]
    b = [0] + list(range(CHAIN, 2 * CHAIN - 1)) + [t]
    u, v = [], []
    for x, y in zip(a[:-1], a[1:]):
        u += [x, x]
        v += [y, y]
    for x, y in zip(b[:-1], b[1:]):
        u.append(x)
        v.append(y)
    for x in range(t, t + 3):
        u.append(x)
        v.append(x + 1)
    return bx._csr(t + 4, u, v, directed)


TWO_CHAINS_T = 2 * CHAIN - 1
TWO_CHAINS_N = TWO_CHAINS_T + 4


def _ends(n):
    return [0, n // 2, n - 1]


# name -> (builder(directed), sources)
GRAPHS = {
    # past the limit: 2^3000, 3^2000 ~ 2^3170, 210^600 ~ 2^4629 on 16-bit levels ...
    "doubled3000": (lambda d: bx.multi_path([2] * 3000, d), _ends(3001)),
    "tripled2000": (lambda d: bx.multi_path([3] * 2000, d), _ends(2001)),
    "mult2357x600": (lambda d: bx.multi_path([2, 3, 5, 7] * 600, d), _ends(2401)),
    # ... and 20^250 ~ 2^1080 within the 255 levels a one-byte matrix holds
    "x20_250": (lambda d: bx.multi_path([20] * 250, d), _ends(251)),
    "two_chains": (two_chains, [0, TWO_CHAINS_N - 1, 750]),
    # 7^800 ~ 2^2246 into rows of 80 / 140 entries (directed: 40 / 70)
    "tail40x8w": (lambda d: bx.thick_tail(7, 800, 40, 8, d), _ends(801 + 320)),
    "tail70x6w": (lambda d: bx.thick_tail(7, 800, 70, 6, d), _ends(801 + 420)),
}
PAST = [(g, d) for g in ("doubled3000", "tripled2000", "mult2357x600", "x20_250") for d in (False, True)]
LONG_ROWS = [(g, d) for g in ("tail40x8w", "tail70x6w") for d in (False, True)]
ORACLE_CASES = PAST + [("two_chains", False)] + LONG_ROWS
SAME_BITS = ["grid40x40", "grid20x300", "tail40x8"]  # (of betweenness_exact_cases: every count fits a double)
SPREAD64 = [round(i * 2000 / 63) for i in range(64)]  # tripled2000's full pass
AUTO_SOURCES = list(range(1, 129)) + [512, 1024]      # doubled1024: the third pass overflows

_csr_cache = {}
_exact_cache = {}


def host_csr(name, directed):
    if name in bx.GRAPHS:
        return bx.host_csr(name, directed)
    key = (name, directed)
    if key not in _csr_cache:
        _csr_cache[key] = GRAPHS[name][0](directed)
    return _csr_cache[key]


def sources(name):
    return bx.sources(name) if name in bx.GRAPHS else list(GRAPHS[name][1])


def exact(name, directed, srcs=None):
    """The reference of a case, computed once per run and never written to."""
    if name in bx.GRAPHS:
        return bx.exact(name, directed, srcs)
    srcs = sources(name) if srcs is None else list(srcs)
    key = (name, directed, tuple(srcs))
    if key not in _exact_cache:
        _exact_cache[key] = bx.exact_brandes(host_csr(name, directed), srcs, directed)
    return _exact_cache[key]


# ---- the comparison --------------------------------------------------------------------

def check_form(label, mant, exp, shape):
    """frexp's convention: mant in [0.5, 1), or (0.0, 0)."""
    mant, exp = np.asarray(mant), np.asarray(exp)
    assert mant.dtype == np.float64 and exp.dtype == np.int32 and mant.shape == exp.shape == shape, label
    zero = mant == 0.0
    assert np.all(exp[zero] == 0), f"{label}: a zero count with an exponent"
    assert np.all((mant[~zero] >= 0.5) & (mant[~zero] < 1.0)), f"{label}: a mantissa outside [0.5, 1)"


def check_counts_wide(label, mant, exp, ex):
    check_form(label, mant, exp, (len(ex.sigma), len(ex.dep)))
    bound = Fraction(101, 100) * ex.depth * (ex.max_row - 1) * U
    worst = Fraction(0)
    for i, ref in enumerate(ex.sigma):
        # mant * 2^exp = m53 * 2^(exp - 53) with m53 an integer: compared in integers
        m53 = np.ldexp(np.asarray(mant[i]), 53).astype(np.int64).tolist()
        sh = (np.asarray(exp[i], dtype=np.int64) - 53).tolist()
        for v, s in enumerate(ref):
            got_num, ref_num = (m53[v] << sh[v], s) if sh[v] >= 0 else (m53[v], s << -sh[v])
            if s < 2 ** 53:
                assert got_num == ref_num, f"{label}: count [{i}][{v}] is {mant[i][v]!r} * 2^{exp[i][v]}, exactly {s}"
            elif got_num != ref_num:
                worst = max(worst, Fraction(abs(got_num - ref_num), ref_num))
    print(f"wide-error {label} counts {float(worst):.3g} bound {float(bound):.3g}")
    assert worst <= bound, f"{label}: counts off by {float(worst):.3g} relative, bound {float(bound):.3g}"


def check_dep_wide(label, got, ex, k):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == (len(ex.dep),)
    assert np.all(np.isfinite(got)), f"{label}: {np.count_nonzero(~np.isfinite(got))} dependency sums are not finite"
    bound = 4 * ex.depth * (ex.max_row + 2) * U
    worst, flushed = Fraction(0), 0
    for v, (g, ref) in enumerate(zip(got.tolist(), ex.dep)):
        if ref == 0:
            assert g == 0.0, f"{label}: dependency of {v} is {g!r}, exactly 0"
            continue
        err = abs(Fraction(g) - ref)
        assert err <= bound * ref + k * TINY, \
            f"{label}: dependency of {v} is {g!r}, off by {float(err / ref):.3g} relative, bound {float(bound):.3g}"
        if err > bound * ref:
            flushed += 1
        else:
            worst = max(worst, err / ref)
    print(f"wide-error {label} dependencies {float(worst):.3g} bound {float(bound):.3g} "
          f"(+ {flushed} within {k} * 2^-1074)")


def _label(rt, name, directed, extra=""):
    return f"{rt.backend.name.split()[0]} {name}{' directed' if directed else ''}{extra}"


def make_bfs(rt, name, directed, split=None):
    bfs = dbfs.BFS(host_csr(name, directed), rt, mode="td" if directed else "do", directed=directed)
    if split is not None:
        bfs.engine.set_option("bc_split_row", split)
    return bfs


def run_wide(rt, name, directed, split=None, bfs=None, srcs=None, wide=True):
    """run_batch(betweenness, path_counts, wide_counts) of the case against the
    reference; -> (res, dep, mant, exp)."""
    srcs = sources(name) if srcs is None else srcs
    ex = exact(name, directed, srcs)
    bfs = bfs or make_bfs(rt, name, directed, split)
    res = bfs.run_batch(srcs, betweenness=True, path_counts=True, wide_counts=wide)
    assert max(res.depth) == ex.depth
    if wide is True:
        assert res.wide_count_passes == res.passes
    label = _label(rt, name, directed, ("" if split is None else f" split {split}") + f" wide={wide}")
    dep = bfs.batch_betweenness()
    mant, exp = bfs.batch_path_counts_wide()
    check_counts_wide(label, mant, exp, ex)
    check_dep_wide(label, dep, ex, len(srcs))
    return res, dep, mant, exp


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the cases -------------------------------------------------------------------------

def past_the_limit(rt, name, directed):
    """Case 1: counts past 2^1024 on 16-bit levels, and (x20_250) on one-byte ones."""
    ex = exact(name, directed)
    assert max(ex.sigma[0]) > 2 ** 1024
    res, dep, mant, exp = run_wide(rt, name, directed)
    assert res.wide_levels == (name != "x20_250")
    if name != "doubled3000":
        return
    # every operation is exact in binary: every bit is the reference's
    n = len(ex.dep)
    assert np.array_equal(mant[0], np.full(n, 0.5)) and exp[0].tolist() == list(range(1, n + 1))
    for i, ref in enumerate(ex.sigma):
        assert [Fraction(m) * Fraction(2) ** e for m, e in zip(mant[i].tolist(), exp[i].tolist())] == ref
    assert dep.tolist() == [float(d) for d in ex.dep] and all(Fraction(float(d)) == d for d in ex.dep)
    # from source 0 alone: n - 1 - v (the source takes no share)
    bfs = make_bfs(rt, name, directed)
    bfs.run_batch([0], betweenness=True, wide_counts=True)
    want = np.arange(n - 1, -1, -1, dtype=np.float64)
    want[0] = 0.0
    assert np.array_equal(bfs.batch_betweenness(), want)


def alignment_and_underflow(rt):
    """Case 2: 2^1500 + 1 rounds to 2^1500 (the 1 is aligned, not dropped early
    or added twice), and a dependency of 4 / (2^1500 + 1) is below every double."""
    name = "two_chains"
    ex = exact(name, False)
    t, last_single = TWO_CHAINS_T, TWO_CHAINS_T - 1
    assert ex.sigma[0][t] == 2 ** CHAIN + 1
    ex0 = exact(name, False, [0])
    assert ex0.dep[last_single] == Fraction(4, 2 ** CHAIN + 1) < TINY
    _, _, mant, exp = run_wide(rt, name, False)
    assert (mant[0][t], exp[0][t]) == (0.5, CHAIN + 1)
    _, dep, _, _ = run_wide(rt, name, False, srcs=[0])
    assert dep[last_single] in (0.0, 2.0 ** -1074)


def long_rows(rt, name, directed, split):
    """Case 3: 7^800 ~ 2^2246 through rows of 80 / 140 entries (directed: 40 /
    70), by the workgroup-per-row launch (split 16: two and three waves, the
    partial sums wide in LDS) and by one wave (0)."""
    assert max(exact(name, directed).sigma[0]) > 2 ** 2246
    run_wide(rt, name, directed, split=split)


def deterministic(rt, name, split):
    bfs = make_bfs(rt, name, False, split)
    _, dep, mant, exp = run_wide(rt, name, False, split=split, bfs=bfs)
    dep, mant, exp = dep.copy(), mant.copy(), exp.copy()
    bfs.run_batch(sources(name), betweenness=True, path_counts=True, wide_counts=True)
    m2, e2 = bfs.batch_path_counts_wide()
    assert np.array_equal(_bits(dep), _bits(bfs.batch_betweenness()))
    assert np.array_equal(_bits(mant), _bits(m2)) and np.array_equal(exp, e2)


def full_pass(rt):
    """Case 4: one pass of 64 lanes on different levels.  A vertex's 64 counts
    lie on both sides of 2^1024 (the lanes of near sources are in a double's
    range there, those of far ones are not); every lane passes it somewhere,
    the middle source's last of all (3^1000 ~ 2^1585)."""
    res, _, mant, exp = run_wide(rt, "tripled2000", False, srcs=SPREAD64)
    assert res.passes == 1 and len(SPREAD64) == len(set(SPREAD64)) == 64
    top = exp.max(axis=1)
    assert top.min() > 1585 and top.max() > 3169 and len(set(top.tolist())) > 16
    assert ((exp > 1024).any(axis=0) & ((exp < 1024) & (mant > 0)).any(axis=0)).all()


def same_bits(rt, name):
    """Case 5: wide against double where every count fits a double."""
    srcs = sources(name)
    bfs = make_bfs(rt, name, False, split=16 if name.startswith("tail") else None)
    bfs.run_batch(srcs, betweenness=True, path_counts=True)
    dep, sig = bfs.batch_betweenness().copy(), bfs.batch_path_counts().copy()
    assert sig.max() < 2.0 ** 1022  # (no coefficient (1 + delta) / sigma is subnormal)
    # (a double batch's counts in the wide form: frexp on the host)
    m0, e0 = bfs.batch_path_counts_wide()
    check_form(name, m0, e0, sig.shape)
    assert np.array_equal(_bits(np.ldexp(m0, e0)), _bits(sig))
    res = bfs.run_batch(srcs, betweenness=True, path_counts=True, wide_counts=True)
    assert res.wide_count_passes == res.passes
    mant, exp = bfs.batch_path_counts_wide()
    check_form(name, mant, exp, sig.shape)
    assert np.array_equal(_bits(np.ldexp(mant, exp)), _bits(sig))
    assert np.array_equal(_bits(bfs.batch_betweenness()), _bits(dep))
    assert np.array_equal(_bits(bfs.batch_path_counts()), _bits(sig))  # (case 7: every count fits)


def auto_redoes_one_pass(rt, pytest):
    """Case 6: of three passes only the third overflows."""
    name = "doubled1024"
    bfs = make_bfs(rt, name, False)
    with pytest.raises(Exception, match=f"from source 1024 {bx.OVERFLOW}"):
        bfs.run_batch(AUTO_SOURCES, betweenness=True, path_counts=True, wide_counts=False)
    res, _, mant, exp = run_wide(rt, name, False, bfs=bfs, srcs=AUTO_SOURCES, wide="auto")
    assert res.passes == 3 and res.wide_count_passes == 1
    bfs.run_batch(AUTO_SOURCES[:128], betweenness=True, path_counts=True)
    sig = bfs.batch_path_counts()
    assert np.array_equal(_bits(np.ldexp(mant[:128], exp[:128])), _bits(sig))


def auto_stays_double(rt):
    name = "grid40x40"
    srcs = sources(name)
    bfs = make_bfs(rt, name, False)
    bfs.run_batch(srcs, betweenness=True, path_counts=True)
    dep, sig = bfs.batch_betweenness().copy(), bfs.batch_path_counts().copy()
    res = bfs.run_batch(srcs, betweenness=True, path_counts=True, wide_counts="auto")
    assert res.wide_count_passes == 0
    mant, exp = bfs.batch_path_counts_wide()
    check_form(name, mant, exp, sig.shape)
    assert np.array_equal(_bits(np.ldexp(mant, exp)), _bits(sig))
    assert np.array_equal(_bits(bfs.batch_path_counts()), _bits(sig))
    assert np.array_equal(_bits(bfs.batch_betweenness()), _bits(dep))


def counts_as_doubles_after_wide(rt, pytest):
    """Case 7: batch_path_counts() after a wide batch raises, naming the wide
    reader, when a count exceeds a double -- and returns the doubles otherwise."""
    bfs = make_bfs(rt, "doubled1024", False)
    for wide in (True, "auto"):
        bfs.run_batch([0], betweenness=True, path_counts=True, wide_counts=wide)
        with pytest.raises(Exception, match=NAMES_WIDE):
            bfs.batch_path_counts()
        assert np.all(np.isfinite(bfs.batch_betweenness()))
        bfs.run_batch([512], path_counts=True, wide_counts=wide)
        assert bfs.batch_path_counts()[0].tolist() == [2.0 ** abs(v - 512) for v in range(1025)]
    for bad in ("yes", 1, 0, None, np.array([True, False])):
        with pytest.raises(ValueError, match="wide_counts"):
            bfs.run_batch([0], betweenness=True, wide_counts=bad)


def oracle_matches_exact(name, directed):
    """Case 8: cpu_betweenness(wide_counts=True) under the same bounds."""
    ex, srcs = exact(name, directed), sources(name)
    dep, (mant, exp) = dbfs.cpu_betweenness(host_csr(name, directed), srcs, directed, True, True)
    label = f"oracle {name}{' directed' if directed else ''}"
    check_counts_wide(label, mant, exp, ex)
    check_dep_wide(label, dep, ex, len(srcs))
    dep2, none = dbfs.cpu_betweenness(host_csr(name, directed), srcs, directed, wide_counts=True)
    assert none is None and np.array_equal(_bits(dep), _bits(dep2))


def virtual_ranks(name, directed, P, device, split=None):
    """Case 9: three ranks, the value records all-gathered after every launch."""
    srcs, csr, ex = sources(name), host_csr(name, directed), exact(name, directed)

    def body(rt):
        bfs = dbfs.BFS(csr, rt, mode="td" if directed else "do", directed=directed)
        if split is not None:
            bfs.engine.set_option("bc_split_row", split)
        res = bfs.run_batch(srcs, betweenness=True, path_counts=True, wide_counts=True)
        return res.wide_count_passes, bfs.batch_betweenness(), bfs.batch_path_counts_wide()

    for r, (wp, dep, (mant, exp)) in enumerate(run_virtual_ranks(P, body, device=device)):
        assert wp == 1
        check_counts_wide(f"{device} {name} rank {r}/{P}", mant, exp, ex)
        check_dep_wide(f"{device} {name} rank {r}/{P}", dep, ex, len(srcs))


def ranks_auto(device):
    """Three ranks, "auto": the overflowing count (2^1024 at vertex 1024) is
    rank 2's, every rank redoes the pass, and a second batch finds them in step."""
    name = "doubled1024"
    csr = host_csr(name, False)
    first, second = [0, 512], [512]

    def body(rt):
        bfs = dbfs.BFS(csr, rt)
        res = bfs.run_batch(first, betweenness=True, path_counts=True, wide_counts="auto")
        a = (res.wide_count_passes, bfs.batch_betweenness(), bfs.batch_path_counts_wide())
        res = bfs.run_batch(second, betweenness=True, path_counts=True, wide_counts="auto")
        return a, (res.wide_count_passes, bfs.batch_betweenness(), bfs.batch_path_counts())

    ex1, ex2 = exact(name, False, first), exact(name, False, second)
    for r, ((wp, dep, (mant, exp)), (wp2, dep2, sig2)) in enumerate(run_virtual_ranks(3, body, device=device)):
        assert (wp, wp2) == (1, 0), (r, wp, wp2)
        assert (mant[0][1024], exp[0][1024]) == (0.5, 1025)
        check_counts_wide(f"{device} auto rank {r}/3", mant, exp, ex1)
        check_dep_wide(f"{device} auto rank {r}/3", dep, ex1, 2)
        bx.check_counts(f"{device} after auto rank {r}/3", sig2, ex2)
        bx.check_dep(f"{device} after auto rank {r}/3", dep2, ex2)


# ---- CLI -------------------------------------------------------------------------------

def cli_wide(bfs_bin, tmp_dir, flags, form):
    """Case 10: the 2100-vertex doubled path, which fails with doubles, passes
    its oracle comparison with wide and auto counts."""
    dest = os.path.join(str(tmp_dir), f"bc_{form}_out.txt")
    if os.path.exists(dest):
        os.remove(dest)
    out = dc.run_cli(bfs_bin, ["0", bx.cli_file(tmp_dir), "--roots", "3", "--batch", "--betweenness", "--json",
                               "--betweenness-counts", form, "--betweenness-out", dest] + flags)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Betweenness OK!" in out.stdout and "Wrong output!" not in out.stdout, out.stdout
    lines = out.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("batch betweenness sources 3 bc_ms ")]
    assert len(at) == 1 and lines[at[0] + 1] == "batch betweenness wide passes 1 of 1", out.stdout
    assert '"wide_count_passes":1' in out.stdout
    with open(dest) as f:
        vals = [float(x) for x in f.read().split()]
    assert len(vals) == 2100 and all(math.isfinite(x) and x >= 0.0 for x in vals) and max(vals) > 0.0


def cli_double_unchanged(bfs_bin, tmp_dir, flags):
    """--betweenness-counts double is the default: the existing failure."""
    bx.cli_overflow(bfs_bin, tmp_dir, flags + ["--betweenness-counts", "double"])


def cli_usage(bfs_bin, tmp_dir, flags):
    for args, msg in ((["--roots", "3", "--batch", "--betweenness-counts", "wide"],
                       "--betweenness-counts needs --betweenness"),
                      (["--roots", "3", "--batch", "--betweenness", "--betweenness-counts", "triple"],
                       "--betweenness-counts must be double, wide or auto")):
        out = dc.run_cli(bfs_bin, ["0", bx.cli_file(tmp_dir)] + args + flags)
        assert out.returncode == 2 and msg in out.stderr, out.stdout + out.stderr
        assert "batch roots" not in out.stdout


# ---- the road grid (GPU only) ------------------------------------------------------------

GRID = 1056


def road_grid(rt):
    """Case 11: the smallest square grid on which a corner source overflows a
    double with a margin: C(2110, 1055) ~ 2^2105.  Labels are row-major, so
    from the corner the count at offset (dx, dy) is C(dx + dy, dx)."""
    n = GRID * GRID
    bfs = dbfs.BFS(dbfs.grid_params(GRID, GRID), rt)
    centre = (GRID // 2) * GRID + GRID // 2
    depth, r = 2 * GRID - 1, 4
    count_bound = Fraction(101, 100) * depth * (r - 1) * U
    for src in (0, centre):
        res = bfs.run_batch([src], betweenness=True, path_counts=src == 0, wide_counts=True)
        assert res.wide_count_passes == 1 and res.reached[0] == n and res.wide_levels
        assert res.depth[0] == (depth if src == 0 else GRID + 1)
        dep_bound = 4 * res.depth[0] * (r + 2) * U + n * U
        dep = bfs.batch_betweenness()
        assert dep.shape == (n,) and np.all(np.isfinite(dep))
        # the pair dependencies of one source sum to d(s, t) - 1 per target
        total, want = Fraction(math.fsum(dep.tolist())), res.dist_sum[0] - (res.reached[0] - 1)
        print(f"wide-error grid{GRID} source {src} dependency total {float(abs(total - want) / want):.3g} "
              f"bound {float(dep_bound):.3g}")
        assert abs(total - want) <= dep_bound * want
        if src != 0:
            continue
        mant, exp = bfs.batch_path_counts_wide()
        check_form("grid", mant, exp, (1, n))
        assert exp.max() > 2100
        worst = Fraction(0)
        cells = [(i, i) for i in range(GRID)] + [(i, GRID - 1) for i in range(GRID)] + [(GRID - 1, i) for i in range(GRID)]
        for dx, dy in cells:
            v, ref = dy * GRID + dx, math.comb(dx + dy, dx)
            got = Fraction(float(mant[0][v])) * Fraction(2) ** int(exp[0][v])
            if ref < 2 ** 53:
                assert got == ref, (dx, dy)
            worst = max(worst, abs(got - ref) / ref)
        print(f"wide-error grid{GRID} corner counts {float(worst):.3g} bound {float(count_bound):.3g}")
        assert worst <= count_bound
