"""The device-checked kernels over every form the engine can be forced into.

tests/test_checked_build.py runs bin/bfs_checked at its defaults; the forms
that tests/test_gpu_shard_sizes.py and tests/test_gpu_engine.py force by
option run through the Python extension, which is never a checked build.  An
out-of-range read that happens to give the right levels is invisible to
those oracle comparisons; here every form runs with its DBFS_DCHECK sites
compiled, through the CLI's --opt:

    bin/bfs_checked <graph> <src> --roots 1 --validate --json [--mode M] [--opt name=value ...]

Every run must exit 0 (a recorded violation fails it, naming code and file),
print `Output OK!` (the levels from <src>, element-wise against the
sequential oracle) and `Validation OK`, call its backend `...+checked`, and
show the forced form in the "chains" of its JSON lines (the run from <src>,
the maximum-degree vertex, and the run from the root --roots 1 samples).
Everything is an integer: no tolerance.

Graphs, the smallest at which a form still has work (the options force the
forms, so no size threshold needs crossing):
  rmat16     --rmat 16: hubs, rows of thousands of entries, every top-down and
             bottom-up form.  Every case below that forces a form shows its
             letter at this scale; none needed 17 or 18 (direction-optimising
             runs with the binned options alone: see TD_FORMS).
  uniform    --uniform 266317:800000: 65 units of 4096 vertices plus 77, so a
             partial last word and unit.  One scan chunk: SCAN_CHUNK is 1024
             units (asserted below), so several chunks would take 4 M
             vertices, which test_gpu_shard_sizes.py's graphs A-C cover.
The option sets and the evidence are those of TD_FORMS, test_split_levels,
test_forced_unvisited_filter, test_sparse_level_from_bitmap,
test_bottom_up_forms, test_bottom_up_lane_limit_1, test_hub_cut and
test_host_loop (test_gpu_shard_sizes.py) and of test_binned_top_down_gpu,
test_td_hub_filter_gpu, test_sparse_top_down_levels_gpu and
test_td_direct_levels_gpu (test_gpu_engine.py).  "chains" has no field for
the hub filter, the direct level bytes or the bottom-up words per wave: those
cases assert that a chain of the kind the option acts on ran.

Batch kernels (ms_kernels.hip, codes 20-26): 70 roots in two passes, every
--batch-direction, undirected RMAT-14 and the directed list of
directed_cases.cli_file, 1 and 3 virtual ranks (the push form runs on one
rank only: run_batch refuses it on several).  In-edge routing
(graph_kernels.hip, codes 40-43): the directed list on 1, 3 and 8 ranks,
unsorted, and a list whose vertex count is no multiple of the rank count (a
short last slice).

Wall time of the module on an MI355X, within a run of the whole suite: 53 s
for its 133 cases, 0.28 to 0.57 s each (the slowest:
test_in_edge_routing_short_last_slice); the yardstick
test_checked_build.py::test_checked_build_clean[1-do] took 0.37 s in the same
run, so no case is near three times that."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import directed_cases as dc
import distributed_cuda_bfs_amd as dbfs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED_BIN = os.path.join(REPO, "bin", "bfs_checked")
N = dbfs.native
BIG = float(1 << 40)

GRAPHS = {
    "rmat16": (["--rmat", "16"], lambda: dbfs.rmat_params(16, 16, 1)),
    "uniform": (["--uniform", "266317:800000"], lambda: dbfs.uniform_params(266317, 800000, 1)),
}


@functools.lru_cache(maxsize=None)
def hub_root(graph):
    """The maximum-degree vertex of the graph the CLI generates (--seed 1)."""
    csr = dbfs.host_csr_from_params(GRAPHS[graph][1]())
    return int(np.argmax(np.diff(np.asarray(csr.row_off))))


def run_checked(args, timeout=120):
    assert os.path.exists(CHECKED_BIN), "bin/bfs_checked missing: run `make checked` (make all builds it)"
    out = subprocess.run([CHECKED_BIN] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (args, out.stdout[-2000:], out.stderr[-4000:])
    assert "Wrong output!" not in out.stdout and "Validation FAILED" not in out.stdout, out.stdout[-2000:]
    return out


def run_form(graph, mode, options, extra=()):
    """One checked run: the hub root validated and compared with the oracle,
    a sampled root after it.  Returns the form letters of both runs' chains
    ('TTSB...|TS...') and the chains themselves."""
    args = GRAPHS[graph][0] + [str(hub_root(graph)), "--roots", "1", "--validate", "--json", "--mode", mode]
    for k, v in options.items():
        args += ["--opt", "%s=%r" % (k, v)]
    out = run_checked(args + list(extra))
    assert "Output OK!" in out.stdout and "Validation OK" in out.stdout, out.stdout[-2000:]
    runs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{") and '"source"' in l]
    assert len(runs) == 2 and runs[0]["source"] == hub_root(graph), out.stdout[-2000:]
    assert all(r["backend"].endswith("+checked") for r in runs), [r["backend"] for r in runs]
    assert all(r["reached"] > 1 and r["depth"] > 1 for r in runs)
    chains = [c for r in runs for c in r["chains"]]
    return "|".join("".join(c["form"] for c in r["chains"]) for r in runs), chains


def test_graph_geometry():
    """What the uniform graph is there for: a partial last word and unit, one scan chunk."""
    n = 266317
    assert n == 65 * N.UNIT_VERTICES + 77 and n % 64 != 0
    assert N.SCAN_CHUNK == 1024 and -(-n // N.UNIT_VERTICES) <= N.SCAN_CHUNK
    assert hub_root("rmat16") != hub_root("uniform")


# ---- defaults, device loop and host loop ------------------------------------------------

@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("mode", ["td", "bu", "do"])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_defaults_device_loop(graph, mode, narrow):
    forms, _ = run_form(graph, mode, {"narrow_levels": narrow})
    assert forms.strip("|"), forms
    if mode == "bu":
        assert set(forms) <= set("B|"), forms
    if mode == "td":
        assert "B" not in forms, forms


@pytest.mark.parametrize("mode", ["td", "do"])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_host_loop(graph, mode):
    """scan_units with its finish and a compaction on every level; no chain."""
    forms, chains = run_form(graph, mode, {"device_loop": 0})
    assert chains == [] and forms == "|"


# ---- top-down forms ----------------------------------------------------------------------

TD_FORMS = {
    "dense": {"td_sparse_edges": 0},  # every level dense and compacted
    "bytes_default": {},
    "bytes_all": {"td_byte_edges": 0},
    "direct_all": {"td_direct_edges": 0},
    "direct_some": {"td_direct_edges": 1 << 16},
    "direct_never": {"td_direct_edges": BIG},
    # Binned levels: every non-sparse top-down level before the first bottom-up
    # one (1), those of >= 2^20 frontier edges only (2^20), none (0).  These
    # two run in mode td alone: a direction-optimising run at the default
    # td_sparse_edges goes from its sparse levels straight to bottom-up ones
    # (chains SSBBBSS at RMAT-16, 17 and 18, SSSSSBBBBBSS on the uniform graph,
    # on the MI355X as on the CPU backend; at RMAT-18 one sampled root in four
    # shows one X), and every level of >= 2^20 frontier edges is a bottom-up
    # one there, so neither option set forces a binned level in mode do.
    "binned": {"td_bin_edges": 1, "td_bin_min_rows": 0},
    "binned_large": {"td_bin_edges": 1 << 20, "td_bin_min_rows": 0},
    # ... with every level dense, mode do has a dense level before its first
    # bottom-up one on both graphs (chains TXBBBTT): binned in both modes
    "binned_dense": {"td_bin_edges": 1, "td_bin_min_rows": 0, "td_sparse_edges": 0},
    "binned_never": {"td_bin_edges": 0, "td_bin_min_rows": 0},
}
TD_ONLY = ("binned", "binned_large")


@pytest.mark.parametrize("mode,form", [(m, f) for f in TD_FORMS for m in ("td", "do") if m == "td" or f not in TD_ONLY])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_top_down_forms(graph, mode, form):
    forms, _ = run_form(graph, mode, TD_FORMS[form])
    if form == "dense":
        assert "S" not in forms and "T" in forms, forms
    elif form in ("binned", "binned_large"):
        assert "X" in forms and "S" in forms, forms
    elif form == "binned_dense":
        assert "X" in forms and "S" not in forms, forms
    elif form == "binned_never":
        assert "X" not in forms, forms
    if mode == "td":
        assert "T" in forms, forms  # (a dense level, which the byte / direct options act on)


@pytest.mark.parametrize("sparse_edges", [64, 1 << 16, 1 << 40])
@pytest.mark.parametrize("mode", ["td", "do"])
def test_sparse_top_down_levels(mode, sparse_edges):
    """(0, every level dense: TD_FORMS' `dense`.)"""
    forms, _ = run_form("rmat16", mode, {"td_sparse_edges": float(sparse_edges)})
    assert "S" in forms, forms
    if sparse_edges == 1 << 40 and mode == "td":
        assert set(forms) <= set("S|"), forms


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_forced_unvisited_filter(graph, narrow):
    _, chains = run_form(graph, "td", {"td_unvis_edges": 1, "td_unvis_vis_frac": 0.0, "td_unvis_max_density": 1.0,
                                       "narrow_levels": narrow})
    assert any(c["unvis"] for c in chains), chains


@pytest.mark.parametrize("bits", [1, 0])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_sparse_level_from_bitmap(graph, bits):
    """The sparse level after a bottom-up one: from the output bitmap or from a compacted list."""
    forms, _ = run_form(graph, "do", {"td_sparse_bits": bits})
    assert "BS" in forms, forms


@pytest.mark.parametrize("bitmap", [False, True])
@pytest.mark.parametrize("mode", ["td", "do"])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_split_levels(graph, mode, bitmap):
    """Every direct top-down level split in 4 parts (below 2^25 vertices never 8)."""
    opts = {"td_split_edges": 1, "td_split_parts": 4, "td_sparse_edges": 0}
    opts.update({"td_direct_edges": BIG} if bitmap else {"td_byte_edges": 0})
    _, chains = run_form(graph, mode, opts)
    parts = [c["split"] for c in chains]
    assert max(parts) <= 4 and 4 in parts, parts


@pytest.mark.parametrize("vis_frac", [0.0, 0.75])
@pytest.mark.parametrize("mode", ["td", "do"])
def test_td_hub_filter(mode, vis_frac):
    """Hub filter on every dense level (hubs' visited bits in LDS, hub-encoded td_col)."""
    forms, _ = run_form("rmat16", mode, {"td_hub_edges": 1, "td_hub_vis_frac": vis_frac, "td_direct_edges": 1})
    assert "T" in forms, forms


@pytest.mark.parametrize("mode", ["td", "do"])
def test_td_hub_filter_bitmap_levels(mode):
    forms, _ = run_form("rmat16", mode, {"td_hub_edges": 1, "td_direct_edges": BIG, "td_sparse_edges": 0})
    assert "T" in forms and "S" not in forms, forms


# ---- bottom-up forms -----------------------------------------------------------------------

@pytest.mark.parametrize("whole,small", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
@pytest.mark.parametrize("mode", ["bu", "do"])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_bottom_up_forms(graph, mode, whole, small):
    """Whole units per wave forced and forbidden, 4 words per wave on first levels forced and forbidden."""
    forms, _ = run_form(graph, mode, {"bu_whole_units": whole, "bu_small_waves": small})
    assert "B" in forms, forms


@pytest.mark.parametrize("mode", ["bu", "do"])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_bottom_up_lane_limit_1(graph, mode):
    forms, _ = run_form(graph, mode, {"bu_lane_limit": 1})
    assert "B" in forms, forms


@pytest.mark.parametrize("narrow", [1, 0])
@pytest.mark.parametrize("cut", [1 << 40, 0])
@pytest.mark.parametrize("mode", ["bu", "do"])
def test_hub_cut(mode, cut, narrow):
    """The hub-cut first bottom-up level on, whatever its frontier's edges, and off."""
    forms, chains = run_form("rmat16", mode, {"bu_cut_edges": float(cut), "narrow_levels": narrow})
    cuts = [c["cut"] for c in chains]
    assert "B" in forms, forms
    if cut == 0:
        assert not any(cuts)
    elif mode == "bu":  # (level 0 is a first bottom-up level of a few frontier edges)
        assert any(cuts), chains


# ---- several ranks: owner lists ------------------------------------------------------------

@pytest.mark.parametrize("lists", [True, False])
@pytest.mark.parametrize("mode", ["td", "do"])
def test_owner_lists_three_ranks(mode, lists):
    """3 virtual ranks: sparse chains appending remote targets to owner lists,
    and with the lists off (list_form_edges=0) dense chains in their place.
    (list_cap_factor sizes the lists of fixed-size transports only: it forces
    nothing on virtual ranks.)"""
    forms, _ = run_form("rmat16", mode, {} if lists else {"list_form_edges": 0}, extra=["--virtual-ranks", "3"])
    if lists:
        assert "S" in forms, forms
    else:
        assert "S" not in forms and "T" in forms, forms


# ---- batch kernels ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tmp_path_factory.mktemp("checked_forms")


def run_batch(graph_args, direction, ranks, extra=()):
    args = graph_args + ["--roots", "70", "--batch", "--validate", "--batch-direction", direction, "--json"] + list(extra)
    if ranks > 1:
        args += ["--virtual-ranks", str(ranks)]
    out = run_checked(args)
    assert dc.CLEAN + " gap 0 cross 0 orphan 0" in out.stdout, out.stdout[-2000:]
    # (the single run from <src> and every source of the batch, against the oracle)
    assert out.stdout.count("Output OK!") == 2 and "Validation OK" in out.stdout, out.stdout[-2000:]
    recs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    (single,) = [r for r in recs if "source" in r]
    (batch,) = [r for r in recs if r.get("batch")]
    assert single["backend"].endswith("+checked") and single["ranks"] == ranks
    assert (batch["roots"], batch["passes"], batch["validated_sources"]) == (70, 2, "70/70")
    return single


BATCH_CASES = [(d, 1) for d in ("push", "pull", "alternate", "auto")] + [(d, 3) for d in ("pull", "alternate", "auto")]


@pytest.mark.parametrize("direction,ranks", BATCH_CASES)
def test_batch_undirected(direction, ranks):
    run_batch(["--rmat", "14"], direction, ranks)


@pytest.mark.parametrize("direction,ranks", BATCH_CASES)
def test_batch_directed(files, direction, ranks):
    run_batch(["0", dc.cli_file(files), "--directed"], direction, ranks)


# ---- in-edge routing ----------------------------------------------------------------------------

@pytest.mark.parametrize("ranks,hub_sort", [(1, True), (3, True), (8, True), (1, False), (3, False)])
def test_in_edge_routing(files, ranks, hub_sort):
    """build_in_edges (the batch's first step on a directed graph): the count
    and fill passes route every entry to its column's owner."""
    run_batch(["0", dc.cli_file(files), "--directed"], "auto", ranks, [] if hub_sort else ["--no-hub-sort"])


def test_in_edge_routing_short_last_slice(files):
    """n no multiple of the rank count: the last rank's slice is short, and
    every column id still divides into a rank below the count."""
    path = os.path.join(str(files), "uniform5003.txt")
    N.write_generated_edge_list(path, dbfs.uniform_params(5003, 12000, 4))
    single = run_batch(["0", path, "--directed"], "auto", 8)
    n = single["n"]
    p = N.Partition(n, 8)  # (the engine's slices: whole bitmap words per rank)
    assert n % 8 != 0 and 0 < p.hi(7) - p.lo(7) < p.hi(0) - p.lo(0) == p.part, (n, p.lo(7), p.hi(7), p.part)
