"""Device-checked build: bin/bfs_checked is the CLI with every
kernel file that has DBFS_DCHECK sites compiled with -DDBFS_CHECKED (`make
checked`, part of `make all`): csrc/kernels/{bfs,td,bu,ms,ms_bc,cc,graph}_kernels.hip,
the Makefile's CHECKED_SRC.  Kernels verify the bounds of their work lists,
owner lists, rows and vertex ids and record the first violation in their
file's word; the engine reads every word after every traversal, batch pass,
validation and build step (Engine::check_device) and fails the call, naming
the file.  DBFS_FAULT_INJECT kind=device[,file=td_kernels|bu_kernels] /
batch_device / bc_device / cc_device / in_edges_device records violation 99 in
the word of the file whose kernels that phase runs: one case per word proves
that it is compiled, read and cleared."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import directed_cases as dc
import distributed_cuda_bfs_amd as dbfs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED_BIN = os.path.join(REPO, "bin", "bfs_checked")
KERNELS = os.path.join(REPO, "csrc", "kernels")
DATA = os.path.join(REPO, "tests", "data")


# ---- every file with check sites is in the checked build ------------------------------------

def _check_site_files():
    """The .hip files under csrc/kernels with a DBFS_DCHECK site of their own,
    or that include -- through csrc/kernels/*.hpp, transitively -- a header
    with one (the macro's two definitions in kernel_common.hpp are no site)."""
    text = {}
    for name in sorted(os.listdir(KERNELS)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(KERNELS, name)) as f:
                text[name] = f.read()
    code = {name: re.sub(r"//[^\n]*", "", t) for name, t in text.items()}  # (a comment naming the macro is no site)
    sites = {name: len(re.findall(r"DBFS_DCHECK\(", t)) - len(re.findall(r"#define\s+DBFS_DCHECK\(", t))
             for name, t in code.items()}
    assert len(re.findall(r"#define\s+DBFS_DCHECK\(", code["kernel_common.hpp"])) == 2

    def includes(name):
        return [i for i in re.findall(r'#include\s+"([^"/]+)"', text[name]) if i in text]

    def has_site(name, seen):
        if name in seen:
            return False
        seen.add(name)
        return sites[name] > 0 or any(has_site(i, seen) for i in includes(name))

    return sorted(n for n in text if n.endswith(".hip") and has_site(n, set()))


def test_checked_src_lists_every_file_with_check_sites():
    with open(os.path.join(REPO, "Makefile")) as f:
        lines = [l for l in f.read().splitlines() if re.match(r"CHECKED_SRC\s*:?=", l)]
    assert len(lines) == 1 and not lines[0].rstrip().endswith("\\"), lines
    listed = {os.path.basename(p) for p in lines[0].split("=", 1)[1].split()}
    kept = _check_site_files()
    # (the walk itself: files known to have sites of their own are found)
    assert {"td_kernels.hip", "bu_kernels.hip", "bfs_kernels.hip"} <= set(kept)
    missing = [n for n in kept if n not in listed]
    assert not missing, f"DBFS_DCHECK sites compiled in no build: {missing} missing from CHECKED_SRC"


# ---- each injection kind reports the file it names (CPU backend) ---------------------------

def _cpu_calls():
    """kind -> (DBFS_FAULT_INJECT, file, make the engine, the call that must fail)."""
    p = dbfs.rmat_params(10, 16, 3)
    u, v = dbfs.generate_edges(p)
    directed = dbfs.build_csr(p.n, u, v, directed=True)
    rt = dbfs.init_runtime("cpu")
    und = lambda: dbfs.BFS(p, rt)
    drc = lambda: dbfs.BFS(directed, rt, mode="td", directed=True)
    root = lambda b: b.sample_roots(1, seed=1)[0]
    return {
        "device": ("rank=0,level=1,kind=device", "bfs_kernels", und, lambda b: b.run(root(b))),
        "device_td": ("rank=0,level=1,kind=device,file=td_kernels", "td_kernels", und, lambda b: b.run(root(b))),
        "device_bu": ("rank=0,level=1,kind=device,file=bu_kernels", "bu_kernels", und, lambda b: b.run(root(b))),
        "batch_device": ("rank=0,level=1,kind=batch_device", "ms_kernels", und,
                         lambda b: b.run_batch(b.sample_roots(8, seed=1))),
        "bc_device": ("rank=0,kind=bc_device", "ms_bc_kernels", und,
                      lambda b: b.run_batch(b.sample_roots(8, seed=1), betweenness=True)),
        "cc_device": ("rank=0,kind=cc_device", "cc_kernels", und, lambda b: b.components()),
        "in_edges_device": ("rank=0,kind=in_edges_device", "graph_kernels", drc, lambda b: b.build_in_edges()),
    }


@pytest.mark.parametrize("kind", ["device", "device_td", "device_bu", "batch_device", "bc_device", "cc_device",
                                  "in_edges_device"])
def test_injected_violation_names_its_file_cpu(monkeypatch, kind):
    inject, file, make, call = _cpu_calls()[kind]
    monkeypatch.setenv("DBFS_FAULT_INJECT", inject)
    with pytest.raises(Exception) as err:
        call(make())
    assert re.search(r"device check failed on rank 0: code 99, detail 0, file %s$" % file, str(err.value)), str(err.value)
    # the violation is consumed: the next clean call passes
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    call(make())


def test_injected_device_violation_fails_run_cpu(monkeypatch):
    monkeypatch.setenv("DBFS_FAULT_INJECT", "rank=0,level=1,kind=device")
    p = dbfs.rmat_params(10, 16, 3)
    bfs = dbfs.BFS(p, dbfs.init_runtime("cpu"))
    with pytest.raises(Exception, match="device check failed on rank 0: code 99"):
        bfs.run(bfs.sample_roots(1, seed=1)[0])
    # the violation is consumed: the next clean traversal passes
    monkeypatch.delenv("DBFS_FAULT_INJECT")
    bfs2 = dbfs.BFS(p, dbfs.init_runtime("cpu"))
    bfs2.run(bfs2.sample_roots(1, seed=1)[0])


def test_fault_file_key_is_checked(monkeypatch):
    """file= names a traversal kernel file and goes with kind=device only."""
    p = dbfs.rmat_params(10, 16, 3)
    for spec in ("rank=0,level=1,kind=device,file=ms_kernels", "rank=0,kind=cc_device,file=td_kernels"):
        monkeypatch.setenv("DBFS_FAULT_INJECT", spec)
        with pytest.raises(Exception, match="DBFS_FAULT_INJECT: file"):
            dbfs.BFS(p, dbfs.init_runtime("cpu"))


# ---- the CLI's engine options and chain records (CPU backend: no GPU) -------------------------

def _run(args, env=None, timeout=180):
    assert os.path.exists(CHECKED_BIN), "bin/bfs_checked missing: run `make checked` (make all builds it)"
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CHECKED_BIN] + args, capture_output=True, text=True, timeout=timeout, env=e)


def _json_runs(out):
    return [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{") and '"source"' in x]


def test_cli_opt_usage_errors():
    chain8 = os.path.join(DATA, "chain8.txt")
    for flags, msg in ((["--opt", "no_such_option=1"], "unknown engine option 'no_such_option'"),
                       (["--opt", "td_bin_edges=many"], "value is not a number"),
                       (["--opt", "td_bin_edges=1x"], "value is not a number"),
                       (["--opt", "td_bin_edges"], "--opt expects NAME=VALUE"),
                       (["--opt", "=1"], "--opt expects NAME=VALUE"),
                       (["--opt"], "missing value for --opt")):
        out = _run(["0", chain8, "--cpu"] + flags)
        assert out.returncode == 2 and msg in out.stderr, (flags, out.returncode, out.stderr[-500:])
    out = _run(["--help"])
    assert out.returncode == 2 and "--opt NAME=VALUE" in out.stderr and '"chains"' in out.stderr


def test_cli_opt_sets_the_engine_and_chains_are_reported():
    """--opt reaches the engines: the host loop enqueues no chain, the device
    loop's chains are listed with the fields RunResult.chains has."""
    base = ["--rmat", "12", "--cpu", "--mode", "td", "--json", "--quiet"]
    out = _run(base)
    assert out.returncode == 0, out.stderr[-2000:]
    (run,) = _json_runs(out)
    assert run["chains"] and all(set(c) == {"l", "form", "unvis", "split", "cut"} for c in run["chains"])
    assert [c["l"] for c in run["chains"]][:2] == [0, 1] and {c["form"] for c in run["chains"]} <= set("TSX")
    assert not run["backend"].endswith("+checked")  # (the CPU backend has no check sites)
    out = _run(base + ["--opt", "device_loop=0"])
    assert out.returncode == 0, out.stderr[-2000:]
    (host,) = _json_runs(out)
    assert host["chains"] == [] and host["levels"] and host["reached"] == run["reached"]
    # the last of a repeated option holds
    out = _run(base + ["--opt", "device_loop=0", "--opt", "device_loop=1"])
    assert out.returncode == 0 and _json_runs(out)[0]["chains"]


# ---- split levels and the level bytes of the last word's padding ---------------------------------

SPLIT_ARGS = ["--uniform", "266317:800000", "19397", "--mode", "td", "--validate", "--json",
              "--opt", "td_split_edges=1", "--opt", "td_split_parts=4"]


def split_level_bytes(run_cli):
    """A split top-down level ends in an update that takes every level byte
    equal to the level's as a new vertex, visited or not.  n = 266317 leaves 51
    padding bytes in the last word, which init_run used not to fill: a stale
    byte there was a vertex past the rows, its degree read off the end of
    row_off and summed into the level's totals (found as heap corruption of
    `bfs --cpu`).  DBFS_POISON_ALLOC makes unwritten memory read as the byte of
    each split level in turn: the runs stay exact, and the checked kernels
    (bfs_kernels site 16; the CPU backend's check) record nothing."""
    out = run_cli(SPLIT_ARGS, {})
    assert out.returncode == 0, out.stderr[-2000:]
    (run,) = _json_runs(out)
    split_levels = sorted({c["l"] for c in run["chains"] if c["split"] > 1})
    assert len(split_levels) >= 2, run["chains"]
    for l in split_levels:
        # (one-byte levels, the process's first run: level l + 1 is stored as the byte l + 1)
        out = run_cli(SPLIT_ARGS, {"DBFS_POISON_ALLOC": str(l + 1)})
        assert out.returncode == 0, (l, out.stdout[-1000:], out.stderr[-2000:])
        assert "Output OK!" in out.stdout and "Validation OK" in out.stdout, (l, out.stdout[-1000:])
        (poisoned,) = _json_runs(out)
        # (the totals and level records the padding vertices' degrees were summed into)
        records = lambda r: [(x["l"], x["frontier"], x["edges"], x["new"]) for x in r["levels"]]
        assert (poisoned["reached"], poisoned["edges"]) == (run["reached"], run["edges"]), l
        assert records(poisoned) == records(run), l


def test_split_level_ignores_padding_level_bytes_cpu():
    split_level_bytes(lambda args, env: _run(args + ["--cpu"], env=env))


# ---- the checked build on the GPU -------------------------------------------------------------

@pytest.mark.gpu
def test_split_level_ignores_padding_level_bytes_gpu():
    split_level_bytes(lambda args, env: _run(args, env=env))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["do", "td", "bu", "ref"])
@pytest.mark.parametrize("ranks", [1, 3])
def test_checked_build_clean(mode, ranks):
    args = ["--rmat", "16", "--roots", "4", "--validate", "--mode", mode, "--json", "--quiet"]
    if ranks > 1:
        args += ["--virtual-ranks", str(ranks)]
    out = _run(args)
    assert out.returncode == 0, out.stderr[-4000:]
    runs = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert runs and all(r["backend"].endswith("+checked") for r in runs), out.stdout[-2000:]


@pytest.mark.gpu
def test_checked_build_reports_violation():
    out = _run(["--rmat", "14", "--roots", "2", "--quiet"], env={"DBFS_FAULT_INJECT": "rank=0,level=0,kind=device"})
    assert out.returncode != 0
    assert "device check failed on rank 0: code 99" in out.stderr, out.stderr[-4000:]
    assert "file bfs_kernels" in out.stderr, out.stderr[-4000:]


def _word_cases(tmp_dir):
    chain8 = os.path.join(DATA, "chain8.txt")
    directed = ["0", dc.cli_file(tmp_dir), "--directed", "--roots", "70", "--batch", "--validate"]
    return {
        "bfs_kernels": ("rank=0,level=1,kind=device", ["0", chain8]),
        "td_kernels": ("rank=0,level=1,kind=device,file=td_kernels", ["0", chain8]),
        "bu_kernels": ("rank=0,level=1,kind=device,file=bu_kernels", ["--rmat", "10"]),
        "ms_kernels": ("rank=0,level=1,kind=batch_device", directed),
        "ms_bc_kernels": ("rank=0,kind=bc_device", ["--rmat", "10", "--roots", "70", "--batch", "--betweenness"]),
        "cc_kernels": ("rank=0,kind=cc_device", ["--rmat", "10", "--components"]),
        "graph_kernels": ("rank=0,kind=in_edges_device", directed),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("file", ["bfs_kernels", "td_kernels", "bu_kernels", "ms_kernels", "ms_bc_kernels", "cc_kernels",
                                  "graph_kernels"])
def test_each_files_word_is_live(tmp_path_factory, file):
    """Violation 99 recorded by a kernel of `file`, in that file's word: the
    run fails naming it; without the injection the same command is clean (the
    word was compiled, is read, and a clean run leaves it zero)."""
    inject, args = _word_cases(tmp_path_factory.getbasetemp())[file]
    out = _run(args + ["--json"], env={"DBFS_FAULT_INJECT": inject})
    assert out.returncode != 0, out.stdout[-2000:]
    assert "device check failed on rank 0: code 99, detail 0, file %s\n" % file in out.stderr, out.stderr[-4000:]
    out = _run(args + ["--json"])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    runs = _json_runs(out)
    assert runs and all(r["backend"].endswith("+checked") for r in runs), out.stdout[-2000:]
    assert "Output OK!" in out.stdout and "Wrong output!" not in out.stdout
