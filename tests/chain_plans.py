"""The device loop's chain plans, compared with recordings from an earlier commit.

Which chains a traversal enqueues -- (level, form, cap, gather, push, unvis,
split, cut) each -- is decided on the host from the integer totals the levels
stamp, so it is reproducible exactly.  Tests that already run device-loop
traversals hand their results to check(), which compares every chain tuple,
`mispredicts`, (reached, edges, depth) and the stripped level records with
tests/golden/chain_plans_{cpu,gpu}.json.  The fixtures name the commit whose
csrc produced them.

Recording (with the csrc to record from built):
    DBFS_CHAIN_PLANS_RECORD=cpu.raw.json python -m pytest tests -m "not gpu"
    DBFS_CHAIN_PLANS_RECORD=gpu.raw.json python -m pytest tests -m gpu
    python tests/chain_plans.py write <commit> cpu.raw.json gpu.raw.json
check() then asserts nothing and collects; `write` refuses unless the two
recordings together cover everything listed in COVERAGE.
"""
import atexit
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = os.environ.get("DBFS_CHAIN_PLANS_RECORD")

_fixtures = {}
_recorded = {}


def summary(res):
    """What is compared of one run, as plain JSON values (virtual-rank bodies
    return this instead of the result object)."""
    return {
        "chains": [[c[0], c[1], int(c[2])] + [int(x) for x in c[3:]] for c in res.chains],
        "mispredicts": int(res.mispredicts),
        "totals": [int(res.reached), int(res.edges), int(res.depth)],
        "levels": [[l["dir"], int(l["frontier"]), int(l["frontier_edges"]), int(l["discovered"])] for l in res.levels],
    }


def key(*parts):
    """A case key from its parts; option dicts in sorted order."""
    out = []
    for p in parts:
        if isinstance(p, dict):
            p = ",".join(f"{k}={float(v):g}" for k, v in sorted(p.items())) or "-"
        out.append(str(p))
    return "/".join(out)


def _fixture(backend):
    if backend not in _fixtures:
        with open(os.path.join(GOLDEN, f"chain_plans_{backend}.json")) as f:
            _fixtures[backend] = json.load(f)
    return _fixtures[backend]


def check(backend, case, runs):
    """`runs`: the case's results (or their summary()), in order.  backend:
    'cpu' or 'gpu'."""
    got = [r if isinstance(r, dict) else summary(r) for r in runs]
    if RECORD:
        # (a case that several tests run records the same plans each time)
        assert _recorded.setdefault(case, got) == got, f"chain plans of {case} differ between two runs"
        return
    fx = _fixture(backend)
    assert case in fx["cases"], f"no recorded chain plans for {case} (tests/chain_plans.py records them)"
    want = fx["cases"][case]
    assert len(got) == len(want), (case, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for field in ("chains", "mispredicts", "totals", "levels"):
            assert g[field] == w[field], (f"{case} run {i}: {field} differ from commit {fx['parent']}'s:\n"
                                          f"  now      {g[field]}\n  recorded {w[field]}")


if RECORD:
    @atexit.register
    def _dump():
        if _recorded:
            with open(RECORD, "w") as f:
                json.dump(_recorded, f)


# ---- what the recordings must contain ------------------------------------------------


def _live_forms(run):
    """Per level, the form of the last chain enqueued for it."""
    live = {}
    for c in run["chains"]:
        live[c[0]] = c[1]
    return live


def _outgrew_cap(run):
    """A sparse chain replaced because its level had more frontier edges than its cap."""
    ch, lv = run["chains"], run["levels"]
    return any(c[1] == "S" and c[2] > 0 and c[0] < len(lv) and lv[c[0]][0] == "T" and lv[c[0]][2] > c[2]
               and any(d[0] == c[0] for d in ch[i + 1:]) for i, c in enumerate(ch))


def _third_bottom_up(run):
    """A bottom-up level at index >= 2 enqueued after two bottom-up levels."""
    live = _live_forms(run)
    return any(L >= 2 and L < len(run["levels"]) and live.get(L - 1) == "B" and live.get(L - 2) == "B"
               for L, f in live.items() if f == "B")


COVERAGE = {
    "a chain of form S": lambda k, r: any(c[1] == "S" for c in r["chains"]),
    "a chain of form T": lambda k, r: any(c[1] == "T" for c in r["chains"]),
    "a chain of form X": lambda k, r: any(c[1] == "X" for c in r["chains"]),
    "a chain of form B": lambda k, r: any(c[1] == "B" for c in r["chains"]),
    "a chain with unvis": lambda k, r: any(c[5] for c in r["chains"]),
    "a chain with split > 1": lambda k, r: any(c[6] > 1 for c in r["chains"]),
    "a chain with cut": lambda k, r: any(c[7] for c in r["chains"]),
    "a chain with gather": lambda k, r: any(c[3] for c in r["chains"]),
    "a run with mispredicts > 0": lambda k, r: r["mispredicts"] > 0,
    "a sparse chain re-enqueued because its level outgrew cap": lambda k, r: _outgrew_cap(r),
    "a third consecutive bottom-up level (whole_units rule)": lambda k, r: _third_bottom_up(r),
    "a non-predicting run (device_loop_predict = 0)": lambda k, r: "predict=0" in k and bool(r["chains"]),
}


def covered(cases):
    """COVERAGE item -> the first case key that shows it (or None)."""
    out = {}
    for name, test in COVERAGE.items():
        out[name] = next((k for k, runs in sorted(cases.items()) if any(test(k, r) for r in runs)), None)
    return out


def write(parent, cpu_raw, gpu_raw):
    raw = {}
    for backend, path in (("cpu", cpu_raw), ("gpu", gpu_raw)):
        with open(path) as f:
            raw[backend] = json.load(f)
    both = {f"{b}:{k}": v for b, cases in raw.items() for k, v in cases.items()}
    cov = covered(both)
    for name, where in cov.items():
        print(f"{name}: {where}")
    missing = [name for name, where in cov.items() if where is None]
    if missing:
        sys.exit("not written: the recordings lack " + "; ".join(missing))
    os.makedirs(GOLDEN, exist_ok=True)
    for backend, cases in raw.items():
        path =os.path.join(GOLDEN, f"chain_plans_{backend}.json")
        with open(path, "w") as f:
            f.write('{"parent": %s, "cases": {\n' % json.dumps(parent))
            f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}"
                               for k, v in sorted(cases.items())))
            f.write("\n}}\n")
        print(f"{path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "write":
        write(*sys.argv[2:])
    else:
        sys.exit("usage: chain_plans.py write <commit> <cpu recording> <gpu recording>")
