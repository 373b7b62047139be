"""Cases shared by the chain-guard tests (test_chain_guard.py on the CPU backend,
test_chain_guard_gpu.py on the GPU): device-loop traversals whose enqueued
chains include no-op ones of every form -- mispredicted chains, sparse chains
whose level outgrew their cap, the chain trailing the traversal's end.  Every
kernel of such a chain must do nothing (ChainGuard::live); one that ran would
change levels, records or totals.  Each run is compared with the host loop,
which has no chains, and with the sequential oracle."""
import numpy as np

import chain_plans
import distributed_cuda_bfs_amd as dbfs

MODE = "do"
OPTION_SETS = {
    "default": {},
    "no_predict": {"device_loop_predict": 0},
    "sparse_binned": {"td_sparse_edges": 512, "td_bin_min_rows": 0, "td_bin_edges": 1024},
}
FORMS = {"S", "T", "B", "X"}

_shared = {}   # runtime -> (params, roots, per root: oracle levels, host levels, host result)
_results = {}  # (runtime, option set) -> forms of the no-op chains


def params():
    return dbfs.rmat_params(12, 16, 41)


def _reference(rt):
    """Roots, oracle levels and host-loop runs: computed once per runtime."""
    if id(rt) not in _shared:
        p = params()
        csr = dbfs.host_csr_from_params(p)
        host = dbfs.BFS(p, rt, mode=MODE)
        host.engine.set_option("device_loop", 0)
        roots = host.sample_roots(4, seed=3) + [0]
        ref = {}
        for src in roots:
            res = host.run(src)
            ref[src] = (dbfs.cpu_bfs(csr, src)[0], host.levels().copy(), res)
        _shared[id(rt)] = (p, roots, ref)
    return _shared[id(rt)]


def _strip(res):
    return [(l["dir"], l["frontier"], l["frontier_edges"], l["discovered"]) for l in res.levels]


def noop_forms(res):
    """Forms of the chains that were no-ops: enqueued again later for the same
    level, or for a level past the last one recorded."""
    chains = [(c[0], c[1]) for c in res.chains]
    nlev = len(res.levels)
    return {form for i, (level, form) in enumerate(chains)
            if level >= nlev or any(l == level for l, _ in chains[i + 1:])}


def check_option_set(rt, name):
    """Runs every root with the option set on the device loop; asserts levels,
    per-level records and totals against the host loop and the oracle.
    Returns the forms of the no-op chains seen."""
    if (id(rt), name) in _results:
        return _results[(id(rt), name)]
    p, roots, ref = _reference(rt)
    dev = dbfs.BFS(p, rt, mode=MODE)
    for k, v in OPTION_SETS[name].items():
        dev.engine.set_option(k, v)
    assert dict(dev.engine.get_options())["device_loop"] == 1.0
    forms = set()
    runs = []
    for src in roots:
        oracle, host_levels, b = ref[src]
        a = dev.run(src)
        assert np.array_equal(dev.levels(), oracle), (name, src)
        assert np.array_equal(dev.levels(), host_levels), (name, src)
        assert _strip(a) == _strip(b), (name, src)
        assert (a.reached, a.edges, a.depth) == (b.reached, b.edges, b.depth), (name, src)
        forms |= noop_forms(a)
        runs.append(a)
    chain_plans.check("gpu" if rt.is_gpu else "cpu", chain_plans.key("chain_guard", name), runs)
    print(f"chain guard: option set {name}: no-op chain forms {sorted(forms)}")
    _results[(id(rt), name)] = forms
    return forms


def check_every_form(rt):
    """Over the option sets, no-op chains of every form were enqueued (and, by
    check_option_set, changed nothing)."""
    seen = set()
    for name in OPTION_SETS:
        seen |= check_option_set(rt, name)
    assert seen >= FORMS, sorted(seen)
