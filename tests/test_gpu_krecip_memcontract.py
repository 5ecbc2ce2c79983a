"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the six launching entry points of
k-reciprocal re-ranking: mdx_krecip_sets, mdx_krecip_raw_offsets, mdx_krecip_raw_fill, mdx_krecip_expand_offsets,
mdx_krecip_expand_fill, mdx_krecip_rerank.  Two shapes each, so that the leftovers of one call are the stale pre-fill of the other;
every caller pointer at the smallest alignment include/mdx.h allows, its element size (the rows of raw_fill at 4 bytes and a stride
that is no multiple of 4: the chain then takes its scalar loads); the workspace of rerank at 16 bytes.  The oracle is the float64
restatement of test_gpu_krecip.py on host-made lists: integer outputs exactly, values within its bound."""
import functools

import numpy as np
import pytest

import memguard
from test_gpu_krecip import F32, bound, clustered, close, csr_of, database64, ell, query64, same_bits
from test_gpu_memcontract import Lazy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = []


def add(name, made, larger=None, **kw):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger, **kw)
    case.release = made.release
    CASES.append(case)
    return case


@functools.lru_cache(maxsize=None)
def problem(n, d, ld, k, k2, nq, r, lds):
    """Host inputs and the restatement's outputs of every stage for one shape."""
    x, q, _ = clustered(n + d, n=n, d=d, nq=nq, nc=max(2, n // 7))
    wide = np.random.default_rng(n).standard_normal((n, ld)).astype(F32)
    wide[:, :d] = x
    s = x @ x.T
    ids = np.argsort(-s, axis=1, kind="stable")[:, :k].astype(np.int64)
    sims = np.take_along_axis(s, ids, axis=1).astype(F32)
    x64 = x.astype(np.float64)
    rk, rh, raw, exp = database64(ids, sims, lambda i, j: F32(x64[i] @ x64[j]), k2)
    p = {"wide": wide, "ids": ids, "sims": sims, "n": n, "d": d, "k": k, "k2": k2, "r": r}
    p["rk"], p["rkc"] = ell(rk, k)
    p["rh"], p["rhc"] = ell(rh, (k + 1) // 2)
    p["raw"], p["exp"] = csr_of(raw), csr_of(exp)
    p["kth"] = np.ascontiguousarray(sims[:, k - 1])
    sq = np.random.default_rng(nq).standard_normal((nq, lds)).astype(F32)
    sq[:, :n] = q @ x.T
    p["scores"] = sq
    p["tq"] = np.argsort(-sq[:, :n], axis=1, kind="stable")[:, :r].astype(np.int64)
    wants, s_qe = [], max(len(c) for c in exp)
    for i in range(nq):
        want, nqe = query64(sq[i, :n], p["tq"][i], p["kth"], rh, raw, exp, k, k2, 0.3)
        wants.append(want)
        s_qe = max(s_qe, nqe)
    p["wants"] = wants
    p["tol"] = bound(max(len(c) for c in raw), k2, s_qe)
    return p


SHAPES = {"big": (300, 20, 24, 9, 3, 5, 60, 304), "small": (67, 7, 7, 4, 2, 2, 67, 67)}


def _sets(env, p):
    return tuple(env.put(name, p[name]) for name in ("rk", "rkc", "rh", "rhc"))


def _csr(env, p, which, values=True):
    o, c, v = p[which]
    return (env.put(which + "_offsets", o), env.put(which + "_cols", c), env.put(which + "_vals", v.astype(F32)) if values else None)


def _stage(entry, run, verify):
    """The two cases of one entry point: run(env, p) -> outputs, verify(outputs, p)."""
    def case(shape, larger=None, **kw):
        def make():
            p = problem(*SHAPES[shape])
            return [(lambda env: run(env, p), lambda o: verify(o, p))]
        return add("%s[%s]" % (entry, shape), Lazy(make), larger, **kw)
    return case


def _eq(o, p, **names):
    for name, want in names.items():
        assert o[name].dtype == want.dtype and np.array_equal(o[name], want), name


def _run_sets(env, p):
    rk, rkc, rh, rhc = env.ops.krecip_sets(env.put("ids", p["ids"]))
    return {"rk": rk, "rkc": rkc, "rh": rh, "rhc": rhc}


def _run_raw_fill(env, p):
    rows = env.put("rows", p["wide"])[:, :p["d"]]
    cols, vals = env.ops.krecip_raw_fill(rows, env.put("ids", p["ids"]), env.put("sims", p["sims"]), _sets(env, p),
                                         env.put("offsets", p["raw"][0]), len(p["raw"][1]))
    return {"cols": cols, "vals": vals}


def _run_expand_fill(env, p):
    cols, vals = env.ops.krecip_expand_fill(env.put("ids", p["ids"]), p["k2"], _csr(env, p, "raw"), env.put("offsets", p["exp"][0]),
                                            len(p["exp"][1]))
    return {"cols": cols, "vals": vals}


def _verify_fill(which):
    def verify(o, p):
        _eq(o, p, cols=p[which][1])
        assert o["vals"].dtype == F32 and close(o["vals"], p[which][2], p["tol"])
    return verify


def _run_rerank(env, p):
    scores = env.put("scores", p["scores"])[:, :p["n"]]
    out = env.ops.krecip_rerank((env.put("rh", p["rh"]), env.put("rhc", p["rhc"])), env.put("kth", p["kth"]), p["k"], p["k2"],
                                _csr(env, p, "raw"), _csr(env, p, "exp"), scores, env.put("top_ids", p["tq"]), 0.3)
    return {"out": out}


def _verify_rerank(o, p):
    out, n = o["out"], p["n"]
    base = p["scores"][:, :n] - F32(3)
    for q, want in enumerate(p["wants"]):
        g = np.array(sorted(want), np.int64)
        rest = np.ones(n, bool)
        rest[g] = False
        assert same_bits(out[q, rest], base[q, rest])
        assert close(out[q, g], [want[v] for v in g], p["tol"])


STAGES = {
    "krecip_sets": (_run_sets, lambda o, p: _eq(o, p, rk=p["rk"], rkc=p["rkc"], rh=p["rh"], rhc=p["rhc"]), {}),
    "krecip_raw_offsets": (lambda env, p: {"offsets": env.ops.krecip_raw_offsets(_sets(env, p))},
                           lambda o, p: _eq(o, p, offsets=p["raw"][0]), {}),
    "krecip_raw_fill": (_run_raw_fill, _verify_fill("raw"), {}),
    "krecip_expand_offsets": (lambda env, p: {"offsets": env.ops.krecip_expand_offsets(env.put("ids", p["ids"]), p["k2"],
                                                                                         _csr(env, p, "raw", values=False))},
                              lambda o, p: _eq(o, p, offsets=p["exp"][0]), {}),
    "krecip_expand_fill": (_run_expand_fill, _verify_fill("exp"), {}),
    "krecip_rerank": (_run_rerank, _verify_rerank, {"workspace_align": 16}),
}

for _entry, (_run, _verify, _kw) in STAGES.items():
    _case = _stage(_entry, _run, _verify)
    _big = _case("big", **_kw)
    _big.larger = _case("small", larger=_big, **_kw)

# entry point -> its cases.  The census of tests/test_memguard_host.py does not see these entry points (their prototypes are in
# include/mdx_krecip.h); tests/test_krecip_host.py::test_every_krecip_entry_point_is_covered reads this table instead.
COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in STAGES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_memory_contract(case):
    from mdir_amd import ops
    log = []
    assert case.larger is not None and case.larger is not case
    try:
        memguard.run_contract(ops, case, DEV, alignment_run=True, log=log.append)
        assert "stale" in log and any(step.startswith("align ") for step in log), log
    finally:
        case.release()
        case.larger.release()
        print("%s: %s" % (case.name, "; ".join(log)))
