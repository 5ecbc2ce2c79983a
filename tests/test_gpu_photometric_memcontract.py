"""The memory contract (tests/memguard.py; the runs are described in test_gpu_memcontract.py) of the two conversions of
include/mdx_photometric.h: mdx_histmatch_u8_to_chw and mdx_gamma_u8_to_chw.  Two shapes each, so that the leftovers of one call --
the counters among them, which the library zeroes in-stream -- are the stale pre-fill of the other: B = 2 with an odd width (the
scalar kernels), and a width of 64 whose four-pixel kernels give way to the scalar ones when `out` is only 4-byte aligned: same bits.
Every caller pointer at the smallest alignment include/mdx_photometric.h allows (images 1, target_cdf 8, out 4, the workspace 16).
The oracle and its bounds are those of test_gpu_photometric.py."""
import ctypes

import numpy as np
import pytest
import torch

import memguard
import photometric_restatement as R
from test_gpu_memcontract import WORKSPACE_ALIGN, Lazy, bits_equal
from test_gpu_photometric import check_lightness, clipped_root

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32

CASES = []


def add(name, made, larger=None):
    case = memguard.Case(name, lambda env: made.get(0)[0](env), lambda outs: made.get(0)[1](outs), larger=larger, workspace_align=WORKSPACE_ALIGN)
    case.release = made.release
    CASES.append(case)
    return case


def _hist_case(b, h, w, named, larger=None):
    def make():
        img = R.images(b, h, w, [1.0, 0.3][:b])
        cdf = np.cumsum(R.target_histogram()) if named else None

        def run(env):
            on_dev = env.put("target_cdf", cdf) if named else None
            out, x, counts, fp, mapped = env.ops.histmatch_u8_to_chw(env.put("images", img), R.MEAN, R.STD, on_dev, return_intermediates=True)
            return {"out": out, "x": x, "counts": counts, "fp": fp, "mapped": mapped}

        def verify(o):
            for i in range(b):
                spc = R.normspace(img[i])
                check_lightness(o["x"][i], spc[..., 0])
                bits_equal(o["counts"][i], np.histogram(o["x"][i], R.EDGES)[0].astype(np.int32))
                bits_equal(o["fp"][i], R.fp_table(o["counts"][i], h * w, cdf))
                bits_equal(o["mapped"][i], np.interp(o["x"][i], R.CENTRES, o["fp"][i]).astype(F32))
                np.testing.assert_allclose(o["out"][i], R.finish(spc, o["mapped"][i]), rtol=0, atol=1e-4)
        return [(run, verify)]
    return add("histmatch_u8_to_chw[%dx%dx%d %s]" % (b, h, w, "named" if named else "eq"), Lazy(make), larger)


def _gamma_case(b, h, w, target, larger=None):
    def make():
        img = R.images(b, h, w, [1.0, 0.3][:b])

        def run(env):
            out, x, gamma, info = env.ops.gamma_u8_to_chw(env.put("images", img), target, R.MEAN, R.STD, return_intermediates="solver")
            return {"out": out, "x": x, "gamma": gamma, "info": info}

        def verify(o):
            for i in range(b):
                spc = R.normspace(img[i])
                check_lightness(o["x"][i], spc[..., 0])
                assert abs(o["gamma"][i] - clipped_root(o["x"][i], target)) <= 1e-4
                assert 1 <= o["info"][i, 0] <= 50 and o["info"][i, 1] == 0
                np.testing.assert_allclose(o["out"][i], R.finish(spc, R.gamma_map(o["x"][i], o["gamma"][i])), rtol=0, atol=1e-4)
        return [(run, verify)]
    return add("gamma_u8_to_chw[%dx%dx%d target %g]" % (b, h, w, target), Lazy(make), larger)


_hm_odd = _hist_case(2, 37, 53, True)
_hm_odd.larger = _hist_case(1, 40, 64, False, larger=_hm_odd)
_ga_odd = _gamma_case(2, 37, 53, 0.5)
_ga_odd.larger = _gamma_case(1, 40, 64, 0.3, larger=_ga_odd)

COVERED = {entry: [c for c in CASES if c.name.startswith(entry + "[")] for entry in ("histmatch_u8_to_chw", "gamma_u8_to_chw")}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_memory_contract(case):
    from mdir_amd import ops
    log = []
    assert case.larger is not None and case.larger is not case and len(COVERED[case.name.split("[")[0]]) == 2
    try:
        memguard.run_contract(ops, case, DEV, alignment_run=True, log=log.append)
        assert "stale" in log and any(step.startswith("align ") and "out0@4" in step for step in log), log
    finally:
        case.release()
        case.larger.release()
        print("%s: %s" % (case.name, "; ".join(log)))


def test_a_workspace_one_byte_short_is_refused():
    """MDX_ERR_WORKSPACE (-4) from both conversions, with real device buffers: nothing is launched, `out` keeps its pre-fill."""
    from mdir_amd import _lib
    h = _lib.lib()
    b, hh, w = 2, 37, 53
    need = h.mdx_photometric_workspace(b, hh, w)
    u8 = torch.from_numpy(R.images(b, hh, w)).to(DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((b, 3, hh, w), 7.0, dtype=torch.float32, device=DEV)
    mean, std = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert h.mdx_histmatch_u8_to_chw(p(u8), b, hh, w, None, mean, std, p(ws), need - 1, p(out), None) == -4
    assert b"mdx_histmatch_u8_to_chw: workspace" in h.mdx_last_error()
    assert h.mdx_gamma_u8_to_chw(p(u8), b, hh, w, 0.5, mean, std, p(ws), need - 1, p(out), None) == -4
    assert b"mdx_gamma_u8_to_chw: workspace" in h.mdx_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="status -4"):
        _lib.check(h.mdx_gamma_u8_to_chw(p(u8), b, hh, w, 0.5, mean, std, p(ws), need - 1, p(out), None), "mdx_gamma_u8_to_chw")
    assert h.mdx_gamma_u8_to_chw(p(u8), b, hh, w, 0.5, mean, std, p(ws), need, p(out), None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())
