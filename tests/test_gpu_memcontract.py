"""The memory contract of every kernel entry point of include/mdx.h on the MI355X (tests/memguard.py is the harness).

The value tests compare what a kernel returns; this file looks at what it reads and writes around that.  ``TABLE`` maps an
entry point to its cases; ``memguard.run_contract`` executes each case (1) under ordinary allocations against the oracle,
(2) with every input, output and workspace in a guarded buffer of exactly the promised size at a 256-byte address, pre-filled
0xFF, (3) pre-filled 0x00 and with the stale contents a larger call of the same entry point left, (4) with the bytes after
every input 0x00 instead of 0xFF, (5) with every caller pointer, one at a time and then all together, at the smallest
alignment the header allows (include/mdx.h, "Alignment").  Runs 2-5 must return the bits of run 2, leave every guard byte alone and leave the
inputs as they were uploaded; a refusal at an alignment the header calls legal fails run 5 (refusals below it have tests of their own).

No tolerance is new: each case names the existing test whose oracle and bound it repeats (``tol``).  Shapes are the smallest
that reach each kernel of an entry point and end inside a tile in every dimension.

As a script -- ``python tests/test_gpu_memcontract.py rank_full topk ...`` -- it runs the cases of the named entry points in
this process (the sort's switches MDX_SORT_NO_PACK / MDX_SORT_RANK are read once per process)."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import memguard
from conftest import ROOT, sparse_map
from oracle import chain as OC
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORKSPACE_ALIGN = 16            # include/mdx.h "Alignment": every workspace
F32 = np.float32

TABLE = {}


class Lazy:
    """The (run, verify) pairs of one builder, made -- host data, oracle inputs and all -- when a case first runs and dropped
    again by ``release``: importing this module builds names and closures only."""

    def __init__(self, make):
        self.make, self.pairs = make, None

    def get(self, i):
        if self.pairs is None:
            self.pairs = self.make()
        return self.pairs[i]

    def release(self):
        self.pairs = None


def add(entry, name, made, i, tol, **kw):
    """Registers a case of ``mdx_<entry>``: pair ``i`` of the builder's ``made``; ``tol``: the existing test whose oracle and
    tolerance its ``verify`` repeats."""
    case = memguard.Case("%s[%s]" % (entry, name), lambda env: made.get(i)[0](env), lambda outs: made.get(i)[1](outs),
                         workspace_align=WORKSPACE_ALIGN, **kw)
    case.tolerance, case.release = tol, made.release
    TABLE.setdefault(entry, []).append(case)
    return case


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8), err_msg=what)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(F32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30).astype(F32)


def lib():
    from mdir_amd import _lib
    return _lib.lib()


def check(status, what):
    from mdir_amd import _lib
    _lib.check(status, what)


# =============================================================================================== pooling and tail
# H*W % 4 == 0 (the 16-byte loads, reached with a misaligned base only in run 5) and H*W odd.

MAPS = [(2, 5, 4, 6), (1, 7, 3, 5)]


def _pool_case(shape, kind, p):
    def make():
        x = sparse_map(sum(shape), shape)
        x[-1, 0] = 0.0                                                          # an all-zero plane

        def run(env):
            return {"out": env.ops.pool_l2n(env.put("feat", x), kind, p)}

        def verify(o):
            pool = {"gem": lambda a: O.gem(a, p), "mac": O.mac, "spoc": O.spoc}[kind]
            np.testing.assert_allclose(o["out"], O.l2n(pool(x)), rtol=1e-5, atol=1e-7)
        return [(run, verify)]
    made = Lazy(make)
    add("pool_l2n", "%s %s" % (shape, kind), made, 0,
        "test_gpu_kernels.test_pool_batch_and_zero_map: rtol 1e-5, atol 1e-7")


# (2, 5, 4, 6) gem / spoc, and the pool_multi case below, are the regression cases of what run 5 found: the sum of a plane with
# H*W % 4 == 0 used to be taken in another order when the map did not start at a 16-byte address, so a sliced feature map
# pooled to other bits than its aligned copy (mdx_pool.hip: the 16-byte loads are now issued at dword alignment).
for _shape in MAPS:
    for _kind, _p in (("gem", 2.92), ("mac", 1.0), ("spoc", 1.0)):
        _pool_case(_shape, _kind, _p)


def _regions(h, w):
    return [(0, 0, h, w)] + [(i, j, s, s) for i, j, s in O.rmac_regions(h, w, 3)]


def _rmac_case(shape):
    def make():
        rng = np.random.default_rng(sum(shape))
        x = (rng.standard_normal(shape) * (rng.random(shape) > 0.5)).astype(F32)

        def run(env):
            return {"out": env.ops.rmac(env.put("feat", x), _regions(*shape[2:]), 1e-6)}

        def verify(o):
            np.testing.assert_allclose(o["out"], O.rmac(x, 3, 1e-6), rtol=2e-6, atol=2e-6)

        def run_roi(env):
            return {"out": env.ops.roipool(env.put("feat", x), _regions(*shape[2:]), "gem", 2.5, 1e-6)}

        def verify_roi(o):
            np.testing.assert_allclose(o["out"], O.roipool(x, lambda a: O.gem(a, 2.5, 1e-6)), rtol=2e-5, atol=2e-6)
        return [(run, verify), (run_roi, verify_roi)]
    made = Lazy(make)
    add("rmac", str(shape), made, 0,
        "test_gpu_round5.test_rmac_on_the_device: rtol 2e-6, atol 2e-6")
    add("roipool", str(shape), made, 1,
        "test_gpu_round5.test_regional_pooling_on_the_device: rtol 2e-5, atol 2e-6")


for _shape in [(2, 6, 5, 7), (1, 4, 4, 8)]:
    _rmac_case(_shape)


def _region_sum_case(shape, eps):
    def make():
        rng = np.random.default_rng(shape[2])
        v = rng.standard_normal(shape).astype(F32)

        def run(env):
            return {"out": env.ops.region_sum(env.put("vecs", v), eps)}

        def verify(o):
            want = np.zeros((shape[0], shape[2]), F32)
            for r in range(shape[1]):
                want = (want + (v[:, r] if eps is None else O.l2n(v[:, r], eps))).astype(F32)
            np.testing.assert_allclose(o["out"], want, rtol=2e-5, atol=2e-6)
        return [(run, verify)]
    made = Lazy(make)
    add("region_sum", "%s eps=%s" % (shape, eps), made, 0,
        "test_gpu_round5.test_regional_pooling_on_the_device: rtol 2e-5, atol 2e-6")


_region_sum_case((2, 5, 8), None)
_region_sum_case((3, 4, 7), 1e-6)


def _pyramid_cases(B, C, sizes):
    tag = "B%d C%d %s" % (B, C, sizes)
    tol = "test_gpu_kernels.test_pool_multi_l2n_aggregate_two_launch_tail: rtol 1e-5, atol 1e-7"
    def make():
        maps = [sparse_map(30 + i, (B, C, h, w)) + F32(0.01) for i, (h, w) in enumerate(sizes)]
        per = np.stack([O.l2n(O.gem(m, 2.92)) for m in maps])                   # [S, B, C]
        pooled = np.stack([O.gem(m, 2.92) for m in maps])
        want = np.stack([O.ms_aggregate(per[:, b], 2.92) for b in range(B)])

        def run_multi(env):
            return {"out": env.ops.pool_multi([env.put("feat%d" % i, m) for i, m in enumerate(maps)], "gem", 2.92)}

        def run_agg(env):
            return {"out": env.ops.l2n_aggregate(env.put("pooled", pooled), 1e-6, 2.92)}

        def run_batch(env):
            return {"out": env.ops.ms_aggregate_batch([env.put("scale%d" % i, per[i]) for i in range(len(maps))], 2.92)}

        def run_one(env):
            return {"out": env.ops.ms_aggregate([env.put("scale%d" % i, per[i, 0]) for i in range(len(maps))], 2.92)}
        return [(run_multi, lambda o: np.testing.assert_allclose(o["out"], pooled, rtol=1e-5, atol=1e-7)), (run_agg, lambda o: np.testing.assert_allclose(o["out"], want, rtol=1e-5, atol=1e-7)), (run_batch, lambda o: np.testing.assert_allclose(o["out"], want, rtol=1e-5, atol=1e-8)), (run_one, lambda o: np.testing.assert_allclose(o["out"], want[0], rtol=1e-5, atol=1e-8))]
    made = Lazy(make)
    add("pool_multi", tag, made, 0,
        tol)
    add("l2n_aggregate", tag, made, 1,
        tol)
    add("ms_aggregate_batch", tag, made, 2,
        "test_gpu_kernels.test_ms_aggregate_batch_golden: rtol 1e-5, atol 1e-8")
    add("ms_aggregate", tag, made, 3,
        "test_gpu_kernels.test_ms_aggregate_golden: rtol 1e-5, atol 1e-8")


_pyramid_cases(2, 8, [(4, 6), (3, 5), (2, 2)])
_pyramid_cases(3, 7, [(3, 3), (1, 5)])


def _l2n_rows_case(r, d, with_bias):
    def make():
        rng = np.random.default_rng(r * d)
        x = rng.standard_normal((r, d)).astype(F32)
        x[r // 2] = 0.0
        b = rng.standard_normal(d).astype(F32) if with_bias else None

        def run(env):
            xt = env.put("x", x)
            return {"x": env.ops.l2n_rows_(xt, env.put("bias", b) if with_bias else None, 1e-6)}

        def verify(o):
            y = ((x + b).astype(F32) if with_bias else x).astype(np.float64)    # the sum is one fp32 addition, as in the kernel
            np.testing.assert_allclose(o["x"], y / (np.linalg.norm(y, axis=1, keepdims=True) + 1e-6), rtol=1e-6, atol=1e-9)
        return [(run, verify)]
    made = Lazy(make)
    add("l2n_rows", "%dx%d bias=%s" % (r, d, with_bias), made, 0,
        "test_gpu_kernels.test_l2n_rows_golden: rtol 1e-6, atol 1e-9", inplace=("x",))


_l2n_rows_case(5, 8, False)
_l2n_rows_case(3, 7, True)


# =============================================================================================== trunk and input

def _bn_act_case(shape, use_res, relu, affine):
    def make():
        rng = np.random.default_rng(sum(shape))
        c = shape[1]
        x = (rng.standard_normal(shape) * 2).astype(F32)
        res = rng.standard_normal(shape).astype(F32)
        mean, var = rng.standard_normal(c).astype(F32), rng.uniform(0.2, 3.0, c).astype(F32)
        wt, bs = rng.uniform(0.5, 1.5, c).astype(F32), rng.standard_normal(c).astype(F32)

        def run(env):
            return {"x": env.ops.bn_act_(env.put("x", x), env.put("mean", mean), env.put("var", var), env.put("weight", wt) if affine else None,
                                         env.put("bias", bs) if affine else None, 1e-5, env.put("residual", res) if use_res else None, relu)}

        def verify(o):
            want = O.bn_act(x, mean, var, wt if affine else None, bs if affine else None, 1e-5, res if use_res else None, relu)
            np.testing.assert_allclose(o["x"], want, rtol=2e-6, atol=2e-6)
        return [(run, verify)]
    made = Lazy(make)
    add("bn_act", "%s res=%s relu=%s affine=%s" % (shape, use_res, relu, affine), made, 0,
        "test_gpu_kernels.test_bn_act_vs_oracle_and_torch: rtol 2e-6, atol 2e-6", inplace=("x",))


_bn_act_case((2, 3, 4, 6), True, True, True)
_bn_act_case((1, 5, 3, 5), True, False, True)
_bn_act_case((1, 2, 2, 4), False, True, False)


def _conv_cases(n, cin, cout, h, w, use_res):
    tag = "%dx%dx%dx%d -> %d res=%s" % (n, cin, h, w, cout, use_res)
    def make():
        rng = np.random.default_rng(cin + cout + h * w)
        x = rng.standard_normal((n, cin, h, w)).astype(F32)
        wt = (rng.standard_normal((cout, cin)) / cin ** 0.5).astype(F32)
        mean, var = (rng.standard_normal(cout) * 0.1).astype(F32), rng.uniform(0.5, 1.5, cout).astype(F32)
        gamma, beta = rng.uniform(0.5, 1.5, cout).astype(F32), (rng.standard_normal(cout) * 0.1).astype(F32)
        idt = rng.standard_normal((n, cout, h, w)).astype(F32)

        def run_t(env):
            return {"wt": env.ops.conv1x1_transpose_weights(env.put("weight", wt))}

        def run(env):
            return {"out": env.ops.conv1x1_bn_act(env.put("x", x), env.put("weight_t", np.ascontiguousarray(wt.T)), env.put("mean", mean),
                                                  env.put("var", var), env.put("gamma", gamma), env.put("beta", beta), 1e-5,
                                                  env.put("residual", idt) if use_res else None, True)}

        def verify(o):
            y = np.einsum("oc,nchw->nohw", wt.astype(np.float64), x.astype(np.float64))
            y = (y - mean.astype(np.float64).reshape(1, -1, 1, 1)) * (gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)).reshape(1, -1, 1, 1) \
                + beta.astype(np.float64).reshape(1, -1, 1, 1)
            if use_res:
                y = y + idt
            y = np.maximum(y, 0)
            assert float(np.abs(o["out"] - y).max() / np.abs(y).max()) < 3e-6
        return [(run_t, lambda o: bits_equal(o["wt"], np.ascontiguousarray(wt.T))), (run, verify)]
    made = Lazy(make)
    add("conv1x1_transpose_weights", "%dx%d" % (cout, cin), made, 0,
        "a transpose: bit-equality (test_gpu_round3.test_conv1x1_bn_act_vs_float64 reads it)")
    add("conv1x1_bn_act", tag, made, 1,
        "test_gpu_round3.test_conv1x1_bn_act_vs_float64: max error < 3e-6 of the largest value")


_conv_cases(1, 16, 64, 3, 5, True)
_conv_cases(2, 32, 64, 4, 4, False)


def _u8_case(shape, mean, std):
    def make():
        u8 = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)

        def run(env):
            return {"out": env.ops.u8_to_chw(env.put("images", u8), mean, std)}

        def verify(o):
            want = ((u8.astype(F32) / F32(255.0)) - np.array(mean, F32)) / np.array(std, F32)
            bits_equal(o["out"], np.ascontiguousarray(want.transpose(0, 3, 1, 2)))
        return [(run, verify)]
    made = Lazy(make)
    add("u8_to_chw", str(shape), made, 0,
        "test_gpu_kernels.test_u8_to_chw_matches_host_chain: bit-equality")


_u8_case((2, 5, 7, 3), [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
_u8_case((1, 4, 6, 3), [0.1, 0.2, 0.3], [1.0, 0.5, 2.0])
_u8_case((1, 5, 3, 1), [0.5], [0.25])


def _clahe_case(b, h, w, clip, grid):
    def make():
        rng = np.random.default_rng(h * w + b)
        base = rng.integers(0, 256, (b, h // 8 + 1, w // 8 + 1, 3))
        img = np.clip(np.kron(base, np.ones((1, 8, 8, 1)))[:, :h, :w] + rng.normal(0, 12, (b, h, w, 3)), 0, 255).astype(np.uint8)
        mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        g = grid if isinstance(grid, tuple) else (grid, grid)

        def run(env):
            out, l8, luts, l8_eq = env.ops.clahe_u8_to_chw(env.put("images", img), clip, grid, mean, std, return_intermediates=True)
            return {"out": out, "l8": l8, "luts": luts, "l8_eq": l8_eq}

        def verify(o):
            for i in range(b):
                _, want_l8 = O.apply_clahe_rgb(img[i], clip, g)
                diff = o["l8"][i].astype(int) - want_l8.astype(int)
                assert np.abs(diff).max() <= 1 and (diff != 0).mean() < 1e-3
                want_luts, tile = O.clahe_luts(o["l8"][i], clip, g)
                np.testing.assert_array_equal(o["luts"][i], want_luts)
                eq = O.clahe_apply(o["l8"][i], want_luts, tile)
                np.testing.assert_array_equal(o["l8_eq"][i], eq)
                lab = O.rgb_to_lab(img[i].astype(F32) / F32(255))
                spc = ((lab + np.array([0, 128, 128], F32)) / np.array([100, 255, 255], F32)).astype(F32)
                spc[..., 0] = eq.astype(F32) / F32(255)
                rgb = O.lab_to_rgb(((spc * np.array([100, 255, 255], F32)).astype(F32) - np.array([0, 128, 128], F32)).astype(F32))
                np.testing.assert_allclose(o["out"][i], ((rgb - F32(mean)) / F32(std)).transpose(2, 0, 1), rtol=0, atol=1e-4)
        return [(run, verify)]
    made = Lazy(make)
    add("clahe_u8_to_chw", "%dx%dx%d grid %s" % (b, h, w, grid), made, 0,
        "test_gpu_round3.test_clahe_kernels_vs_restatement: lightness +-1 level on < 0.1 %, LUTs and blend bit-exact, output atol 1e-4")


_clahe_case(2, 37, 53, 4, 8)
_clahe_case(1, 16, 24, 2, (2, 3))


def _pyramid_case(shape, scales):
    def make():
        x = np.random.default_rng(shape[2]).standard_normal(shape).astype(F32)

        def run(env):
            got = env.ops.bilinear_pyramid(env.put("x", x), scales)
            return {"level%d" % i: t for i, t in enumerate(got) if scales[i] != 1}

        def verify(o):
            import torch.nn.functional as Fn
            for i, s_ in enumerate(scales):
                if s_ != 1:
                    want = Fn.interpolate(torch.from_numpy(x), scale_factor=s_, mode="bilinear", align_corners=False).numpy()
                    assert o["level%d" % i].shape == want.shape
                    np.testing.assert_allclose(o["level%d" % i], want, rtol=0, atol=2e-6)
        return [(run, verify)]
    made = Lazy(make)
    add("bilinear_pyramid", str(shape), made, 0,
        "test_gpu_kernels.test_bilinear_pyramid_is_f_interpolate: atol 2e-6 of torch's CPU kernel")


_pyramid_case((1, 2, 9, 7), [1, 1. / np.sqrt(2), 0.5])
_pyramid_case((2, 3, 8, 12), [0.5, 0.3])


def _resample_case(shape, axis, out_len):
    def make():
        from mdir_amd.resample import PRECISION_BITS, lanczos_taps
        img = np.random.default_rng(out_len).integers(0, 256, shape, dtype=np.uint8)
        bounds, taps = lanczos_taps(shape[1 + (axis == 1)], out_len)

        def run(env):
            return {"out": env.ops.resample_u8(env.put("images", img), axis, env.put("bounds", bounds), env.put("taps", taps))}

        def verify(o):
            x = np.moveaxis(img.astype(np.int64), 1 + (axis == 1), 0)
            res = np.empty((out_len,) + x.shape[1:], dtype=np.uint8)
            for k, (lo, cnt) in enumerate(bounds):
                acc = np.tensordot(taps[k, :cnt].astype(np.int64), x[lo:lo + cnt], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
                res[k] = np.clip(acc >> PRECISION_BITS, 0, 255)
            bits_equal(o["out"], np.ascontiguousarray(np.moveaxis(res, 0, 1 + (axis == 1))))
        return [(run, verify)]
    made = Lazy(make)
    add("resample_u8", "%s axis %d -> %d" % (shape, axis, out_len), made, 0,
        "test_gpu_kernels.test_device_thumbnail_is_pillow: pixel for pixel")


_resample_case((2, 9, 11, 3), 1, 6)
_resample_case((1, 9, 11, 3), 0, 5)
_resample_case((1, 8, 12, 1), 1, 5)


def _jpeg_case(w, h, subsampling):
    def make():
        from PIL import Image
        rng = np.random.default_rng(w * h)
        pic = np.clip(np.kron(rng.integers(0, 255, (h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w] + rng.normal(0, 10, (h, w, 3)), 0, 255)
        buf = io.BytesIO()
        Image.fromarray(pic.astype(np.uint8)).save(buf, format="JPEG", quality=88, subsampling=subsampling)
        data = buf.getvalue()
        state = {}

        def item():
            if "item" not in state:
                from mdir_amd import jpeg
                state["item"] = jpeg.entropy_decode(data)
                assert state["item"] is not None
            return state["item"]

        def run(env):
            it = item()
            info = it.info
            coef, quant = env.put("coef", it.coef.numpy()), env.put("quant", it.quant.numpy())
            planes = env.empty("planes", (info.nblocks * 64,), torch.uint8)
            rgb = env.empty("rgb", (1, info.height, info.width, 3), torch.uint8)
            check(lib().mdx_jpeg_pixels(P(coef), P(quant), ctypes.byref(info), P(planes), P(rgb), env.ops._stream()), "mdx_jpeg_pixels")
            return {"rgb": rgb}

        def verify(o):
            bits_equal(o["rgb"][0], np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        return [(run, verify)]
    made = Lazy(make)
    add("jpeg_pixels", "%dx%d %s" % (w, h, subsampling), made, 0,
        "test_gpu_kernels.test_jpeg_pixels_is_pillow: pixel for pixel", aligns={"planes": 4})


_jpeg_case(37, 29, "4:2:0")
_jpeg_case(24, 16, "4:4:4")


# =============================================================================================== index and similarity
# n in {1, 17, 32768 + 1} (64- and 128-row workgroups), d in {1, 63, 65, 100}, nq in {1, 17, 129, 257} (the 4x4x1 leftover tile
# of a last tile of <= 8 queries under 128-row workgroups, the grouped launch above 256 queries); the [nq, n] output with
# neither a multiple of 16 is the point.  The largest buffer stays at a few MB: 32 769 rows have at most 65 columns and meet at
# most 17 queries; d = 100 is met at n = 17.

SCORE_SHAPES = [(1, 1, 1), (17, 63, 17), (17, 65, 129), (17, 100, 257), (1, 100, 17), (32769, 1, 1), (32769, 63, 17), (32769, 63, 1),
                (32769, 65, 17)]


def _score_problem(n, d, nq):
    rng = np.random.default_rng(n + 7 * d + 131 * nq)
    db = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(F32)
    qv = (rng.standard_normal((nq, d)) / np.sqrt(d)).astype(F32)
    m = rng.normal(0, 0.05, d).astype(F32)
    return db, qv, m


def _scores_ex_case(n, d, nq, storage, mode, layout, with_center):
    tol = {"i8": "test_gpu_i8.test_scores_equal_the_restatement: bit-equality", "f16": "test_gpu_round4.test_retile_odd_shapes_both_layouts_and_storages: atol 3e-5",
           "f32": "test_gpu_kernels.test_scores_bit_exact_vs_chain: bit-equality" if mode == "chain" else
           "test_gpu_round4.test_split3/split2_scores_within_summation_order_of_the_chain: 2e-6 of the chain"}[storage]
    def make():
        db, qv, m = _score_problem(n, d, nq)
        src = db if layout == "ND" else np.ascontiguousarray(db.T)
        q = qv if layout == "ND" else np.ascontiguousarray(qv.T)
        qc = (qv - m).astype(F32) if with_center else qv

        def run(env):
            ix = env.ops.DescriptorIndex(env.put("vecs", src), layout, storage=storage)
            out = ix.scores(env.put("queries", q), layout, center=env.put("center", m) if with_center else None, compute=mode)
            ix.close()
            return {"scores": out}

        def verify(o):
            got = o["scores"]
            if storage == "i8":
                from test_i8_host import quantize_np, scores_np
                cq, sq = quantize_np(qc)
                cx, sx = quantize_np(db)
                bits_equal(got, scores_np(cq, sq, cx, sx))
            elif storage == "f16":
                ref = qc.astype(np.float16).astype(np.float64) @ db.astype(np.float16).astype(np.float64).T
                np.testing.assert_allclose(got, ref, rtol=0, atol=3e-5)
            elif mode == "chain":
                bits_equal(got, OC.gemm_nt_chain(qc, db))
            else:
                assert float(np.abs(got - OC.gemm_nt_chain(qc, db)).max()) <= 2e-6
        return [(run, verify)]
    made = Lazy(make)
    return add("scores_ex", "%dx%d nq=%d %s %s %s center=%s" % (n, d, nq, storage, mode, layout, with_center), made, 0,
        tol, aligns={"out0": 256})


_ring = 0
for _n, _d, _nq in SCORE_SHAPES:
    for _storage in ("f32", "f16", "i8"):
        _scores_ex_case(_n, _d, _nq, _storage, "chain", ("ND", "DN")[_ring % 2], _ring % 3 == 0)
        _ring += 1
for _n, _d, _nq in [(17, 63, 17), (17, 100, 257), (32769, 63, 1), (32769, 65, 17)]:
    for _mode in ("split3", "split2"):
        _scores_ex_case(_n, _d, _nq, "f32", _mode, ("ND", "DN")[_ring % 2], _ring % 3 == 0)
        _ring += 1
for _case in TABLE["scores_ex"]:                                             # stale: the largest shape of the same storage ran first
    if not _case.name.startswith("scores_ex[32769x65"):
        _case.larger = next(c for c in TABLE["scores_ex"] if c.name.startswith("scores_ex[32769x65") and _case.name.split()[2] == c.name.split()[2]
                            and "chain" in c.name)


def _index_case(entry, n, d, nq, layout, storage):
    """mdx_index_create / mdx_index_create_ex (the library allocates the tiles) read through mdx_scores / mdx_scores_ex; index_create_in
    through the wrapper, whose tiles come from the arena."""
    def make():
        db, qv, m = _score_problem(n, d, nq)
        src = db if layout == "ND" else np.ascontiguousarray(db.T)
        from mdir_amd import _lib
        lay = _lib.MDX_ROW_MAJOR if layout == "ND" else _lib.MDX_DIM_MAJOR

        def run(env):
            vecs, queries, center = env.put("vecs", src), env.put("queries", qv), env.put("center", m)
            out = env.empty("scores", (nq, n), torch.float32)
            h = lib()
            handle = ctypes.c_void_p()
            if entry == "index_create_in":
                ix = env.ops.DescriptorIndex(vecs, layout, storage=storage)
                handle = ix._h
            elif entry == "index_create_ex":
                check(h.mdx_index_create_ex(ctypes.byref(handle), P(vecs), n, d, lay, 0, _lib.STORAGE[storage], env.ops._stream()), "mdx_index_create_ex")
            else:
                check(h.mdx_index_create(ctypes.byref(handle), P(vecs), n, d, lay, 0, env.ops._stream()), "mdx_index_create")
            try:
                if entry in ("index_create", "scores"):
                    need = h.mdx_scores_workspace(nq, d)
                    ws = env.workspace("workspace", need)
                    check(h.mdx_scores(handle, P(queries), nq, _lib.MDX_ROW_MAJOR, P(center), P(out), P(ws), need, env.ops._stream()), "mdx_scores")
                else:
                    need = h.mdx_scores_workspace_ex(nq, d, 0)
                    ws = env.workspace("workspace", need)
                    check(h.mdx_scores_ex(handle, P(queries), nq, _lib.MDX_ROW_MAJOR, P(center), P(out), P(ws), need, 0, env.ops._stream()), "mdx_scores_ex")
                torch.cuda.synchronize()
            finally:
                if entry == "index_create_in":
                    ix.close()
                else:
                    check(h.mdx_index_destroy(handle), "mdx_index_destroy")
            return {"scores": out}

        def verify(o):
            qc = (qv - m).astype(F32)
            if storage == "i8":
                from test_i8_host import quantize_np, scores_np
                cq, sq = quantize_np(qc)
                cx, sx = quantize_np(db)
                bits_equal(o["scores"], scores_np(cq, sq, cx, sx))
            elif storage == "f16":
                np.testing.assert_allclose(o["scores"], qc.astype(np.float16).astype(np.float64) @ db.astype(np.float16).astype(np.float64).T, rtol=0, atol=3e-5)
            else:
                bits_equal(o["scores"], OC.gemm_nt_chain(qc, db))
        return [(run, verify)]
    made = Lazy(make)
    add(entry, "%dx%d nq=%d %s %s" % (n, d, nq, layout, storage), made, 0,
        "test_gpu_kernels.test_scores_bit_exact_vs_chain / test_gpu_i8 / test_gpu_round4.test_retile_odd_shapes: bit-equality (f32, i8), atol 3e-5 (f16)", aligns={"out0": 256})


for _n, _d, _nq in [(17, 63, 17), (1001, 101, 7)]:
    for _layout in ("ND", "DN"):
        _index_case("index_create", _n, _d, _nq, _layout, "f32")
        _index_case("scores", _n, _d, 129 if _n == 17 else 1, _layout, "f32")
        for _storage in ("f32", "f16", "i8"):
            _index_case("index_create_ex", _n, _d, _nq, _layout, _storage)
            _index_case("index_create_in", _n, _d, _nq, _layout, _storage)
_index_case("scores", 32769, 65, 17, "ND", "f32")
for _entry in ("index_create", "scores", "index_create_ex", "index_create_in"):     # stale: the largest case of the same storage first
    for _case in TABLE[_entry]:
        _same = [c for c in TABLE[_entry] if c.name.split()[-1] == _case.name.split()[-1] and c is not _case]
        _case.larger = max(_same, key=lambda c: int(c.name.split("[")[1].split("x")[0]))


def _rowmajor_case(n, d, nq, qlayout, with_center, own_out):
    def make():
        db, qv, m = _score_problem(n, d, nq)
        q = qv if qlayout == "ND" else np.ascontiguousarray(qv.T)

        def run(env):
            out = env.empty("scores", (nq, n), torch.float32) if own_out else None
            return {"scores": env.ops.scores_rowmajor(env.put("db", db), env.put("queries", q), qlayout,
                                                      center=env.put("center", m) if with_center else None, out=out)}

        def verify(o):
            bits_equal(o["scores"], OC.gemm_nt_chain((qv - m).astype(F32) if with_center else qv, db))
        return [(run, verify)]
    made = Lazy(make)
    return add("scores_rowmajor", "%dx%d nq=%d %s center=%s out=%s" % (n, d, nq, qlayout, with_center, own_out), made, 0,
        "test_gpu_round4.test_scores_rowmajor_bit_exact_vs_chain: bit-equality")


_big = _rowmajor_case(32769, 64, 17, "ND", True, False)
for _i, (_n, _d, _nq) in enumerate([(1, 4, 1), (17, 100, 17), (17, 64, 129), (17, 100, 257), (32769, 4, 1), (32769, 32, 17)]):
    _rowmajor_case(_n, _d, _nq, ("ND", "DN")[_i % 2], _i % 3 == 0, _i % 2 == 1).larger = _big


def _quantize_case(n, d, layout):
    def make():
        from test_gpu_i8 import rows
        x = rows(n, d, seed=d)

        def run(env):
            codes, scales = env.ops.quantize_i8(env.put("vecs", x if layout == "ND" else np.ascontiguousarray(x.T)), layout)
            return {"codes": codes, "scales": scales}

        def verify(o):
            from test_i8_host import quantize_np
            want_c, want_s = quantize_np(x)
            bits_equal(o["codes"], want_c)
            bits_equal(o["scales"], want_s)
        return [(run, verify)]
    made = Lazy(make)
    add("quantize_i8", "%dx%d %s" % (n, d, layout), made, 0,
        "test_gpu_i8.test_quantize_i8_equals_the_restatement: bit-equality")


_quantize_case(17, 63, "ND")
_quantize_case(300, 64, "DN")
_quantize_case(5, 1, "ND")


def _center_rows_case(nq, d, qlayout, with_center):
    def make():
        rng = np.random.default_rng(nq + d)
        q, c = rng.standard_normal((nq, d)).astype(F32), rng.standard_normal(d).astype(F32)

        def run(env):
            return {"x": env.ops.center_rows(env.put("queries", q if qlayout == "ND" else np.ascontiguousarray(q.T)), qlayout,
                                             env.put("center", c) if with_center else None)}
        return [(run, lambda o: bits_equal(o["x"], (q - c[None, :]).astype(F32) if with_center else q))]
    made = Lazy(make)
    add("center_rows", "%dx%d %s center=%s" % (nq, d, qlayout, with_center), made, 0,
        "test_gpu_join.test_range_search_with_a_center_and_dim_major_queries: one fp32 subtraction, bit-equality")


_center_rows_case(5, 7, "ND", True)
_center_rows_case(17, 64, "DN", True)
_center_rows_case(3, 5, "DN", False)


# =============================================================================================== ranking
# rank_small<ITEMS> classes (n <= LS_CAP = 8192), tiled passes with packed words above; nq = 1 and 3.

RANK_N = [2048, 2049, 4097, 6145, 8192, 8193, 4096 * 3 + 1]


def _rank_scores(n, nq):
    rng = np.random.default_rng(n * 7 + nq)
    sc = rng.standard_normal((nq, n)).astype(F32)
    sc[:, 10:40] = sc[:, 5:6]                                                # runs of exact ties
    sc[0, 50], sc[0, 51], sc[0, 52] = np.nan, -0.0, 0.0
    return sc


def _rank_full_case(n, nq, own):
    def make():
        sc = _rank_scores(n, nq)

        def run(env):
            s = env.put("scores", sc)
            if own:                                                              # the form the graph-replay code calls
                out = env.empty("ranks", (nq, n), torch.int64)
                ws = env.workspace("workspace", env.ops.rank_workspace_bytes(n, nq))
                return {"ranks": env.ops.rank_full(s, id_offset=1000, out=out, workspace=ws)}
            return {"ranks": env.ops.rank_full(s, id_offset=1000)}
        return [(run, lambda o: bits_equal(o["ranks"], OC.rank_full(sc) + 1000))]
    made = Lazy(make)
    return add("rank_full", "n=%d nq=%d own=%s" % (n, nq, own), made, 0,
        "test_gpu_kernels.test_rank_full_bit_exact: bit-equality")


def _rank_segments_case(n, nq, own):
    def make():
        sc = _rank_scores(n, nq)
        cuts = [0, n // 3 + 1, n // 3 + 1, n - 5, n]                              # a block that ends inside a tile, an empty block, a short one

        def run(env):
            blocks = [env.put("block%d" % g, sc[:, cuts[g]:cuts[g + 1]]) for g in range(4)]
            if own:
                out = env.empty("ranks", (nq, n), torch.int64)
                ws = env.workspace("workspace", env.ops.rank_workspace_bytes(n, nq))
                return {"ranks": env.ops.rank_full_segments(blocks, id_offset=11, out=out, workspace=ws)}
            return {"ranks": env.ops.rank_full_segments(blocks, id_offset=11)}
        return [(run, lambda o: bits_equal(o["ranks"], OC.rank_full(sc) + 11))]
    made = Lazy(make)
    return add("rank_full_segments", "n=%d nq=%d own=%s" % (n, nq, own), made, 0,
        "test_gpu_kernels.test_rank_full_segments_equals_rank_full: bit-equality")


for _make, _entry in ((_rank_full_case, "rank_full"), (_rank_segments_case, "rank_full_segments")):
    _bigger = {True: _make(20001, 3, True), False: _make(20001, 3, False)}
    for _i, _n in enumerate(RANK_N):
        for _nq in (1, 3):
            _make(_n, _nq, (_i + _nq) % 2 == 0).larger = _bigger[(_i + _nq) % 2 == 0]
    for _own in (True, False):
        _bigger[_own].larger = _make(30011, 3, _own)


# mdx_topk's three routes, on both sides of each condition (mdx_rank.hip: sampled when n >= 16384, k <= 1024 and 256 k <= n; else
# select when 4 (k + 4096) <= n; else the full sort trimmed in its last pass); each with top_ids only, top_scores only and both.
TOPK = [(16384, 64, "sampled"), (16384, 65, "trimmed tiled sort"), (16784, 100, "select"), (16783, 100, "trimmed"), (25600, 100, "sampled"),
        (25599, 100, "select"), (8000, 10, "rank_small with a k limit"), (2049, 2049, "k = n"), (12289, 12289, "k = n, tiled")]


def _topk_case(n, k, route, which):
    def make():
        nq = 2
        rng = np.random.default_rng(n + k)
        sc = (rng.standard_normal((nq, n)) * 0.022).astype(F32)
        sc[:, 100:164] = sc[:, 99:100]
        sc[1, 7] = np.nan

        def run(env):
            s = env.put("scores", sc)
            if which == "both":                                                  # the wrapper; its workspace= parameter where k is even
                ws = env.workspace("workspace", env.ops.rank_workspace_bytes(n, nq)) if k % 2 == 0 else None
                ids, vals = env.ops.topk(s, k, id_offset=7, workspace=ws)
                return {"ids": ids, "scores": vals}
            ids = env.empty("top_ids", (nq, k), torch.int64) if which == "ids" else None
            vals = env.empty("top_scores", (nq, k), torch.float32) if which == "scores" else None
            need = env.ops.rank_workspace_bytes(n, nq)
            ws = env.workspace("workspace", need)
            check(lib().mdx_topk(P(s), n, nq, k, 7, P(ids), P(vals), P(ws), ws.numel(), env.ops._stream()), "mdx_topk")
            return {"ids": ids} if which == "ids" else {"scores": vals}

        def verify(o):
            want = OC.rank_full(sc)[:, :k]
            if "ids" in o:
                bits_equal(o["ids"], want + 7)
            if "scores" in o:
                bits_equal(o["scores"], np.take_along_axis(sc, want, axis=1))
        return [(run, verify)]
    made = Lazy(make)
    return add("topk", "n=%d k=%d (%s) %s" % (n, k, route, which), made, 0,
        "test_gpu_kernels.test_topk_radix_select: bit-equality")


_topk_big = {w: _topk_case(40000, 300, "select, the stale source", w) for w in ("both", "ids", "scores")}
for _n, _k, _route in TOPK:
    for _which in ("both", "ids", "scores"):
        _topk_case(_n, _k, _route, _which).larger = _topk_big[_which]


def _rank_of_case(n, nq, sizes):
    def make():
        rng = np.random.default_rng(n)
        sc = (np.round(rng.standard_normal((nq, n)) * 40) / 40).astype(F32)
        sc[nq - 1, ::7] = np.nan
        lists = [rng.choice(n, size=s, replace=False) for s in sizes]

        def run(env):
            pos, idsc, off = env.ops.rank_of(env.put("scores", sc), lists)
            return {"pos": pos, "id_scores": idsc}

        def verify(o):
            off = np.concatenate([[0], np.cumsum(sizes)])
            for q in range(nq):
                np.testing.assert_array_equal(o["pos"][off[q]:off[q + 1]], OC.rank_of(sc[q], lists[q]))
                bits_equal(o["id_scores"][off[q]:off[q + 1]], sc[q][lists[q]])
        return [(run, verify)]
    made = Lazy(make)
    add("rank_of", "n=%d lists %s" % (n, sizes), made, 0,
        "test_gpu_kernels.test_topk_and_rank_of: bit-equality")


_rank_of_case(5001, 3, (5, 0, 300))
_rank_of_case(257, 2, (1, 17))


def _rank_positions_case(n, width, nq, sizes):
    def make():
        rng = np.random.default_rng(width)
        full = np.stack([rng.permutation(width) for _ in range(nq)]).astype(np.int64)
        lists = [np.unique(rng.integers(0, width + 50, size=s)) for s in sizes]

        def run(env):
            pos, off = env.ops.rank_positions(env.put("ranks", full)[:, :n], lists)
            return {"pos": pos}

        def verify(o):
            off = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
            for q in range(nq):
                where = {int(v): i for i, v in enumerate(full[q, :n])}
                np.testing.assert_array_equal(o["pos"][off[q]:off[q + 1]], [where.get(int(v), -1) for v in lists[q]])
        return [(run, verify)]
    made = Lazy(make)
    add("rank_positions", "n=%d of %d lists %s" % (n, width, sizes), made, 0,
        "test_gpu_round4.test_rank_positions_vs_numpy_isin: bit-equality")


_rank_positions_case(777, 777, 3, (600, 0, 17))
_rank_positions_case(4000, 5001, 2, (1, 250))


def _gather_count_cases(n, nq, sizes):
    tag = "n=%d lists %s" % (n, sizes)
    def make():
        rng = np.random.default_rng(n + nq)
        sc = (np.round(rng.standard_normal((nq, n)) * 40) / 40).astype(F32)
        lists = [rng.choice(n, size=s, replace=False).astype(np.int64) for s in sizes]
        ids = np.concatenate(lists)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        ref = np.concatenate([sc[q][lists[q]] for q in range(nq)])

        def run_gather(env):
            return {"out": env.ops.gather_scores(env.put("scores", sc), env.put("ids", ids), env.put("offsets", off))}

        def run_count(env):
            cnt = env.put("cnt", np.full(len(ids), 5, np.int64))                 # accumulated into (the header): 5 + this shard's count
            return {"cnt": env.ops.rank_count_(cnt, env.put("scores", sc), 100, env.put("ref_scores", ref), env.put("ref_ids", ids + 100),
                                               env.put("offsets", off))}

        def verify_count(o):
            want = np.concatenate([OC.rank_of(sc[q], lists[q]) for q in range(nq)]) + 5
            np.testing.assert_array_equal(o["cnt"], want)
        return [(run_gather, lambda o: bits_equal(o["out"], ref)), (run_count, verify_count)]
    made = Lazy(make)
    add("gather_scores", tag, made, 0,
        "test_gpu_api.test_full_size_shards_equal_whole: bit-equality")
    add("rank_count", tag, made, 1,
        "test_gpu_api.test_full_size_shards_equal_whole: bit-equality with the ranking's positions", inplace=("cnt",))


_gather_count_cases(5001, 3, (5, 0, 300))
_gather_count_cases(257, 2, (1, 17))


# =============================================================================================== re-ranking

def _knn_aggregate_case(n, d, nq, k, with_self):
    def make():
        from test_gpu_rerank import _problem, aggregate64
        rows, ids, sims, self_rows = _problem(np.random.default_rng(1000 * d + 10 * k + nq), n, d, nq, k)

        def run(env):
            return {"out": env.ops.knn_aggregate(env.put("rows", rows), env.put("ids", ids), env.put("sims", sims), 3.0,
                                                 self_rows=env.put("self_rows", self_rows) if with_self else None)}

        def verify(o):
            assert np.isfinite(o["out"]).all()
            assert np.abs(o["out"] - aggregate64(rows, ids, sims, 3.0, self_rows if with_self else None)).max() <= 2e-6
        return [(run, verify)]
    made = Lazy(make)
    add("knn_aggregate", "%dx%d nq=%d k=%d self=%s" % (n, d, nq, k, with_self), made, 0,
        "test_gpu_rerank.test_knn_aggregate_against_float64: 2e-6 absolute")


_knn_aggregate_case(301, 12, 5, 3, True)
_knn_aggregate_case(301, 7, 3, 10, False)
_knn_aggregate_case(50, 130, 70, 1, True)


def _lists(n, k, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n, (n, k)).astype(np.int64)
    bad = rng.random((n, k)) < 0.1
    ids[bad] = rng.choice(np.array([-1, n, n + 3, -(1 << 40), 1 << 40], dtype=np.int64), bad.sum())
    sims = rng.uniform(-0.5, 1.0, (n, k)).astype(F32)
    sims[5] = -np.abs(sims[5]) - 0.01
    return ids, sims


def _knn_graph_cases(n, k, gamma):
    def make():
        ids, sims = _lists(n, k, n + k)

        def run(env):
            cols, vals, counts = env.ops.knn_graph(env.put("ids", ids), env.put("sims", sims), gamma)
            return {"cols": cols, "vals": vals, "counts": counts}

        def verify(o):
            from test_gpu_diffusion import check_graph
            check_graph(torch.from_numpy(o["cols"]), torch.from_numpy(o["vals"]), torch.from_numpy(o["counts"]), ids, sims, gamma)

        def run_w(env):
            cols, w, counts = env.ops.knn_graph_weights(env.put("ids", ids), env.put("sims", sims), gamma)
            return {"cols": cols, "w": w, "counts": counts}

        def verify_w(o):
            from test_gpu_diffusion_truncated import weights64
            c64, w64, n64 = weights64(ids, sims, gamma)
            assert np.array_equal(o["cols"].astype(np.int64), c64) and np.array_equal(o["counts"], n64)
            ok = c64 >= 0
            assert np.all(o["w"][~ok] == 0)
            err = np.abs(o["w"][ok] - w64[ok]) / np.maximum(np.abs(w64[ok]), 1e-30)
            assert err.size == 0 or err.max() <= 2e-6, err.max()
        return [(run, verify), (run_w, verify_w)]
    made = Lazy(make)
    add("knn_graph", "n=%d k=%d gamma=%g" % (n, k, gamma), made, 0,
        "test_gpu_diffusion.test_knn_graph_odd_lists: mask and order exact, vals rtol 2e-6")
    add("knn_graph_weights", "n=%d k=%d gamma=%g" % (n, k, gamma), made, 1,
        "test_gpu_diffusion_truncated.test_knn_graph_weights: cols / counts exact, w rtol 2e-6")


_knn_graph_cases(40, 55, 3.0)
_knn_graph_cases(203, 7, 0.5)
for _entry in ("knn_graph", "knn_graph_weights"):
    TABLE[_entry][0].larger = TABLE[_entry][1]


def _symmetric_lists(n, k, seed):
    """Top-k lists of unit rows against themselves, in float64 (what feeds the graph in use)."""
    from test_gpu_diffusion import topk64
    x = unit_rows(np.random.default_rng(seed), n, 16).astype(np.float64)
    return topk64(x @ x.T, k)


def _diffusion_case(n, k, nq, kq, in_place):
    def make():
        from test_gpu_diffusion import cg64, dense, final64, graph64, seeds64, topk64
        gamma, alpha, iters, tol = 3.0, 0.9, 8, 1e-6
        ids, sims = _symmetric_lists(n, k, n + k)
        c64, v64, n64 = graph64(ids, sims.astype(F32), gamma)
        cols, vals, counts = c64.astype(np.int32), v64.astype(F32), n64.astype(np.int32)
        rng = np.random.default_rng(nq)
        s = (rng.standard_normal((nq, n)) * 0.3).astype(F32)
        sid, ssim = topk64(s.astype(np.float64), kq)
        sid, ssim = sid.astype(np.int64), ssim.astype(F32)

        def run(env):
            st = env.put("scores", s)
            out, res, steps = env.ops.diffusion((env.put("cols", cols), env.put("vals", vals), env.put("counts", counts)), st, env.put("seed_ids", sid),
                                                env.put("seed_sims", ssim), gamma, alpha, iters, tol, out=st if in_place else None, return_residual=True)
            return {"out": out, "residual": res, "steps": steps}

        def verify(o):
            S = dense(cols, vals.astype(np.float64), counts, n)
            hist = []
            f, res64, steps64 = cg64(S, seeds64(sid, ssim, n, gamma), alpha, iters, tol, hist)
            want, scale = final64(f, s), np.abs(f).max(axis=0)
            clear = f.T > 1e-3 * scale[:, None]
            assert clear.sum() > 0 and (np.abs(o["out"] - want) / scale[:, None])[clear].max() <= 1e-4
            unreached = f.T == 0
            bits_equal(o["out"][unreached], (s - F32(3))[unreached])
            np.testing.assert_allclose(o["residual"], res64, rtol=1e-2, atol=1e-6)
        return [(run, verify)]
    made = Lazy(make)
    return add("diffusion", "n=%d k=%d nq=%d kq=%d in_place=%s" % (n, k, nq, kq, in_place), made, 0,
        "test_gpu_diffusion.test_diffusion_solve_against_float64_cg: 1e-4 of the column's largest value, unreached rows bit-equal, residual rtol 1e-2", inplace=("scores",) if in_place else ())


_dif_big = _diffusion_case(600, 6, 5, 4, False)
_diffusion_case(200, 5, 3, 4, False).larger = _dif_big
_diffusion_case(203, 5, 1, 3, False).larger = _dif_big
_diffusion_case(200, 5, 3, 4, True).larger = _dif_big
_diffusion_case(203, 5, 2, 3, True).larger = _dif_big


def _truncated_case(n, k, nq, r, kq, in_place):
    def make():
        from test_gpu_diffusion import topk64
        from test_gpu_diffusion_truncated import truncated64, weights64
        gamma, alpha, iters, tol = 3.0, 0.9, 8, 1e-6
        ids, sims = _symmetric_lists(n, k, n + k + 1)
        c64, w64, n64 = weights64(ids, sims.astype(F32), gamma)
        cols, w, counts = c64.astype(np.int32), w64.astype(F32), n64.astype(np.int32)
        s = (np.random.default_rng(nq + r).standard_normal((nq, n)) * 0.3).astype(F32)
        tid, tsim = topk64(s.astype(np.float64), r)
        tid, tsim = tid.astype(np.int64), tsim.astype(F32)

        def run(env):
            st = env.put("scores", s)
            out, res, steps = env.ops.diffusion_truncated((env.put("cols", cols), env.put("w", w), env.put("counts", counts)), st, env.put("top_ids", tid),
                                                          env.put("top_sims", tsim), kq, gamma, alpha, iters, tol, out=st if in_place else None,
                                                          return_residual=True)
            return {"out": out, "residual": res, "steps": steps}

        def verify(o):
            want, res64, steps64, fs, hists = truncated64(s, tid, tsim, cols.astype(np.int64), w.astype(np.float64), counts, kq, gamma, alpha, iters, tol)
            base = s - F32(3)
            for q in range(nq):
                inside = np.zeros(n, dtype=bool)
                inside[tid[q]] = True
                bits_equal(o["out"][q, ~inside], base[q, ~inside])
                f = fs[q]
                bits_equal(o["out"][q, tid[q][f == 0]], base[q, tid[q][f == 0]])
                scale = np.abs(f).max()
                if scale > 0:
                    clear = tid[q][f > 1e-3 * scale]
                    assert (np.abs(o["out"][q, clear] - want[q, clear]) / scale).max() <= 1e-4
        return [(run, verify)]
    made = Lazy(make)
    return add("diffusion_truncated", "n=%d k=%d nq=%d R=%d kq=%d in_place=%s" % (n, k, nq, r, kq, in_place), made, 0,
        "test_gpu_diffusion_truncated.check_against64: 1e-4 of the largest value, outside the subgraph and unreached bit-equal", inplace=("scores",) if in_place else ())


_trunc_big = _truncated_case(600, 6, 4, 100, 5, False)
_truncated_case(200, 5, 3, 16, 4, False).larger = _trunc_big
_truncated_case(203, 5, 1, 33, 40, False).larger = _trunc_big
_truncated_case(203, 5, 2, 16, 4, True).larger = _trunc_big


# =============================================================================================== int8 follow-ups
# rescore / join_resolve: ld == d and ld > d, d % 4 != 0, K = 1 and K not a multiple of the wave.

def _rescore_case(n, d, ld, nq, K, qlayout, with_center):
    def make():
        from test_gpu_rescore import expected
        rng = np.random.default_rng(d * 7919 + K + ld)
        wide = unit_rows(rng, n, ld)
        wide[3] = wide[2]                                                        # duplicate rows: equal scores, ascending id
        x = np.ascontiguousarray(wide[:, :d])
        qn = unit_rows(rng, nq, d)
        c = rng.normal(0, 0.01, d).astype(F32)
        ids = np.stack([rng.permutation(n)[:K] for _ in range(nq)]).astype(np.int64)
        ids[0, 0] = n + 5                                                        # out of range: NaN, sorted last

        def run(env):
            rows = env.put("rows", wide)[:, :d]
            out_ids, out_sc = env.ops.rescore(rows, env.put("queries", qn if qlayout == "ND" else np.ascontiguousarray(qn.T)), env.put("ids", ids), qlayout,
                                              env.put("center", c) if with_center else None)
            return {"ids": out_ids, "scores": out_sc}

        def verify(o):
            full = OC.gemm_nt_chain((qn - c).astype(F32) if with_center else qn, x)
            want_ids, want_sc = expected(full, ids, n)
            bits_equal(o["ids"], want_ids)
            bits_equal(o["scores"], want_sc)
        return [(run, verify)]
    made = Lazy(make)
    return add("rescore", "%dx%d ld=%d nq=%d K=%d %s center=%s" % (n, d, ld, nq, K, qlayout, with_center), made, 0,
        "test_gpu_rescore.test_rescore_equals_the_fp32_index: bit-equality")


_rs_big = _rescore_case(500, 100, 100, 5, 300, "ND", False)
_rescore_case(45, 7, 7, 3, 1, "ND", True).larger = _rs_big
_rescore_case(45, 7, 9, 2, 40, "DN", False).larger = _rs_big
_rescore_case(200, 8, 8, 3, 70, "DN", True).larger = _rs_big
_rescore_case(200, 8, 12, 1, 70, "ND", False).larger = _rs_big


def _i8_rows(n, d, seed):
    x = unit_rows(np.random.default_rng(seed), n, d)
    x[1] = 0
    x[2] = x[3]
    return x


def _bounds_case(n, d):
    def make():
        x = _i8_rows(n, d, n + d)

        def run(env):
            ix = env.ops.DescriptorIndex(env.put("vecs", x), "ND", storage="i8")
            out = ix.i8_bounds()
            torch.cuda.synchronize()
            ix.close()
            return {"bounds": out}

        def verify(o):
            from test_rescore_host import bounds_np
            raw = o["bounds"]
            got = (float(raw[0]), float(raw[1]), float(raw[2]), int(raw[3:4].view(np.int32)[0]))
            assert got == bounds_np(x), (got, bounds_np(x))
        return [(run, verify)]
    made = Lazy(make)
    add("index_i8_bounds", "%dx%d" % (n, d), made, 0,
        "test_gpu_rescore (bounds_np): equality", aligns={"out0": 256})


_bounds_case(17, 63)
_bounds_case(1001, 100)


def _certify_case(n, d, nq, K, qlayout, with_center):
    def make():
        from test_rescore_host import bounds_np, depth_np, upper_np
        from test_i8_host import quantize_np, scores_np
        rng = np.random.default_rng(n + d + K)
        x = _i8_rows(n, d, n + d)
        q = (x[rng.integers(0, n, nq)] + 0.02 * rng.standard_normal((nq, d))).astype(F32)
        c = rng.normal(0, 0.01, d).astype(F32)
        qc = (q - c).astype(F32) if with_center else q
        want_b = bounds_np(x)
        packed = np.array([want_b[0], want_b[1], want_b[2], 0.0], np.float64)
        packed[3:4].view(np.int32)[0] = want_b[3]
        s8 = scores_np(*quantize_np(qc), *quantize_np(x))
        t = np.sort(s8, axis=1)[:, ::-1][:, K - 1].astype(F32)                   # the K-th int8 score
        exact = OC.gemm_nt_chain(qc, x)
        short = np.argsort(-s8, axis=1, kind="stable")[:, :K]
        sc = -np.sort(-np.take_along_axis(exact, short, axis=1), axis=1)         # rescore's sorted scores of the int8 shortlist

        def run(env):
            depth, upper = env.ops.rescore_certify(env.put("scores", sc), env.put("t", t), env.put("queries", q if qlayout == "ND" else np.ascontiguousarray(q.T)),
                                                   env.put("bounds", packed), n, qlayout, env.put("center", c) if with_center else None)
            return {"depth": depth, "upper": upper}

        def verify(o):
            u = upper_np(t, qc, want_b, d)
            got = o["upper"].astype(np.float64)
            assert not np.isnan(u).any() and (got >= u).all() and (got - u <= 1e-5 * np.abs(u)).all()
            np.testing.assert_array_equal(o["depth"], depth_np(sc, got, n))
        return [(run, verify)]
    made = Lazy(make)
    add("rescore_certify", "%dx%d nq=%d K=%d %s center=%s" % (n, d, nq, K, qlayout, with_center), made, 0,
        "test_gpu_rescore (upper_np / depth_np): upper >= the float64 bound and within 1e-5 of it, depth equal")


_certify_case(300, 63, 5, 1, "ND", False)
_certify_case(300, 64, 3, 70, "DN", True)


def _join_rows(n, d, seed, ld=None):
    """Unit rows with planted near duplicates (pairs above the thresholds); ``ld``: as the first d columns of a wider matrix."""
    rng = np.random.default_rng(seed)
    x = unit_rows(rng, n, d)
    for k in range(0, n // 2, 5):
        v = x[k] + F32(0.05) * rng.standard_normal(d).astype(F32)
        x[n - 1 - k] = v / np.linalg.norm(v)
    x = x.astype(F32)
    if ld is None:
        return x
    wide = rng.standard_normal((n, ld)).astype(F32)
    wide[:, :d] = x
    return wide


def _join_stats_case(n, d, ld):
    def make():
        wide = _join_rows(n, d, n + ld, ld)
        x = np.ascontiguousarray(wide[:, :d])

        def run(env):
            ix = env.ops.DescriptorIndex(env.put("vecs", x), "ND", storage="i8")
            st = env.ops.join_stats(ix, env.put("rows", wide)[:, :d])
            torch.cuda.synchronize()
            ix.close()
            return {"stats": st}

        def verify(o):
            from test_join_host import row_factors
            p, q, r, w, _ = row_factors(x)
            bits_equal(o["stats"][:, 0], p)
            for col, want in ((1, q), (2, r), (3, w)):                           # rounded up, never down: the bars of the certificate's bound
                got = o["stats"][:, col].astype(np.float64)
                assert (got >= want).all() and (got - want <= 1e-5 * np.abs(want)).all(), col
        return [(run, verify)]
    made = Lazy(make)
    add("join_stats", "%dx%d ld=%d" % (n, d, ld), made, 0,
        "test_join_host.row_factors in float64; p bit-equal, {q, r, w} >= it and within 1e-5 (the bars of test_gpu_rescore's upper bound)", aligns={"out0": 256, "out1": 16})


_join_stats_case(200, 64, 64)
_join_stats_case(131, 7, 9)


def _join_candidates_case(n, d, tau, symmetric, capacity, raw=False):
    """capacity: a number, or "count" / "count-1" (resolved inside the run from a first call with capacity 0).  ``raw``: the
    second call goes straight to the C ABI with ``pairs`` and ``count`` from the arena -- the wrapper hands over a zeroed count,
    so only this form sees whether the library clears the counter its atomics add to."""
    def make():
        x = _join_rows(n, d, n + d)

        def run(env):
            ops = env.ops
            ix = ops.DescriptorIndex(env.put("vecs", x), "ND", storage="i8")
            st = ops.join_stats(ix, env.put("rows", x))
            _, count = ops.join_candidates(ix, st, ix, st, tau, 0, n, symmetric, 0)
            cap = {"count": count, "count-1": max(count - 1, 0)}.get(capacity, capacity)
            if raw:
                pairs_t, count_t = env.empty("pairs", (max(cap, 1),), torch.int64), env.empty("count", (1,), torch.int64)
                check(lib().mdx_join_candidates(ix._h, P(st), ix._h, P(st), 0, n, int(symmetric), tau, P(pairs_t), cap, P(count_t),
                                                ops._stream()), "mdx_join_candidates")
                count2 = int(count_t.item())
                pairs = pairs_t[:min(count2, cap)]
            else:
                pairs, count2 = ops.join_candidates(ix, st, ix, st, tau, 0, n, symmetric, cap)
            assert count2 == count and pairs.numel() == min(count, cap), (count, count2, cap)
            ix.close()
            out = {"count": np.array([count2], np.int64)}
            if cap >= count:
                out["pairs"] = np.sort(pairs.cpu().numpy())                     # the order comes from an atomic: compared as a sorted set
            return out

        def verify(o):
            exact = OC.gemm_nt_chain(x, x)
            hit = exact >= F32(tau)
            if symmetric:
                hit &= np.arange(n)[None, :] > np.arange(n)[:, None]
            i, j = np.nonzero(hit)
            assert o["count"][0] >= len(i) > 0
            if "pairs" in o:
                got = o["pairs"]
                assert len(np.unique(got)) == len(got) == o["count"][0]
                assert np.isin((i.astype(np.int64) << 32) | j.astype(np.int64), got).all()           # every exact hit is a candidate
                gi, gj = got >> 32, got & 0xFFFFFFFF
                assert (gi >= 0).all() and (gi < n).all() and (gj < n).all() and (not symmetric or (gj > gi).all())
        return [(run, verify)]
    made = Lazy(make)
    add("join_candidates", "%dx%d tau=%g symmetric=%s capacity=%s%s" % (n, d, tau, symmetric, capacity, " raw" if raw else ""), made, 0,
        "test_gpu_join.test_small_candidate_capacity_gives_the_same_bits: the sorted set; a superset of the exact hits (test_join_host)", aligns={"out0": 256, "out1": 16})


for _cap in (0, 3, "count-1", "count", 1 << 16):
    _join_candidates_case(300, 64, 0.8, True, _cap)
_join_candidates_case(131, 7, 0.9, False, "count")
_join_candidates_case(131, 7, 0.9, False, 3)
_join_candidates_case(300, 64, 0.8, True, "count", raw=True)
_join_candidates_case(131, 7, 0.9, False, 3, raw=True)


def _join_resolve_case(n, d, ld, tau):
    def make():
        from test_gpu_join import brute
        wide = _join_rows(n, d, n + d, ld)
        x = np.ascontiguousarray(wide[:, :d])
        exact = OC.gemm_nt_chain(x, x)
        i, j = np.nonzero((exact >= F32(tau - 0.3)) & (np.arange(n)[None, :] > np.arange(n)[:, None]))     # a superset of the hits, unique
        perm = np.random.default_rng(n).permutation(len(i))
        pairs = ((i.astype(np.int64) << 32) | j.astype(np.int64))[perm]

        def run(env):
            a = env.put("rows_a", wide)[:, :d]
            b = env.put("rows_b", wide)[:, :d]
            off, ids, sc = env.ops.join_resolve(a, b, env.put("pairs", pairs), tau, 0, n)
            return {"offsets": off, "ids": ids, "scores": sc}

        def verify(o):
            want = brute(exact, tau, upper_from=0)
            assert want[1].size > 0
            bits_equal(o["offsets"], want[0])
            bits_equal(o["ids"], want[1])
            bits_equal(o["scores"], want[2])
        return [(run, verify)]
    made = Lazy(make)
    return add("join_resolve", "%dx%d ld=%d tau=%g" % (n, d, ld, tau), made, 0,
        "test_gpu_join.test_small_candidate_capacity_gives_the_same_bits (brute force): bit-equality")


_jr_big = _join_resolve_case(400, 100, 100, 0.7)
_join_resolve_case(131, 7, 7, 0.9).larger = _jr_big
_join_resolve_case(131, 7, 9, 0.9).larger = _jr_big
_join_resolve_case(200, 8, 12, 0.8).larger = _jr_big
_join_resolve_case(200, 8, 8, 0.8).larger = _jr_big


def _range_select_case(m, n, ld, quantile, diag, capacity):
    def make():
        from test_gpu_join import brute
        rng = np.random.default_rng(m * n + ld)
        wide = (np.round(rng.standard_normal((m, ld)) * 20) / 20).astype(F32)    # ties at the threshold
        wide[0, 3] = np.nan
        s = np.ascontiguousarray(wide[:, :n])
        tau = float(np.quantile(s[np.isfinite(s)], quantile))
        want = brute(s, tau, upper_from=diag)
        hits = len(want[1])
        cap = {"hits": hits, "hits-1": max(hits - 1, 0)}.get(capacity, capacity)

        def run(env):
            off, ids, sc = env.ops.range_select(env.put("scores", wide)[:, :n], tau, diag, cap)
            return {"offsets": off, "ids": ids, "scores": sc}

        def verify(o):
            assert hits > 3
            bits_equal(o["offsets"], want[0])
            bits_equal(o["ids"], want[1])
            bits_equal(o["scores"], want[2])
        return [(run, verify)]
    made = Lazy(make)
    return add("range_select", "%dx%d ld=%d q=%g diag=%s capacity=%s" % (m, n, ld, quantile, diag, capacity), made, 0,
        "test_gpu_join.test_range_search_equals_brute_force: bit-equality")


_rsel_big = _range_select_case(70, 1001, 1001, 0.5, None, 1 << 16)
for _cap in (0, 3, "hits-1", "hits", 1 << 16):
    _range_select_case(5, 301, 301, 0.9, None, _cap).larger = _rsel_big
_range_select_case(17, 300, 303, 0.9, 0, "hits").larger = _rsel_big
_range_select_case(17, 300, 303, 0.9, 128, 3).larger = _rsel_big


# =============================================================================================== f64 kernels

def _gram_case(d, n, with_center):
    def make():
        A = np.random.default_rng(d + n).standard_normal((d, n))
        m = A.mean(axis=1)

        def run(env):
            return {"out": env.ops.gram_f64(env.put("a", A), env.put("center", m) if with_center else None)}

        def verify(o):
            Ac = A - m[:, None] if with_center else A
            scale = np.sqrt(np.outer((Ac * Ac).sum(1), (Ac * Ac).sum(1))) + 1e-300
            assert np.max(np.abs(o["out"] - Ac @ Ac.T) / scale) < 1e-13
            np.testing.assert_array_equal(o["out"], o["out"].T)
        return [(run, verify)]
    made = Lazy(make)
    return add("gram_f64", "%dx%d center=%s" % (d, n, with_center), made, 0,
        "test_gpu_round3.test_gram_f64_vs_numpy: 1e-13 of the row norms")


_gram_big = _gram_case(130, 600, True)
_gram_case(64, 16, False).larger = _gram_big
_gram_case(24, 77, True).larger = _gram_big
_gram_case(17, 33, False).larger = _gram_big


def _project_case(dout, d, n, with_center):
    def make():
        rng = np.random.default_rng(dout + d + n)
        Pm, X, m = rng.standard_normal((dout, d)), rng.standard_normal((d, n)), rng.standard_normal(d)

        def run(env):
            return {"out": env.ops.project_f64(env.put("p", Pm), env.put("x", X), env.put("center", m) if with_center else None)}

        def verify(o):
            Xc = X - m[:, None] if with_center else X
            bound = np.sqrt((Pm * Pm).sum(1))[:, None] * np.sqrt((Xc ** 2).sum(0))[None, :]
            assert np.max(np.abs(o["out"] - Pm @ Xc) / bound) < 1e-13
        return [(run, verify)]
    made = Lazy(make)
    return add("project_f64", "%dx%d n=%d center=%s" % (dout, d, n, with_center), made, 0,
        "test_gpu_round3.test_project_f64_vs_numpy: 1e-13 of the norms' product")


_proj_big = _project_case(100, 130, 600, True)
_project_case(24, 24, 64, True).larger = _proj_big
_project_case(5, 30, 77, False).larger = _proj_big
_project_case(17, 33, 1, True).larger = _proj_big


def _l2n_cols_case(d, n):
    def make():
        X = np.random.default_rng(d * n).standard_normal((d, n))
        X[:, n // 2] = 0

        def run(env):
            return {"x": env.ops.l2n_cols_f64_(env.put("x", X), 1e-6)}
        return [(run, lambda o: np.testing.assert_allclose(o["x"], X / (np.linalg.norm(X, ord=2, axis=0, keepdims=True) + 1e-6), rtol=0, atol=1e-12))]
    made = Lazy(make)
    add("l2n_cols_f64", "%dx%d" % (d, n), made, 0,
        "test_gpu_round5.test_whitenapply_in_float64_and_random_map_problems_on_the_device: atol 1e-12", inplace=("x",))


_l2n_cols_case(17, 33)
_l2n_cols_case(64, 256)


# =============================================================================================== the runner

# Run 3's stale half needs, for every case, a differently shaped call of the same entry point that ran first: where the builders
# above named none, it is the entry point's largest case (the one the others already point to, else the one listed here); the
# largest case itself takes the leftovers of another shape (smaller: they cover the head of its buffers).
BIGGEST = {"pool_l2n": 0, "rmac": 0, "roipool": 0, "region_sum": 1, "pool_multi": 0, "l2n_aggregate": 0, "ms_aggregate_batch": 0, "ms_aggregate": 0,
           "l2n_rows": 0, "bn_act": 0, "conv1x1_transpose_weights": 1, "conv1x1_bn_act": 1, "u8_to_chw": 0, "clahe_u8_to_chw": 0,
           "bilinear_pyramid": 1, "resample_u8": 0, "jpeg_pixels": 0, "quantize_i8": 1, "center_rows": 1, "rank_of": 0, "rank_positions": 0,
           "gather_scores": 0, "rank_count": 0, "knn_aggregate": 2, "index_i8_bounds": 1, "rescore_certify": 0, "join_stats": 0, "join_candidates": 4,
           "l2n_cols_f64": 1}
for _entry, _cases in TABLE.items():
    _pointed = [c.larger for c in _cases if c.larger is not None]
    _largest = max(_pointed, key=_pointed.count) if _pointed else _cases[BIGGEST[_entry]]
    for _case in _cases:
        if _case.larger is None:
            _case.larger = _largest if _case is not _largest else next(c for c in _cases if c is not _largest)

CASES = [(entry, i) for entry in TABLE for i in range(len(TABLE[entry]))]


def _run(entry, i, log=None):
    from mdir_amd import ops
    return memguard.run_contract(ops, TABLE[entry][i], DEV, alignment_run=True, log=log)


@pytest.mark.parametrize("entry,i", CASES, ids=[TABLE[e][i].name for e, i in CASES])
def test_memory_contract(entry, i):
    log = []
    assert TABLE[entry][i].larger is not None and TABLE[entry][i].larger in TABLE[entry]
    try:
        _run(entry, i, log.append)
        assert "stale" in log and any(step.startswith("align ") for step in log), log
    finally:
        TABLE[entry][i].release()
        TABLE[entry][i].larger.release()
        print("%s (%s): %s" % (TABLE[entry][i].name, TABLE[entry][i].tolerance, "; ".join(log)))


def test_the_arena_sees_a_store_past_the_end_on_the_device():
    """The harness itself on the device (its logic is proven on the CPU in test_memguard_host.py): one float stored right
    after, and one right before, a guarded buffer -- inside the arena's own allocation -- is reported with the buffer's name."""
    for where, side in ((lambda t: t.storage_offset() + t.numel(), "after"), (lambda t: t.storage_offset() - 1, "before")):
        arena = memguard.Arena(DEV)
        t = arena.empty((3, 5), torch.float32, "victim", 0xFF, 4)
        assert t.is_cuda and t.data_ptr() % 16 == 4
        arena.check()
        t.as_strided((1,), (1,), where(t)).fill_(1.0)
        with pytest.raises(memguard.ContractViolation, match="guard %s buffer 'victim'" % side):
            arena.check()


WITH_WORKSPACE = ["rmac", "clahe_u8_to_chw", "scores", "scores_ex", "scores_rowmajor", "rank_full", "rank_full_segments", "topk", "knn_graph",
                  "knn_graph_weights", "diffusion", "diffusion_truncated", "rescore", "join_resolve", "range_select", "gram_f64", "project_f64"]


@pytest.mark.parametrize("entry", WITH_WORKSPACE)
def test_a_workspace_below_16_bytes_is_refused(entry):
    """include/mdx.h "Alignment": every workspace is 16-byte aligned, MDX_ERR_INVALID otherwise -- before anything is launched
    (no guard touched, no input modified).  Both forms of a call that has them (the wrapper's own workspace, the caller's)."""
    from mdir_amd import ops
    seen = set()
    for case in TABLE[entry]:
        names = memguard.workspace_names(ops, case, DEV)
        assert names, case.name
        if tuple(names) in seen:
            continue
        seen.add(tuple(names))
        for name in names:
            assert memguard.refuses(ops, case, DEV, {name: 8}), (case.name, name)
            assert not memguard.refuses(ops, case, DEV, {name: 16}), (case.name, name)


def test_the_other_stated_alignments_are_refused_below():
    """The rest of the header's table: the tiles of mdx_index_create_in below 256 bytes, the stats of mdx_join_stats / mdx_join_candidates
    below 16, the planes of mdx_jpeg_pixels below 4."""
    from mdir_amd import ops
    for entry, name, below in (("index_create_in", "out0", 128), ("join_stats", "out1", 8), ("jpeg_pixels", "planes", 2)):
        case = TABLE[entry][0]
        assert memguard.refuses(ops, case, DEV, {name: below}), (case.name, name)
        assert not memguard.refuses(ops, case, DEV, {name: case.aligns[name]}), (case.name, name)
    # stats_a / stats_b of mdx_join_candidates: made by a plain call, handed over at 8 mod 16
    x = _join_rows(200, 64, 1)
    rows = torch.from_numpy(x).to(DEV)
    ix = ops.DescriptorIndex(rows, "ND", storage="i8")
    good = ops.join_stats(ix, rows)
    arena = memguard.Arena(DEV)
    bad = arena.put(good.cpu().numpy(), 8, 0xFF, "stats")
    for a, b in ((bad, good), (good, bad)):
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.join_candidates(ix, a, ix, b, 0.8, 0, 200, True, 16)
    ops.join_candidates(ix, good, ix, good, 0.8, 0, 200, True, 16)
    arena.check()
    ix.close()


@pytest.mark.parametrize("switch", ["MDX_SORT_NO_PACK=1", "MDX_SORT_RANK=ballot"])
def test_ranking_contract_under_the_sort_switches(switch):
    """The ranking entry points once more with the packed intermediate words off / the ballot form of the wave rank: the
    switches are read when the library first ranks, so each gets a process of its own (as test_gpu_round3.test_rank_forms)."""
    key, value = switch.split("=")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "rank_full", "rank_full_segments", "topk"], env=dict(os.environ, **{key: value}),
                          text=True, capture_output=True, timeout=1500)
    assert proc.returncode == 0 and "MEMCONTRACT-OK" in proc.stdout, (proc.stdout[-3000:], proc.stderr[-3000:])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    for _entry in sys.argv[1:]:
        for _i in range(len(TABLE[_entry])):
            _run(_entry, _i)
            TABLE[_entry][_i].release()
    print("MEMCONTRACT-OK")
