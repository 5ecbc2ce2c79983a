"""The int8 shard (MDX_I8, include/mdx.h) on a CPU-only box: the C ABI, its argument checks, the host keys, and the numpy
restatement of the quantisation contract that tests/test_gpu_i8.py compares the device with bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

I8_MAX_D = 133120            # largest d with 127^2 * round_up(d, 64) < 2^31
E_SLOP = 2.0 ** -15          # ||x - scale c||_inf <= scale (1/2 + 2^-15)  (include/mdx.h, MDX_I8)


# ------------------------------------------------------------------ the contract, restated in numpy (also used on the GPU)

def quantize_np(x):
    """(codes int8 [n, d], scales fp32 [n]) of fp32 rows ``x`` [n, d]: IEEE fp32, round to nearest even, nothing fused."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(127.0) / a                          # fp32 division, correctly rounded
        y = x * inv[:, None]                                 # one fp32 product per element
    c = np.clip(np.rint(y), -127, 127)                       # rint: half to even
    c[a == 0] = 0
    scales = (a / np.float32(127.0)).astype(np.float32)
    return c.astype(np.int8), scales


def scores_np(cq, sq, cx, sx):
    """[nq, n] scores of the contract: the int32 sum (exact in float64: every partial sum is an integer below 2^53), rounded
    to fp32, times the fp32 product of the two scales."""
    acc = cq.astype(np.float64) @ cx.astype(np.float64).T
    prod = sx[None, :].astype(np.float32) * sq[:, None].astype(np.float32)
    return acc.astype(np.float32) * prod


def error_bound(x, q, cx, sx, cq, sq, s):
    """Per pair: E_x ||q||_1 + scale_x ||c_x||_1 E_q + 2^-22 |s|, with E = scale (1/2 + 2^-15) (include/mdx.h)."""
    ex = sx.astype(np.float64) * (0.5 + E_SLOP)
    eq = sq.astype(np.float64) * (0.5 + E_SLOP)
    q1 = np.abs(q.astype(np.float64)).sum(axis=1)
    c1 = np.abs(cx.astype(np.float64)).sum(axis=1)
    return ex[None, :] * q1[:, None] + (sx.astype(np.float64) * c1)[None, :] * eq[:, None] + 2.0 ** -22 * np.abs(s.astype(np.float64))


# ------------------------------------------------------------------ C ABI

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_int8_shard():
    from mdir_amd import _lib
    text, code = _declared()
    assert re.search(r"\bMDX_I8\s*=\s*2\b", code)
    assert re.search(r"int\s+mdx_quantize_i8\s*\(\s*const float \*src,\s*int64_t n,\s*int64_t d,\s*int layout,\s*int8_t \*codes,"
                     r"\s*float \*scales,\s*void \*stream\s*\)", code)
    assert "mdx_quantize_i8" in _lib.EXPORTS
    assert _lib.STORAGE["i8"] == _lib.MDX_I8 == 2
    assert re.search(r"#define MDX_ABI_VERSION 3\b", code)


def test_library_exports_quantize_i8():
    from mdir_amd import _lib
    _lib.build()
    assert hasattr(_lib.lib(), "mdx_quantize_i8")


def _index_bytes_formula(n, d):
    rt = -(-(-(-n // 16)) // 8) * 8
    d_pad = -(-d // 64) * 64
    return rt * 16 * d_pad + rt * 16 * 4 + 256


@pytest.mark.parametrize("n,d", [(1, 1), (16, 64), (17, 65), (333, 100), (128, 2048), (1004993, 2048), (7, I8_MAX_D)])
def test_index_bytes_of_an_int8_shard(n, d):
    from mdir_amd import _lib
    h = _lib.lib()
    assert h.mdx_index_bytes(n, d, 2) == _index_bytes_formula(n, d)
    assert h.mdx_index_bytes(n, d, 2) < h.mdx_index_bytes(n, d, 1) < h.mdx_index_bytes(n, d, 0)


def test_index_bytes_headline_and_refusals():
    from mdir_amd import _lib
    h = _lib.lib()
    assert h.mdx_index_bytes(1004993, 2048, 2) == 62816 * (32 * 1024 + 64) + 256          # 2.06 GB
    assert h.mdx_index_bytes(8, 8, 7) == 0
    assert h.mdx_index_bytes(8, I8_MAX_D + 1, 2) == 0
    assert h.mdx_index_bytes(8, I8_MAX_D + 1, 0) > 0
    assert h.mdx_index_bytes(0, 8, 2) == 0 and h.mdx_index_bytes(8, 0, 2) == 0
    # the scores workspace is unchanged: the int8 query tiles and their scales fit in it for every d
    for nq in (1, 16, 17, 70, 129):
        for d in (1, 63, 64, 65, 100, 2048, I8_MAX_D):
            need = h.mdx_scores_workspace(nq, d)
            assert need == -(-nq // 16) * 16 * (-(-d // 64) * 64) * 4
            assert -(-nq // 16) * 16 * (-(-d // 64) * 64 + 4) <= need


def test_quantize_i8_refuses_bad_arguments():
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    assert h.mdx_quantize_i8(None, 4, 4, 1, p, p, None) == -1 and b"NULL" in h.mdx_last_error()
    assert h.mdx_quantize_i8(p, 4, 4, 1, None, p, None) == -1 and b"NULL" in h.mdx_last_error()
    assert h.mdx_quantize_i8(p, 4, 4, 1, p, None, None) == -1 and b"NULL" in h.mdx_last_error()
    assert h.mdx_quantize_i8(p, 0, 4, 1, p, p, None) == -1 and b"positive" in h.mdx_last_error()
    assert h.mdx_quantize_i8(p, 4, -1, 1, p, p, None) == -1 and b"positive" in h.mdx_last_error()
    assert h.mdx_quantize_i8(p, 4, I8_MAX_D + 1, 1, p, p, None) == -1 and b"too large" in h.mdx_last_error()
    assert h.mdx_quantize_i8(p, 4, 4, 7, p, p, None) == -1 and b"layout" in h.mdx_last_error()


def test_int8_index_refusals_before_any_device_work():
    from mdir_amd import _lib
    h = _lib.lib()
    out = ctypes.c_void_p()
    p = ctypes.c_void_p(256)
    assert h.mdx_index_create_ex(ctypes.byref(out), p, 8, I8_MAX_D + 1, 1, 0, 2, None) == -1
    assert b"too large" in h.mdx_last_error() and b"int8" in h.mdx_last_error()
    assert h.mdx_index_create_ex(ctypes.byref(out), None, 8, 8, 1, 0, 2, None) == -1 and b"NULL" in h.mdx_last_error()
    assert h.mdx_index_create_ex(ctypes.byref(out), p, 8, 8, 1, 0, 3, None) == -1 and b"storage 3" in h.mdx_last_error()
    assert h.mdx_scores_ex(None, p, 4, 1, None, p, p, 1 << 20, 1, None) == -1 and b"NULL" in h.mdx_last_error()


def test_split_modes_refuse_an_int8_shard_on_the_host():
    from mdir_amd.sharded import ShardedIndex
    for compute in ("split3", "split2"):
        with pytest.raises(ValueError, match="stored as i8"):
            ShardedIndex(None, "ND", 8, storage="i8", compute=compute)


# ------------------------------------------------------------------ criterion keys

def _score(tmp_path, **criterion):
    from mdir_amd.score import initialize_score
    (tmp_path / "db.csv").write_text("identifier\na.jpg\nb.jpg\nc.jpg\n")
    (tmp_path / "q.tsv").write_text('query\tbbx\tok\tjunk\na.jpg\t\t["b.jpg"]\t[]\n')
    dataset = {"name": "toy", "imgdir": "/img", "queries": str(tmp_path / "q.tsv"), "db": str(tmp_path / "db.csv")}
    params = {"type": "cirdatasetap", "image_size": 64, "transforms": "pil2np | totensor | normalize",
              "mean_std": [[0.4] * 3, [0.2] * 3], "dataset": dataset}
    params.update(criterion)
    return initialize_score(params)


def test_criterion_accepts_storage_i8(tmp_path):
    assert _score(tmp_path, storage="i8").storage == "i8"
    assert _score(tmp_path, storage="i8", query_expansion={"k": 2, "alpha": 3.0}).storage == "i8"


@pytest.mark.parametrize("criterion", [{"storage": "bf16"}, {"storage": "i8", "similarity": "split3"},
                                       {"storage": "i8", "similarity": "split2"}])
def test_criterion_refuses(tmp_path, criterion):
    with pytest.raises(AssertionError):
        _score(tmp_path, **criterion)


def test_int8_overlay_parses():
    import yaml
    with open(os.path.join(ROOT, "scenarios", "eval_int8.yml")) as f:
        doc = yaml.safe_load(f)
    assert doc["validation"]["247tokyo1k"]["criterion"] == {"storage": "i8"}


# ------------------------------------------------------------------ the numpy restatement is self-consistent

def test_half_way_ties_round_to_even():
    # a = 127: inv = 1 exactly, so x * inv = x; a = 254: inv = 0.5 exactly
    x = np.array([[127.0, 2.5, 3.5, -2.5, -0.5, 0.5, 1.5, -1.5, 126.5],
                  [254.0, 5.0, 7.0, -5.0, -1.0, 1.0, 3.0, -3.0, 253.0]], np.float32)
    c, s = quantize_np(x)
    want = [127, 2, 4, -2, 0, 0, 2, -2, 126]
    np.testing.assert_array_equal(c, [want, want])
    np.testing.assert_array_equal(s, np.float32([1.0, 2.0]))


def test_zero_rows_single_entries_and_extremes():
    x = np.zeros((4, 70), np.float32)
    x[1, 5] = -3.25e-3
    x[2, 69] = 7.0
    x[3, :] = np.linspace(-2.0, 2.0, 70, dtype=np.float32)
    c, s = quantize_np(x)
    assert not c[0].any() and s[0] == 0                                   # all-zero row: zero codes and scale
    assert c[1, 5] == -127 and np.count_nonzero(c[1]) == 1 and s[1] == np.float32(3.25e-3) / np.float32(127)
    assert c[2, 69] == 127 and np.count_nonzero(c[2]) == 1
    assert c[3, 0] == -127 and c[3, -1] == 127                            # +-absmax -> +-127
    assert np.abs(c.astype(np.int32)).max() <= 127
    sc = scores_np(c, s, c, s)
    assert sc[0].tolist() == [0.0] * 4 and sc[:, 0].tolist() == [0.0] * 4


def test_restated_bound_holds_on_random_rows():
    rng = np.random.default_rng(5)
    for d in (1, 63, 100, 512):
        x = rng.standard_normal((200, d)).astype(np.float32)
        x[::7] *= np.float32(1e-3)
        q = rng.standard_normal((9, d)).astype(np.float32)
        cx, sx = quantize_np(x)
        cq, sq = quantize_np(q)
        # the per-element bound ||x - scale c||_inf <= scale (1/2 + 2^-15)
        err = np.abs(x.astype(np.float64) - sx[:, None].astype(np.float64) * cx)
        assert (err <= sx[:, None].astype(np.float64) * (0.5 + E_SLOP)).all()
        s = scores_np(cq, sq, cx, sx)
        exact = q.astype(np.float64) @ x.astype(np.float64).T
        assert (np.abs(exact - s) <= error_bound(x, q, cx, sx, cq, sq, s)).all()
        # restated twice from independently ordered sums: the same bits
        perm = rng.permutation(d)
        np.testing.assert_array_equal(scores_np(cq[:, perm], sq, cx[:, perm], sx).view(np.uint32), s.view(np.uint32))
