"""The guard-band harness (tests/memguard.py) catches what it is for: seven numpy "kernels" over arena views, each wrong
in one way, are rejected by the contract runner with the buffer named, and the correct one passes.  No GPU here.  Also:
every function include/mdx.h declares is either in the coverage table of test_gpu_memcontract.py or in the fixed list of
entry points the memory contract does not apply to."""
import types

import numpy as np
import pytest
import torch

import memguard
from test_cabi import _declared

# A stand-in for mdir_amd/ops.py: it allocates through the names ``torch`` and ``_workspace`` of its own module, which is
# all ``memguard.guarded`` relies on.  ``double_and_sum``: out = 2 x, total = sum(x) accumulated in a workspace counter.
# An out-of-bounds access is made only where the tensor's storage has room for it -- as on the device, where the overrun
# lands in a neighbour's block: under ordinary allocations nothing is seen (and a fresh workspace block holds zeros).
_FAKE_OPS = '''
import numpy as np
import torch


def double_and_sum_workspace(n):
    return 8 + 4 * n            # a counter (int64) and n partial values


def _workspace(nbytes, device):
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _beyond(t, first, count):
    """numpy view of ``count`` elements of ``t``'s storage starting ``first`` elements from t[0], or None without room."""
    lo = t.storage_offset() + first
    if lo < 0 or (lo + count) * t.element_size() > t.untyped_storage().nbytes():
        return None
    return t.as_strided((count,), (1,), lo).numpy()


def double_and_sum(x, flaw=None):
    n = x.numel()
    out = torch.empty(n, dtype=torch.int32, device=x.device)
    total = torch.empty(1, dtype=torch.int64, device=x.device)
    need = double_and_sum_workspace(n)
    ws = _workspace(need, x.device)
    xs, o = x.numpy(), out.numpy()
    counter = ws[:8].view(torch.int64).numpy()
    partial = ws[8:8 + 4 * n].view(torch.int32).numpy()
    if flaw != "counter":
        counter[0] = 0
    partial[:] = xs
    counter[0] += int(partial.astype(np.int64).sum())
    if flaw == "tail":
        extra = _beyond(x, n, 1)
        counter[0] += 0 if extra is None else int(extra[0])
    # under ordinary allocations the caching allocator hands back the block the previous, identical call filled
    keep = o[n // 2] if _beyond(out, n, 1) is not None else 2 * xs[n // 2]
    o[:] = 2 * xs
    if flaw == "unwritten":
        o[n // 2] = keep
    total.numpy()[0] = counter[0]
    if flaw == "past":
        extra = _beyond(out, n, 1)
        if extra is not None:
            extra[0] = 7
    if flaw == "before":
        extra = _beyond(out, -1, 1)
        if extra is not None:
            extra[0] = 7
    if flaw == "ws_more":
        extra = _beyond(ws, need, 8)
        if extra is not None:
            extra[:] = 1
    if flaw == "input":
        xs[1] += 1
    return out, total
'''


def _fake_ops():
    mod = types.ModuleType("fake_memguard_ops")
    exec(compile(_FAKE_OPS, "fake_memguard_ops", "exec"), mod.__dict__)
    return mod


def _case(n, flaw=None, seed=0, larger=None):
    data = np.random.default_rng(seed + n).integers(-1000, 1000, n).astype(np.int32)

    def run(env):
        out, total = env.ops.double_and_sum(env.put("x", data), flaw)
        return {"out": out, "total": total}

    def verify(outs):
        np.testing.assert_array_equal(outs["out"], 2 * data, err_msg="output 'out'")
        np.testing.assert_array_equal(outs["total"], [data.astype(np.int64).sum()], err_msg="output 'total'")

    return memguard.Case("double_and_sum(n=%d, flaw=%s)" % (n, flaw), run, verify, aligns={"ws0": 8}, larger=larger)        # the counter is an int64


def test_the_correct_kernel_passes_every_run():
    ops = _fake_ops()
    runs = []
    memguard.run_contract(ops, _case(37, larger=_case(101)), "cpu", log=runs.append)
    assert runs[:6] == ["baseline", "guards", "prefill", "stale", "tails", "align x@4: same bits"]
    assert runs[-1].startswith("align ") and "x@4" in runs[-1] and "out0@4" in runs[-1] and "ws0@8" in runs[-1]
    assert ops.torch is torch                   # the swap was undone


@pytest.mark.parametrize("flaw,names", [
    ("past", r"guard after buffer 'out0' .*offset 0 relative to the buffer's end"),
    ("before", r"guard before buffer 'out0' .*offset -4 relative to the buffer's start"),
    ("ws_more", r"guard after buffer 'ws0' \(workspace, 156 bytes\)"),
    ("counter", r"workspace 'ws0' is read before the library initialises it"),
    ("unwritten", r"an element of 'out' is left unwritten"),
    ("input", r"input 'x' was modified: first at byte 4 \(element 1\)"),
    ("tail", r"bytes after input 'x'"),
])
def test_each_wrong_kernel_is_rejected_with_the_buffer_named(flaw, names):
    ops = _fake_ops()
    with pytest.raises(AssertionError, match=names):
        memguard.run_contract(ops, _case(37, flaw, larger=_case(101, flaw)), "cpu")
    assert ops.torch is torch


def test_a_refusal_at_a_legal_alignment_is_a_violation():
    """Run 5 puts every pointer where the header says it may lie: a ValueError there fails the contract, naming the buffer,
    unless the case lists that buffer in ``may_refuse``."""
    ops = _fake_ops()
    plain = ops.double_and_sum

    def strict(x, flaw=None):
        if x.data_ptr() % 16:
            raise ValueError("x must be 16-byte aligned")
        return plain(x, flaw)
    ops.double_and_sum = strict
    with pytest.raises(memguard.ContractViolation, match=r"refused with ValueError at an alignment the header calls legal \(x@4\): buffer 'x'"):
        memguard.run_contract(ops, _case(37), "cpu")
    allowed = _case(37)
    allowed.may_refuse = frozenset(["x"])
    runs = []
    memguard.run_contract(ops, allowed, "cpu", log=runs.append)
    assert "align x@4: refused" in runs and runs[-1].endswith("refused")


def test_arena_buffers_are_exact_and_exactly_aligned():
    arena = memguard.Arena("cpu")
    for align in (4, 8, 16, 64, 256):
        t = arena.empty((3, 5), torch.float32, "t%d" % align, 0xFF, align)
        assert t.data_ptr() % 512 == align and t.shape == (3, 5) and bool(torch.isnan(t).all())
    z = arena.empty((7,), torch.int64, "z", 0x00, 8)
    assert z.data_ptr() % 16 == 8 and int(z.abs().sum()) == 0
    p = arena.put(np.arange(5, dtype=np.float64), 8, 0x00, "p")
    assert p.data_ptr() % 16 == 8 and p.tolist() == [0, 1, 2, 3, 4]
    wide = arena.empty((2, 40000), torch.float32, "wide", 0x00)
    assert arena.buffers[-1].guard >= 16 * 40000 * 4 and all(b.guard >= 64 * 1024 for b in arena.buffers)
    arena.check()
    arena.check_inputs()
    wide.as_strided((1,), (1,), wide.storage_offset() + wide.numel() + 16 * 40000 - 1).fill_(1.0)     # the last float of row 16 past the end
    with pytest.raises(memguard.ContractViolation, match="after buffer 'wide'"):
        arena.check()


def test_guarded_zeros_are_zeros_and_other_devices_pass_through():
    ops = _fake_ops()
    arena = memguard.Arena("cpu")
    with memguard.guarded(ops, arena, fill_out=0xFF):
        z = ops.torch.zeros(5, dtype=torch.int64, device="cpu")
        e = ops.torch.empty((2, 3), dtype=torch.int32, device=torch.device("cpu"))
        plain = ops.torch.empty(4)                          # no device given: not an output of a wrapper
        assert ops.torch.float32 is torch.float32
    assert z.tolist() == [0] * 5 and e.tolist() == [[-1] * 3] * 2 and len(arena.buffers) == 2 and plain.shape == (4,)
    assert [b.name for b in arena.buffers] == ["out0", "out1"]


# ------------------------------------------------------------- header coverage

# Fixed by the issue this layer was built for: host-only code, handles, peer / IPC memory of rank processes, and the size
# functions (exercised by being believed: every workspace in the contract is exactly as large as they say).
EXCLUDED = {
    "mdx_abi_version", "mdx_last_error", "mdx_capture_recover", "mdx_jpeg_probe", "mdx_jpeg_coefficients",
    "mdx_index_destroy", "mdx_index_info", "mdx_index_bytes", "mdx_query_bounds", "mdx_rank_route", "mdx_topk_route",
    "mdx_comm_unique_id", "mdx_comm_init", "mdx_comm_destroy", "mdx_comm_info",
    "mdx_allgather_scores", "mdx_exchange_scores", "mdx_scores_p2p",
    "mdx_p2p_create", "mdx_p2p_connect", "mdx_p2p_connect_ptrs", "mdx_p2p_base", "mdx_p2p_bytes", "mdx_p2p_close_step",
    "mdx_p2p_status", "mdx_p2p_destroy",
}


def test_every_declared_entry_point_is_covered_or_excluded():
    from test_gpu_memcontract import TABLE
    declared = set(_declared())
    sizes = {n for n in declared if "_workspace" in n}
    excluded = EXCLUDED | sizes
    assert len(declared) == 86 and len(sizes) == 13 and len(excluded) == 39 and excluded <= declared
    covered = {"mdx_" + name for name in TABLE}
    assert not covered & excluded, sorted(covered & excluded)
    assert covered | excluded == declared, "not covered: %s; unknown: %s" % (sorted(declared - covered - excluded), sorted(covered - declared))
    assert len(covered) == 47 and all(TABLE[name] for name in TABLE)
