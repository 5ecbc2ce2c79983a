"""Guard bands and poison for the memory contract of the C ABI (a helper module, imported by test_memguard_host.py and
test_gpu_memcontract.py; it works on CPU tensors as well as on the device).

What the value tests cannot see is what a kernel reads and writes outside the numbers it returns.  Here every buffer a
call touches -- inputs, outputs, workspaces -- is a view into an allocation of its own laid out as

    [ front guard | buffer | back guard ]

with the buffer holding EXACTLY the requested bytes at EXACTLY the requested alignment (an address that is ``align`` modulo
512, so "4" is 4 mod 16 and never a coarser boundary), the guards filled with 0xA5 (an input's back guard with the poison
of its ``tail``: 0xFF or 0x00) and the buffer itself pre-filled with 0x00, 0xFF (NaN as f16 / f32 / f64, -1 as an integer)
or the stale bytes an earlier, differently shaped call left.

Guard size, per side and per buffer: at least 64 KiB (a 4096-element tile of 16-byte sort records; 16 rows of a 1024-float
matrix), and at least 16 rows of the buffer where it has two or more dimensions (the 16-row x 16/128-query score tiles
store whole rows, so a padded tile lands inside).  AN OVERRUN BEYOND A GUARD IS NOT SEEN: it falls into memory this module
does not own.  The guards catch the tail stores and the one-tile-too-far stores, not a wild pointer.

``run_contract`` is the contract itself: one case, executed under ordinary allocations and then under guards with different
pre-fills, input tails and alignments; every run must return the same bits and leave guards and inputs alone.
"""
import contextlib

import numpy as np
import torch

GUARD_BYTE = 0xA5
MIN_GUARD = 64 * 1024
GUARD_ROWS = 16
_MODULUS = 512                  # the alignment of a fresh torch device block: "align" means ``address % 512 == align``
DEFAULT_ALIGN = 256


REFUSALS = (ValueError,)        # MDX_ERR_INVALID / MDX_ERR_WORKSPACE reach Python as ValueError (mdir_amd._lib.check)


class ContractViolation(AssertionError):
    """A run of the contract disagreed; the message names the buffer."""


def _nbytes(shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return n * torch.empty(0, dtype=dtype).element_size()


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class _Buffer:
    def __init__(self, name, role, raw, off, nbytes, guard, back_byte):
        self.name, self.role, self.raw, self.off, self.nbytes, self.guard, self.back_byte = name, role, raw, off, nbytes, guard, back_byte
        self.tensor = None
        self.uploaded = None            # inputs: the bytes that were put there
        self.itemsize = 1

    def bytes(self):
        return self.raw[self.off:self.off + self.nbytes]


class Arena:
    """Hands out guarded tensors on ``device`` and checks the guards afterwards."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buffers = []
        self.stale = {}                 # ``snapshot()`` of an earlier arena: the pre-fill of ``fill="stale"``

    # ------------------------------------------------------------ allocation
    def _alloc(self, name, role, shape, dtype, align, back_byte=GUARD_BYTE):
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty(0, dtype=dtype).element_size()
        nbytes = _nbytes(shape, dtype)
        align = int(align)
        if align < itemsize or align > _MODULUS // 2 or align & (align - 1):
            raise ValueError("%s: alignment %d (a power of two in [%d, %d])" % (name, align, itemsize, _MODULUS // 2))
        row = shape[-1] * itemsize if len(shape) >= 2 else 0
        guard = max(MIN_GUARD, GUARD_ROWS * row)
        guard = -(-guard // _MODULUS) * _MODULUS
        raw = torch.empty(2 * guard + nbytes + 2 * _MODULUS, dtype=torch.uint8, device=self.device)
        raw.fill_(GUARD_BYTE)
        off = guard + (align - (raw.data_ptr() + guard)) % _MODULUS      # the first address >= base + guard that is ``align`` mod 512
        assert (raw.data_ptr() + off) % _MODULUS == align and off + nbytes + guard <= raw.numel()
        buf = _Buffer(name, role, raw, off, nbytes, guard, back_byte)
        buf.itemsize = itemsize
        if back_byte != GUARD_BYTE:
            raw[off + nbytes:].fill_(back_byte)
        buf.tensor = buf.bytes().view(dtype).view(shape) if nbytes else torch.empty(shape, dtype=dtype, device=self.device)
        self.buffers.append(buf)
        return buf

    def empty(self, shape, dtype, name, fill=0xFF, align=DEFAULT_ALIGN, role="output"):
        """A guarded, pre-filled tensor.  ``fill``: 0x00, 0xFF, a uint8 array of stale bytes, or "stale": what the buffer of this
        name -- else the buffer of this role and position -- held in the arena ``self.stale`` was snapshot from (shorter than
        the buffer, or none: the rest is 0xFF)."""
        if isinstance(fill, str):
            nth = sum(1 for b in self.buffers if b.role == role)
            fill = self.stale.get(name, self.stale.get((role, nth), 0xFF))
        buf = self._alloc(name, role, shape, dtype, align)
        dst = buf.bytes()
        if isinstance(fill, int):
            dst.fill_(fill)
        else:
            stale = torch.as_tensor(np.asarray(fill, dtype=np.uint8)).to(self.device)
            dst.fill_(0xFF)
            k = min(stale.numel(), dst.numel())
            dst[:k].copy_(stale[:k])
        return buf.tensor

    def put(self, array, align=DEFAULT_ALIGN, tail=0xFF, name="input"):
        """An input: ``array`` copied into the arena at ``align``; the bytes after it are ``tail`` (0xFF or 0x00), not 0xA5."""
        array = np.ascontiguousarray(array)
        dtype = torch.from_numpy(np.empty(0, dtype=array.dtype)).dtype
        buf = self._alloc(name, "input", array.shape, dtype, align, back_byte=tail)
        flat = torch.from_numpy(array.reshape(-1).view(np.uint8).copy())
        buf.bytes().copy_(flat.to(self.device))
        buf.uploaded = flat
        return buf.tensor

    # ---------------------------------------------------------------- checks
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check(self):
        """Synchronises; every guard byte must be untouched.  Names the buffer and the first damaged offset."""
        self._sync()
        for b in self.buffers:
            front = b.raw[:b.off]
            back = b.raw[b.off + b.nbytes:]
            for side, region, byte in (("before", front, GUARD_BYTE), ("after", back, b.back_byte)):
                bad = region != byte
                if bool(bad.any()):
                    first = int(bad.nonzero()[0])
                    where = first if side == "after" else first - b.off
                    raise ContractViolation("guard %s buffer %r (%s, %d bytes) damaged: first at byte offset %d relative to the buffer's %s"
                                            % (side, b.name, b.role, b.nbytes, where, "end" if side == "after" else "start"))

    def check_inputs(self, except_for=()):
        """Every input still holds the bytes that were uploaded (``except_for``: names documented as updated in place)."""
        self._sync()
        for b in self.buffers:
            if b.role != "input" or b.name in except_for:
                continue
            now = b.bytes().cpu()
            if not torch.equal(now, b.uploaded):
                first = int((now != b.uploaded).nonzero()[0])
                raise ContractViolation("input %r was modified: first at byte %d (element %d)" % (b.name, first, first // b.itemsize))

    def snapshot(self, roles=("workspace", "output")):
        """The bytes of every buffer of the given roles as they are now, by name and by (role, position): the stale pre-fill
        of a later run."""
        self._sync()
        snap, nth = {}, {}
        for b in self.buffers:
            if b.role in roles:
                snap[b.name] = snap[(b.role, nth.get(b.role, 0))] = b.bytes().cpu().numpy().copy()
                nth[b.role] = nth.get(b.role, 0) + 1
        return snap

    def names(self, roles=("input", "output", "workspace")):
        return [(b.name, b.itemsize) for b in self.buffers if b.role in roles]


class _TorchProxy:
    """``torch`` as one module sees it: everything forwarded, the allocation functions taken from an arena."""

    def __init__(self, real, hook):
        self.__dict__["_real"] = real
        self.__dict__["_hook"] = hook

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _wanted(self, device):
        return device is not None and torch.device(device).type == self._hook.arena.device.type

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._wanted(device):
            return self._real.empty(*size, dtype=dtype, device=device, **kw)
        return self._hook.output(_shape_of(size), dtype or torch.float32, zero=False)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._wanted(device):
            return self._real.zeros(*size, dtype=dtype, device=device, **kw)
        return self._hook.output(_shape_of(size), dtype or torch.float32, zero=True)

    def empty_like(self, t, **kw):
        if not self._wanted(t.device) or kw:
            return self._real.empty_like(t, **kw)
        return self._hook.output(tuple(t.shape), t.dtype, zero=False)

    def zeros_like(self, t, **kw):
        if not self._wanted(t.device) or kw:
            return self._real.zeros_like(t, **kw)
        return self._hook.output(tuple(t.shape), t.dtype, zero=True)


class _Hook:
    def __init__(self, arena, fill_out, fill_ws, align, stale):
        self.arena, self.fill_out, self.fill_ws, self.align = arena, fill_out, fill_ws, align
        if stale:
            arena.stale, self.fill_out, self.fill_ws = stale, "stale", "stale"
        self.n_out = self.n_ws = 0

    def _align(self, name, itemsize):
        a = self.align.get(name, self.align.get("*", DEFAULT_ALIGN)) if isinstance(self.align, dict) else self.align
        return max(int(a), itemsize)

    def output(self, shape, dtype, zero):
        name = "out%d" % self.n_out
        self.n_out += 1
        fill = 0x00 if zero else self.fill_out
        return self.arena.empty(shape, dtype, name, fill, self._align(name, torch.empty(0, dtype=dtype).element_size()))

    def workspace(self, nbytes, device):
        name = "ws%d" % self.n_ws
        self.n_ws += 1
        return self.arena.empty((max(int(nbytes), 16),), torch.uint8, name, self.fill_ws, self._align(name, 1), role="workspace")


@contextlib.contextmanager
def guarded(ops_module, arena, fill_out=0xFF, fill_ws=0xFF, align=DEFAULT_ALIGN, stale=None):
    """Inside, the wrappers of ``ops_module`` take their outputs (``torch.empty`` / ``empty_like`` / ``zeros``, which still
    returns zeros) and their workspaces (``_workspace``) from ``arena``: outputs are named ``out0, out1, ...`` and workspaces
    ``ws0, ws1, ...`` in the order the wrapper asks for them.  Only the names ``torch`` and ``_workspace`` AS SEEN FROM THAT
    MODULE are swapped; both are put back on exit.  ``align``: one number, or ``{buffer name: alignment, "*": default}``.
    ``stale``: ``{buffer name: bytes}`` of an earlier run (``Arena.snapshot``) used as the pre-fill."""
    hook = _Hook(arena, fill_out, fill_ws, align, stale)
    real_torch, real_ws = ops_module.torch, getattr(ops_module, "_workspace", None)
    ops_module.torch = _TorchProxy(real_torch, hook)
    if real_ws is not None:
        ops_module._workspace = hook.workspace
    try:
        yield hook
    finally:
        ops_module.torch = real_torch
        if real_ws is not None:
            ops_module._workspace = real_ws


# ------------------------------------------------------------------ the contract

class Case:
    """One call of one entry point.

    ``run(env) -> {name: tensor or ndarray}``: builds host inputs (from a seed of its own), uploads them with
    ``env.put(name, array)``, calls the wrapper (``env.ops``) and returns the outputs' DEFINED extent (a list whose order
    comes from an atomic is returned sorted).  Caller-allocated outputs / workspaces come from ``env.empty(name, shape,
    dtype)`` / ``env.workspace(name, nbytes)``.
    ``verify(outs)``: compares the numpy outputs of the baseline run with the oracle, at the tolerance of the entry point's
    existing test.  ``inplace``: inputs the header documents as updated in place.  ``aligns``: ``{buffer name: bytes}`` where
    the header asks for more than the element size (``workspace_align``: of every workspace).  ``may_refuse``: buffer names
    for which a ValueError at that alignment is an accepted answer of run 5; for every other buffer the alignment is one the
    header calls legal, and a refusal there is a violation.  ``larger``: a case of the same entry point and a bigger shape whose
    leftovers are the stale pre-fill."""

    def __init__(self, name, run, verify, inplace=(), aligns=None, larger=None, workspace_align=1, may_refuse=()):
        self.name, self.run, self.verify, self.inplace, self.aligns, self.larger = name, run, verify, tuple(inplace), dict(aligns or {}), larger
        self.workspace_align = workspace_align          # what the header asks of every workspace pointer
        self.may_refuse = frozenset(may_refuse)         # buffers whose minimal alignment the entry point may refuse (none, normally)


class _Env:
    def __init__(self, ops_module, device, arena=None, hook=None, align=DEFAULT_ALIGN, tail=0xFF, tails=None, fill_out=0xFF, fill_ws=0xFF,
                 stale=None):
        self.ops, self.device, self.arena, self.hook = ops_module, torch.device(device), arena, hook
        self.align, self.tail, self.tails = align, tail, tails or {}
        self.fill_out, self.fill_ws = ("stale", "stale") if stale else (fill_out, fill_ws)

    def _align(self, name, itemsize):
        a = self.align.get(name, self.align.get("*", DEFAULT_ALIGN)) if isinstance(self.align, dict) else self.align
        return max(int(a), itemsize)

    def put(self, name, array):
        array = np.ascontiguousarray(array)
        if self.arena is None:
            return torch.from_numpy(array.copy()).to(self.device)
        return self.arena.put(array, self._align(name, array.dtype.itemsize), self.tails.get(name, self.tail), name)

    def empty(self, name, shape, dtype):
        if self.arena is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return self.arena.empty(shape, dtype, name, self.fill_out, self._align(name, torch.empty(0, dtype=dtype).element_size()))

    def workspace(self, name, nbytes):
        if self.arena is None:
            return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
        return self.arena.empty((max(int(nbytes), 16),), torch.uint8, name, self.fill_ws, self._align(name, 1), role="workspace")


def _host(outs):
    res = {}
    for k, v in outs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().contiguous().numpy()
        res[k] = np.ascontiguousarray(v).copy()
    return res


def _differs(a, b):
    """None, or (name, what) of the first output whose bits differ."""
    for k in a:
        if k not in b:
            return k, "is missing"
        if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
            return k, "has shape %s %s, not %s %s" % (b[k].shape, b[k].dtype, a[k].shape, a[k].dtype)
        x, y = a[k].reshape(-1).view(np.uint8), b[k].reshape(-1).view(np.uint8)
        if not np.array_equal(x, y):
            first = int(np.flatnonzero(x != y)[0]) // a[k].dtype.itemsize
            return k, "differs in %d of %d elements, first at flat index %d (%r, not %r)" % (
                int((a[k].reshape(-1) != b[k].reshape(-1)).sum()) or 1, a[k].size, first, b[k].reshape(-1)[first], a[k].reshape(-1)[first])
    return None


def _guarded_run(ops_module, case, device, **kw):
    arena = Arena(device)
    with guarded(ops_module, arena, kw.get("fill_out", 0xFF), kw.get("fill_ws", 0xFF), kw.get("align", DEFAULT_ALIGN), kw.get("stale")) as hook:
        env = _Env(ops_module, device, arena, hook, **kw)
        outs = _host(case.run(env))
    arena.check()
    arena.check_inputs(case.inplace)
    return outs, arena


def workspace_names(ops_module, case, device):
    """Names of the workspaces one guarded run of ``case`` takes."""
    _, arena = _guarded_run(ops_module, case, device)
    return [n for n, _ in arena.names(("workspace",))]


def _run_or_refusal(ops_module, case, device, align):
    """The outputs of ``case`` with its buffers at ``align``, or None when the call is refused with ValueError; either way no
    guard is touched and no input modified."""
    arena = Arena(device)
    outs = None
    with guarded(ops_module, arena, align=align) as hook:
        try:
            outs = _host(case.run(_Env(ops_module, device, arena, hook, align=align)))
        except REFUSALS:
            pass
    arena.check()
    arena.check_inputs(case.inplace)
    return outs


def refuses(ops_module, case, device, align):
    """True when ``case`` with its buffers at ``align`` (``{buffer name: alignment}``, the rest at 256) is refused with ValueError."""
    return _run_or_refusal(ops_module, case, device, dict(align, **{"*": DEFAULT_ALIGN})) is None


def _same(case, what, want, got, blame):
    d = _differs(want, got)
    if d is not None:
        raise ContractViolation("%s: %s: output %r %s -- %s" % (case.name, what, d[0], d[1], blame))


def run_contract(ops_module, case, device, alignment_run=True, log=None):
    """The five runs of the memory contract for one case; raises ``ContractViolation`` naming the buffer.  ``log``: a callable
    that is told every run made.  Returns the outputs of run 2."""
    say = log or (lambda s: None)
    # 1. baseline: ordinary allocations equal the oracle
    base = _host(case.run(_Env(ops_module, device)))
    case.verify(base)
    say("baseline")
    # 2. guards, exact sizes, 256-byte alignment, everything the call writes pre-filled 0xFF
    ref, arena = _guarded_run(ops_module, case, device)

    def tails(ref):
        """Raises if the bytes after an input reach the result, naming the input."""
        outs, _ = _guarded_run(ops_module, case, device, tail=0x00)
        if _differs(ref, outs) is None:
            return
        for name, _ in arena.names(("input",)):
            one, _ = _guarded_run(ops_module, case, device, tails={name: 0x00})
            d = _differs(ref, one)
            if d is not None:
                raise ContractViolation("%s: output %r %s when the bytes after input %r are 0x00 instead of 0xFF: a load past the end "
                                        "of %r reaches the result" % (case.name, d[0], d[1], name, name))
        _same(case, "input tails 0x00", ref, outs, "loads past the end of several inputs reach the result")

    # (a difference from the baseline is reported after runs 3 and 4, which can say which buffer is to blame)
    pointers = arena.names()
    ws_floor = {n: case.workspace_align for n, _ in arena.names(("workspace",))}
    say("guards")
    # 3. pre-fill 0x00 of the outputs, of the workspaces, and stale contents of a larger call
    outs, _ = _guarded_run(ops_module, case, device, fill_out=0x00)
    d = _differs(ref, outs)
    if d is not None:
        raise ContractViolation("%s: output %r %s between an output pre-fill of 0xFF and of 0x00: an element of %r is left unwritten "
                                "(or an output is read before it is written)" % (case.name, d[0], d[1], d[0]))
    ws_names = [n for n, _ in arena.names(("workspace",))]
    outs, _ = _guarded_run(ops_module, case, device, fill_ws=0x00)
    _same(case, "workspace pre-filled 0x00 instead of 0xFF", ref, outs,
          "workspace %s is read before the library initialises it" % ", ".join(repr(n) for n in ws_names))
    say("prefill")
    if case.larger is not None:
        _, big = _guarded_run(ops_module, case.larger, device)
        outs, _ = _guarded_run(ops_module, case, device, stale=big.snapshot())
        _same(case, "buffers left by the larger call %r" % case.larger.name, ref, outs,
              "workspace %s (or an output) keeps state from an earlier call" % ", ".join(repr(n) for n in ws_names))
        say("stale")
    # 4. the bytes after every input 0x00 instead of 0xFF
    tails(ref)
    say("tails")
    _same(case, "guards + exact sizes (pre-fill 0xFF)", base, ref, "the result depends on what lies in or around its buffers")
    # 5. every caller pointer at the smallest alignment the header allows: one at a time, then all together
    if alignment_run:
        least = {n: max(isz, case.aligns.get(n, 1), ws_floor.get(n, 1)) for n, isz in pointers}
        trials = [{n: a, "*": DEFAULT_ALIGN} for n, a in least.items() if a < DEFAULT_ALIGN]
        trials.append(dict(least, **{"*": DEFAULT_ALIGN}))
        for align in trials:
            which = ", ".join("%s@%d" % (n, a) for n, a in align.items() if n != "*")
            outs = _run_or_refusal(ops_module, case, device, align)
            if outs is None:
                moved = {n for n in align if n != "*"}
                if not moved & case.may_refuse:
                    raise ContractViolation("%s: refused with ValueError at an alignment the header calls legal (%s): buffer %s"
                                            % (case.name, which, ", ".join(repr(n) for n in sorted(moved))))
                say("align %s: refused" % which)
                continue
            _same(case, "pointers at their minimal alignment (%s)" % which, ref, outs, "the result depends on where a buffer lies")
            say("align %s: same bits" % which)
    return ref
