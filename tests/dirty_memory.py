"""Dirty memory for the tests: while `dirty(byte)` is open, torch.empty and torch.empty_like hand out memory whose every byte
is `byte`, so a kernel that reads a word of an output or a workspace before it wrote it, or leaves a ragged tile of its
output unwritten, computes something else than it does on the zero pages a fresh process gets.  torch.zeros, torch.full and
the rest are left alone: memory the header says the caller must zero stays zero.

    0x00   the deterministic "clean" run
    0xFF   NaN as fp32 / fp64, -1 as int32 / int64
    0xC2   a finite, plausible fp32 (about -97.38), a finite fp64, a negative int32

The window must never be open during a hipGraph capture (the fills would become graph nodes).

`recorded(lib)` wraps the abn_* attributes of the loaded library object for a while and records which entries were called,
so a case can prove that it reached the entries it claims.  A plain helper module: no fixture, not a conftest."""
import contextlib

import torch

PATTERNS = (0x00, 0xFF, 0xC2)


class Count(object):
    """What `dirty` yields: the number of allocations it filled, and their bytes."""

    def __init__(self):
        self.n = 0
        self.nbytes = 0

    def __int__(self):
        return self.n

    def __repr__(self):
        return 'Count(n=%d, nbytes=%d)' % (self.n, self.nbytes)


def fill_bytes(t, byte):
    """Every byte of the memory `t` covers := byte, through a flat uint8 view (any dtype, 0-dim, pinned, CPU or device).  A
    fresh allocation that is dense but not contiguous (empty_like of a permuted tensor) is filled through its storage, which
    it owns alone."""
    if t.numel() == 0:
        return t
    t = t.detach()
    if t.is_contiguous():
        flat = t.reshape(-1).view(torch.uint8)
    else:
        flat = torch.zeros(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    flat.fill_(byte)
    return t


@contextlib.contextmanager
def dirty(byte):
    assert 0 <= byte <= 0xFF
    count = Count()
    empty, empty_like = torch.empty, torch.empty_like

    def poison(t):
        if isinstance(t, torch.Tensor) and t.numel() > 0:
            fill_bytes(t, byte)
            count.n += 1
            count.nbytes += t.numel() * t.element_size()
        return t

    def dirty_empty(*args, **kwargs):
        return poison(empty(*args, **kwargs))

    def dirty_empty_like(*args, **kwargs):
        return poison(empty_like(*args, **kwargs))

    torch.empty, torch.empty_like = dirty_empty, dirty_empty_like
    try:
        yield count
    finally:
        torch.empty, torch.empty_like = empty, empty_like


@contextlib.contextmanager
def recorded(lib):
    """Yields the list of abn_* entries called through `lib` (abnet3_amd._lib.load()) while the block runs, in call order."""
    from abnet3_amd import _lib
    calls, saved = [], {}

    def wrap(name, fn):
        def call(*args):
            calls.append(name)
            return fn(*args)
        return call

    for name in _lib.SYMBOLS:
        fn = getattr(lib, name)
        saved[name] = fn
        setattr(lib, name, wrap(name, fn))
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def bits(a):
    """An array's bytes as unsigned integers of its item size: NaN compares equal to the same NaN."""
    import numpy as np
    a = np.ascontiguousarray(a)
    if a.dtype.kind in 'iub':
        return a
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
