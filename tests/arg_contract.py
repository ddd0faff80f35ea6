"""The argument contract for the tests: what lies between a caller's tensor and an abn_* call.

`guarded(lib)` wraps the entries of the loaded library object the way dirty_memory.recorded does and looks at the ctypes
arguments of every entry that is not a pure query BEFORE it forwards the call:

    block_all=True     the call is noted in log.blocked and ReachedLibrary(name) is raised: nothing is ever launched.  For
                       calls whose arguments the wrapper must refuse on its own (a wrong rank, a narrower table): the kernel
                       never sees them, whether the wrapper is right or not.
    forbidden=[(b, e)] every pointer-valued argument -- also the pointer fields, one level deep, of a ctypes Structure passed
                       by value or byref (TowerDesc, the sampler's tables) -- is compared with the byte ranges [b, e): one
                       inside raises LeakedPointer(name, argument index) and the call is not forwarded.  For mutants that
                       keep the values but not the layout or the dtype: a wrapper may convert them or refuse them, it must
                       not hand their memory to a kernel that reads it as contiguous fp32.

Both exceptions derive from Exception directly, so that no `except (ValueError, AssertionError, HipLibraryError)` mistakes
them for a wrapper's refusal.  The view builders return the same shape and values carved out of an allocation at least as
large, `wider` the same values in a dtype of at least as many bytes: a wrapper that ignored strides or dtype would still
read inside the allocation.  A plain helper module: no fixture, not a conftest."""
import contextlib
import ctypes

import numpy as np

from test_dirty_memory_host import QUERIES


class ReachedLibrary(Exception):
    def __init__(self, name):
        Exception.__init__(self, '%s was called with arguments the wrapper had to refuse' % name)
        self.name = name


class LeakedPointer(Exception):
    def __init__(self, name, index):
        Exception.__init__(self, 'argument %d of %s points into memory the kernel must not read as it stands' % (index, name))
        self.name, self.index = name, index


class Log(object):
    """What `guarded` yields: `calls` every entry forwarded, in order (queries included); `launched` those of them that are
    not queries; `blocked` the entries stopped (block_all, or a leaked pointer)."""

    def __init__(self):
        self.calls, self.launched, self.blocked = [], [], []


_BYREF = type(ctypes.byref(ctypes.c_int()))


def _field_pointers(s):
    out = []
    for field in s._fields_:
        name, ftype = field[0], field[1]
        if ftype is ctypes.c_void_p:
            out.append(getattr(s, name))
        elif isinstance(ftype, type) and issubclass(ftype, ctypes.Array) and ftype._type_ is ctypes.c_void_p:
            out.extend(getattr(s, name))
    return [int(p) for p in out if p]


def pointers_of(arg, argtype=ctypes.c_void_p):
    """The addresses `arg` hands to a parameter of `argtype`: of a pointer-valued argument its value, of a Structure (by value
    or byref) its pointer fields one level deep; nothing of integers passed for a size."""
    if arg is None:
        return []
    if isinstance(arg, ctypes.Structure):
        return _field_pointers(arg)
    if isinstance(arg, _BYREF):
        obj = arg._obj
        return _field_pointers(obj) if isinstance(obj, ctypes.Structure) else []
    if isinstance(arg, ctypes._Pointer):
        obj = arg.contents if arg else None
        return ([ctypes.addressof(obj)] + (_field_pointers(obj) if isinstance(obj, ctypes.Structure) else [])) if arg else []
    if isinstance(arg, (ctypes.c_void_p, ctypes.c_char_p)):
        return [int(arg.value)] if arg.value else []
    if argtype is not ctypes.c_void_p:
        return []
    if isinstance(arg, (int, np.integer)):
        return [int(arg)] if arg else []
    if hasattr(arg, '_as_parameter_'):
        return pointers_of(arg._as_parameter_, argtype)
    return []


def all_symbols():
    """Every entry abnet3_amd._lib binds: the numbered ABI (SYMBOLS) and the sections of abnet3_hip_next.h."""
    from abnet3_amd import _lib
    out = dict(_lib.SYMBOLS)
    for k in sorted(vars(_lib)):
        if k.startswith('NEXT') and k.endswith('_SYMBOLS'):
            out.update(getattr(_lib, k))
    return out


# the pure host functions among the entries of abnet3_hip_next.h (sizes and limits), as QUERIES lists those of the numbered ABI
NEXT_QUERIES = {
    'abnx_viterbi_dur_max', 'abny_hmm_dense_max_k', 'abny_hmm_dense_ws_bytes', 'abnz_hmm_dense_viterbi_ws_bytes',
    'abnw_hmm_dense_viterbi_dur_ws_bytes', 'abnv_hmm_hard_stats_ws_bytes', 'abnu_hmm_hsmm_max_duration',
    'abnu_hmm_hsmm_viterbi_ws_bytes', 'abnt_nce_max_d', 'abnt_nce_ws_bytes',
}


def _inside(p, ranges):
    return any(b <= p < e for b, e in ranges)


@contextlib.contextmanager
def guarded(lib, forbidden=(), block_all=False, allow=QUERIES):
    allow = set(allow) | NEXT_QUERIES
    forbidden = [(int(b), int(e)) for b, e in forbidden]
    log, saved = Log(), {}

    def wrap(name, fn, argtypes):
        def query(*args):
            log.calls.append(name)
            return fn(*args)

        def entry(*args):
            if block_all:
                log.blocked.append(name)
                raise ReachedLibrary(name)
            for i, arg in enumerate(args):
                if any(_inside(p, forbidden) for p in pointers_of(arg, argtypes[i] if i < len(argtypes) else ctypes.c_void_p)):
                    log.blocked.append(name)
                    raise LeakedPointer(name, i)
            log.calls.append(name)
            log.launched.append(name)
            return fn(*args)
        return query if name in allow else entry

    for name, (_, argtypes) in all_symbols().items():
        fn = getattr(lib, name)
        saved[name] = fn
        setattr(lib, name, wrap(name, fn, argtypes))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


# ----------------------------------------------------------------------------------------------------------------------
# views and dtypes that keep the values
# ----------------------------------------------------------------------------------------------------------------------
def _is_np(t):
    return isinstance(t, np.ndarray)


def _zeros(t, shape):
    return np.zeros(shape, dtype=t.dtype) if _is_np(t) else t.new_zeros(shape)


def _contiguous(t):
    return t.flags['C_CONTIGUOUS'] if _is_np(t) else t.is_contiguous()


def same_values(v, t):
    """Element for element equal, a NaN equal to a NaN."""
    if _is_np(v):
        return bool(np.array_equal(v, t, equal_nan=v.dtype.kind == 'f'))
    both_nan = (v != v) & (t != t)
    return bool(((v == t) | both_nan).all())


def _checked(v, t):
    assert tuple(v.shape) == tuple(t.shape) and v.dtype == t.dtype and not _contiguous(v), (tuple(v.shape), v.dtype)
    assert same_values(v, t)
    lo, hi = span(v)
    assert hi - lo >= (t.nbytes if _is_np(t) else t.numel() * t.element_size())
    return v


def strided_cols(t):
    """[rows, D]: every second column of a [rows, 2 D] base."""
    assert t.ndim == 2 and t.shape[1] > 0 and t.shape[0] > 0
    base = _zeros(t, (t.shape[0], 2 * t.shape[1]))
    base[:, ::2] = t
    return _checked(base[:, ::2], t)


def transposed(t):
    """[rows, D]: the transpose of a [D, rows] base."""
    assert t.ndim == 2 and t.shape[0] > 1 and t.shape[1] > 1
    base = _zeros(t, (t.shape[1], t.shape[0]))
    if _is_np(t):
        base[...] = t.T
        return _checked(base.T, t)
    base.copy_(t.t())
    return _checked(base.t(), t)


def strided_rows(t):
    """[n, ...]: every second row of a [2 n, ...] base."""
    assert t.ndim >= 1 and t.shape[0] > 1
    base = _zeros(t, (2 * t.shape[0],) + tuple(t.shape[1:]))
    base[::2] = t
    return _checked(base[::2], t)


def _wider_table():
    import torch
    return {torch.float32: torch.float64, torch.int32: torch.int64, torch.uint8: torch.int32, torch.int64: torch.float64,
            np.dtype(np.float32): np.dtype(np.float64), np.dtype(np.int32): np.dtype(np.int64),
            np.dtype(np.uint8): np.dtype(np.int32), np.dtype(np.int64): np.dtype(np.float64)}


def wider(t):
    """The same values in a dtype of at least as many bytes (never fewer: a wrapper that handed the raw pointer on would make
    the kernel read past the allocation); None for a dtype that has no such partner here."""
    to = _wider_table().get(t.dtype)
    if to is None:
        return None
    w = t.astype(to) if _is_np(t) else t.to(to)
    assert tuple(w.shape) == tuple(t.shape) and _contiguous(w)
    assert (w.itemsize if _is_np(w) else w.element_size()) >= (t.itemsize if _is_np(t) else t.element_size())
    back = w.astype(t.dtype) if _is_np(t) else w.to(t.dtype)
    assert same_values(back, t)
    return w


def span(t):
    """[begin, end): the bytes of the whole allocation `t` lives in (a view's base, a tensor's storage)."""
    if _is_np(t):
        root = t
        while isinstance(root.base, np.ndarray):
            root = root.base
        return root.ctypes.data, root.ctypes.data + max(root.nbytes, 1)
    st = t.untyped_storage()
    return st.data_ptr(), st.data_ptr() + max(st.nbytes(), 1)
