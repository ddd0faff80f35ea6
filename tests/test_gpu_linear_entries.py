"""The five single-Linear entries (abn_linear_forward / _dgrad / _wgrad / _backward / _backward_prec) against float64
matmuls, on every GEMM tile (ABN_GEMM_TILE forces 128x128, 128x64, 64x128, 64x64: the dispatcher alone picks 64x64 at
every shape small enough for a test), in every arithmetic, with gemm_bwd_pair_kernel on and off (ABN_BWD_PAIR).

The shapes (rows, in_dim, out_dim) are the smallest at which every tile has a ragged last row block, column block and
k step: 130 = 128 + 2 rows, 136 = 128 + 8 columns, 72 = 2 x 32 + 8 in k; (130, 72, 136) takes the vectorised builds,
(130, 37, 67) the element-wise ones, (130, 72, 67) vectorised operands with an element-wise epilogue.  Every output and
the split-K scratch are NaN before a call and sit in the middle of an allocation filled with a sentinel (a store past a
ragged tile edge shows); every input sits between NaN guards (a row read past the end of an operand and not masked
poisons the result).

Bars: conftest.rel_err < 1e-5 per tensor against float64 products of the fp32 inputs (the bar of BASELINE.json and of
test_linear_backward_entry_matches_the_two_single_gemm_entries), the activation derivative taken in float64 from the
fp32 activations.  The bf16 arithmetic (precision 1) is held to the SAME bar against float64 products of the operands
rounded to bf16 (round to nearest even, as v_cvt_pk_bf16_f32 does): a product of two bf16 values is exact in fp32, so
only the accumulation order remains."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENTINEL = 12345.0
GUARD = 64                 # floats in front of and behind every output (a multiple of 4: the slice stays 16-byte aligned)
E_ARG, E_WORKSPACE = -1, -3

VEC, ELEMENTWISE, MIXED = (130, 72, 136), (130, 37, 67), (130, 72, 67)
# (300, 72, 136): split_count (csrc/tower.hip) gives min(ceil(512 / 4), 300 // 128) = 2 slices of k_chunk = align_up(150, 32) =
# 160 rows, the second one ragged (140 rows).
# (770, 72, 136): 770 // 128 = 6 slices of k_chunk = align_up(ceil(770 / 6) = 129, 32) = 160 rows; the sixth starts at row
# 5 x 160 = 800 > 770: it is EMPTY (test_an_empty_split_k_slice_writes_exact_zeros asserts the slice count).
TWO_SLICES, EMPTY_SLICE = (300, 72, 136), (770, 72, 136)
BACKWARD_SHAPES = [VEC, ELEMENTWISE, MIXED, TWO_SLICES, EMPTY_SLICE]
FORWARD_SHAPES = [VEC, ELEMENTWISE, MIXED, (1, 72, 136), (1, 37, 67), (0, 72, 136), (0, 37, 67)]
TILES = [0, 1, 2, 3]       # 128x128, 128x64, 64x128, 64x64 (prepare_gemm's codes)
# (precision, ABN_BF16X3_PLANES): the switch only matters to the bf16 x 3 arithmetic (precision 3 runs as 2 here)
ARITHMETICS = [(0, None), (1, None), (2, 1), (2, 0), (3, 1), (3, 0)]


def lib_():
    from abnet3_amd import _lib
    return _lib, _lib.load()


def bf16_round(a):
    """fp32 -> bf16 -> fp32, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def act_f64(z, code):
    return [z, 1.0 / (1.0 + np.exp(-z)), np.maximum(z, 0.0), np.tanh(z)][code]


def act_grad_f64(a, code):
    """The derivative expressed on the activation's output, as autograd keeps it."""
    return [np.ones_like(a), a * (1.0 - a), (a > 0).astype(np.float64), 1.0 - a * a][code]


@functools.lru_cache(maxsize=None)
def case(rows, k, n):
    """Standard-normal inputs of one shape (fixed seed per shape) and their float64 products, computed once and shared
    (nothing writes to them).  'bf': the same products of the operands rounded to bf16."""
    rng = np.random.default_rng(1000003 * rows + 1009 * k + n)
    c = {name: rng.standard_normal(shape).astype(np.float32)
         for name, shape in (('x', (rows, k)), ('W', (n, k)), ('b', (n,)), ('dz', (rows, n)))}
    c['x64'], c['W64'], c['dz64'] = c['x'].astype(np.float64), c['W'].astype(np.float64), c['dz'].astype(np.float64)
    c['z'] = c['x64'] @ c['W64'].T
    c['exact'] = dict(dW=c['dz64'].T @ c['x64'], db=c['dz64'].sum(0), dx=c['dz64'] @ c['W64'])
    return c


def bf16_products(c):
    if 'bf' not in c:
        dz, x, W = (bf16_round(c[q]).astype(np.float64) for q in ('dz', 'x', 'W'))
        c['bf'] = dict(dW=dz.T @ x, db=dz.sum(0), dx=dz @ W)
    return c['bf']


class Guarded(object):
    """A tensor in the middle of a larger allocation: `t` is the [shape] view, NaN to begin with (fill=None) or a copy
    of `fill`; the floats around it hold `guard_value` and intact() says whether they still do."""

    def __init__(self, shape, fill=None, guard=GUARD, guard_value=SENTINEL, shift=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * guard + shift,), float(guard_value), device='cuda')
        self.lo, self.hi = guard + shift, guard + shift + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if fill is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
        self.before = self.buf.clone()

    def intact(self):
        a, b = self.buf.view(torch.int32), self.before.view(torch.int32)       # (by bits: NaN guards compare too)
        return bool(torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.hi:], b[self.hi:]))

    def untouched(self):
        """Not a single float of the whole allocation changed (NaN compares by bits)."""
        return bool(torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)))

    def ptr(self):
        """The view's address (torch gives an EMPTY view, rows = 0, a null data_ptr(): the entries refuse NULL)."""
        import ctypes
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.lo)

    def np(self):
        return self.t.cpu().numpy()


def operand(a, ld):
    """An input between NaN guards of 256 rows each: whatever a kernel reads outside the operand and fails to mask
    turns its output into NaN (the empty split-K slice of EMPTY_SLICE would start 30 rows behind the last one)."""
    return Guarded(a.shape, fill=a, guard=256 * ld, guard_value=float('nan'))


def check(out, ref, what):
    e = rel_err(out.np(), ref)
    print('%s: rel_err %.3g' % (what, e))
    assert e < TOL, (what, e)          # (a NaN left in the output fails this too)
    assert out.intact(), what + ': wrote outside its output'


# ---------------------------------------------------------------------------------------------------------------------
# abn_linear_forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', FORWARD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('tile', TILES)
def test_linear_forward(tile, shape, monkeypatch):
    """y = act(x W^T + b) for every activation code, with an aligned bias (vectorised epilogue where out_dim allows), a
    bias one float off a 16-byte boundary (the bias pointer is part of the vectorisation condition: element-wise
    epilogue) and no bias.  rows = 0: ABN_OK, nothing written."""
    monkeypatch.setenv('ABN_GEMM_TILE', str(tile))
    _lib, lib = lib_()
    rows, k, n = shape
    c = case(*shape)
    x, W = operand(c['x'], k), operand(c['W'], k)
    for bias in ('aligned', 'misaligned', 'none'):
        b = None if bias == 'none' else Guarded((n,), fill=c['b'], shift=int(bias == 'misaligned'))
        assert b is None or (b.t.data_ptr() % 16 == 0) == (bias == 'aligned')
        for act in range(4):
            y = Guarded((rows, n))
            rc = lib.abn_linear_forward(x.ptr(), W.ptr(), b.ptr() if b else None, rows, k, n, act,
                                        y.ptr(), _lib.stream())
            _lib.check(rc, 'abn_linear_forward')
            if rows == 0:
                assert y.untouched()
                continue
            ref = act_f64(c['z'] + (c['b'].astype(np.float64) if b else 0.0), act)
            check(y, ref, 'forward tile %d bias %s act %d' % (tile, bias, act))


# ---------------------------------------------------------------------------------------------------------------------
# abn_linear_dgrad
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', FORWARD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('tile', TILES)
def test_linear_dgrad(tile, shape, monkeypatch):
    """dx = (dz W) * act'(a_prev) for every activation code, and the plain dz W of a NULL a_prev."""
    monkeypatch.setenv('ABN_GEMM_TILE', str(tile))
    _lib, lib = lib_()
    rows, k, n = shape
    c = case(*shape)
    dz, W, a = operand(c['dz'], n), operand(c['W'], k), operand(c['x'], k)
    for act, with_a in ((0, True), (1, True), (2, True), (3, True), (1, False)):
        dx = Guarded((rows, k))
        rc = lib.abn_linear_dgrad(dz.ptr(), W.ptr(), rows, k, n, a.ptr() if with_a else None, act,
                                  dx.ptr(), _lib.stream())
        _lib.check(rc, 'abn_linear_dgrad')
        if rows == 0:
            assert dx.untouched()
            continue
        ref = c['exact']['dx'] * (act_grad_f64(c['x64'], act) if with_a else 1.0)
        check(dx, ref, 'dgrad tile %d act %d a_prev %s' % (tile, act, with_a))


# ---------------------------------------------------------------------------------------------------------------------
# abn_linear_wgrad
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', BACKWARD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('tile', TILES)
def test_linear_wgrad(tile, shape, monkeypatch):
    monkeypatch.setenv('ABN_GEMM_TILE', str(tile))
    _lib, lib = lib_()
    rows, k, n = shape
    c = case(*shape)
    dz, a = operand(c['dz'], n), operand(c['x'], k)
    sc_n = lib.abn_linear_wgrad_scratch_floats(rows, k, n)
    sc, dW, db = Guarded((sc_n,)), Guarded((n, k)), Guarded((n,))
    _lib.check(lib.abn_linear_wgrad(dz.ptr(), a.ptr(), rows, k, n, dW.ptr(), db.ptr(), sc.ptr(),
                                    sc_n, _lib.stream()), 'abn_linear_wgrad')
    check(dW, c['exact']['dW'], 'wgrad dW tile %d' % tile)
    check(db, c['exact']['db'], 'wgrad db tile %d' % tile)
    assert sc.intact()


# ---------------------------------------------------------------------------------------------------------------------
# abn_linear_backward_prec / abn_linear_backward
# ---------------------------------------------------------------------------------------------------------------------
def run_backward(shape, precision, act, dz, W, a, entry='prec', reduce=True):
    """One call with fresh NaN outputs and scratch; returns (dW, db, dx, scratch) as Guarded."""
    _lib, lib = lib_()
    rows, k, n = shape
    sc_n = lib.abn_linear_wgrad_scratch_floats(rows, k, n)
    sc, dW, db, dx = Guarded((sc_n,)), Guarded((n, k)), Guarded((n,)), Guarded((rows, k))
    pW, pb = (dW.ptr(), db.ptr()) if reduce else (None, None)
    if entry == 'prec':
        rc = lib.abn_linear_backward_prec(dz.ptr(), W.ptr(), a.ptr(), rows, k, n, act, precision, pW, pb,
                                          dx.ptr(), sc.ptr(), sc_n, _lib.stream())
    else:
        rc = lib.abn_linear_backward(dz.ptr(), W.ptr(), a.ptr(), rows, k, n, act, pW, pb, dx.ptr(),
                                     sc.ptr(), sc_n, _lib.stream())
    _lib.check(rc, 'abn_linear_backward' + ('_prec' if entry == 'prec' else ''))
    return dW, db, dx, sc


def check_backward(out, c, precision, act, what):
    dW, db, dx, sc = out
    ref = bf16_products(c) if precision == 1 else c['exact']
    check(dW, ref['dW'], what + ' dW')
    check(db, ref['db'], what + ' db')
    check(dx, ref['dx'] * act_grad_f64(c['x64'], act), what + ' dx')      # (the derivative is never rounded to bf16)
    assert sc.intact(), what + ': wrote outside its scratch'


def set_arithmetic(monkeypatch, planes):
    if planes is not None:
        monkeypatch.setenv('ABN_BF16X3_PLANES', str(planes))


@pytest.mark.parametrize('shape', BACKWARD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('precision,planes', ARITHMETICS)
@pytest.mark.parametrize('tile', TILES)
def test_linear_backward_prec(tile, precision, planes, shape, monkeypatch):
    """dW, db and dx of every arithmetic on every tile against float64, with the pair grid (gemm_bwd_pair_kernel: what
    tile 1 takes when the weight gradient's workgroups are a multiple of 8, TWO_SLICES and EMPTY_SLICE here) and with
    two launches (ABN_BWD_PAIR=0): the same kernel bodies, bit-identical results."""
    monkeypatch.setenv('ABN_GEMM_TILE', str(tile))
    set_arithmetic(monkeypatch, planes)
    c = case(*shape)
    rows, k, n = shape
    dz, W, a = operand(c['dz'], n), operand(c['W'], k), operand(c['x'], k)
    act = (tile + precision + BACKWARD_SHAPES.index(shape)) % 4          # every activation code on every tile
    out = {}
    for pair in (1, 0):
        monkeypatch.setenv('ABN_BWD_PAIR', str(pair))
        out[pair] = run_backward(shape, precision, act, dz, W, a)
    check_backward(out[1], c, precision, act, 'backward_prec tile %d precision %d planes %s act %d' % (tile, precision, planes, act))
    for g1, g0 in zip(out[1][:3], out[0][:3]):
        assert torch.equal(g1.t, g0.t)
        assert g0.intact()


@pytest.mark.parametrize('shape', BACKWARD_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('tile', TILES)
def test_linear_backward_is_wgrad_plus_dgrad_on_every_tile(tile, shape, monkeypatch):
    """abn_linear_backward == abn_linear_wgrad + abn_linear_dgrad, bit for bit, under each forced tile (the same kernel
    bodies in one grid or in two)."""
    monkeypatch.setenv('ABN_GEMM_TILE', str(tile))
    _lib, lib = lib_()
    c = case(*shape)
    rows, k, n = shape
    dz, W, a = operand(c['dz'], n), operand(c['W'], k), operand(c['x'], k)
    act = 1 + (tile + BACKWARD_SHAPES.index(shape)) % 3
    dW1, db1, dx1, sc1 = out = run_backward(shape, 0, act, dz, W, a, entry='fp32')
    check_backward(out, c, 0, act, 'backward tile %d act %d' % (tile, act))
    sc_n = lib.abn_linear_wgrad_scratch_floats(rows, k, n)
    sc, dW2, db2, dx2 = Guarded((sc_n,)), Guarded((n, k)), Guarded((n,)), Guarded((rows, k))
    _lib.check(lib.abn_linear_wgrad(dz.ptr(), a.ptr(), rows, k, n, dW2.ptr(), db2.ptr(), sc.ptr(),
                                    sc_n, _lib.stream()), 'abn_linear_wgrad')
    _lib.check(lib.abn_linear_dgrad(dz.ptr(), W.ptr(), rows, k, n, a.ptr(), act, dx2.ptr(),
                                    _lib.stream()), 'abn_linear_dgrad')
    assert torch.equal(dW1.t, dW2.t) and torch.equal(db1.t, db2.t) and torch.equal(dx1.t, dx2.t)
    assert dW2.intact() and db2.intact() and dx2.intact() and sc.intact()


@pytest.mark.parametrize('precision,planes', [(0, None), (1, None), (2, 1), (2, 0)])
@pytest.mark.parametrize('tile', [None] + TILES)
def test_an_empty_split_k_slice_writes_exact_zeros(tile, precision, planes, monkeypatch):
    """EMPTY_SLICE: six split-K slices of 160 rows over 770 rows, the sixth (rows 800 ..) empty.  With dW = db = NULL
    the slabs stay unreduced in the scratch: the empty slice's slab must hold exact zeros (the reduction adds it like
    the others), every slab must be finite although NaN rows follow the operands' last row, and the slabs' float64 sum
    is the gradient."""
    if tile is not None:
        monkeypatch.setenv('ABN_GEMM_TILE', str(tile))
    set_arithmetic(monkeypatch, planes)
    _lib, lib = lib_()
    shape = rows, k, n = EMPTY_SLICE
    c = case(*shape)
    nW, stride = n * k, (n * k + n + 63) // 64 * 64
    assert lib.abn_linear_wgrad_scratch_floats(rows, k, n) == 6 * stride          # six slices ...
    assert 5 * ((-(-rows // 6) + 31) // 32 * 32) >= rows                           # ... and the sixth starts behind the last row
    dz, W, a = operand(c['dz'], n), operand(c['W'], k), operand(c['x'], k)
    dW, db, dx, sc = run_backward(shape, precision, 2, dz, W, a, reduce=False)
    assert dW.untouched() and db.untouched()                                       # (not passed: the reduction did not run)
    assert sc.intact() and dx.intact()
    slabs = sc.np().reshape(6, stride)[:, :nW + n].astype(np.float64)
    assert (slabs[5] == 0.0).all()
    assert np.isfinite(slabs).all()
    ref = bf16_products(c) if precision == 1 else c['exact']
    assert rel_err(slabs[:, :nW].sum(0).reshape(n, k), ref['dW']) < TOL
    assert rel_err(slabs[:, nW:].sum(0), ref['db']) < TOL
    assert rel_err(dx.np(), ref['dx'] * act_grad_f64(c['x64'], 2)) < TOL


@pytest.mark.parametrize('precision,planes', [(0, None), (1, None), (2, 1), (2, 0)])
def test_linear_backward_at_the_natural_128x64_and_64x64_pair(precision, planes, monkeypatch):
    """(8192, 500, 64) with no forced tile: by prepare_gemm the data gradient (8192 x 500) takes 128 x 64 -- 64 x 8 = 512
    workgroups, 128 x 128 would give 256 -- and the weight gradient (64 x 501, 32 slices) 64 x 64 -- 64 x 128 would give
    1 x 4 x 32 = 128 workgroups --, 8 x 32 = 256 of them: the only way into gemm_bwd_pair_kernel<64, 64, ...> (a forced
    tile 3 moves the data gradient off 128 x 64, which the pair grid requires)."""
    set_arithmetic(monkeypatch, planes)
    shape = rows, k, n = 8192, 500, 64
    c = case(*shape)
    dz, W, a = operand(c['dz'], n), operand(c['W'], k), operand(c['x'], k)
    out = {}
    for pair in (1, 0):
        monkeypatch.setenv('ABN_BWD_PAIR', str(pair))
        out[pair] = run_backward(shape, precision, 3, dz, W, a)
    check_backward(out[1], c, precision, 3, 'backward_prec 8192x500x64 precision %d planes %s' % (precision, planes))
    for g1, g0 in zip(out[1][:3], out[0][:3]):
        assert torch.equal(g1.t, g0.t)
        assert g0.intact()


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: back before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_linear_backward_prec_refuses_bad_arguments_before_any_launch():
    _lib, lib = lib_()
    shape = rows, k, n = VEC
    c = case(*shape)
    dz, W, a = operand(c['dz'], n), operand(c['W'], k), operand(c['x'], k)
    sc_n = lib.abn_linear_wgrad_scratch_floats(rows, k, n)
    sc, dW, db, dx = Guarded((sc_n,)), Guarded((n, k)), Guarded((n,)), Guarded((rows, k))

    def call(precision=0, dW_=dW, db_=db, scratch_floats=sc_n):
        rc = lib.abn_linear_backward_prec(dz.ptr(), W.ptr(), a.ptr(), rows, k, n, 1, precision,
                                          dW_.ptr() if dW_ else None, db_.ptr() if db_ else None, dx.ptr(),
                                          sc.ptr(), scratch_floats, _lib.stream())
        torch.cuda.synchronize()
        return rc

    assert call(precision=4) == E_ARG
    assert call(precision=-1) == E_ARG
    assert call(dW_=None) == E_ARG
    assert call(db_=None) == E_ARG
    assert call(scratch_floats=sc_n - 1) == E_WORKSPACE
    assert call(scratch_floats=0) == E_WORKSPACE
    for g in (sc, dW, db, dx):
        assert g.untouched()
    # dW == db == NULL is a legal call: the grid runs, the slabs stay unreduced, dW and db are not written
    assert call(dW_=None, db_=None) == 0
    assert dW.untouched() and db.untouched()
    nW = n * k
    slab = sc.np()[:nW + n].astype(np.float64)             # (one slice at 130 rows)
    assert sc_n == (nW + n + 63) // 64 * 64
    assert rel_err(slab[:nW].reshape(n, k), c['exact']['dW']) < TOL and rel_err(slab[nW:], c['exact']['db']) < TOL
    check(dx, c['exact']['dx'] * act_grad_f64(c['x64'], 1), 'dx of the unreduced call')
    assert sc.intact()
