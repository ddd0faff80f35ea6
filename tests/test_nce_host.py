"""tests/nce_np.py's three restatements of the in-batch contrastive loss against each other, against float64 autograd and
finite differences; its error bars held by the float32 restatements on every case tests/test_gpu_nce.py names, and left by
three wrong kernels; InfoNCELoss's host side and abnt_nce_loss's refusals.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nce_np  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def case_inputs(B, D, kind):
    e1, e2 = nce_np.make_case(B, D)
    return e1, e2, nce_np.labels(B, kind)


_REF = {}


def ref_of(case):
    if case not in _REF:
        B, D, tau, kind = case
        e1, e2, y = case_inputs(B, D, kind)
        _REF[case] = (e1, e2, y, nce_np.reference(e1, e2, y, tau))
    return _REF[case]


def small_cases():
    rng = np.random.default_rng(5)
    out = []
    for B, D, tau, kind, grouped in ((5, 3, 0.1, 'all', False), (7, 4, 0.07, 'alt', True), (6, 2, 0.5, 'none', False),
                                     (9, 5, 0.01, 'one', True), (1, 3, 0.2, 'all', False), (4, 3, 0.3, 'all', True)):
        e1, e2 = nce_np.make_case(B, D, seed=3)
        if B >= 4:
            e1[1] = 0.0                                           # a zero row
            e2[2] *= 1e-8 / max(np.linalg.norm(e2[2]), 1e-30)     # a row of norm 1e-8
        groups = rng.integers(0, 3, size=B).astype(np.int32) if grouped else None
        out.append((e1, e2, nce_np.labels(B, kind), tau, groups))
    return out


@pytest.mark.parametrize('avg', [True, False])
def test_the_three_restatements_agree_in_float64(avg):
    for e1, e2, y, tau, groups in small_cases():
        B = len(y)
        l0, t0 = nce_np.loops(e1, e2, y, tau, groups, avg)
        ref = nce_np.reference(e1, e2, y, tau, groups, avg)
        l2, d1, d2 = nce_np.torch_value_and_grad(e1, e2, y, tau, groups, avg)
        scale = max(1.0, abs(l0))
        assert abs(ref['loss'] - l0) <= 1e-12 * scale and abs(l2 - l0) <= 1e-12 * scale
        assert np.abs(ref['terms'] - t0).max() <= 1e-12 * max(1.0, np.abs(t0).max())
        # the closed-form gradient equals float64 autograd (through the normalisation, the eps branch included)
        for got, want in ((ref['de1'], d1), (ref['de2'], d2)):
            assert np.abs(got - want).max() <= 1e-9 * max(1e-30, np.abs(want).max()) + 1e-18, (B, tau)
        if (y == 1).sum() == 0:
            assert ref['loss'] == 0.0 and not ref['de1'].any() and not ref['de2'].any() and l2 == 0.0


def test_groups_all_equal_and_a_single_row_give_exact_zeros():
    for B in (1, 5):
        e1, e2 = nce_np.make_case(B, 4)
        ref = nce_np.reference(e1, e2, np.ones(B), 0.1, np.zeros(B, dtype=np.int32))
        assert ref['loss'] == 0.0 and not ref['terms'].any() and not ref['de1'].any() and not ref['de2'].any()


def test_finite_differences_on_one_tiny_case():
    e1, e2 = nce_np.make_case(4, 3, seed=9)
    e1, e2 = e1.astype(np.float64), e2.astype(np.float64)
    y, tau, groups = np.array([1, -1, 1, 1]), 0.2, np.array([0, 1, 0, 2], dtype=np.int32)
    ref = nce_np.reference(e1, e2, y, tau, groups)
    h = 1e-6
    for side, key in ((0, 'de1'), (1, 'de2')):
        for i in range(4):
            for k in range(3):
                lo, hi = [e1.copy(), e2.copy()], [e1.copy(), e2.copy()]
                lo[side][i, k] -= h
                hi[side][i, k] += h
                fd = (nce_np.reference(hi[0], hi[1], y, tau, groups)['loss'] - nce_np.reference(lo[0], lo[1], y, tau, groups)['loss']) / (2 * h)
                assert abs(fd - ref[key][i, k]) <= 1e-6 * max(1.0, abs(fd)), (key, i, k)


@pytest.mark.parametrize('case', nce_np.CASES + (nce_np.BIG,))
def test_float32_restatements_hold_the_bars_and_the_named_cases_are_informative(case):
    B, D, tau, kind = case
    e1, e2, y, ref = ref_of(case)
    if B >= 127 and D >= 2 and ref['n'] > 0:
        # (B = 1, 2: log B < 0.5, the window is empty; D = 1: unit rows are +-1 and half the batch ties with the positive)
        assert 0.5 <= ref['loss'] <= math.log(B), ref['loss']
    assert ref['loss'] >= 0.0
    l32, d1, d2 = nce_np.torch_value_and_grad(e1, e2, y, tau, dtype=torch.float32)
    used = nce_np.check(l32, d1, d2, ref, B, D, tau, True, 'torch float32 autograd')
    lc, c1, c2 = nce_np.closed_form_f32(e1, e2, y, tau)
    used2 = nce_np.check(lc, c1, c2, ref, B, D, tau, True, 'float32 closed form')
    print('case %s: loss %.4f, shares of the bars used (loss, de1, de2): autograd %s, closed form %s'
          % (case, ref['loss'], ['%.3g' % v for v in used], ['%.3g' % v for v in used2]))


@pytest.mark.parametrize('mutant', nce_np.MUTANTS)
def test_a_wrong_kernel_leaves_the_bars_on_a_named_case(mutant):
    caught = []
    for case in nce_np.CASES:
        B, D, tau, kind = case
        e1, e2, y, ref = ref_of(case)
        try:
            nce_np.check(*nce_np.closed_form_f32(e1, e2, y, tau, mutant=mutant), ref, B, D, tau, True)
        except AssertionError:
            caught.append(case)
    print('%s: outside the bars on %s' % (mutant, caught))
    assert caught


def test_bars_grow_with_what_they_are_derived_from():
    one = np.ones(3)
    assert nce_np.loss_bar(257, 100, 0.07, 257, True, 3.0) < nce_np.loss_bar(257, 100, 0.01, 257, True, 3.0)
    assert nce_np.loss_bar(257, 100, 0.07, 257, True, 3.0) < nce_np.loss_bar(257, 256, 0.07, 257, True, 3.0)
    assert nce_np.loss_bar(257, 100, 0.07, 257, False, 3.0) > 200 * nce_np.loss_bar(257, 100, 0.07, 257, True, 3.0) * 0.99
    assert (nce_np.grad_bar(257, 100, 0.07, one, one, 1.0) < nce_np.grad_bar(1025, 100, 0.07, one, one, 1.0)).all()
    assert (nce_np.grad_bar(257, 100, 0.07, 0 * one, one, 0.0) == 0).all()             # n = 0: nothing but exact zeros passes
    assert nce_np.loss_bar(257, 100, 0.07, 257, True, 3.0) < 1e-3                 # and they are bars, not fences


# ---- the library's and the class's host side ------------------------------------------------------------------------------------
def test_ledger_queries_and_refusals_before_any_launch(lib, monkeypatch):
    from abnet3_amd import _lib
    assert set(_lib.NEXT7_SYMBOLS) == {'abnt_nce_max_d', 'abnt_nce_ws_bytes', 'abnt_nce_loss'}
    assert lib.abn_abi_version() == 20 and _lib.ABI_VERSION == 20
    assert lib.abnt_nce_max_d() == nce_np.MAX_D >= 128
    monkeypatch.delenv('ABN_NCE_SPLIT', raising=False)
    assert lib.abnt_nce_ws_bytes(0, 4) == -1 and b'abnt_nce_ws_bytes' in lib.abn_last_error()
    assert lib.abnt_nce_ws_bytes(4, 0) == -1 and lib.abnt_nce_ws_bytes(4, 257) == -1 and lib.abnt_nce_ws_bytes((1 << 20) + 1, 4) == -1
    for B, D in ((1, 1), (486, 100), (4096, 100), (4096, 128), (1 << 20, 256)):
        ws = lib.abnt_nce_ws_bytes(B, D)
        dp = -(-D // 4) * 4
        assert ws % 16 == 0 and 2 * B * dp * 4 < ws <= (2 + 2 * 16) * B * dp * 4 + 16 * B * 16 + 1024           # O(B D split), split <= 16
    assert lib.abnt_nce_ws_bytes(4096, 100) < 4096 * 4096 * 4 // 3                  # under a third of ONE B x B matrix at the benchmark's batch
    monkeypatch.setenv('ABN_NCE_SPLIT', '1')
    one = lib.abnt_nce_ws_bytes(1025, 100)
    monkeypatch.setenv('ABN_NCE_SPLIT', '3')                                         # read at every call: no reload
    assert lib.abnt_nce_ws_bytes(1025, 100) > one
    monkeypatch.delenv('ABN_NCE_SPLIT')
    p = 256                                                                          # a non-null, aligned address that is never read
    ok = dict(e1=p, e2=p, y=p, y_dtype=2, groups=0, B=8, D=4, tau=0.1, avg=1, loss=p, terms=0, de1=p, de2=p, ws=p, stream=0)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.abnt_nce_loss(*[a[k] for k in ok])
    for name in ('e1', 'e2', 'y', 'loss', 'ws'):
        assert call(**{name: 0}) == _lib.E_ARG, name
    assert call(B=0) == _lib.E_ARG and call(D=0) == _lib.E_ARG and call(y_dtype=5) == _lib.E_ARG
    for tau in (0.0, -1.0, float('inf'), float('nan'), 1e-45):
        assert call(tau=tau) == _lib.E_ARG, tau
    assert b'tau' in lib.abn_last_error()
    assert call(de1=0) == _lib.E_ARG and call(de2=0) == _lib.E_ARG
    assert call(D=257) == _lib.E_UNSUPPORTED and call(B=(1 << 20) + 1) == _lib.E_UNSUPPORTED
    assert call(ws=p + 4) == _lib.E_ARG and b'aligned' in lib.abn_last_error()


def test_the_class_on_the_host(lib):
    from abnet3_amd import loss
    f = loss.InfoNCELoss()
    assert f.temperature == 0.1 and f.avg is True
    who = loss.InfoNCELoss(temperature=0.07, avg=False).whoami()
    assert who['class_name'] == 'InfoNCELoss' and who['params']['temperature'] == 0.07 and who['params']['avg'] is False
    assert getattr(loss, 'InfoNCELoss') is loss.InfoNCELoss                          # a gridsearch YAML names the class
    for bad in (0.0, -0.1, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='temperature'):
            loss.InfoNCELoss(temperature=bad)
    with pytest.raises(Exception, match='HIP|device'):                               # no CPU fallback
        f(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4))
    multi = loss.weighted_loss_multi(loss_phn=loss.InfoNCELoss(), loss_spk=loss.coscos2(), weight=0.5)
    assert isinstance(multi.loss_phn, loss.InfoNCELoss)
