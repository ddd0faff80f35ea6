"""abnt_nce_loss and InfoNCELoss on the MI355X against tests/nce_np.py: float cases within the derived bars (the same named
cases tests/test_nce_host.py holds the float32 restatements to), exact cases that must EQUAL, refusals, and the loss through
a small network and the trainer.

Bits: the two sweeps of each direction / side are the same code with the sides swapped and every product a * b is
commutative, so swapping (e1, e2) swaps the outputs' BITS (asserted).  A forced split moves the points at which a row's
partial (max, sum) pairs and gradient slabs are merged: the results stay within the bars, the bits are in general NOT equal
(asserted only as 'within the bars'; the test prints whether they were)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import nce_np  # noqa: E402
from conftest import check_grads, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT7_SYMBOLS: the entries the dirty-memory test below reaches, and the host queries
DIRTY_CASES = ('abnt_nce_loss',)
QUERIES = ('abnt_nce_max_d', 'abnt_nce_ws_bytes')
bits = dirty_memory.bits


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def raw(e1, e2, y, tau, groups=None, avg=True, grad=True, want_terms=True, y_dtype=None):
    """(loss, terms, de1, de2) host arrays of abnt_nce_loss with every output and the workspace from torch.empty."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    B, D = e1.shape
    d1, d2 = dev(e1, torch.float32), dev(e2, torch.float32)
    yd = dev(y, y_dtype or torch.int64)
    gd = None if groups is None else dev(groups, torch.int32)
    need = lib.abnt_nce_ws_bytes(B, D)
    assert need > 0
    loss = torch.empty((), dtype=torch.float32, device='cuda')
    terms = torch.empty(B, dtype=torch.float32, device='cuda') if want_terms else None
    de = torch.empty(2, B, D, dtype=torch.float32, device='cuda') if grad else None
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    rc = lib.abnt_nce_loss(p(d1), p(d2), p(yd), _lib.Y_DTYPE[yd.dtype], p(gd), B, D, float(tau), int(avg), p(loss), p(terms),
                           p(de[0]) if grad else None, p(de[1]) if grad else None, p(ws), _lib.stream())
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return (host(loss), host(terms) if want_terms else None, host(de[0]) if grad else None, host(de[1]) if grad else None)


def same(a, b):
    return all((u is None and v is None) or np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


_REF = {}


def ref_of(case):
    """A named case's inputs and float64 restatement: computed once, shared, never written."""
    if case not in _REF:
        B, D, tau, kind = case
        e1, e2 = nce_np.make_case(B, D)
        y = nce_np.labels(B, kind)
        _REF[case] = (e1, e2, y, nce_np.reference(e1, e2, y, tau))
    return _REF[case]


def check_terms(terms, ref, B, D, tau):
    err = np.abs(terms.astype(np.float64) - ref['terms'])
    assert (err <= nce_np.term_bar(B, D, tau, ref['terms'])).all(), float((err / nce_np.term_bar(B, D, tau, ref['terms'])).max())
    assert (terms >= 0).all()                                    # la - z_ii >= 0 in the kernel's own bits


# ---- 1: the ledger and dirty memory ------------------------------------------------------------------------------------------
def test_every_next7_symbol_is_a_dirty_memory_case_or_a_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT7_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert not set(_lib.NEXT7_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS) |
                                          set(_lib.NEXT4_SYMBOLS) | set(_lib.NEXT5_SYMBOLS) | set(_lib.NEXT6_SYMBOLS))
    assert _lib.load().abnt_nce_max_d() == nce_np.MAX_D


@pytest.mark.parametrize('B,D,split', [(129, 33, None), (300, 100, '3')])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(B, D, split, monkeypatch):
    """abnt_nce_loss with loss, terms, both gradients and the workspace from torch.empty under the three patterns: the same
    bits, and they are within the bars of the restatement (so nothing of the pattern leaked in)."""
    from abnet3_amd import _lib
    if split:
        monkeypatch.setenv('ABN_NCE_SPLIT', split)
    e1, e2 = nce_np.make_case(B, D, seed=1)
    y = nce_np.labels(B, 'alt')
    groups = (np.arange(B) // 3).astype(np.int32)
    outs = {}
    with dirty_memory.recorded(_lib.load()) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                outs[byte] = raw(e1, e2, y, 0.07, groups)
            assert int(count) == 4 and count.nbytes > 2 * B * D * 4          # loss, terms, the gradients, the workspace
    assert set(old_calls) <= {'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert same(outs[byte], outs[0x00]), hex(byte)
    ref = nce_np.reference(e1, e2, y, 0.07, groups)
    nce_np.check(outs[0xFF][0], outs[0xFF][2], outs[0xFF][3], ref, B, D, 0.07, True, 'dirty')
    check_terms(outs[0xFF][1], ref, B, D, 0.07)


# ---- 2: float cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', nce_np.CASES)
def test_float_cases_are_within_the_derived_bars(case):
    B, D, tau, kind = case
    e1, e2, y, ref = ref_of(case)
    loss, terms, de1, de2 = raw(e1, e2, y, tau)
    used = nce_np.check(loss, de1, de2, ref, B, D, tau, True, str(case))
    check_terms(terms, ref, B, D, tau)
    print('case %s: loss %.6f (float64 %.6f); shares of the bars used (loss, de1, de2): %s'
          % (case, float(loss), ref['loss'], ['%.3g' % v for v in used]))
    fwd = raw(e1, e2, y, tau, grad=False, want_terms=False)
    assert bits(fwd[0]) == bits(loss)                            # forward only: the same loss bits
    again = raw(e1, e2, y, tau)
    assert same(again, (loss, terms, de1, de2))                  # two calls: the same bits
    if case == (257, 100, 0.07, 'all'):
        total = raw(e1, e2, y, tau, avg=False)
        ref_sum = nce_np.reference(e1, e2, y, tau, avg=False)
        nce_np.check(total[0], total[2], total[3], ref_sum, B, D, tau, False, 'avg=False')


@pytest.mark.parametrize('dtype', [torch.int8, torch.int32, torch.int64, torch.float32, torch.float64])
def test_every_label_dtype(dtype):
    from abnet3_amd import _lib
    assert set(_lib.Y_DTYPE) == {torch.int8, torch.int32, torch.int64, torch.float32, torch.float64}
    case = (127, 100, 0.5, 'alt')
    e1, e2, y, ref = ref_of(case)
    y = y.copy()
    y[1] = 2 if dtype in (torch.int8, torch.int32, torch.int64) else 1                 # 2 is no anchor; 1 is
    if dtype in (torch.float32, torch.float64):
        y = y.astype(np.float64)
        y[3] = 0.999999                                                                  # nearly 1 is no anchor
    ref = nce_np.reference(e1, e2, y, 0.5)
    out = raw(e1, e2, y, 0.5, y_dtype=dtype)
    nce_np.check(out[0], out[2], out[3], ref, 127, 100, 0.5, True, str(dtype))


def test_the_forced_split_reaches_the_merge_and_stays_within_the_bars(monkeypatch):
    B, D, tau, kind = nce_np.BIG
    e1, e2, y, ref = ref_of(nce_np.BIG)
    outs = {}
    for split in ('1', '4'):
        monkeypatch.setenv('ABN_NCE_SPLIT', split)
        outs[split] = raw(e1, e2, y, tau)
        used = nce_np.check(outs[split][0], outs[split][2], outs[split][3], ref, B, D, tau, True, 'split ' + split)
        check_terms(outs[split][1], ref, B, D, tau)
        print('split %s: shares of the bars used %s' % (split, ['%.3g' % v for v in used]))
    monkeypatch.delenv('ABN_NCE_SPLIT')
    auto = raw(e1, e2, y, tau)
    nce_np.check(auto[0], auto[2], auto[3], ref, B, D, tau, True, 'split by the grid')
    # not asserted either way: the merge points move with the split, so equal bits would be a coincidence
    print('split 1 and split 4 give %s bits' % ('the same' if same(outs['1'], outs['4']) else 'different'))


# ---- 3: exact cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,D,split', [(129, 100, None), (257, 33, None), (257, 3, '3'), (1, 100, None), (1, 1, None)])
def test_groups_all_equal_and_a_single_row_are_exactly_zero(B, D, split, monkeypatch):
    """Every lse is a one-term sum, exp(0) = 1, log 1 = 0, G[i][i] = c (1 + 1 - 2): a padding column or an excluded cell
    with any weight at all shows."""
    if split:
        monkeypatch.setenv('ABN_NCE_SPLIT', split)
    e1, e2 = nce_np.make_case(B, D, seed=2)
    groups = None if B == 1 else np.full(B, 7, dtype=np.int32)
    for tau in (0.5, 0.01):
        loss, terms, de1, de2 = raw(e1, e2, np.ones(B, dtype=np.int64), tau, groups)
        assert loss == 0.0 and not terms.any() and not de1.any() and not de2.any(), (tau, float(loss))


@pytest.mark.parametrize('avg', [True, False])
def test_no_anchor_gives_zero_and_zero_gradients(avg):
    e1, e2 = nce_np.make_case(129, 33)
    loss, terms, de1, de2 = raw(e1, e2, -np.ones(129, dtype=np.int64), 0.07, avg=avg)
    assert loss == 0.0 and not de1.any() and not de2.any()
    assert (terms > 0).any()                                     # the terms are every row's, anchors or not


# ---- 4: symmetry, identical candidates, the norm's edge ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(129, 100, 0.01, 'alt'), (257, 2, 0.07, 'alt')])
def test_swapping_the_sides_swaps_the_bits(case):
    """The two directions are one code path with the sides swapped, a * b == b * a and k ascends either way."""
    B, D, tau, kind = case
    e1, e2, y, ref = ref_of(case)
    groups = (np.arange(B) % 5).astype(np.int32)
    a = raw(e1, e2, y, tau, groups)
    b = raw(e2, e1, y, tau, groups)
    assert same((a[0], a[1], a[2], a[3]), (b[0], b[1], b[3], b[2]))


def test_identical_candidates_give_log_B():
    B, D, tau = 257, 100, 0.07
    row = nce_np.make_case(1, D)[0]
    e = np.repeat(row, B, axis=0)
    ref = nce_np.reference(e, e, np.ones(B), tau)
    loss, terms, de1, de2 = raw(e, e, np.ones(B, dtype=np.int64), tau)
    assert abs(ref['loss'] - np.log(B)) < 1e-12
    assert abs(float(loss) - np.log(B)) <= nce_np.loss_bar(B, D, tau, B, True, np.log(B))
    nce_np.check(loss, de1, de2, ref, B, D, tau, True, 'identical')


def test_a_zero_row_and_a_tiny_row_among_ordinary_ones():
    B, D, tau = 130, 33, 0.07
    e1, e2 = nce_np.make_case(B, D, seed=4)
    e1[3] = 0.0
    e2[3] *= 1e-8 / np.linalg.norm(e2[3])
    e1[128] *= 1e-8 / np.linalg.norm(e1[128])
    e2[129] = 0.0
    y = np.ones(B, dtype=np.int64)
    ref = nce_np.reference(e1, e2, y, tau)
    assert ref['inv_a'][3] == 1e6 and ref['inv_b'][129] == 1e6 and np.abs(ref['de2'][3]).max() > 1.0
    loss, terms, de1, de2 = raw(e1, e2, y, tau)
    nce_np.check(loss, de1, de2, ref, B, D, tau, True, 'norm edge')


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    """Every refusal with real device buffers holding a sentinel: the codes, and nothing written (a launch would have)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    B, D = 8, 4
    e = torch.randn(B, D, device='cuda')
    y = torch.ones(B, dtype=torch.int64, device='cuda')
    outs = torch.full((1 + B + 2 * B * D,), -7.0, device='cuda')
    ws = torch.full((lib.abnt_nce_ws_bytes(B, D) // 4 + 4,), -7.0, device='cuda')
    loss, terms, de1, de2 = outs[0:1], outs[1:1 + B], outs[1 + B:1 + B + B * D], outs[1 + B + B * D:]
    ok = dict(e1=p(e), e2=p(e), y=p(y), y_dtype=2, groups=None, B=B, D=D, tau=0.1, avg=1, loss=p(loss), terms=p(terms), de1=p(de1),
              de2=p(de2), ws=p(ws), stream=_lib.stream())

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.abnt_nce_loss(*[a[k] for k in ok])
    E_ARG, E_UNSUPPORTED = _lib.E_ARG, _lib.E_UNSUPPORTED
    for name in ('e1', 'e2', 'y', 'loss', 'ws'):
        assert call(**{name: None}) == E_ARG, name
    assert call(B=0) == E_ARG and call(D=0) == E_ARG and call(B=-3) == E_ARG
    for tau in (0.0, -0.5, float('inf'), float('nan')):
        assert call(tau=tau) == E_ARG, tau
    assert call(de1=None) == E_ARG and call(de2=None) == E_ARG
    assert call(D=lib.abnt_nce_max_d() + 1) == E_UNSUPPORTED
    assert call(ws=_lib.C.c_void_p(ws.data_ptr() + 4)) == E_ARG
    torch.cuda.synchronize()
    assert bool((outs == -7.0).all()) and bool((ws == -7.0).all())
    assert call() == 0                                            # and the same buffers are fine as they stand
    torch.cuda.synchronize()
    assert bool((outs != -7.0).all())
    from abnet3_amd.loss import InfoNCELoss
    with pytest.raises(ValueError, match='abnt_nce_max_d'):
        InfoNCELoss()(torch.zeros(4, 300, device='cuda'), torch.zeros(4, 300, device='cuda'), torch.ones(4, device='cuda'))
    with pytest.raises(ValueError, match='labels'):
        InfoNCELoss()(e, e, y[:3])


# ---- 6: through the network and the trainer ----------------------------------------------------------------------------------------
def small_net(seed=0):
    from abnet3_amd.model import SiameseNetwork
    torch.manual_seed(seed)
    return SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=32, output_dim=16, p_dropout=0.0,
                          activation_layer='sigmoid', output_path='/tmp/abn_nce_test').cuda()


def planted_batch(rng, proto, n=96, noise=0.3):
    which = rng.integers(0, len(proto), size=n)
    x1 = (proto[which] + noise * rng.standard_normal((n, proto.shape[1]))).astype(np.float32)
    x2 = (x1 + noise * rng.standard_normal(x1.shape)).astype(np.float32)
    return dev(x1), dev(x2), torch.ones(n, dtype=torch.int64, device='cuda')


def test_loss_and_parameter_gradients_through_a_small_network():
    """InfoNCELoss through a 40 -> 32 -> 16 sigmoid network against nce_np.torch_loss through the same network, with
    conftest.check_grads at its existing 2e-5.  Sigmoid embeddings are nearly parallel (cosines 0.9 .. 1) and the output
    bias gradient is a sum over the batch that cancels: a similarity formed as one fp32 chain that sums to 1 lands
    1.5e-5 .. 2.5e-5 from float64 on that tensor (an earlier form of the kernel and torch_loss in float32 alike).  The
    kernel forms it over the rows less their mean instead (csrc/nce.hip) and measures 8e-7 .. 1.6e-6 there."""
    from abnet3_amd.loss import InfoNCELoss, unit_grad
    rng = np.random.default_rng(0)
    proto = rng.standard_normal((8, 40))
    x1, x2, y = planted_batch(rng, proto)
    y[::3] = -1
    groups = torch.arange(96, device='cuda') // 2
    net = small_net()
    net.train()
    for grp in (None, groups):
        f = InfoNCELoss(temperature=0.07)
        net.zero_grad()
        loss = f(*net(x1, x2), y, groups=grp)
        loss.backward()
        mine = {k: host(p.grad).copy() for k, p in net.named_parameters()}
        # the reference: nce_np.torch_loss on the same device through the same network, its own arithmetic in float64 (the
        # embeddings are cast behind the network, the gradient comes back through the cast).  Sigmoid embeddings are nearly
        # parallel, the gradient is a small remainder of large terms, and torch_loss in float32 is itself 1.1e-5 .. 1.7e-5
        # from float64 on the output layer's bias here (measured on the MI355X; printed below): most of check_grads' 2e-5,
        # which is meant for the code under test.
        net.zero_grad()
        e1, e2 = net(x1, x2)
        want = nce_np.torch_loss(e1.double(), e2.double(), y, 0.07, grp)
        want.backward()
        ref = {k: host(p.grad).copy() for k, p in net.named_parameters()}
        net.zero_grad()
        nce_np.torch_loss(*net(x1, x2), y, 0.07, grp).backward()
        ref32 = {k: host(p.grad).copy() for k, p in net.named_parameters()}
        gmax = max(np.abs(ref[k]).max() for k in ref)
        for k in ref:
            print('groups %s %-24s kernel against float64 %.3g, float32 torch_loss against float64 %.3g (check_grads: 2e-5)'
                  % (grp is not None, k, rel_err(mine[k], ref[k], floor=1e-2 * gmax), rel_err(ref32[k], ref[k], floor=1e-2 * gmax)))
        assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
        check_grads(mine, ref, list(ref), False)
    # the cached unit seed is taken as it stands, another seed scales
    e1, e2 = (t.detach().requires_grad_(True) for t in net(x1, x2))
    f = InfoNCELoss(temperature=0.07)
    torch.autograd.backward(f(e1, e2, y), unit_grad(e1.device))
    g1 = e1.grad.clone()
    e1.grad = None
    torch.autograd.backward(f(e1, e2, y), torch.full((), 2.0, device='cuda'))
    assert torch.equal(e1.grad, 2.0 * g1)
    val, de = f.value_and_grad(e1.detach(), e2.detach(), y)
    assert torch.equal(de[0], g1) and de.shape == (2, 96, 16)
    with torch.no_grad():                                         # the dev pass: forward only, a finite loss
        dev_loss = f(*net(x1, x2), y)
    assert dev_loss.dim() == 0 and bool(torch.isfinite(dev_loss)) and bits(host(dev_loss)) == bits(host(val))


def test_the_trainer_takes_the_autograd_path_and_the_loss_falls():
    from abnet3_amd.loss import InfoNCELoss, coscos2, weighted_loss_multi
    from abnet3_amd.trainer import TrainerSiamese
    rng = np.random.default_rng(1)
    proto = rng.standard_normal((8, 40))
    net = small_net(1)
    tr = TrainerSiamese(network=net, loss=InfoNCELoss(temperature=0.1), optimizer_type='adadelta', lr=0.5, dataloader=None,
                        log_dir='/tmp/abn_runs')
    assert not tr._direct_ok() and tr._planned(True) is None and tr._loss_is_mean()
    net.train()
    losses = [float(tr.train_step(planted_batch(rng, proto), True)) for _ in range(30)]
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    dev_loss = tr.train_step(planted_batch(rng, proto), False)
    assert bool(torch.isfinite(dev_loss))
    # as a sub-loss of the multi-task loss, unchanged
    multi = weighted_loss_multi(loss_phn=InfoNCELoss(temperature=0.1), loss_spk=coscos2(), weight=0.25)
    x1, x2, y = planted_batch(rng, proto)
    a, b = (t.detach().requires_grad_(True) for t in net(x1, x2))
    out = multi(a, a, b, b, y, y)
    want = 0.25 * coscos2()(a, b, y) + 0.75 * InfoNCELoss(temperature=0.1)(a, b, y)
    assert abs(float(out) - float(want)) <= 1e-6 * abs(float(want))
    out.backward()
    assert bool(torch.isfinite(a.grad).all()) and bool(a.grad.abs().sum() > 0)
