"""KLLoss (abnet3/loss.py:108-137) on the MI355X: the fused kernel (csrc/loss.hip, kl_pair_loss_kernel) in both input
forms against the reference's own outputs (tests/golden/kl_loss.npz, tools/make_golden.py G12), its padded mode and
dropout masks, a softmax network trained with it through TrainerSiamese's direct step, a captured step, the canonical
loader, and the multitask loss.  Needs an MI355X: run with -m gpu."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

import kl_np
from conftest import check_grads, check_params, load_golden, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CASES_A = ['a0', 'a1', 'a2', 'a3', 'a4', 'a5']
CASES_B = ['b0', 'b1', 'b2', 'b3']
CASES_U = ['u0', 'u1']


def g12():
    return load_golden('kl_loss.npz')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_rows(mine, ref, tag):
    """Each gradient row within 2e-5 of its own largest entry (check_loss_grads' rule)."""
    for r in range(ref.shape[0]):
        scale = max(np.abs(ref[r]).max(), 1e-30)
        assert np.abs(mine[r] - ref[r]).max() <= 2e-5 * scale, (tag, r)


def check_rows_f64(mine, ref32, ref64, tag):
    """The float64 yardstick (tests/test_gpu_timed_path.py): per row, the error against the reference's float64
    evaluation is no larger than twice the reference fp32's own error against it, plus 1e-9 of the row's scale."""
    for r in range(ref64.shape[0]):
        t = ref64[r]
        e_mine = np.abs(mine[r].astype(np.float64) - t).max()
        e_ref = np.abs(ref32[r].astype(np.float64) - t).max()
        assert e_mine <= 2 * e_ref + 1e-9 * np.abs(t).max(), (tag, r, e_mine, e_ref)


def kl(g, n):
    from abnet3_amd.loss import KLLoss
    return KLLoss(margin=float(g[n + '.margin']), avg=bool(g[n + '.avg']))


@pytest.mark.parametrize('n', CASES_A)
def test_probability_form_vs_reference(n):
    """KLLoss(...)(p, q, y).backward() on probability rows: loss at 1e-5, gradient rows at 2e-5."""
    g = g12()
    p = dev(g[n + '.in1']).requires_grad_(True)
    q = dev(g[n + '.in2']).requires_grad_(True)
    lv = kl(g, n)(p, q, dev(g[n + '.y']))
    lv.backward()
    assert abs(float(lv.detach()) - g[n + '.loss']) <= 1e-5 * abs(g[n + '.loss']), (float(lv.detach()), g[n + '.loss'])
    check_rows(p.grad.cpu().numpy(), g[n + '.g1'], n)
    check_rows(q.grad.cpu().numpy(), g[n + '.g2'], n)
    # value_and_grad is the same launch without autograd
    lv2, de = kl(g, n).value_and_grad(p.detach(), q.detach(), dev(g[n + '.y']))
    assert float(lv2) == float(lv.detach())
    assert torch.equal(de[0], p.grad) and torch.equal(de[1], q.grad)


@pytest.mark.parametrize('n', CASES_B + CASES_U)
def test_logits_form_vs_reference(n):
    """value_and_dz(z1, z2, y, 'softmax') = nn.Softmax() + KLLoss + autograd to the logits, in one launch."""
    g = g12()
    lv, dz = kl(g, n).value_and_dz(dev(g[n + '.in1']), dev(g[n + '.in2']), dev(g[n + '.y']), 'softmax', None)
    assert abs(float(lv.detach()) - g[n + '.loss']) <= 1e-5 * abs(g[n + '.loss']), (float(lv.detach()), g[n + '.loss'])
    dz = dz.cpu().numpy()
    for side, key in ((0, '.g1'), (1, '.g2')):
        if n in CASES_U:       # near-uniform rows: the reference's fp32 gradient is itself a cancelled difference
            check_rows_f64(dz[side], g[n + key], g[n + key + '.f64'], n)
        else:
            check_rows(dz[side], g[n + key], n)


def _padded(kind_loss, e1, e2, y, nv, margin, avg, acc):
    from abnet3_amd import _lib
    from abnet3_amd.loss import _scratch
    lib = _lib.load()
    B, D = e1.shape
    loss = torch.empty((), dtype=torch.float32, device='cuda')
    de = torch.full((2, B, D), 7.0, dtype=torch.float32, device='cuda')
    ws = _scratch(lib.abn_pair_loss_ws_bytes(B), e1.device)
    _lib.check(lib.abn_pair_loss_padded(
        _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(y), _lib.Y_DTYPE[y.dtype], B, D, _lib.LOSS[kind_loss], float(margin),
        int(avg), _lib.ptr(nv), _lib.ptr(loss), _lib.ptr(acc), _lib.ptr(de[0]), _lib.ptr(de[1]), _lib.ptr(ws),
        _lib.stream()), 'abn_pair_loss_padded')
    return loss, de


@pytest.mark.parametrize('n', ['a2', 'a0'])
@pytest.mark.parametrize('avg', [True, False])
def test_padded_mode(n, avg):
    """abn_pair_loss_padded with ABN_LOSS_KL: only the first n_valid pairs count, a mean divides by n_valid, the padded
    rows get zero gradient, loss_accum accumulates over calls."""
    g = g12()
    p, q, y = g[n + '.in1'], g[n + '.in2'], g[n + '.y']
    B = p.shape[0]
    nvalid = B - max(3, B // 3)
    margin = float(g[n + '.margin'])
    ref, r1, r2 = kl_np.kl_prob(p[:nvalid], q[:nvalid], y[:nvalid], margin, avg)
    nv = torch.tensor([nvalid], dtype=torch.int32, device='cuda')
    acc = torch.zeros((), dtype=torch.float64, device='cuda')
    loss, de = _padded('KLLoss', dev(p), dev(q), dev(y), nv, margin, avg, acc)
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    de = de.cpu().numpy()
    assert np.all(de[:, nvalid:] == 0.0)
    check_rows(de[0, :nvalid], r1, n)
    check_rows(de[1, :nvalid], r2, n)
    loss2, _ = _padded('KLLoss', dev(p), dev(q), dev(y), nv, margin, avg, acc)
    assert float(loss2) == float(loss)
    assert float(acc) == 2 * float(np.float32(float(loss)))


@pytest.mark.parametrize('n', ['b0', 'b1', 'u1'])
def test_dropout_masks_are_folded_in_last(n):
    """value_and_dz(..., 'softmax', masks) = the unmasked dz times the mask, bit for bit (D = 100: 16-byte path; 39: scalar)."""
    g = g12()
    z1, z2, y = dev(g[n + '.in1']), dev(g[n + '.in2']), dev(g[n + '.y'])
    torch.manual_seed(0)
    keep = 1.0 / (1.0 - 0.3)
    m1 = (torch.rand_like(z1) > 0.3).float() * keep
    m2 = (torch.rand_like(z2) > 0.3).float() * keep
    l0, dz0 = kl(g, n).value_and_dz(z1, z2, y, 'softmax', None)
    l1, dz1 = kl(g, n).value_and_dz(z1, z2, y, 'softmax', (m1, m2))
    assert float(l0) == float(l1)
    assert torch.equal(dz1[0], dz0[0] * m1) and torch.equal(dz1[1], dz0[1] * m2)


# -- a softmax network trained with KLLoss (G12 c) --------------------------------------------------------------------

LR = {'sgd': 0.001, 'adadelta': 0.1}


def c_net(g, bn):
    """The reference's initial network: its Linear layers' parameters from the fixture (the same with and without
    BatchNorm), BatchNorm at its constructor's values (weight 1, bias 0, running statistics 0 / 1)."""
    from abnet3_amd.model import SiameseNetwork
    kw = ast.literal_eval(str(g['c.bn%d.kw' % bn]))
    net = SiameseNetwork(output_path='/tmp/abn_kl_test', **kw)
    pre = 'c.p.'
    sd = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(pre)}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith(('input_emb.2.', 'output_layer.2.')) for k in missing), (missing, unexpected)
    assert len(sd) == 4
    return net.cuda()


def c_trainer(net, oname, direct=True):
    from abnet3_amd.loss import KLLoss
    from abnet3_amd.trainer import TrainerSiamese
    tr = TrainerSiamese(network=net, loss=KLLoss(), optimizer_type=oname, lr=LR[oname], momentum=0.9, dataloader=None,
                        log_dir='/tmp/abn_runs')
    if not direct:
        tr.direct_steps = False
    assert tr._direct_ok() == direct
    return tr


def grads_of(net):
    return {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}


def params_of(net):
    return {k: p.detach().cpu().numpy().copy() for k, p in net.named_parameters()}


def run3(g, bn, oname, mode, direct=True):
    net = c_net(g, bn)
    tr = c_trainer(net, oname, direct)
    batch = (dev(g['c.x1']), dev(g['c.x2']), dev(g['c.y']))
    net.train()
    if mode == 'eager':
        losses = [float(tr.train_step(batch, True))]
        grads = grads_of(net)
        losses += [float(tr.train_step(batch, True)) for _ in range(2)]
    else:
        step = tr.make_graphed_step(batch, warmup=1)        # its warm-up step is step 1
        grads = None
        losses = [float(step.warmup_loss)] + [float(step(batch)) for _ in range(2)]
    assert tr.optimizer.step_count == 3
    return losses, grads, params_of(net)


@pytest.mark.parametrize('bn', [0, 1])
@pytest.mark.parametrize('oname', ['sgd', 'adadelta'])
@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_softmax_kl_training_vs_reference(bn, oname, mode):
    """G12 (c): three steps of TrainerSiamese.train_step's direct path (softmax, loss and gradient in one launch)
    -- and of a captured step -- against the reference's losses, first-step gradients and parameters after 3 steps;
    and against the autograd path (direct_steps = False) at the same bars.  (The reference's own fp32 run is within
    3e-6 of its float64 run on every compared tensor here -- the fixture's float64 losses show the same -- so the fp32
    bars of check_grads / check_params apply as they stand.)"""
    g = g12()
    tag = 'c.bn%d.%s' % (bn, oname)
    pre = 'c.bn%d.grad0.' % bn
    keys = [k[len(pre):] for k in g if k.startswith(pre)]
    losses, grads, params = run3(g, bn, oname, mode)
    assert np.allclose(losses, g[tag + '.losses'], rtol=1e-5, atol=0), (losses, g[tag + '.losses'])
    assert np.allclose(g[tag + '.losses'], g[tag + '.f64.losses'], rtol=1e-6, atol=0)
    check_params(params, {k: g['%s.after.%s' % (tag, k)] for k in keys}, keys, bool(bn))
    if grads is not None:
        check_grads(grads, {k: g[pre + k] for k in keys}, keys, bool(bn))
        a_losses, a_grads, a_params = run3(g, bn, oname, 'eager', direct=False)
        assert np.allclose(losses, a_losses, rtol=1e-5, atol=0), (losses, a_losses)
        check_grads(grads, a_grads, keys, bool(bn))
        check_params(params, a_params, keys, bool(bn))


def test_graphed_step_equals_eager_autograd_bit_for_bit():
    """make_graphed_step captures the autograd path (forward_pair_rows, then KLLoss.forward): five steps of it
    (one warm-up, four replays) equal five eager direct_steps = False steps bit for bit."""
    g = g12()
    rng = np.random.default_rng(5)
    batches = [(dev(rng.standard_normal((64, 40)).astype(np.float32)), dev(rng.standard_normal((64, 40)).astype(np.float32)),
                dev(rng.choice([1, -1], 64))) for _ in range(3)]
    res = []
    for mode in ('eager', 'graph'):
        net = c_net(g, 0)
        tr = c_trainer(net, 'adadelta', direct=False)
        net.train()
        if mode == 'eager':
            losses = [float(tr.train_step(batches[s % 3], True)) for s in range(5)]
        else:
            step = tr.make_graphed_step(batches[0], warmup=1)
            losses = [float(step.warmup_loss)] + [float(step(batches[s % 3])) for s in range(1, 5)]
        res.append((losses, params_of(net)))
    assert res[0][0] == res[1][0]
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k


def test_original_loader_trains_with_kl(tmp_path):
    """The canonical loader (8 word pairs a batch) with KLLoss: no planned passes (their loss rides in the backward,
    which has the cosine losses only), the iterator with the direct step; the losses are finite and those of a run
    with planned_passes = False."""
    from test_gpu_pipeline import _loader
    from tools.c5_corpus import sample_pairs, synth_corpus
    from abnet3_amd.loss import KLLoss
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    corpus = synth_corpus(n_utts=30, n_types=20, seed=3, device='cuda')
    train_pairs, dev_pairs = sample_pairs(corpus, n_pairs=160, seed=3)
    res = []
    for planned in (True, False):
        dl = _loader('original', (corpus, train_pairs, dev_pairs))
        np.random.seed(0)
        torch.manual_seed(0)
        net = SiameseNetwork(input_dim=280, num_hidden_layers=1, hidden_dim=128, output_dim=32, p_dropout=0.0,
                             activation_layer='sigmoid', last_non_linearity='softmax', output_path=str(tmp_path / ('n%d' % planned)))
        tr = TrainerSiamese(network=net, loss=KLLoss(margin=1), num_epochs=1, patience=5, optimizer_type='adadelta', lr=0.1,
                            dataloader=dl, log_dir=str(tmp_path / 'runs'))
        tr.planned_passes = planned
        assert tr._direct_ok() and tr._planned(True) is None
        tr.train()
        assert not getattr(tr, '_buckets', None)
        res.append((list(tr.train_losses), list(tr.dev_losses), params_of(net)))
    (tl_a, dl_a, p_a), (tl_b, dl_b, p_b) = res
    assert all(np.isfinite(tl_a)) and all(np.isfinite(dl_a)) and len(tl_a) == 2
    assert tl_a == tl_b and dl_a == dl_b
    for k in p_a:
        assert np.array_equal(p_a[k], p_b[k]), k


def test_existing_kinds_unaffected():
    """ABN_ACT_SOFTMAX belongs to KLLoss alone; abn_tower_backward_loss has no KL; softmax + coscos2 keeps autograd."""
    from abnet3_amd import _lib
    from abnet3_amd.loss import coscos2, _scratch
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    lib = _lib.load()
    B, D = 16, 8
    e = torch.rand(2, B, D, device='cuda') + 0.1
    y = torch.ones(B, dtype=torch.int64, device='cuda')
    loss = torch.empty((), device='cuda')
    dz = torch.empty(2, B, D, device='cuda')
    ws = _scratch(lib.abn_pair_loss_ws_bytes(B), e.device)
    rc = lib.abn_pair_loss_dz(_lib.ptr(e[0]), _lib.ptr(e[1]), _lib.ptr(y), _lib.Y_DTYPE[y.dtype], B, D, _lib.LOSS['coscos2'],
                              0.0, 1, _lib.ACT_SOFTMAX, None, None, _lib.ptr(loss), _lib.ptr(dz[0]), _lib.ptr(dz[1]),
                              _lib.ptr(ws), _lib.stream())
    assert rc == _lib.E_UNSUPPORTED
    rc = lib.abn_tower_backward_loss(None, None, None, _lib.ptr(y), _lib.Y_DTYPE[y.dtype], _lib.LOSS['KLLoss'], 1.0, 1, 2 * B,
                                     None, None, 0, _lib.ptr(loss), _lib.ptr(ws), None, None, _lib.stream())
    assert rc == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    # the cosine losses still run on the same scratch afterwards (nothing was launched)
    lv, _ = coscos2().value_and_grad(e[0], e[1], y)
    assert np.isfinite(float(lv.detach()))
    net = SiameseNetwork(input_dim=40, num_hidden_layers=0, hidden_dim=100, output_dim=50, p_dropout=0.0,
                         activation_layer='sigmoid', last_non_linearity='softmax', output_path='/tmp/abn_kl_test').cuda()
    tr = TrainerSiamese(network=net, loss=coscos2(), optimizer_type='sgd', lr=0.001, dataloader=None, log_dir='/tmp/abn_runs')
    assert tr._direct_ok() is False


def test_direct_backward_loss_declines_kl_before_any_launch():
    """SiameseNetwork.direct_backward_loss with KLLoss returns None without a launch, without a KeyError and without
    leaving _fused_loss_refused set for a later cosine loss."""
    g = g12()
    net = c_net(g, 0)
    net.train()
    emb, state = net.direct_forward(dev(g['c.x1']), dev(g['c.x2']))
    assert net.direct_backward_loss(state, dev(g['c.y']), 'KLLoss', 1.0, True) is None
    assert net._fused_loss_refused is None


def test_weighted_loss_multi_with_kl_sub_losses():
    """weighted_loss_multi(loss_spk=KLLoss(), loss_phn=KLLoss()) on a sigmoid SiameseMultitaskNetwork (positive
    outputs: the probability form is defined on them, unnormalised KL as the reference computes it): one autograd
    step whose loss and gradients are the weighted sum of the two separate losses'."""
    import abnet3_amd.loss as L
    from abnet3_amd.model import SiameseMultitaskNetwork
    g = load_golden('multitask_sig.npz')
    w = 0.3

    def fresh():
        net = SiameseMultitaskNetwork(**ast.literal_eval(str(g['kw'])))
        net.load_state_dict({k[2:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith('p.')})
        return net.cuda().train()
    x1, x2 = dev(g['x1']), dev(g['x2'])
    y_spk, y_phn = dev(g['y_spk']), dev(g['y_phn'])
    spk, phn = L.KLLoss(margin=1), L.KLLoss(margin=0.5, avg=False)
    net = fresh()
    opt = torch.optim.SGD(net.parameters(), lr=0.001, momentum=0.9)
    emb = net(x1, x2)
    lv = L.weighted_loss_multi(loss_spk=spk, loss_phn=phn, weight=w)(emb[0], emb[1], emb[2], emb[3], y_spk, y_phn)
    opt.zero_grad()
    lv.backward()
    live = [k for k, p in net.named_parameters() if p.grad is not None]
    total = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters() if p.grad is not None}
    parts = []
    for which in ('spk', 'phn'):
        n2 = fresh()
        e = n2(x1, x2)
        part = spk(e[0], e[2], y_spk) if which == 'spk' else phn(e[1], e[3], y_phn)
        part.backward()
        parts.append((float(part.detach()), {k: p.grad.detach().cpu().numpy() if p.grad is not None else 0.0
                                    for k, p in n2.named_parameters()}))
    assert np.isfinite(float(lv.detach()))
    lval = float(lv.detach())
    assert abs(lval - (w * parts[0][0] + (1 - w) * parts[1][0])) <= 1e-6 * abs(lval)
    for k in live:
        ref = w * parts[0][1][k] + (1 - w) * parts[1][1][k]
        assert rel_err(total[k], ref) < 1e-5, (k, rel_err(total[k], ref))
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt.step()
    assert any(not torch.equal(before[k], p) for k, p in net.named_parameters())
