"""The multimodal family on the MI355X: the integration kernel (csrc/integrate.hip) against the float64
restatement (tests/mm_np.py), MultimodalSiameseNetwork trained against the reference's own outputs
(tests/golden/multimodal.npz, tools/make_golden.py G13), the headstart schedules, MultimodalDataLoader's batches,
MultimodalTrainer.train() on files, save / load and MultimodalEmbedder.  Needs an MI355X: run with -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

import mm_np
from conftest import load_golden, rel_err
from test_multimodal_host import CONFIG_TABLE, SEEDS, build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def g13():
    return load_golden('multimodal.npz')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def launch(mode, kind, x1, x2, g=None, w=None, wc=None, z=None, act='sigmoid', K=1):
    """abn_integrate_forward (+ abn_integrate_backward when g is given) straight through the C ABI:
    (out, w_out, dx1, dx2, dz, dw) as numpy."""
    from abnet3_amd import _lib
    from abnet3_amd.loss import _scratch
    lib = _lib.load()
    kinds = {'none': _lib.W_NONE, 'fixed': _lib.W_FIXED, 'scalar': _lib.W_SCALAR, 'attention': _lib.W_ATTENTION}
    k = kinds[kind]
    R, d1, d2 = x1.shape[0], x1.shape[1], x2.shape[1]
    x1, x2 = dev(x1), dev(x2)
    z1 = z2 = None
    if z is not None:
        z1 = dev(z[0])
        z2 = dev(z[1])
    wp = dev(np.array([w], np.float32)) if kind == 'scalar' else None
    wf = float(w) if kind == 'fixed' else 0.0
    wcf = float(wc) if kind == 'fixed' else 0.0
    dout = d1 if mode == 'sum' else d1 + d2
    out = torch.empty(R, dout, device='cuda')
    w_out = torch.empty(R, K, device='cuda') if kind == 'attention' else None
    a = _lib.ACT[act]
    _lib.check(lib.abn_integrate_forward(_lib.ptr(x1), d1, _lib.ptr(x2), d2, R, _lib.INTEGRATE_MODE[mode], k, wf, wcf,
                                         _lib.ptr(wp), _lib.ptr(z1), _lib.ptr(z2), K, a, _lib.ptr(out), _lib.ptr(w_out),
                                         _lib.stream()), 'forward')
    res = [out.cpu().numpy(), None if w_out is None else w_out.cpu().numpy(), None, None, None, None]
    if g is not None:
        g = dev(g)
        dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
        dz = torch.empty(R, K, device='cuda') if kind == 'attention' else None
        dw = torch.full((1,), 7.0, device='cuda') if kind == 'scalar' else None
        ws = _scratch(lib.abn_integrate_ws_bytes(R), x1.device)
        _lib.check(lib.abn_integrate_backward(_lib.ptr(x1), d1, _lib.ptr(x2), d2, R, _lib.INTEGRATE_MODE[mode], k, wf, wcf,
                                              _lib.ptr(wp), _lib.ptr(w_out), K, a, _lib.ptr(g), _lib.ptr(dx1), _lib.ptr(dx2),
                                              _lib.ptr(dz), _lib.ptr(dw), _lib.ptr(ws), _lib.stream()), 'backward')
        res[2:] = [dx1.cpu().numpy(), dx2.cpu().numpy(), None if dz is None else dz.cpu().numpy(),
                   None if dw is None else dw.cpu().numpy()]
    return res


def rel(a, b):
    return rel_err(a, b, floor=1e-30)


SHAPES = [(0, 13, 13), (1, 13, 13), (37, 13, 13), (37, 13, 7), (8192, 500, 500), (8192, 12, 20), (5, 4, 8)]


KERNEL_CASES = [(R, d1, d2, mode, kind) for R, d1, d2 in SHAPES for mode in ('sum', 'concat')
                for kind in ('none', 'fixed', 'scalar', 'attention_k1', 'attention_kd', 'attention_kd_tanh')
                if d1 == d2 or (mode == 'concat' and not kind.startswith('attention_kd'))]   # (what the kernel takes)


@pytest.mark.parametrize('R,d1,d2,mode,kind', KERNEL_CASES)
def test_kernel_against_numpy(R, d1, d2, mode, kind):
    rng = np.random.default_rng(R * 7 + d1 + d2)
    x1 = rng.standard_normal((R, d1)).astype(np.float32)
    x2 = rng.standard_normal((R, d2)).astype(np.float32)
    g = rng.standard_normal((R, d1 if mode == 'sum' else d1 + d2)).astype(np.float32)
    act = 'tanh' if kind.endswith('tanh') else 'sigmoid'
    if kind.startswith('attention'):
        K = 1 if kind == 'attention_k1' else d1
        z = (rng.standard_normal((R, K)).astype(np.float32), rng.standard_normal((R, K)).astype(np.float32))
        out, w_out, dx1, dx2, dz, _ = launch(mode, 'attention', x1, x2, g, z=z, act=act, K=K)
        zs = z[0] + z[1]                          # (fp32, as the kernel and torch's add)
        w, wc = mm_np.weights('attention', R, z=zs, act_name=act)
        assert R == 0 or rel(w_out, w) <= 1e-6
        ref = mm_np.forward(mode, x1, x2, w, wc)
        rdx1, rdx2, rdz, _ = mm_np.backward(mode, 'attention', x1, x2, g, w, wc, act)
        if R:
            assert rel(out, ref) <= 1e-5 and rel(dx1, rdx1) <= 1e-5 and rel(dx2, rdx2) <= 1e-5
            assert rel(dz, rdz) <= 1e-5
        return
    wv = {'none': 1.0, 'fixed': 0.3, 'scalar': 0.6}[kind]
    wcv = float(np.float32(1 - wv)) if kind == 'fixed' else None
    out, _, dx1, dx2, _, dw = launch(mode, kind, x1, x2, g, w=wv, wc=wcv)
    w32 = np.float32(wv)
    wc32 = np.float32(wcv) if kind == 'fixed' else np.float32(np.float32(1) - w32)
    if kind == 'none':
        exact = x1 + x2 if mode == 'sum' else np.concatenate((x1, x2), 1)
    elif mode == 'sum':
        exact = w32 * x1 + wc32 * x2
    else:
        exact = np.concatenate((w32 * x1, wc32 * x2), 1)
    assert np.array_equal(out, exact)            # bit for bit: the float32 expression, no contraction
    w, wc = mm_np.weights(kind, R, w=float(w32)) if kind != 'none' else mm_np.weights('none', R)
    if kind == 'fixed':
        wc = np.full_like(w, float(wc32))
    rdx1, rdx2, _, rdw = mm_np.backward(mode, kind, x1, x2, g, w, wc)
    if R:
        assert rel(dx1, rdx1) <= 1e-5 and rel(dx2, rdx2) <= 1e-5
    if kind == 'scalar':
        if R == 0:
            assert dw[0] == 0.0
        else:
            assert abs(float(dw[0]) - rdw[0]) <= 1e-5 * max(abs(rdw[0]), np.abs(g).sum() * 1e-3)
            again = launch(mode, kind, x1, x2, g, w=wv)[5]
            assert np.array_equal(again.view(np.uint32), dw.view(np.uint32))     # the same bits, run after run


def test_kernel_rejects_bad_arguments():
    from abnet3_amd import _lib
    lib = _lib.load()
    x = dev(np.zeros((4, 6), np.float32))
    out = torch.empty(4, 6, device='cuda')
    # sum of unequal widths, attention K that is neither 1 nor the width
    assert lib.abn_integrate_forward(_lib.ptr(x), 6, _lib.ptr(x), 5, 4, 0, 0, 0.0, 0.0, None, None, None, 1, 1,
                                     _lib.ptr(out), None, _lib.stream()) != 0
    assert lib.abn_integrate_forward(_lib.ptr(x), 6, _lib.ptr(x), 6, 4, 0, 3, 0.0, 0.0, None, _lib.ptr(x), _lib.ptr(x), 3,
                                     1, _lib.ptr(out), None, _lib.stream()) != 0


def g13_net(name):
    net = build(name).cuda()
    net.train()
    return net


def pre_bn_bias(k, bn):
    """A Linear bias in front of a BatchNorm (module index j % 4 == 0 of a pre-net or the post-net): its gradient is
    rounding noise on both sides."""
    if not bn or not k.endswith('.bias'):
        return False
    parts = k.split('.')
    j = int(parts[2]) if parts[0] == 'pre_nets' else int(parts[1]) if parts[0] == 'post_net' else 1
    return j % 4 == 0


def check_grad(mine, ref32, ref64, floor, k):
    """Within 2e-5 of the reference's fp32 gradient (relative to the tensor's largest entry, at least `floor`), or, where
    that one is itself further from the float64 evaluation (tiny towers: the post-net bias gradient is a heavily cancelled
    sum, the reference's own fp32 error reaches 1e-3 there), no further from the float64 value than twice the
    reference's fp32 error plus 1e-5 (the float64 yardstick of tests/test_gpu_kl_loss.py)."""
    e32 = rel_err(mine, ref32, floor=floor)
    if e32 <= 2e-5:
        return
    scale = max(np.abs(ref64).max(), floor)
    e_mine = np.abs(mine - ref64).max() / scale
    e_ref = np.abs(ref32 - ref64).max() / scale
    assert e_mine <= 2 * e_ref + 1e-5, (k, e32, e_mine, e_ref)


def check_state(sd, g, pfx, bn):
    """Every tensor of the network against the reference's after some steps, within 1e-5 of its largest entry or of 1 %
    of the largest entry in the model, whichever is larger: a bias that started at zero and moved by 1e-5 holds the
    (relative) error of its heavily cancelled gradient, which check_grad bounds against float64."""
    keys = [k[len(pfx):] for k in g if k.startswith(pfx)]
    assert sorted(keys) == sorted(sd)
    big = max(np.abs(g[pfx + k]).max() for k in keys if 'running' not in k and 'num_batches' not in k)
    for k in keys:
        if pre_bn_bias(k, bn) or k.endswith('num_batches_tracked'):
            continue
        e = rel_err(sd[k], g[pfx + k], floor=1e-2 * big)
        assert e <= 1e-5, (pfx, k, e)


def batch(g, prefix):
    X1 = [dev(g['%s.X1_%d' % (prefix, m)]) for m in range(2)]
    X2 = [dev(g['%s.X2_%d' % (prefix, m)]) for m in range(2)]
    return X1, X2, torch.from_numpy(g[prefix + '.y']).cuda()


def trainer(net, optim, lr, tmp_path, headstart=None):
    from abnet3_amd.dataloader import MultimodalDataLoader
    from abnet3_amd.loss import coscos2
    from abnet3_amd.trainer import MultimodalTrainer
    dl = MultimodalDataLoader('unused', ['m0', 'm1'])
    return MultimodalTrainer(headstart=headstart, network=net, loss=coscos2(avg=False), optimizer_type=optim, lr=lr,
                             momentum=0.9, dataloader=dl, log_dir=str(tmp_path))


@pytest.mark.parametrize('name', sorted(CONFIG_TABLE))
@pytest.mark.parametrize('optim', ['sgd', 'adadelta'])
def test_g13_training(name, optim, tmp_path):
    g = g13()
    bn = CONFIG_TABLE[name][4].get('batch_norm', False)
    net = g13_net(name)
    tr = trainer(net, optim, 0.001 if optim == 'sgd' else 0.1, tmp_path)
    X1, X2, y = batch(g, name)
    losses = []
    for s in range(3):
        if s == 0:
            # (a look at the first forward; the BatchNorm running statistics it moves are put back)
            keep = {k: v.clone() for k, v in net.state_dict().items()}
            e1, e2 = net(X1, X2)
            net.load_state_dict(keep)
            assert rel(e1.detach().cpu().numpy(), g[name + '.e1']) <= 1e-5
            assert rel(e2.detach().cpu().numpy(), g[name + '.e2']) <= 1e-5
            if name + '.w_last' in g:
                assert rel(net.integration_unit.get_weights().cpu().numpy(), g[name + '.w_last']) <= 1e-5
        losses.append(float(tr.train_step((X1, X2, y), True)))
        if s == 0:
            grads = {k: p.grad.cpu().numpy() for k, p in net.named_parameters() if p.grad is not None}
            keys = [k[len(name + '.grad.'):] for k in g if k.startswith(name + '.grad.')]
            assert sorted(grads) == sorted(keys)
            gmax = max(np.abs(g['%s.grad.%s' % (name, k)]).max() for k in keys)
            for k in keys:
                ref = g['%s.grad.%s' % (name, k)]
                if pre_bn_bias(k, bn):
                    assert np.abs(grads[k]).max() <= 1e-4 * gmax, k
                    continue
                check_grad(grads[k], ref, g['%s.f64.grad.%s' % (name, k)], 1e-2 * gmax, k)
    ref_losses = g['%s.%s.losses' % (name, optim)]
    assert abs(losses[0] - g[name + '.loss']) <= 1e-5 * abs(g[name + '.loss'])
    assert abs(losses[0] - g[name + '.f64.loss']) <= 1e-5 * abs(g[name + '.f64.loss'])
    assert np.abs(np.array(losses) - ref_losses).max() <= 1e-5 * np.abs(ref_losses).max()
    pfx = '%s.%s.after.' % (name, optim)
    check_state({k: v.cpu().numpy() for k, v in net.state_dict().items()}, g, pfx, bn)


@pytest.mark.parametrize('tag,hs', [('hs_true', (2, True, 0.3)), ('hs_false', (2, False, 0.3))])
def test_headstart_schedules(tag, hs, tmp_path):
    g = g13()
    net = build('deep_k1_sum', seed=1500).cuda()
    sd0 = net.state_dict()
    for k, v in sd0.items():
        assert np.array_equal(v.cpu().numpy(), g[tag + '.init.' + k]), k
    tr = trainer(net, 'adadelta', 0.1, tmp_path, headstart=hs)
    batches = [batch(g, '%s.b%d' % (tag, b)) for b in range(2)]
    tr.dataloader.batch_iterator = lambda train_mode=True: iter(batches if train_mode else [])
    tr.train_losses, tr.dev_losses = [], []
    before = None
    for epoch in range(4):
        tr.optimize_model(True)
        sd = {k: v.cpu().numpy() for k, v in net.state_dict().items()}
        check_state(sd, g, '%s.epoch%d.' % (tag, epoch), False)
        frozen = [k for k in sd if k.startswith('integration_unit.')] if epoch < 2 else \
            ([k for k in sd if k.startswith('post_net.')] if not hs[1] and epoch >= 2 else [])
        for k in frozen:                     # a frozen parameter: no update at all
            assert before is not None or epoch == 0
            ref = before[k] if before is not None else sd0[k].cpu().numpy()
            assert np.array_equal(sd[k], ref), (epoch, k)
        before = sd
        ref_loss = g[tag + '.losses'][2 * epoch:2 * epoch + 2].mean()
        assert abs(tr.train_losses[-1] - ref_loss) <= 1e-5 * abs(ref_loss)


def test_headstart_needs_a_unit_that_takes_one(tmp_path):
    net = g13_net('fixed_sum')
    with pytest.raises(TypeError, match='set_headstart_weight'):
        trainer(net, 'sgd', 0.1, tmp_path, headstart=(1, True, 0.5))


def _pairs(arr):
    out = []
    for line in arr:
        f1, s1, e1, f2, s2, e2, t = str(line).split()
        out.append((f1, float(s1), float(e1), f2, float(s2), float(e2), t))
    return out


def _loader(g, **kw):
    from abnet3_amd.dataloader import MultimodalDataLoader
    names = sorted(k[len('dl.feat0.'):] for k in g if k.startswith('dl.feat0.'))
    f0 = {k: g['dl.feat0.' + k] for k in names}
    f1 = {k: g['dl.feat1.' + k] for k in names}
    times = {k: np.arange(len(v)) * 0.01 + 0.0025 for k, v in f0.items()}
    dl = MultimodalDataLoader('unused', ['m0', 'm1'], **kw)
    dl.set_data([f0, f1], times, _pairs(g['dl.train_pairs']), _pairs(g['dl.dev_pairs']))
    return dl, f0, f1, times


@pytest.mark.parametrize('name', ['dl_rand', 'dl_sub'])
def test_loader_batches_bit_exact(name):
    import ast
    g = g13()
    dl, *_ = _loader(g, **ast.literal_eval(str(g[name + '.kw'])))
    assert dl.plan(True) is None
    np.random.seed(int(g[name + '.seed']))
    X1s, X2s, Ys, sizes = [[], []], [[], []], [], []
    for mode in 'TDT':
        for X1, X2, y in dl.batch_iterator(train_mode=(mode == 'T')):
            for m in range(2):
                X1s[m].append(X1[m].cpu().numpy()); X2s[m].append(X2[m].cpu().numpy())
            Ys.append(y.cpu().numpy()); sizes.append(len(y))
    assert sizes == list(g[name + '.sizes'])
    for m in range(2):
        assert np.array_equal(np.vstack(X1s[m]), g['%s.X1_%d' % (name, m)])
        assert np.array_equal(np.vstack(X2s[m]), g['%s.X2_%d' % (name, m)])
    assert np.array_equal(np.concatenate(Ys).astype(np.float64), g[name + '.y'].astype(np.float64))


def test_loader_rejects_inconsistent_modalities():
    g = g13()
    dl, f0, f1, times = _loader(g)
    bad = dict(f1)
    k = next(iter(bad))
    bad[k] = bad[k][:-1]
    with pytest.raises(ValueError):
        dl.set_data([f0, bad], times)
    with pytest.raises(ValueError):
        dl.set_data([f0, {kk: v for kk, v in f1.items() if kk != k}], times)


def test_save_load_round_trip_and_reference_files(tmp_path):
    net = g13_net('deep_kd_concat_async1_bn')
    path = str(tmp_path) + '/'
    net.output_path = path
    net.integration_unit.output_path = path
    net.save_network()
    assert os.path.exists(path + 'network.pth') and os.path.exists(path + 'integration.pth')
    other = build('deep_kd_concat_async1_bn', seed=77).cuda()
    other.load_network(path)
    for (k, a), b in zip(net.state_dict().items(), other.state_dict().values()):
        assert torch.equal(a, b), k
    # a file written by the reference: no pre-net keys -- the pre-nets keep their weights, one warning
    sd = {k: v for k, v in net.state_dict().items() if not k.startswith('pre_nets.')}
    torch.save(sd, path + 'refnetwork.pth')
    torch.save(net.integration_unit.state_dict(), path + 'refintegration.pth')
    third = build('deep_kd_concat_async1_bn', seed=78).cuda()
    pre_before = {k: v.clone() for k, v in third.state_dict().items() if k.startswith('pre_nets.')}
    with pytest.warns(UserWarning, match='pre-net'):
        third.load_network(path + 'ref')
    for k, v in third.state_dict().items():
        assert torch.equal(v, pre_before[k] if k.startswith('pre_nets.') else net.state_dict()[k]), k
    X1, X2, y = batch(g13(), 'deep_kd_concat_async1_bn')
    third.train()
    e1, _ = third(X1, X2)
    assert torch.isfinite(e1).all()


def test_embedder_and_observer(tmp_path):
    from abnet3_amd.embedder import MultimodalEmbedder
    net = g13_net('deep_k1_sum')
    emb = MultimodalEmbedder(network=net, output_path=str(tmp_path) + '/')
    assert len(emb.observers) == 1
    rng = np.random.default_rng(3)
    lens = [17, 1, 40]
    f0 = [rng.standard_normal((n, 10)).astype(np.float32) for n in lens]
    f1 = [rng.standard_normal((n, 6)).astype(np.float64) for n in lens]
    out = emb.embed_features([f0, f1])
    obs = emb.observers[0].intern_responses
    assert len(out) == len(lens) and len(obs) == len(lens)
    net.eval()
    with torch.no_grad():
        for i, n in enumerate(lens):
            ref = net.forward_once([dev(f0[i]), dev(f1[i].astype(np.float32))]).cpu().numpy()
            assert out[i].shape == (n, 8) and np.array_equal(out[i], ref)
            assert obs[i].shape == (n, 1)
            assert np.array_equal(obs[i], net.integration_unit.get_weights().cpu().numpy())


def test_train_on_files(tmp_path, monkeypatch):
    """MultimodalTrainer.train() end to end: two h5features files (the fake stand-in of tests/fake_h5features.py),
    pairs files, the network saved, then MultimodalEmbedder.embed() on the files."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_h5features as h5features
    monkeypatch.setitem(sys.modules, 'h5features', h5features)
    from abnet3_amd.dataloader import MultimodalDataLoader
    from abnet3_amd.embedder import MultimodalEmbedder
    from abnet3_amd.loss import coscos2
    from abnet3_amd.trainer import MultimodalTrainer
    from abnet3_amd.utils import write_dataset
    g = g13()
    names = sorted(k[len('dl.feat0.'):] for k in g if k.startswith('dl.feat0.'))
    paths = []
    for m, d in ((0, 12), (1, 7)):
        p = str(tmp_path / ('m%d.features' % m))
        feats = [g['dl.feat%d.%s' % (m, k)] for k in names]
        h5features.write(p, 'features', names, [np.arange(len(f)) * 0.01 + 0.0025 for f in feats], feats)
        paths.append(p)
    for sub, key in (('train_pairs', 'dl.train_pairs'), ('dev_pairs', 'dl.dev_pairs')):
        (tmp_path / 'pairs' / sub).mkdir(parents=True)
        write_dataset(str(tmp_path / 'pairs' / sub / 'dataset'), _pairs(g[key]))
    from abnet3_amd import integration
    from abnet3_amd.model import MultimodalSiameseNetwork
    torch.manual_seed(0)
    np.random.seed(0)
    unit = integration.BiWeightedDeepLearnt(net_params=[[16, 1], [16, 1]], output_path=str(tmp_path) + '/')
    net = MultimodalSiameseNetwork(integration_unit=unit, pre_integration_net_params=[[12, 16], [7, 16]],
                                   post_integration_net_params=[16, 8], activation_layer='sigmoid',
                                   output_path=str(tmp_path) + '/')
    dl = MultimodalDataLoader(str(tmp_path / 'pairs'), paths, batch_size=16, randomize_dataset=True)
    tr = MultimodalTrainer(headstart=(1, False, 0.5), network=net, loss=coscos2(avg=False), optimizer_type='adadelta',
                           lr=0.1, num_epochs=3, patience=5, dataloader=dl, log_dir=str(tmp_path / 'logs'))
    tr.train()
    assert len(tr.train_losses) == 4 and np.isfinite(tr.train_losses).all()
    assert os.path.exists(str(tmp_path) + '/network.pth') and os.path.exists(str(tmp_path) + '/integration.pth')
    emb = MultimodalEmbedder(network=net, network_path=str(tmp_path) + '/', feature_path=paths,
                             output_path=str(tmp_path) + '/')
    emb.embed()
    with h5features.Reader(str(tmp_path) + '/embedded.features', 'features') as fh:
        e = fh.read()
    assert list(e.items()) == names
    with h5features.Reader(str(tmp_path) + '/attention_weights.features', 'features') as fh:
        w = fh.read()
    for k in names:
        n = len(g['dl.feat0.' + k])
        assert e.dict_features()[k].shape == (n, 8) and w.dict_features()[k].shape == (n, 1)
