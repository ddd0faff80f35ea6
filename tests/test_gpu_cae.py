"""abnr_recon_loss, CorrespondenceLoss, CorrespondenceAutoencoder and TrainerCorrespondence on the MI355X against
tests/cae_np.py.

The kernel's bars: the inputs are fp32, every difference and every sum is float64, and each output is
rounded to fp32 once -- 2^-24 relative, plus float64 noise (at most D 2^-53 per row sum) and the restatement's own.  The
tests hold loss and terms to 4 * 2^-24 and every gradient element to 3 * 2^-24 of the float64 value; rows outside R, and dr2
without `symmetric`, to exactly 0.  The network is held to the project's bars: 1e-5 by conftest.rel_err against the float32
torch-CPU evaluation of the same modules, and for gradients and trained parameters the float64 yardstick of
test_gpu_timed_path.test_c2_backward_judged_against_float64."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cae_np  # noqa: E402
import dirty_memory  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

bits = dirty_memory.bits
EPS = 2.0 ** -24
VALUE_BAR, GRAD_BAR = 4 * EPS, 3 * EPS
BS, DS = (1, 7, 8, 9, 33, 257), (1, 3, 4, 39, 40, 65, 280, 513)
VARIANTS = list(itertools.product(cae_np.MODES, (True, False), (True, False)))          # mode, symmetric, avg
Y_DTYPES = (torch.int8, torch.int32, torch.int64, torch.float32, torch.float64)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def raw(r1, r2, x1, x2, y, mode, symmetric, avg, grad=True, want_terms=True):
    """(loss, terms, dr1, dr2) host arrays of abnr_recon_loss on DEVICE tensors as they are (no copy: a test may hand in a
    misaligned view), every output and the workspace from torch.empty."""
    from abnet3_amd import _lib
    from abnet3_amd.loss import RECON_MODE
    lib, p = _lib.load(), _lib.ptr
    B, D = r1.shape
    need = lib.abnr_recon_ws_bytes(B, D)
    assert need > 0
    loss = torch.empty((), dtype=torch.float32, device='cuda')
    terms = torch.empty(B, dtype=torch.float32, device='cuda') if want_terms else None
    dr = torch.empty(2, B, D, dtype=torch.float32, device='cuda') if grad else None
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    rc = lib.abnr_recon_loss(p(r1), p(r2), p(x1), p(x2), p(y), _lib.Y_DTYPE[y.dtype] if y is not None else 0, B, D, RECON_MODE[mode],
                             int(symmetric), int(avg), p(loss), p(terms), p(dr[0]) if grad else None, p(dr[1]) if grad else None, p(ws),
                             _lib.stream())
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return (host(loss), host(terms) if want_terms else None, host(dr[0]) if grad else None, host(dr[1]) if grad else None)


def same(a, b):
    return all((u is None and v is None) or np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


_CASE = {}


def case(B, D, seed=0):
    """A shape's inputs (host and device) and the float64 restatement of every variant: made once, shared, never written."""
    key = (B, D, seed)
    if key not in _CASE:
        h = cae_np.draw(np.random.default_rng(1000 * B + D + seed), B, D)
        if B > 1:
            h[4][0], h[4][1] = 1, -1                                                     # a counted and an uncounted row at least
        _CASE[key] = (h, tuple(dev(a) for a in h), {v: cae_np.recon_loss(*h, *v) for v in VARIANTS})
    return _CASE[key]


def check(got, ref, counted, symmetric, tag):
    loss, terms, dr1, dr2 = got
    lv, t64, g1, g2 = ref
    assert abs(float(loss) - lv) <= VALUE_BAR * abs(lv), (tag, float(loss), lv)
    assert (np.abs(terms.astype(np.float64) - t64) <= VALUE_BAR * np.abs(t64)).all(), tag
    for g, w in ((dr1, g1), (dr2, g2)):
        err = np.abs(g.astype(np.float64) - w)
        assert (err <= GRAD_BAR * np.abs(w)).all(), (tag, float((err / np.maximum(np.abs(w), 1e-300)).max()))
    # exact zeros (as bits: +0.0, not -0.0 and nothing tiny)
    assert not bits(terms[~counted]).any() and not bits(dr1[~counted]).any() and not bits(dr2[~counted]).any(), tag
    if not symmetric:
        assert not bits(dr2).any(), tag
    if not counted.any():
        assert bits(loss) == 0, tag


# ---- 1: the kernel against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('B', BS)
def test_every_shape_mode_and_scale_is_within_the_derived_bars(B, D):
    h, d, refs = case(B, D)
    for mode, symmetric, avg in VARIANTS:
        got = raw(*d, mode, symmetric, avg)
        check(got, refs[(mode, symmetric, avg)], cae_np.counted_rows(h[4], mode, B), symmetric, (B, D, mode, symmetric, avg))
        value_only = raw(*d, mode, symmetric, avg, grad=False, want_terms=False)
        assert bits(value_only[0]) == bits(got[0])


@pytest.mark.parametrize('dtype', Y_DTYPES)
def test_every_label_dtype(dtype):
    h, d, refs = case(33, 40)
    y = d[4].to(dtype)
    want = raw(*d, 'correspondence', True, True)
    got = raw(*d[:4], y, 'correspondence', True, True)
    assert same(got, want)
    if dtype in (torch.float32, torch.float64):                                         # 1.5 and 0.999 are not 'same'
        y = y.clone()
        y[1], y[2] = 1.5, 0.999
        hy = h[4].astype(np.float64)
        hy[1], hy[2] = 1.5, 0.999
        check(raw(*d[:4], y, 'correspondence', True, True), cae_np.recon_loss(*h[:4], hy), cae_np.counted_rows(hy, 'correspondence', 33),
              True, str(dtype))


@pytest.mark.parametrize('avg', [True, False])
def test_no_same_row_is_exactly_zero_and_the_autoencoder_needs_no_labels(avg):
    h, d, refs = case(33, 39)
    y = torch.full((33,), -1, dtype=torch.int64, device='cuda')
    loss, terms, dr1, dr2 = raw(*d[:4], y, 'correspondence', True, avg)
    assert bits(loss) == 0 and not bits(terms).any() and not bits(dr1).any() and not bits(dr2).any()
    got = raw(*d[:4], None, 'autoencoder', True, avg)
    assert same(got, raw(*d[:4], y, 'autoencoder', True, avg))
    check(got, refs[('autoencoder', True, avg)], np.ones(33, dtype=bool), True, 'y = None')


@pytest.mark.parametrize('B,D', [(33, 40), (257, 39)])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(B, D):
    h, d, refs = case(B, D)
    for v in (('correspondence', True, True), ('correspondence', False, False), ('autoencoder', True, True)):
        outs = {}
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                outs[byte] = raw(*d, *v)
            assert int(count) == 4 and count.nbytes > 2 * B * D * 4                      # loss, terms, the gradients, the workspace
        for byte in dirty_memory.PATTERNS[1:]:
            assert same(outs[byte], outs[0x00]), (v, hex(byte))
        check(outs[0xFF], refs[v], cae_np.counted_rows(h[4], v[0], B), v[1], 'dirty')


@pytest.mark.parametrize('B,D', [(33, 40), (9, 280)])
def test_misaligned_tables_give_the_aligned_bits(B, D):
    """Tables 4 bytes past a 16-byte boundary at D % 4 == 0 take the 4-byte loads: the same columns per lane in the same
    order, so the same bits."""
    h, d, _ = case(B, D)

    def shifted(t):
        buf = torch.empty(B * D + 1, dtype=torch.float32, device='cuda')
        out = buf[1:].view(B, D)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4
        return out
    for v in VARIANTS:
        want = raw(*d, *v)
        assert same(raw(*(shifted(t) for t in d[:4]), d[4], *v), want), v
        assert same(raw(shifted(d[0]), *d[1:], *v), want), v


# ---- 2: reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,D', [(257, 65), (33, 280)])
def test_two_calls_a_forced_grid_and_swapped_sides(B, D, monkeypatch):
    h, d, _ = case(B, D)
    r1, r2, x1, x2, y = d
    for v in VARIANTS:
        want = raw(*d, *v)
        assert same(raw(*d, *v), want), v
        for rows in ('1', '5', '64', '4096'):
            monkeypatch.setenv('ABN_RECON_ROWS', rows)
            assert same(raw(*d, *v), want), (v, rows)
        monkeypatch.delenv('ABN_RECON_ROWS')
    for mode in cae_np.MODES:
        for avg in (True, False):
            a = raw(r1, r2, x1, x2, y, mode, True, avg)
            b = raw(r2, r1, x2, x1, y, mode, True, avg)          # (r1, x2) <-> (r2, x1): each reconstruction keeps its target
            assert same((a[0], a[1], a[2], a[3]), (b[0], b[1], b[3], b[2])), (mode, avg)


def test_value_and_grad_forward_backward_and_a_scaled_seed():
    from abnet3_amd.loss import CorrespondenceLoss, unit_grad
    h, d, refs = case(33, 40)
    r1, r2, x1, x2, y = d
    for mode, symmetric, avg in VARIANTS:
        f = CorrespondenceLoss(avg=avg, symmetric=symmetric, mode=mode)
        val, dr = f.value_and_grad(r1, r2, x1, x2, y)
        want = raw(*d, mode, symmetric, avg)
        assert bits(host(val)) == bits(want[0]) and same((host(dr[0]), host(dr[1])), want[2:])
        a, b = r1.clone().requires_grad_(True), r2.clone().requires_grad_(True)
        i1, i2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        out = f(a, b, i1, i2, y)
        out.backward()
        assert bits(host(out)) == bits(want[0]) and torch.equal(a.grad, dr[0]) and torch.equal(b.grad, dr[1])
        assert i1.grad is None and i2.grad is None                                      # the inputs get no gradient
        a.grad = b.grad = None
        torch.autograd.backward(f(a, b, x1, x2, y), unit_grad(a.device))
        assert torch.equal(a.grad, dr[0])
        a.grad = b.grad = None
        torch.autograd.backward(f(a, b, x1, x2, y), torch.full((), 2.0, device='cuda'))
        assert torch.equal(a.grad, 2.0 * dr[0]) and torch.equal(b.grad, 2.0 * dr[1])
    f = CorrespondenceLoss()
    f.mode = 'autoencoder'                                                                # reassigned between passes
    assert bits(host(f(r1, r2, x1, x2))) == bits(raw(*d[:4], None, 'autoencoder', True, True)[0])
    with torch.no_grad():
        assert bits(host(f(r1, r2, x1, x2, y))) == bits(host(f.value_and_grad(r1, r2, x1, x2, y)[0]))


def test_wrapper_refusals():
    from abnet3_amd._lib import HipLibraryError
    from abnet3_amd.loss import CorrespondenceLoss
    h, d, _ = case(33, 40)
    r1, r2, x1, x2, y = d
    f = CorrespondenceLoss()
    with pytest.raises(HipLibraryError):
        f(r1, r2, x1.cpu(), x2, y)
    with pytest.raises(TypeError):
        f(r1.double(), r2, x1, x2, y)
    with pytest.raises(ValueError):
        f(r1, r2[:, :-1], x1, x2, y)
    with pytest.raises(ValueError):
        f(r1, r2, x1, x2, y[:-1])
    with pytest.raises(TypeError):
        f(r1, r2, x1, x2, None)                                                           # labels are needed in this mode
    with pytest.raises(TypeError):
        f(r1, r2, x1, x2, y.to(torch.int16))
    f.mode = 'denoising'
    with pytest.raises(ValueError, match='mode'):
        f(r1, r2, x1, x2, y)


def test_a_captured_call_replays_to_the_eager_bits():
    from abnet3_amd.loss import CorrespondenceLoss
    h, d, _ = case(257, 280)
    static = [t.clone() for t in d]
    f = CorrespondenceLoss(avg=True, symmetric=True)             # (avg in correspondence mode: the count runs inside the graph)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f.value_and_grad(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        val, dr = f.value_and_grad(*static)
    for seed in (0, 1):                                          # the captured inputs, then other values and other labels
        _, src, _ = case(257, 280, seed)
        for dst, s in zip(static, src):
            dst.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        want = raw(*src, 'correspondence', True, True)
        assert bits(host(val)) == bits(want[0]) and same((host(dr[0]), host(dr[1])), want[2:]), seed


# ---- 3: the network ------------------------------------------------------------------------------------------------------
SHAPES = {'small': (dict(input_dim=39, hidden_dim=64, output_dim=13, num_hidden_layers=1), 33),
          'wide': (dict(input_dim=40, hidden_dim=100, output_dim=32, num_hidden_layers=2), 96)}
NETS = list(itertools.product(sorted(SHAPES), (False, True), ('sigmoid', 'relu')))


def make_net(shape, bn, act, seed=0, tmp='/tmp/abn_cae_test'):
    from abnet3_amd.model import CorrespondenceAutoencoder
    torch.manual_seed(seed)
    kw, B = SHAPES[shape]
    return CorrespondenceAutoencoder(p_dropout=0.0, batch_norm=bn, activation_layer=act, output_path=tmp, **kw).cuda(), B


def net_batches(shape, n=2):
    kw, B = SHAPES[shape]
    out = []
    for s in range(n):
        rng = np.random.default_rng(50 + s)
        x1 = rng.standard_normal((B, kw['input_dim'])).astype(np.float32)
        x2 = (x1 + 0.3 * rng.standard_normal(x1.shape)).astype(np.float32)
        y = np.where(np.arange(B) % 3 == 2, -1, 1).astype(np.int64)
        out.append((torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(y)))
    return out


@pytest.mark.parametrize('shape,bn,act', NETS)
def test_forward_forward_once_and_reconstruct_against_the_cpu_modules(shape, bn, act):
    net, B = make_net(shape, bn, act)
    x1, x2, _ = net_batches(shape, 1)[0]
    d1, d2 = x1.cuda(), x2.cuda()
    for train in (True, False):
        net.train(train)
        cpu = cae_np.CpuCae(net, torch.float32)                  # (a fresh copy per mode: the running statistics as they stand)
        with torch.no_grad():
            w1, w2 = cpu.forward(x1, x2)
            cpu2 = cae_np.CpuCae(net, torch.float32)
            w_code, w_rec = cpu2.forward_once(x1), cae_np.CpuCae(net, torch.float32).reconstruct(x1)
            r1, r2 = net(d1, d2)
            code = net.forward_once(d1)
            rec = net.reconstruct(d1)
        assert r1.shape == (B, net.input_dim) and code.shape == (B, net.output_dim)
        for got, want, what in ((r1, w1, 'recon1'), (r2, w2, 'recon2'), (code, w_code, 'code'), (rec, w_rec, 'reconstruct')):
            assert rel_err(host(got), host(want)) <= 1e-5, (what, train, rel_err(host(got), host(want)))


@pytest.mark.parametrize('shape,bn,act', NETS)
def test_backward_and_five_adadelta_steps_judged_against_float64(shape, bn, act, tmp_path):
    """test_c2_backward_judged_against_float64's yardstick: the HIP path no further from the float64 evaluation of the same
    modules than factor x the float32 torch-CPU evaluation's own distance + 3e-6 of the tensor's largest entry (factor 1.5,
    4 with BatchNorm); on the first step's gradients, on the parameters after five Adadelta steps, and on the losses."""
    from abnet3_amd.loss import CorrespondenceLoss
    from abnet3_amd.trainer import TrainerCorrespondence
    net, B = make_net(shape, bn, act, tmp=str(tmp_path / 'cae'))
    net.train()
    batches = net_batches(shape)
    adadelta = lambda p: torch.optim.Adadelta(p, lr=1.0)
    l64, g64, p64 = cae_np.CpuCae(net, torch.float64).run_steps(batches, 5, adadelta)
    l32, g32, p32 = cae_np.CpuCae(net, torch.float32).run_steps(batches, 5, adadelta)
    tr = TrainerCorrespondence(network=net, loss=CorrespondenceLoss(), optimizer_type='adadelta', lr=1.0, dataloader=None,
                               log_dir=str(tmp_path / 'runs'))
    assert not tr._direct_ok() and tr._planned(True) is None and tr._loss_is_mean()
    dev_batches = [tuple(t.cuda() for t in b) for b in batches]
    losses = []
    for s in range(5):
        losses.append(float(tr.train_step(dev_batches[s % 2], True)))
        if s == 0:
            ghip = {k: q.grad.double().cpu().numpy() for k, q in net.named_parameters()}
    err = lambda a, t: float(np.abs(a.astype(np.float64) - t).max() / max(np.abs(t).max(), 1e-30))
    gmax = max(np.abs(v).max() for v in g64.values())
    factor = 4.0 if bn else 1.5
    assert set(ghip) == set(g64)
    for k in g64:
        if cae_np.pre_bn_bias(k, bn):                                                    # mathematically zero: rounding noise on every side
            assert np.abs(ghip[k]).max() <= 1e-4 * gmax, k
            continue
        e_hip, e_ref = err(ghip[k], g64[k]), err(g32[k], g64[k])
        print('%-28s gradient: hip %.3g, float32 cpu %.3g' % (k, e_hip, e_ref))
        assert e_hip <= factor * e_ref + 3e-6, (k, e_hip, e_ref)
    for a, b, c in zip(losses, l32, l64):
        print('loss: hip %.9g, float32 cpu %.9g, float64 %.12g' % (a, b, c))
        assert abs(a - c) <= abs(b - c) + 2e-6 * abs(c), (a, b, c)
    sd = {k: v.double().cpu().numpy() for k, v in net.state_dict().items()}
    for k in p64:
        if 'num_batches' in k:
            assert int(sd[k]) == int(p64[k]) == 10                                       # two tower calls per step
            continue
        if cae_np.pre_bn_bias(k, bn):
            continue
        e_hip, e_ref = err(sd[k], p64[k]), err(p32[k], p64[k])
        print('%-28s after 5 steps: hip %.3g, float32 cpu %.3g' % (k, e_hip, e_ref))
        if 'running' in k:
            assert rel_err(sd[k], p64[k]) <= 1e-5, (k, rel_err(sd[k], p64[k]))           # the statistics: the parity bar
            continue
        assert e_hip <= factor * e_ref + 3e-6, (k, e_hip, e_ref)


# ---- 4: behaviour on a planted corpus ---------------------------------------------------------------------------------------
class ListLoader(object):
    def __init__(self, train, dev_batches):
        self.train, self.dev = train, dev_batches

    def batch_iterator(self, train_mode=True):
        return iter(self.train if train_mode else self.dev)

    def whoami(self):
        return {'class_name': 'ListLoader'}


def planted_batches(seed, n_batches, n=96):
    rng = np.random.default_rng(seed)
    x1, x2, y = cae_np.planted_corpus(rng, n_batches * n)
    return [tuple(torch.from_numpy(a[i * n:(i + 1) * n]).cuda() for a in (x1, x2, y)) for i in range(n_batches)]


def planted_trainer(tmp_path, loader=None, seed=0):
    from abnet3_amd.loss import CorrespondenceLoss
    from abnet3_amd.model import CorrespondenceAutoencoder
    from abnet3_amd.trainer import TrainerCorrespondence
    torch.manual_seed(seed)
    net = CorrespondenceAutoencoder(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=16, p_dropout=0.0, activation_layer='tanh',
                                    last_non_linearity=None, output_path=str(tmp_path / 'cae'))
    return TrainerCorrespondence(network=net, loss=CorrespondenceLoss(), optimizer_type='adadelta', lr=1.0, dataloader=loader,
                                 log_dir=str(tmp_path / 'runs'))


def test_pretraining_and_correspondence_steps_lower_their_losses(tmp_path):
    batches = planted_batches(0, 8)
    tr = planted_trainer(tmp_path, ListLoader(batches[:6], batches[6:]))
    got = tr.pretrain(3)
    assert len(got) == 3 and np.isfinite(got).all() and got[-1] < got[0], got
    assert tr.loss.mode == 'correspondence' and tr.train_losses == got and len(tr.dev_losses) == 3
    tr.network.train()
    losses = [float(tr.train_step(batches[s % 6], True)) for s in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_a_batch_without_a_same_row_changes_no_parameter(tmp_path):
    batches = planted_batches(1, 2)
    tr = planted_trainer(tmp_path)
    tr.network.train()
    tr.train_step(batches[0], True)                              # (the optimizer has state by now)
    before = {k: v.clone() for k, v in tr.network.state_dict().items()}
    x1, x2, y = batches[1]
    loss = tr.train_step((x1, x2, torch.full_like(y, -1)), True)
    assert bits(host(loss)) == 0
    for k, v in tr.network.state_dict().items():
        assert torch.equal(v, before[k]) and np.array_equal(bits(host(v)), bits(host(before[k]))), k


def test_the_embedder_and_an_abnet_initialised_from_the_encoder(tmp_path):
    from abnet3_amd.embedder import EmbedderSiamese
    from abnet3_amd.model import SiameseNetwork
    tr = planted_trainer(tmp_path)
    cae = tr.network
    batches = planted_batches(2, 2)
    cae.train()
    tr.train_step(batches[0], True)
    cae.eval()
    table = torch.cat([batches[0][0], batches[1][0][:37]])
    with torch.no_grad():
        want = cae.forward_once(table)
    emb = EmbedderSiamese(network=cae, cuda=True, batch_size=64).embed_table(table)
    assert tuple(emb.shape) == (133, cae.output_dim) and torch.equal(torch.as_tensor(emb).cuda(), want)
    cae.save_encoder(str(tmp_path / 'enc.pth'))
    sia = SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=16, p_dropout=0.0, activation_layer='tanh',
                         last_non_linearity=None).cuda()
    sia.load_network(str(tmp_path / 'enc.pth'))
    sia.eval()
    with torch.no_grad():
        got = sia.forward_once(table)
    assert np.array_equal(bits(host(got)), bits(host(want)))
    cae.save_network()
    other = planted_trainer(tmp_path / 'b', seed=5).network
    other.load_network(str(tmp_path / 'cae.pth'))
    other.eval()
    with torch.no_grad():
        assert torch.equal(other.reconstruct(table), cae.reconstruct(table))
