"""abnq_softdtw_forward / abnq_softdtw_backward, softdtw.soft_dtw, SoftDTWLoss, WordPairDataLoader and TrainerSequencePairs on
the MI355X against tests/sdtw_np.py.

The bars.  Values, derived for float32 cells formed as a float32 dot product of float32 unit rows:
the value is 1-Lipschitz in each cell along an expected path and sum(E) <= n + m - 1, the output is rounded to float32:
    |value - ref| <= (n + m - 1) (2 D + 8) 2^-24 + 2^-23 |ref|
(the kernel's cell is the correctly rounded cosine, half a unit in the last place, so it needs little of the first term)
Gradients, measured on the float32-cell yardstick's own error against the float64 restatement on the same case:
    max |g - ref| <= 16 (yardstick's max |g - ref|) + 4 * 2^-24 max |ref|
The loss adds float32 arithmetic on the [P] vectors (the division by the lengths, the margin, 1 / P, the divergence's -1/2 and
the sum of up to three blocks on a row); its gradients are held to the kernel's own bar all the same (all sixteen cases were
measured inside it), and its value to the sum of the pairs' value bars at their own lengths and values (three values each
under the divergence) plus 8 * 2^-24 of the sum of the |terms| for the float32 arithmetic on the terms.  Every test prints its figures before it asserts.

Needs an MI355X: -m gpu."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import sdtw_np as S  # noqa: E402

pytestmark = pytest.mark.gpu

bits = dirty_memory.bits
EPS = 2.0 ** -24
SHAPES = [(1, 1), (1, 9), (9, 1), (63, 64), (64, 65), (65, 64), (65, 130), (130, 65), (256, 3)]
DS = (1, 7, 8, 40)
GAMMAS = (1e-3, 0.1, 10.0)
# every (n, m) with every gamma, D walking through its four values; and every D with every gamma at (65, 64)
CASES = [(n, m, DS[(k + g) % 4], gamma) for k, (n, m) in enumerate(SHAPES) for g, gamma in enumerate(GAMMAS)]
CASES += [(65, 64, D, gamma) for D in DS for gamma in GAMMAS if (65, 64, D, gamma) not in CASES]


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def value_bar(n, m, D, ref):
    return (n + m - 1) * (2 * D + 8) * EPS + 2 * EPS * abs(ref)


def run(e, off1, n1, off2, n2, gamma, w=None, keep=True):
    """(value, g1, g2) host arrays of one forward (+ backward) through the raw Python calls."""
    from abnet3_amd import softdtw
    value, handle = softdtw.soft_dtw_batch(e, off1, n1, off2, n2, gamma, keep=keep)
    if not keep:
        return host(value), None, None
    P = len(n1)
    w = torch.ones(P, dtype=torch.float32, device='cuda') if w is None else w
    g1, g2 = softdtw.soft_dtw_backward(handle, w)
    torch.cuda.synchronize()
    return host(value), host(g1), host(g2)


_CASE = {}


def case(n, m, D, gamma):
    """One problem's inputs and both references: made once, shared, never written."""
    key = (n, m, D, gamma)
    if key not in _CASE:
        rng = np.random.default_rng(1000 * n + 10 * m + D)
        x, y = S.draw(rng, n, m, D)
        _CASE[key] = dict(x=x, y=y, ref=S.problem(x, y, gamma), yard=S.problem(x, y, gamma, cell_dtype=np.float32))
    return _CASE[key]


@pytest.mark.parametrize('n,m,D,gamma', CASES)
def test_value_and_gradients_of_one_problem(n, m, D, gamma):
    c = case(n, m, D, gamma)
    e = dev(np.concatenate([c['x'], c['y']]))
    value, g1, g2 = run(e, [0], [n], [n], [m], gamma)
    ref, yard = c['ref'], c['yard']
    verr, vbar = abs(float(value[0]) - ref['value']), value_bar(n, m, D, ref['value'])
    yerr = max(np.abs(yard['g1'] - ref['g1']).max(), np.abs(yard['g2'] - ref['g2']).max())
    gerr = max(np.abs(g1 - ref['g1']).max(), np.abs(g2 - ref['g2']).max())
    gmax = max(np.abs(ref['g1']).max(), np.abs(ref['g2']).max())
    gbar = 16 * yerr + 4 * EPS * gmax
    print('sdtw case n=%d m=%d D=%d gamma=%g: value err %.3g (bar %.3g, yardstick %.3g), gradient err %.3g (yardstick %.3g, ratio %.3g, '
          'bar %.3g, max |g| %.3g)' % (n, m, D, gamma, verr, vbar, abs(yard['value'] - ref['value']), gerr, yerr,
                                       gerr / yerr if yerr > 0 else float(gerr > 0), gbar, gmax))
    assert np.isfinite(value).all() and np.isfinite(g1).all() and np.isfinite(g2).all()
    assert verr <= vbar
    assert gerr <= gbar
    assert g1.shape == (n, D) and g2.shape == (m, D)


def mixed_table(P=300, D=8, seed=5):
    """P problems of lengths 1 .. 40 over one table: related sides, one problem whose sides are the same rows, a zero row and
    a row of norm 1e-7 (both below the clamp), every length of 1 .. 40 on either side at least once."""
    rng = np.random.default_rng(seed)
    n1 = rng.integers(1, 41, P).astype(np.int32)
    n2 = rng.integers(1, 41, P).astype(np.int32)
    n1[:40], n2[40:80] = np.arange(1, 41), np.arange(1, 41)
    rows, off1, off2 = [], [], []
    o = 0
    for p in range(P):
        x, y = S.draw(rng, int(n1[p]), int(n2[p]), D)
        off1.append(o)
        rows.append(x)
        o += len(x)
        if p == 7:                                   # x against itself: off1 == off2
            n2[p] = n1[p]
            off2.append(off1[-1])
        else:
            off2.append(o)
            rows.append(y)
            o += len(y)
    e = np.concatenate(rows).astype(np.float32)
    e[off1[3]] = 0.0                                 # n1[3] = 4: a zero row ...
    e[off2[5] + 1] = np.float32(1e-7) * e[off2[5] + 1] / np.linalg.norm(e[off2[5] + 1])      # ... and one of norm 1e-7
    w = rng.standard_normal(P).astype(np.float32)
    w[2], w[11], w[12] = 0.0, -1.5, 1.0
    return e, np.asarray(off1, dtype=np.int64), n1, np.asarray(off2, dtype=np.int64), n2, w


def test_300_problems_equal_each_problem_alone_and_the_restatement(monkeypatch):
    e, off1, n1, off2, n2, w = mixed_table()
    P, gamma = len(n1), 0.1
    ed, wd = dev(e), dev(w)
    monkeypatch.delenv('ABN_SDTW_GRID', raising=False)
    value, g1, g2 = run(ed, off1, n1, off2, n2, gamma, wd)
    again = run(ed, off1, n1, off2, n2, gamma, wd)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((value, g1, g2), again)), 'two calls differ'
    for grid in ('7', '256'):                        # 300 problems over 7 and over 256 workgroups: the grid-stride path
        monkeypatch.setenv('ABN_SDTW_GRID', grid)
        strided = run(ed, off1, n1, off2, n2, gamma, wd)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((value, g1, g2), strided)), 'grid %s differs' % grid
    monkeypatch.delenv('ABN_SDTW_GRID')
    # dirty outputs and workspace
    for byte in (0xFF, 0xC2):
        with dirty_memory.dirty(byte) as count:
            dirty = run(ed, off1, n1, off2, n2, gamma, wd)
        assert int(count) >= 4
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((value, g1, g2), dirty)), 'poison %#x shows' % byte
    # keep = 0: the same values
    v0, _, _ = run(ed, off1, n1, off2, n2, gamma, keep=False)
    assert np.array_equal(bits(v0), bits(value))
    # a zero weight: a block of exact zeros; a problem alone: the same bits
    s1, s2 = np.cumsum(n1) - n1, np.cumsum(n2) - n2
    assert not g1[s1[2]:s1[2] + n1[2]].any() and not g2[s2[2]:s2[2] + n2[2]].any()
    assert not np.signbit(g1[s1[2]:s1[2] + n1[2]]).any()
    assert np.isfinite(value).all() and np.isfinite(g1).all() and np.isfinite(g2).all()
    for p in range(P):
        v, a, b = run(ed, off1[p:p + 1], n1[p:p + 1], off2[p:p + 1], n2[p:p + 1], gamma, wd[p:p + 1].clone())
        assert np.array_equal(bits(v), bits(value[p:p + 1])), p
        assert np.array_equal(bits(a), bits(g1[s1[p]:s1[p] + n1[p]])) and np.array_equal(bits(b), bits(g2[s2[p]:s2[p] + n2[p]])), p
    # the restatement: the special problems and a few more
    worst = 0.0
    for p in (2, 3, 5, 7, 11, 12, 39, 79, 150, 299):
        x, y = e[off1[p]:off1[p] + n1[p]], e[off2[p]:off2[p] + n2[p]]
        ref, yard = S.problem(x, y, gamma, float(w[p])), S.problem(x, y, gamma, float(w[p]), cell_dtype=np.float32)
        assert abs(float(value[p]) - ref['value']) <= value_bar(n1[p], n2[p], 8, ref['value']), p
        yerr = max(np.abs(yard['g1'] - ref['g1']).max(), np.abs(yard['g2'] - ref['g2']).max())
        gerr = max(np.abs(g1[s1[p]:s1[p] + n1[p]] - ref['g1']).max(), np.abs(g2[s2[p]:s2[p] + n2[p]] - ref['g2']).max())
        gmax = max(np.abs(ref['g1']).max(), np.abs(ref['g2']).max())
        print('sdtw mixed problem %d (%d x %d, w %.3g): gradient err %.3g, yardstick %.3g, max |g| %.3g' % (p, n1[p], n2[p], w[p], gerr, yerr, gmax))
        assert gerr <= 16 * yerr + 4 * EPS * gmax, p
        worst = max(worst, gerr / yerr if yerr > 0 else 0.0)
    print('sdtw mixed: worst kernel / yardstick ratio %.3g' % worst)


def test_refusals_that_read_the_problem_table():
    from abnet3_amd import _lib, softdtw
    lib, p = _lib.load(), _lib.ptr
    rng = np.random.default_rng(3)
    e = dev(rng.standard_normal((40, 8)).astype(np.float32))
    cap = softdtw.max_len()

    def table(off1, n1, off2, n2):
        return dev(off1, torch.int64), dev(n1, torch.int32), dev(off2, torch.int64), dev(n2, torch.int32)

    def forward(cols, ws, ws_bytes, keep=1, R=40):
        value = torch.full((len(cols[1]),), 7.0, device='cuda')
        rc = lib.abnq_softdtw_forward(p(e), R, 8, p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]), len(cols[1]), 0.1, p(value), p(ws),
                                      ws_bytes, keep, _lib.stream())
        torch.cuda.synchronize()
        return rc, host(value)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')
    ok = table([0, 5], [5, 6], [11, 20], [7, 4])
    n1h, n2h = np.array([5, 6], dtype=np.int32), np.array([7, 4], dtype=np.int32)
    need = [lib.abnq_softdtw_ws_bytes(n1h.ctypes.data, n2h.ctypes.data, 2, 8, k) for k in (0, 1)]
    for cols, code, word in ((table([0, 5], [5, 0], [11, 20], [7, 4]), _lib.E_ARG, b'empty'),
                             (table([0, 5], [5, 6], [11, 20], [-1, 4]), _lib.E_ARG, b'empty'),
                             (table([0, 5], [5, cap + 1], [11, 20], [7, 4]), _lib.E_UNSUPPORTED, b'abnq_softdtw_max_len'),
                             (table([0, 35], [5, 6], [11, 20], [7, 4]), _lib.E_ARG, b'table of 40'),
                             (table([0, 5], [5, 6], [11, 37], [7, 4]), _lib.E_ARG, b'table of 40'),
                             (table([-1, 5], [5, 6], [11, 20], [7, 4]), _lib.E_ARG, b'table of 40')):
        rc, value = forward(cols, ws, ws.numel())
        assert rc == code and word in lib.abn_last_error(), (rc, lib.abn_last_error())
        assert (value == 7.0).all() and not host(ws).any()                        # refused before any launch
    for keep in (0, 1):
        rc, value = forward(ok, ws, need[keep] - 1, keep)
        assert rc == _lib.E_WORKSPACE and (value == 7.0).all() and (keep or not host(ws).any())
        rc, value = forward(ok, ws, need[keep], keep)
        assert rc == 0 and (value != 7.0).all()
    w = torch.ones(2, device='cuda')
    g1, g2 = torch.full((11, 8), 7.0, device='cuda'), torch.full((11, 8), 7.0, device='cuda')

    def backward(cols, ws, ws_bytes, gamma=0.1):
        rc = lib.abnq_softdtw_backward(p(e), 40, 8, p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]), len(cols[1]), gamma, p(w), p(g1), p(g2),
                                       p(ws), ws_bytes, _lib.stream())
        torch.cuda.synchronize()
        return rc
    fresh = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')
    assert backward(ok, fresh, fresh.numel()) == _lib.E_ARG and b'no abnq_softdtw_forward' in lib.abn_last_error()
    assert forward(ok, ws, ws.numel(), keep=0)[0] == 0
    assert backward(ok, ws, ws.numel()) == _lib.E_ARG and b'keep = 0' in lib.abn_last_error()
    assert forward(ok, ws, ws.numel(), keep=1)[0] == 0
    assert backward(ok, ws, ws.numel(), gamma=0.2) == _lib.E_ARG and b'another problem' in lib.abn_last_error()
    assert backward(table([0, 5], [5, 5], [11, 20], [7, 4]), ws, ws.numel()) == _lib.E_ARG and b'another problem' in lib.abn_last_error()
    # the same P, sums and cell count, other lengths (5 x 7 + 6 x 4 = 6 x 4 + 5 x 7): the header's hash of the table differs
    assert backward(table([0, 6], [6, 5], [11, 15], [4, 7]), ws, ws.numel()) == _lib.E_ARG and b'another problem' in lib.abn_last_error()
    assert backward(table([0, 5], [5, 6], [12, 20], [7, 4]), ws, ws.numel()) == _lib.E_ARG and b'another problem' in lib.abn_last_error()
    assert backward(ok, ws, need[1] - 1) == _lib.E_WORKSPACE
    assert (host(g1) == 7.0).all() and (host(g2) == 7.0).all()
    assert backward(ok, ws, need[1]) == 0 and (host(g1) != 7.0).all() and (host(g2) != 7.0).all()
    # the python surface
    value, handle = softdtw.soft_dtw_batch(e, [0], [5], [11], [7], 0.1, keep=False)
    with pytest.raises(ValueError, match='keep=False'):
        softdtw.soft_dtw_backward(handle, w[:1])
    for bad in (dict(n1=[0]), dict(n1=[cap + 1]), dict(off1=[38]), dict(off2=[-1]), dict(n2=[7, 7])):
        a = dict(off1=[0], n1=[5], off2=[11], n2=[7])
        a.update(bad)
        with pytest.raises(ValueError):
            softdtw.soft_dtw_batch(e, a['off1'], a['n1'], a['off2'], a['n2'], 0.1)
    value, handle = softdtw.soft_dtw_batch(e, [], [], [], [], 0.1, keep=True)       # P = 0
    g = softdtw.soft_dtw_backward(handle, torch.zeros(0, device='cuda'))
    assert value.shape == (0,) and g[0].shape == (0, 8) and g[1].shape == (0, 8)


_LOSS = {}


def loss_case():
    if not _LOSS:
        rng = np.random.default_rng(29)
        n1, n2 = np.array([5, 9, 1, 12, 20, 3], dtype=np.int32), np.array([6, 4, 7, 12, 17, 1], dtype=np.int32)
        rows, off1, off2, o = [], [], [], 0
        for a, b in zip(n1, n2):
            x, y = S.draw(rng, int(a), int(b), 6)
            off1.append(o)
            off2.append(o + int(a))
            rows += [x, y]
            o += int(a) + int(b)
        rows.append(rng.standard_normal((3, 6)).astype(np.float32))                  # three rows nobody reads
        _LOSS.update(e=np.concatenate(rows), off1=np.asarray(off1), n1=n1, off2=np.asarray(off2), n2=n2, y=np.array([1, -1, 1, -1, -1, 1]))
    return _LOSS


@pytest.mark.parametrize('normalize,divergence,avg', list(itertools.product((True, False), (True, False), (True, False))))
def test_autograd_and_loss_against_the_restatement(normalize, divergence, avg):
    from abnet3_amd.loss import SoftDTWLoss
    c = loss_case()
    gamma, margin = 0.1, (0.25 if normalize else 4.0)
    args = (c['off1'], c['n1'], c['off2'], c['n2'])
    want, terms, de = S.loss(c['e'], *args, c['y'], gamma, margin, normalize, divergence, avg)
    _, _, de_y = S.loss(c['e'], *args, c['y'], gamma, margin, normalize, divergence, avg, cell_dtype=np.float32)
    print('sdtw loss terms', terms)
    f = SoftDTWLoss(gamma=gamma, margin=margin, normalize=normalize, divergence=divergence, avg=avg)
    e = dev(c['e']).requires_grad_(True)
    y = dev(c['y'])
    lv = f(e, *args, y)
    lv.backward()
    lv2, de2 = f.value_and_grad(e.detach(), *args, y)
    scale = 1.0 / len(c['n1']) if avg else 1.0
    norm = 1.0 / (c['n1'] + c['n2']) if normalize else np.ones(len(c['n1']))
    # a pair's value bar at its own lengths and the restatement's own values; under the divergence also those of (x, x) and (y, y)
    vbar = 8 * EPS * scale * np.abs(terms).sum()
    for p, (n, m) in enumerate(zip(c['n1'], c['n2'])):
        x, yy = c['e'][c['off1'][p]:c['off1'][p] + n], c['e'][c['off2'][p]:c['off2'][p] + m]
        b = value_bar(n, m, 6, S.problem(x, yy, gamma)['value'])
        if divergence:
            b += 0.5 * (value_bar(n, n, 6, S.problem(x, x, gamma)['value']) + value_bar(m, m, 6, S.problem(yy, yy, gamma)['value']))
        vbar += scale * norm[p] * b
    yerr, gmax = np.abs(de_y - de).max(), np.abs(de).max()
    gbar = 16 * yerr + 4 * EPS * gmax
    for tag, val, grad in (('autograd', lv, e.grad), ('value_and_grad', lv2, de2)):
        verr, gerr = abs(float(val) - want), np.abs(host(grad) - de).max()
        print('sdtw loss %s normalize=%s divergence=%s avg=%s: loss %.6g err %.3g (bar %.3g), gradient err %.3g (yardstick %.3g, bar %.3g, '
              'max %.3g)' % (tag, normalize, divergence, avg, want, verr, vbar, gerr, yerr, gbar, gmax))
        assert verr <= vbar and gerr <= gbar
        assert not host(grad)[-3:].any()
    with pytest.raises(ValueError, match='labels'):
        f(e, *args, y[:-1])
    zero = f(e, [], [], [], [], y[:0])
    assert float(zero) == 0.0


def test_autograd_function_with_an_incoming_gradient():
    """softdtw.soft_dtw on its own: sum(w * value).backward() hands the kernel w itself, every table row receives one block row,
    so the kernel's bar applies as it is; e changed in place before the backward is refused by autograd."""
    from abnet3_amd import softdtw
    c = loss_case()
    args = (c['off1'], c['n1'], c['off2'], c['n2'])
    w = np.array([0.75, -1.25, 0.0, 2.0, -0.5, 1.0], dtype=np.float32)
    e = dev(c['e']).requires_grad_(True)
    value = softdtw.soft_dtw(e, *args, 0.1)
    (value * dev(w)).sum().backward()
    got, vh = host(e.grad), host(value)
    assert not got[-3:].any()
    for p, (n, m) in enumerate(zip(c['n1'], c['n2'])):
        a, b = c['off1'][p], c['off2'][p]
        x, y = c['e'][a:a + n], c['e'][b:b + m]
        ref, yard = S.problem(x, y, 0.1, float(w[p])), S.problem(x, y, 0.1, float(w[p]), cell_dtype=np.float32)
        assert abs(float(vh[p]) - ref['value']) <= value_bar(n, m, 6, ref['value'])
        yerr = max(np.abs(yard['g1'] - ref['g1']).max(), np.abs(yard['g2'] - ref['g2']).max())
        gerr = max(np.abs(got[a:a + n] - ref['g1']).max(), np.abs(got[b:b + m] - ref['g2']).max())
        gmax = max(np.abs(ref['g1']).max(), np.abs(ref['g2']).max())
        print('sdtw autograd pair %d (w %.3g): gradient err %.3g, yardstick %.3g, max |g| %.3g' % (p, w[p], gerr, yerr, gmax))
        assert gerr <= 16 * yerr + 4 * EPS * gmax, p
    assert not got[c['off1'][2]:c['off1'][2] + c['n1'][2]].any()                     # w = 0
    t = dev(c['e'])
    leaf = t.clone().requires_grad_(True)
    work = leaf * 1.0
    value = softdtw.soft_dtw(work, *args, 0.1)
    work.mul_(2.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        value.sum().backward()
    with torch.no_grad():                                                             # no graph: keep = 0, the same values
        assert np.array_equal(bits(host(softdtw.soft_dtw(t, *args, 0.1))), bits(vh))


def toy_pairs():
    """A corpus of D = 8 and 16 word pairs of 3 .. 20 frames: 'same' pairs are a token and a warped, noisy copy of it."""
    rng = np.random.default_rng(31)
    feats, times, pairs = {}, {}, []
    for k in range(16):
        n, m = int(rng.integers(3, 21)), int(rng.integers(3, 21))
        x, y = S.draw(rng, n, m, 8)
        if k % 2:
            y = rng.standard_normal((m, 8)).astype(np.float32)
        name = 'utt%02d' % k
        feats[name] = np.concatenate([x, y])
        times[name] = np.arange(n + m) * 0.01 + 0.005
        pairs.append((name, 0.0, n * 0.01, name, n * 0.01, (n + m) * 0.01, 'diff' if k % 2 else 'same'))
    return feats, times, pairs


def toy_trainer(tmp_path, seed=0, lr=0.05):
    from abnet3_amd.dataloader import WordPairDataLoader
    from abnet3_amd.loss import SoftDTWLoss
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSequencePairs
    feats, times, pairs = toy_pairs()
    dl = WordPairDataLoader(None, None, batch_size=16, seed=0)
    dl.set_data(feats, times, train_pairs=pairs, dev_pairs=pairs[:4])
    torch.manual_seed(seed)
    net = SiameseNetwork(input_dim=8, num_hidden_layers=1, hidden_dim=16, output_dim=4, activation_layer='sigmoid', batch_norm=False,
                         p_dropout=0.0, output_path=str(tmp_path / 'net'))
    tr = TrainerSequencePairs(network=net, loss=SoftDTWLoss(gamma=0.1, margin=0.5), optimizer_type='sgd', lr=lr, dataloader=dl,
                              log_dir=str(tmp_path / 'runs'))
    return tr, dl


def test_trainer_on_a_toy_corpus(tmp_path):
    tr, dl = toy_trainer(tmp_path)
    assert not tr._direct_ok() and tr._planned(True) is None and not hasattr(dl, 'plan')
    np.random.seed(0)
    batches = list(dl.batch_iterator(True))
    assert len(batches) == 1
    X, off1, n1, off2, n2, y = batches[0]
    assert len(n1) == 16 and 3 <= min(n1.min(), n2.min()) and max(n1.max(), n2.max()) <= 20 and X.shape == (int(n1.sum() + n2.sum()), 8)
    tr.network.train()
    with torch.no_grad():
        emb = host(tr.network.forward_once(X))
    want, _, _ = S.loss(emb, off1, n1, off2, n2, host(y), 0.1, 0.5, True, False, True)
    first = float(tr.train_step(batches[0], True))
    vals = [S.problem(emb[o1:o1 + a], emb[o2:o2 + b], 0.1)['value'] for o1, a, o2, b in zip(off1, n1, off2, n2)]
    bar = sum(value_bar(int(a), int(b), 4, v) / (int(a) + int(b)) for a, b, v in zip(n1, n2, vals)) / 16 + 8 * EPS * abs(want)
    print('sdtw trainer: first loss %.7g, restatement on the network\'s embeddings %.7g, bar %.3g' % (first, want, bar))
    assert abs(first - want) <= bar
    losses = [first] + [float(tr.train_step(batches[0], True)) for _ in range(8)]
    with torch.no_grad():
        last = float(tr.give_batch_to_network(batches[0]))
    print('sdtw trainer: losses on one batch %s, then %.6g' % (['%.6g' % v for v in losses], last))
    assert np.isfinite(losses).all() and last < first
    # the dev pass goes through keep = 0; a whole epoch runs
    tr.train_losses, tr.dev_losses = [], []                  # (what train() sets up before its first pass)
    tr.optimize_model(True)
    assert len(tr.train_losses) == 1 and np.isfinite(tr.train_losses[0]) and np.isfinite(tr.dev_losses[0])
    st = dl.statistics_training
    assert st['SameType'] > 0 and st['DiffType'] > 0 and st['DroppedEmpty'] == 0 and st['DroppedLong'] == 0
    with pytest.raises(NotImplementedError):
        tr.make_graphed_step(batches[0])


def test_two_runs_from_one_seed_give_identical_parameters(tmp_path):
    out = []
    for run_ in range(2):
        tr, dl = toy_trainer(tmp_path / str(run_), seed=3)
        np.random.seed(0)
        batch = next(iter(dl.batch_iterator(True)))
        tr.network.train()
        for _ in range(4):
            tr.train_step(batch, True)
        torch.cuda.synchronize()
        out.append({k: host(v).copy() for k, v in tr.network.state_dict().items()})
    assert set(out[0]) == set(out[1]) and all(np.array_equal(bits(out[0][k]), bits(out[1][k])) for k in out[0])


def test_loader_from_files_on_the_device(tmp_path, monkeypatch):
    import fake_h5features
    from abnet3_amd.dataloader import WordPairDataLoader
    from abnet3_amd.utils import write_dataset
    monkeypatch.setitem(sys.modules, 'h5features', fake_h5features)
    feats, times, pairs = toy_pairs()
    names = list(feats)
    fake_h5features.write(str(tmp_path / 'f.h5f'), 'features', names, [times[k] for k in names], [feats[k] for k in names])
    for sub in ('train_pairs', 'dev_pairs'):
        os.makedirs(str(tmp_path / sub))
        write_dataset(str(tmp_path / sub / 'dataset'), pairs)
    dl = WordPairDataLoader(str(tmp_path), str(tmp_path / 'f.h5f'), batch_size=5, seed=0)
    np.random.seed(0)
    batches = list(dl.batch_iterator(True))
    assert sorted(len(b[5]) for b in batches) == [1, 5, 5, 5]
    table = host(dl.features.table)
    n_same = 0
    for X, off1, n1, off2, n2, y in batches:
        Xh, yh = host(X), host(y)
        assert X.is_cuda and y.is_cuda and Xh.shape[0] == int(n1.sum() + n2.sum())
        for p in range(len(n1)):
            x, yy = Xh[off1[p]:off1[p] + n1[p]], Xh[off2[p]:off2[p] + n2[p]]
            hit = [k for k in names if feats[k].shape[0] == n1[p] + n2[p] and np.array_equal(feats[k], np.concatenate([x, yy]))]
            assert len(hit) == 1 and yh[p] == (-1 if int(hit[0][3:]) % 2 else 1)
            n_same += int(yh[p] == 1)
    assert n_same == 8 and table.shape == (sum(len(v) for v in feats.values()), 8)
