"""Temporal-coherence pairs on the device: abn_tcl_pairs against its restatement (tests/tcl_np.py) bit for bit,
TemporalCoherenceDataLoader (plan = iterator, persistent arrays, epochs, the dev pass), the mix
OriginalDataLoader(tcl, tcl_seed), and both under TrainerSiamese's planned passes.  Needs an MI355X: run with -m gpu."""
import ctypes
import random
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err

import tcl_np

pytestmark = pytest.mark.gpu

S = tcl_np.SENTINEL


def _run_kernel(row0, lens, n_iter, first, seed, epoch, out_len, dst=None, f64=False, deltas=tcl_np.DELTAS, n_same=1):
    from abnet3_amd import _lib
    lib = _lib.load()
    lens_h = np.ascontiguousarray(lens, dtype=np.int64)
    d_row0, d_len = torch.from_numpy(np.ascontiguousarray(row0, dtype=np.int64)).cuda(), torch.from_numpy(lens_h).cuda()
    d_dst = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).cuda() if dst is not None else None
    dl = np.asarray(deltas, dtype=np.int32)
    i1 = torch.full((out_len,), S, dtype=torch.int64, device='cuda')
    i2 = torch.full((out_len,), S, dtype=torch.int64, device='cuda')
    y = torch.full((out_len,), S, dtype=torch.float64 if f64 else torch.int64, device='cuda')
    rc = lib.abn_tcl_pairs(_lib.ptr(d_row0), _lib.ptr(d_len), lens_h.ctypes.data, len(lens_h), dl.ctypes.data, len(dl), n_same,
                           n_iter, first, seed, epoch, _lib.ptr(d_dst), _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(y), int(f64),
                           out_len, _lib.stream())
    return rc, i1.cpu().numpy(), i2.cpu().numpy(), y.cpu().numpy()


def _files(n_files, rng):
    """Lengths that include exactly 31 (only t = 0), 32 and 100 000, laid out with gaps."""
    special = [31, 32, 100000]
    lens = np.array((special + rng.integers(31, 400, max(0, n_files - 3)).tolist())[:n_files] if n_files > 1 else [31], dtype=np.int64)
    row0 = (np.cumsum(lens + 5) - lens).astype(np.int64)
    return row0, lens


@pytest.mark.parametrize('n_files', [1, 3, 257])
def test_kernel_equals_the_restatement(n_files):
    rng = np.random.default_rng(n_files)
    row0, lens = _files(n_files, rng)
    for n_iter in (1, 63, 64, 65, 1025):
        for seed, epoch, first in ((1, 0, 0), ((7 << 32) + 5, 3, 0), (1, 3, 1000), (1, 0, (1 << 32) - 3)):
            for f64 in (False, True):
                # packed, with room behind the last pair
                out_len = 5 * n_iter + 9
                rc, i1, i2, y = _run_kernel(row0, lens, n_iter, first, seed, epoch, out_len, f64=f64)
                assert rc == 0
                r1, r2, ry = tcl_np.tcl_pairs(row0, lens, n_iter, first, seed, epoch, out_len,
                                              label_dtype=np.float64 if f64 else np.int64)
                assert (i1 == r1).all() and (i2 == r2).all() and (y == ry).all() and y.dtype == ry.dtype
                assert (i1[5 * n_iter:] == S).all() and (i2[5 * n_iter:] == S).all() and (y[5 * n_iter:] == S).all()
            # through a dst table: shuffled places with gaps, sentinel in between
            dst = rng.permutation(n_iter) * 8 + 3
            out_len = 8 * n_iter + 3
            rc, i1, i2, y = _run_kernel(row0, lens, n_iter, first, seed, epoch, out_len, dst=dst, f64=True)
            assert rc == 0
            r1, r2, ry = tcl_np.tcl_pairs(row0, lens, n_iter, first, seed, epoch, out_len, dst=dst, label_dtype=np.float64)
            assert (i1 == r1).all() and (i2 == r2).all() and (y == ry).all()
            assert (i1 == S).sum() == out_len - 5 * n_iter
    if n_files == 1:
        assert (i1[i1 != S] == row0[0]).all()                 # 31 frames: t = 0
    # a dst entry that would write outside the arrays writes nothing
    dst = np.array([0, -1, 16, 10], dtype=np.int64)
    rc, i1, i2, y = _run_kernel(row0, lens, 4, 0, 1, 0, 20, dst=dst)
    r1, r2, ry = tcl_np.tcl_pairs(row0, lens, 4, 0, 1, 0, 20, dst=dst)
    assert rc == 0 and (i1 == r1).all() and (i2 == r2).all() and (y == ry).all() and (i1 == S).sum() == 10
    # other deltas: 16 of them, 3 'same'
    deltas = list(range(1, 17))
    rc, i1, i2, y = _run_kernel(row0, lens, 65, 0, 2, 1, 16 * 65, deltas=deltas, n_same=3)
    r1, r2, ry = tcl_np.tcl_pairs(row0, lens, 65, 0, 2, 1, 16 * 65, deltas=deltas, n_same=3)
    assert rc == 0 and (i1 == r1).all() and (i2 == r2).all() and (y == ry).all()


def test_refused_arguments_launch_nothing():
    from abnet3_amd import _lib
    lib = _lib.load()
    row0, lens = np.array([0, 50, 100], dtype=np.int64), np.array([40, 31, 100], dtype=np.int64)
    ok = dict(n_iter=4, first=0, seed=1, epoch=0, out_len=20)
    bad = [dict(lens=np.array([40, 30, 100])), dict(deltas=[1, 15, 20, 25, 40]), dict(deltas=[]), dict(deltas=list(range(17))),
           dict(n_same=6), dict(n_same=-1), dict(deltas=[1, -15, 20, 25, 30]), dict(out_len=19), dict(n_iter=-1), dict(first=-2)]
    for kw in bad:
        a = dict(ok, lens=lens)
        a.update(kw)
        l = a.pop('lens')
        rc, i1, i2, y = _run_kernel(row0, l, a.pop('n_iter'), a.pop('first'), a.pop('seed'), a.pop('epoch'), a.pop('out_len'), **a)
        assert rc == _lib.E_ARG, kw
        assert lib.abn_last_error().startswith(b'abn_tcl_pairs'), kw
        assert (i1 == S).all() and (i2 == S).all() and (y == S).all(), kw
    d = torch.zeros(8, dtype=torch.int64, device='cuda')
    dl = np.array(tcl_np.DELTAS, dtype=np.int32)
    p = _lib.ptr
    for args in ((0, p(d), p(d), p(d)), (3, None, p(d), p(d)), (3, p(d), None, p(d)), (3, p(d), p(d), None)):
        n_files, a1, a2, ay = args
        assert lib.abn_tcl_pairs(p(d), p(d), lens.ctypes.data, n_files, dl.ctypes.data, 5, 1, 1, 0, 1, 0, None, a1, a2, ay, 0, 8,
                                 _lib.stream()) == _lib.E_ARG, args
    assert lib.abn_tcl_pairs(None, p(d), lens.ctypes.data, 3, dl.ctypes.data, 5, 1, 1, 0, 1, 0, None, p(d), p(d), p(d), 0, 8,
                             _lib.stream()) == _lib.E_ARG
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0


# -- loaders ---------------------------------------------------------------------------------------------------

LENGTHS = (90, 120, 75, 200, 64, 33)


@pytest.fixture(scope='module')
def toy():
    """Six files of 40-d frames, and sampled word pairs (times in seconds) for the dev pass and the mix."""
    rng = np.random.default_rng(12)
    feats = {'utt%d' % k: rng.standard_normal((n, 40)).astype(np.float32) for k, n in enumerate(LENGTHS)}
    times = {k: np.arange(len(v)) * 0.01 + 0.0025 for k, v in feats.items()}
    names = list(feats)

    def token():
        f = names[rng.integers(len(names))]
        n = len(feats[f])
        a = int(rng.integers(0, n - 12))
        return f, a * 0.01, (a + int(rng.integers(6, 12))) * 0.01

    def pairs(n):
        return [token() + token() + ('same' if k % 2 == 0 else 'diff',) for k in range(n)]
    return feats, times, pairs(40), pairs(24)


def _tcl_loader(toy, **kw):
    from abnet3_amd.dataloader import TemporalCoherenceDataLoader
    dl = TemporalCoherenceDataLoader('unused', 'unused', **kw)
    dl.set_data(*toy)
    return dl


def _rows(dl):
    """first table row and length of the files the loader draws from (its train files), by sorted name"""
    c = dl.features
    names = sorted(set(dl.train_files) if dl.train_files is not None else c.names)
    return names, np.array([c.offset[k] for k in names]), np.array([c.length[k] for k in names])


def test_loader_plan_equals_iterator_and_the_restatement(toy):
    a, b = _tcl_loader(toy, batch_size=52, num_max_minibatches=7, seed=5), _tcl_loader(toy, batch_size=52, num_max_minibatches=7, seed=5)
    names, row0, lens = _rows(a)
    its = round(52 / 5)
    ptrs, seen = [], []
    for epoch in range(3):
        it = [tuple(t.clone() for t in batch) for batch in a.batch_iterator(True)]
        plan = b.plan(True)
        assert len(plan) == len(it) == 7 and plan.order == list(range(7))
        ptrs.append((plan.idx1.data_ptr(), plan.idx2.data_ptr(), plan.labels.data_ptr()))
        r1, r2, ry = tcl_np.tcl_pairs(row0, lens, 7 * its, 0, 5, epoch, 7 * its * 5)
        assert (plan.idx1.cpu().numpy() == r1).all() and (plan.idx2.cpu().numpy() == r2).all()
        assert plan.labels.dtype == torch.int64 and (plan.labels.cpu().numpy() == ry).all()
        table = b.features.table
        for k, (x, bid) in enumerate(zip(it, plan.order)):
            y = plan.materialise(bid)
            first, n = plan.span(bid)
            assert n == 5 * its == 50
            for u, v in zip(x, y):
                assert u.dtype == v.dtype and torch.equal(u, v)
            assert torch.equal(y[0], table[plan.idx1[first:first + n]]) and torch.equal(y[1], table[plan.idx2[first:first + n]])
            assert y[2].dtype == torch.int64 and (y[2].cpu().numpy().reshape(-1, 5) == [1, -1, -1, -1, -1]).all()
        seen.append(plan.idx1.cpu().numpy().copy())
    assert ptrs[0] == ptrs[1] == ptrs[2]
    assert (seen[0] != seen[1]).mean() > 0.5 and (seen[1] != seen[2]).mean() > 0.5
    # another seed: other pairs
    c = _tcl_loader(toy, batch_size=52, num_max_minibatches=7, seed=6)
    assert (c.plan(True).idx1.cpu().numpy() != seen[0]).mean() > 0.5


def test_loader_dev_pass_is_the_word_pair_loaders(toy):
    from abnet3_amd.dataloader import OriginalDataLoader
    a = _tcl_loader(toy, batch_size=500, test_words_batch_size=8)
    o = OriginalDataLoader('unused', 'unused', batch_size=500)
    o.set_data(*toy)
    np.random.seed(3)
    got = [tuple(t.clone() for t in b) for b in a.batch_iterator(False)]
    np.random.seed(3)
    ref = [tuple(t.clone() for t in b) for b in o.batch_iterator(False)]
    np.random.seed(3)
    planned = list(a.plan(False))
    assert len(got) == len(ref) == len(planned) == 1           # 24 dev pairs in one batch of (up to) 500 WORD pairs
    for x, y, z in zip(got, ref, planned):
        for u, v, w in zip(x, y, z):
            assert u.dtype == v.dtype == w.dtype and torch.equal(u, v) and torch.equal(u, w)
    assert a.tcl_epoch == 0                                   # the dev pass draws nothing


def test_short_files_are_left_out_with_one_warning(toy):
    from abnet3_amd.dataloader import TemporalCoherenceDataLoader
    feats, times, train, dev = toy
    feats = dict(feats, short=np.zeros((20, 40), dtype=np.float32), edge=np.zeros((30, 40), dtype=np.float32))
    times = {k: np.arange(len(v)) * 0.01 + 0.0025 for k, v in feats.items()}
    dl = TemporalCoherenceDataLoader('unused', 'unused', batch_size=500, num_max_minibatches=4)
    # (the train pairs only say which files train: this loader never aligns them)
    dl.set_data(feats, times, train + [('short', 0.0, 0.1, 'edge', 0.0, 0.1, 'diff')], dev)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        p1 = dl.plan(True)
        i1 = p1.idx1.cpu().numpy().copy()
        i2 = p1.idx2.cpu().numpy().copy()
        dl.plan(True)
        list(dl.batch_iterator(True))
    assert len([x for x in w if 'left out' in str(x.message)]) == 1
    c = dl.features
    for k in ('short', 'edge'):
        lo, hi = c.offset[k], c.offset[k] + c.length[k]
        assert not ((i1 >= lo) & (i1 < hi)).any() and not ((i2 >= lo) & (i2 < hi)).any()
    # every pair inside ONE eligible file
    names = sorted(k for k in c.names if c.length[k] > 30)
    row0 = np.array([c.offset[k] for k in names])
    order = np.argsort(row0)
    f = order[np.searchsorted(row0[order], i1, 'right') - 1]
    assert (i1 >= row0[f]).all() and (i2 < row0[f] + np.array([c.length[names[j]] for j in f])).all()
    # nothing eligible: an error, not a crash inside the draw
    only = TemporalCoherenceDataLoader('unused', 'unused')
    only.set_data({'short': feats['short']}, {'short': times['short']}, [('short', 0.0, 0.1, 'short', 0.05, 0.15, 'diff')], [])
    with pytest.raises(ValueError):
        only.plan(True)
    bad = _tcl_loader(toy)
    bad.TCL_DISTANCE_SAME = [31]
    with pytest.raises(ValueError):
        bad.plan(True)


def _mix_loader(toy, tcl_seed, **kw):
    from abnet3_amd.dataloader import OriginalDataLoader
    dl = OriginalDataLoader('unused', 'unused', batch_size=8, tcl=kw.pop('tcl', 0.3), tcl_seed=tcl_seed, **kw)
    dl.set_data(*toy)
    return dl


def test_mix_head_is_the_word_pair_batch_and_tail_the_restatement(toy):
    from abnet3_amd.dataloader import OriginalDataLoader
    assert _mix_loader(toy, None).plan(True) is None and _mix_loader(toy, 4).plan(False) is None
    base = OriginalDataLoader('unused', 'unused', batch_size=8)
    base.set_data(*toy)
    mix, mix_it = _mix_loader(toy, 4), _mix_loader(toy, 4)
    names, row0, lens = _rows(mix)
    ptrs = []
    for epoch in range(2):
        np.random.seed(8)
        pb = base.plan(True)
        np.random.seed(8)
        pm = mix.plan(True)
        np.random.seed(8)
        it = [tuple(t.clone() for t in b) for b in mix_it.batch_iterator(True)]
        assert pb.order == pm.order and len(it) == len(pm.order) == 5
        ptrs.append((pm.idx1.data_ptr(), pm.idx2.data_ptr(), pm.labels.data_ptr()))
        tails = [tcl_np.mix_tail(0.3, pb.span(b)[1]) for b in range(5)]
        assert sum(tails) > 0
        f, t = tcl_np.draws(lens, 30, sum(tails) // 5, 0, 4, epoch)
        at = np.concatenate(([0], np.cumsum(tails))) // 5
        for k, bid in enumerate(pm.order):
            x1, x2, y = pm.materialise(bid)
            h1, h2, hy = pb.materialise(bid)
            n = len(hy)
            assert len(y) == n + tails[bid] and y.dtype == torch.float64
            assert torch.equal(x1[:n], h1) and torch.equal(x2[:n], h2) and torch.equal(y[:n], hy)
            first = pm.span(bid)[0]
            a = (row0[f] + t)[at[bid]:at[bid + 1]]
            assert (pm.idx1[first + n:first + len(y)].cpu().numpy() == np.repeat(a, 5)).all()
            assert (pm.idx2[first + n:first + len(y)].cpu().numpy() == (a[:, None] + np.array(tcl_np.DELTAS)).ravel()).all()
            assert (y[n:].cpu().numpy().reshape(-1, 5) == [1, -1, -1, -1, -1]).all()
            assert torch.equal(x1[n:], mix.features.table[pm.idx1[first + n:first + len(y)]])
            for u, v in zip(it[k], (x1, x2, y)):
                assert u.dtype == v.dtype and torch.equal(u, v)
    assert ptrs[0] == ptrs[1]
    # a share too small for one draw appends nothing
    none = _mix_loader(toy, 4, tcl=0.001)
    np.random.seed(8)
    pn = none.plan(True)
    assert all(pn.span(b) == pb.span(b) for b in range(5))


# -- the trainer -------------------------------------------------------------------------------------------------

def _train(dl_factory, tmp_path, planned, tag):
    from abnet3_amd.loss import coscos2
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    dl = dl_factory()
    np.random.seed(0)
    random.seed(0)
    torch.manual_seed(0)
    net = SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=32, p_dropout=0.0, batch_norm=False,
                         activation_layer='sigmoid', output_path=str(tmp_path / ('net_%s%d' % (tag, planned))))
    tr = TrainerSiamese(network=net, loss=coscos2(avg=False), num_epochs=2, patience=5, optimizer_type='adadelta', lr=0.1,
                        dataloader=dl, log_dir=str(tmp_path / 'runs'))
    tr.planned_passes = planned
    tr.train()
    if planned:
        assert any(v['graph'] is not None for v in tr._buckets.values())       # captured steps did run
    return list(tr.train_losses), list(tr.dev_losses), {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def _same_training(a, b):
    (tl_a, dl_a, p_a), (tl_b, dl_b, p_b) = a, b
    print('train losses', tl_a, tl_b, 'dev losses', dl_a, dl_b)
    assert len(tl_a) == 3
    assert np.allclose(tl_a, tl_b, rtol=2e-5) and np.allclose(dl_a, dl_b, rtol=2e-5), (tl_a, tl_b, dl_a, dl_b)
    for k in p_a:
        print(k, rel_err(p_a[k], p_b[k]))
        assert rel_err(p_a[k], p_b[k]) < 2e-5, (k, rel_err(p_a[k], p_b[k]))


def test_trainer_planned_pass_trains_like_the_iterator(toy, tmp_path):
    make = lambda: _tcl_loader(toy, batch_size=500, num_max_minibatches=12, seed=1)
    _same_training(_train(make, tmp_path, True, 'tcl'), _train(make, tmp_path, False, 'tcl'))


def test_trainer_planned_mix_trains_like_the_iterator(toy, tmp_path):
    make = lambda: _mix_loader(toy, 2)
    _same_training(_train(make, tmp_path, True, 'mix'), _train(make, tmp_path, False, 'mix'))


def test_a_corpus_with_a_short_file_trains(toy, tmp_path):
    feats, times, train, dev = toy
    feats = dict(feats, short=np.ones((20, 40), dtype=np.float32))
    times = {k: np.arange(len(v)) * 0.01 + 0.0025 for k, v in feats.items()}

    def make():
        from abnet3_amd.dataloader import TemporalCoherenceDataLoader
        dl = TemporalCoherenceDataLoader('unused', 'unused', batch_size=100, num_max_minibatches=6, seed=2)
        dl.set_data(feats, times, train + [('short', 0.0, 0.1, 'utt0', 0.0, 0.1, 'diff')], dev)
        return dl
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        tl, dv, _ = _train(make, tmp_path, True, 'short')
    assert len([x for x in w if 'left out' in str(x.message)]) == 1
    assert len(tl) == 3 and np.isfinite(tl).all() and np.isfinite(dv).all()
