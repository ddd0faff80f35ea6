"""The host side of soft-DTW word-pair training without a GPU: the float64 restatement (tests/sdtw_np.py) against path
enumeration and central differences, the induction properties of the value and of E, the abnq_ ledger of
include/abnet3_hip_next.h, the refusals of the abnq_ entries that need neither a launch nor a device, abnq_softdtw_ws_bytes,
the wrapper's overlap refusal, the batches of WordPairDataLoader (over a host stand-in for the device corpus: the batch's
composition is host code; tests/test_gpu_sdtw.py runs the loader on the device, from files) and the class lookup a gridsearch
experiment does.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdtw_np as S  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abnq_softdtw_max_len', 'abnq_softdtw_max_d', 'abnq_softdtw_ws_bytes', 'abnq_softdtw_forward', 'abnq_softdtw_backward'}
CASES = [(1, 1, 8, 1.0), (5, 7, 8, 1.0), (5, 7, 8, 0.01), (4, 5, 3, 0.1), (3, 3, 1, 10.0), (9, 2, 5, 1e-3)]


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,m,D,gamma', [c for c in CASES if c[0] <= 5 and c[1] <= 5] + [(5, 5, 4, 0.05), (1, 5, 2, 0.3), (5, 1, 2, 0.3)])
def test_value_against_path_enumeration(n, m, D, gamma):
    x, y = S.draw(np.random.default_rng(n * 100 + m), n, m, D)
    q = S.problem(x, y, gamma)
    want = S.brute_value(q['d'], gamma)
    assert abs(q['value'] - want) <= 1e-12 * max(1.0, abs(want))
    assert len(list(S.monotone_paths(2, 2))) == 3 and len(list(S.monotone_paths(3, 3))) == 13          # Delannoy numbers


@pytest.mark.parametrize('n,m,D,gamma', CASES)
def test_gradients_against_central_differences(n, m, D, gamma):
    rng = np.random.default_rng(n + 10 * m)
    x, y = S.draw(rng, n, m, D)
    w = -0.7
    q = S.problem(x, y, gamma, w)
    h = 1e-6
    worst = 0.0
    for tab, grad, side in ((x, q['g1'], 0), (y, q['g2'], 1)):
        for i in range(tab.shape[0]):
            for k in range(D):
                up, dn = tab.astype(np.float64).copy(), tab.astype(np.float64).copy()
                up[i, k] += h
                dn[i, k] -= h
                f = (lambda t: S.problem(t, y, gamma)['value']) if side == 0 else (lambda t: S.problem(x, t, gamma)['value'])
                worst = max(worst, abs(w * (f(up) - f(dn)) / (2 * h) - grad[i, k]))
    assert worst <= 2e-8, worst                  # (h^2 f''' / 6 + 1e-16 / h over values of size 1 .. 10; measured 3e-10 .. 4e-9)
    # dvalue / dd = E: one cell of d moved on its own
    i, j = n // 2, m // 2
    up, dn = q['d'].copy(), q['d'].copy()
    up[i, j] += h
    dn[i, j] -= h
    assert abs((S.value_r(up, gamma)[0] - S.value_r(dn, gamma)[0]) / (2 * h) - q['E'][i, j]) <= 2e-8


def test_clamped_rows_take_the_plain_gradient():
    rng = np.random.default_rng(4)
    x, y = S.draw(rng, 4, 5, 3)
    x[1] = 0.0
    x[2] = np.float32(1e-7) * x[2] / np.linalg.norm(x[2])
    q = S.problem(x, y, 0.1)
    assert np.isfinite(q['g1']).all() and q['g1'][1].any()
    # below the clamp x^ = 1e6 x: a step of 1e-11 in x is one of 1e-5 in x^ (truncation h^2, rounding 1e-16 / 1e-11 on 2e5)
    h = 1e-11
    for i in (1, 2):
        up, dn = x.astype(np.float64).copy(), x.astype(np.float64).copy()
        up[i, 0] += h
        dn[i, 0] -= h
        fd = (S.problem(up, y, 0.1)['value'] - S.problem(dn, y, 0.1)['value']) / (2 * h)
        assert abs(fd - q['g1'][i, 0]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, q['g1'][i, 0])


@pytest.mark.parametrize('n,m,D,gamma', CASES + [(20, 13, 6, 0.1), (13, 20, 6, 1e-3)])
def test_properties_of_value_and_expected_alignment(n, m, D, gamma):
    x, y = S.draw(np.random.default_rng(7 * n + m), n, m, D)
    q = S.problem(x, y, gamma)
    hard = S.hard_cost(q['d'])
    tol = 1e-12 * max(1.0, abs(hard))
    assert q['value'] <= hard + tol
    assert hard - q['value'] <= gamma * np.log(3.0) * (n + m - 2) + tol
    assert max(n, m) - 1e-9 <= q['E'].sum() <= n + m - 1 + 1e-9
    assert (q['E'] >= 0).all() and abs(q['E'][0, 0] - 1.0) <= 1e-9 and q['E'][-1, -1] == 1.0
    t = S.problem(y, x, gamma)
    assert abs(t['value'] - q['value']) <= 1e-12 * max(1.0, abs(q['value']))
    assert np.abs(t['E'].T - q['E']).max() <= 1e-9
    assert np.abs(t['g1'] - q['g2']).max() <= 1e-9 and np.abs(t['g2'] - q['g1']).max() <= 1e-9


@pytest.mark.parametrize('gamma', (1.0, 0.1, 1e-3))
def test_divergence_is_non_negative_and_zero_on_the_diagonal(gamma):
    rng = np.random.default_rng(11)
    x, y = S.draw(rng, 6, 8, 4)
    v, gx, gy = S.divergence(x, y, gamma)
    assert v >= 0.0
    v0, g0x, g0y = S.divergence(x, x.copy(), gamma)
    assert abs(v0) <= 1e-12
    assert np.abs(g0x + g0y).max() <= 1e-9                    # moving both copies together changes nothing
    assert np.abs(g0x).max() <= 1e-9                          # ... and, by symmetry, neither does moving one


def test_loss_restatement_terms_and_gradient():
    rng = np.random.default_rng(13)
    e = rng.standard_normal((30, 4)).astype(np.float32)
    off1, n1, off2, n2, y = [0, 5], [5, 6], [11, 20], [7, 4], [1, -1]
    for normalize in (True, False):
        for div in (True, False):
            for avg in (True, False):
                margin = 0.5 if normalize else 2.5
                L, terms, de = S.loss(e, off1, n1, off2, n2, y, 0.1, margin, normalize, div, avg)
                assert abs(L - terms.sum() / (2 if avg else 1)) <= 1e-14
                for i, k in ((0, 0), (12, 1), (21, 3)):
                    up, dn = e.astype(np.float64).copy(), e.astype(np.float64).copy()
                    up[i, k] += 1e-6
                    dn[i, k] -= 1e-6
                    fd = (S.loss(up, off1, n1, off2, n2, y, 0.1, margin, normalize, div, avg)[0] -
                          S.loss(dn, off1, n1, off2, n2, y, 0.1, margin, normalize, div, avg)[0]) / 2e-6
                    assert abs(fd - de[i, k]) <= 2e-8
                assert not de[24:].any()
    assert S.loss(e, [], [], [], [], [], avg=True)[0] == 0.0 and S.loss(e, [], [], [], [], [], avg=False)[0] == 0.0


def test_float32_cell_yardstick_is_close_to_the_restatement():
    x, y = S.draw(np.random.default_rng(17), 20, 13, 16)
    for gamma in (1.0, 1e-3):
        a, b = S.problem(x, y, gamma), S.problem(x, y, gamma, cell_dtype=np.float32)
        assert b['c'].dtype == np.float64 and S.cells(x, y, np.float32)['c'].dtype == np.float32
        assert 0 < abs(a['value'] - b['value']) <= (20 + 13 - 1) * (2 * 16 + 8) * 2.0 ** -24
        assert 0 < np.abs(a['g1'] - b['g1']).max() <= 1e-5


# ---- the ledger ---------------------------------------------------------------------------------------------------------
def declared(prefix='abnq_'):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, text))


def test_sdtw_symbols_are_the_headers_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib, build
    assert declared() == set(_lib.SDTW_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS) | set(_lib.EVAL_SYMBOLS) | set(_lib.CAE_SYMBOLS)
    for k in vars(_lib):
        if k.startswith('NEXT') and k.endswith('_SYMBOLS'):
            others |= set(getattr(_lib, k))
    assert not NAMES & others and not [k for k in vars(_lib) if k.startswith('NEXT8')]
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abnq_')}
    assert exported == NAMES
    for name, (res, args) in _lib.SDTW_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert len(_lib.SDTW_SYMBOLS['abnq_softdtw_forward'][1]) == 14 and len(_lib.SDTW_SYMBOLS['abnq_softdtw_backward'][1]) == 15
    assert lib.abn_abi_version() == 20 and _lib.ABI_VERSION == 20
    head = open(HEADER).read()
    top = head[:head.index('#ifndef')]
    assert 'abnq_' in top and 'SDTW_SYMBOLS' in top
    assert 'softdtw.hip' in build.SOURCES


def host_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_limits_and_ws_bytes(lib):
    assert lib.abnq_softdtw_max_len() >= 256 and lib.abnq_softdtw_max_d() >= 1024
    cap, dcap = lib.abnq_softdtw_max_len(), lib.abnq_softdtw_max_d()

    def ws(n1, n2, D, keep):
        a, pa = host_i32(n1)
        b, pb = host_i32(n2)
        return lib.abnq_softdtw_ws_bytes(pa, pb, len(a), D, keep)

    def up16(v):
        return (v + 15) // 16 * 16

    def layout(n1, n2, D, keep):                 # the header's formula
        N, cells = sum(n1) + sum(n2), sum(a * b for a, b in zip(n1, n2))
        return 64 + up16(24 * (len(n1) + 1)) + 16 * N + up16(4 * cells) + (16 * cells if keep else 0)
    for n1, n2, D in (([1], [1], 1), ([5, 9, 12], [6, 4, 11], 8), ([cap], [3], 7), ([40] * 7, [33] * 7, 100), ([3], [cap], dcap)):
        for keep in (0, 1):
            assert ws(n1, n2, D, keep) == layout(n1, n2, D, keep), (n1, n2, D, keep)
        assert ws(n1, n2, D, 0) < ws(n1, n2, D, 1)
    base = ws([5, 9], [6, 4], 8, 1)
    assert ws([5, 10], [6, 4], 8, 1) > base and ws([5, 9], [6, 5], 8, 1) > base and ws([5, 9, 1], [6, 4, 1], 8, 1) > base
    assert ws([5, 9], [6, 4], 9, 1) >= base and ws([5, 9], [6, 4], 8, 0) < base          # (nothing in the workspace is D wide)
    assert ws([], [], 8, 1) == 64 + 32                                    # P = 0: the header and one prefix entry
    for n1, n2, D in (([0], [3], 8), ([3], [-1], 8), ([3], [3], 0), ([cap + 1], [3], 8), ([3], [cap + 1], 8), ([3], [3], dcap + 1)):
        assert ws(n1, n2, D, 1) == -1 and b'abnq_softdtw_ws_bytes' in lib.abn_last_error(), (n1, n2, D)
    assert lib.abnq_softdtw_ws_bytes(None, None, 2, 8, 1) == -1 and b'null' in lib.abn_last_error()
    assert lib.abnq_softdtw_ws_bytes(None, None, -1, 8, 1) == -1


def test_refusals_that_need_no_launch(lib):
    """What the entries refuse before they look at the device arrays: scalars, null and misaligned pointers.  (The refusals
    that depend on the arrays' contents -- a length < 1 or beyond the limit, a run outside the table, a small workspace, a
    backward after keep = 0 -- read the arrays from the device: tests/test_gpu_sdtw.py.)"""
    from abnet3_amd import _lib
    p = 256                                                                          # a non-null, aligned address that is never read
    fwd = dict(e=p, R=40, D=8, off1=p, n1=p, off2=p, n2=p, P=3, gamma=0.1, value=p, ws=p, ws_bytes=1 << 20, keep=1, stream=0)
    bwd = dict(e=p, R=40, D=8, off1=p, n1=p, off2=p, n2=p, P=3, gamma=0.1, w=p, g1=p, g2=p, ws=p, ws_bytes=1 << 20, stream=0)

    def call(fn, ok, **kw):
        a = dict(ok)
        a.update(kw)
        return fn(*[a[k] for k in ok])
    for fn, ok, outs in ((lib.abnq_softdtw_forward, fwd, ('value',)), (lib.abnq_softdtw_backward, bwd, ('w', 'g1', 'g2'))):
        assert call(fn, ok, P=-1) == _lib.E_ARG and b'P = -1' in lib.abn_last_error()
        assert call(fn, ok, D=0) == _lib.E_ARG and b'D = 0' in lib.abn_last_error()
        assert call(fn, ok, D=lib.abnq_softdtw_max_d() + 1) == _lib.E_UNSUPPORTED and b'abnq_softdtw_max_d' in lib.abn_last_error()
        assert call(fn, ok, R=-1) == _lib.E_ARG
        for gamma in (0.0, -1.0, float('inf'), float('nan'), 1e-46):
            assert call(fn, ok, gamma=gamma) == _lib.E_ARG and b'gamma' in lib.abn_last_error(), gamma
        assert call(fn, ok, ws_bytes=-1) == _lib.E_ARG
        for name in ('e', 'off1', 'n1', 'off2', 'n2', 'ws') + outs:
            assert call(fn, ok, **{name: 0}) == _lib.E_ARG and b'null' in lib.abn_last_error(), name
        for name, step in (('e', 2), ('n1', 2), ('n2', 1), ('off1', 4), ('off2', 4)):
            assert call(fn, ok, **{name: p + step}) == _lib.E_ARG and b'misaligned' in lib.abn_last_error(), name
        for name in outs:
            assert call(fn, ok, **{name: p + 2}) == _lib.E_ARG and b'misaligned' in lib.abn_last_error(), name
        assert call(fn, ok, ws=p + 8) == _lib.E_ARG and b'16-byte aligned' in lib.abn_last_error()
        # P = 0: a successful no-op that looks at no pointer
        assert call(fn, ok, P=0, **{k: 0 for k in ('e', 'off1', 'n1', 'off2', 'n2', 'ws') + outs}) == 0
    assert call(lib.abnq_softdtw_backward, bwd, ws_bytes=32) == _lib.E_ARG and b'header' in lib.abn_last_error()


# ---- the python surface -------------------------------------------------------------------------------------------------
def test_overlap_refusal_and_column_checks():
    from abnet3_amd import softdtw
    ok = softdtw.require_disjoint('t', [0, 5], [5, 6], [11, 20], [7, 4])
    assert [a.dtype for a in ok] == [np.int64, np.int32, np.int64, np.int32]
    softdtw.require_disjoint('t', [0, 5], [5, 6], [0, 5], [5, 6])                    # the sides may coincide
    softdtw.require_disjoint('t', [5, 0], [6, 5], [20, 11], [4, 7])                  # any order
    softdtw.require_disjoint('t', [], [], [], [])
    with pytest.raises(ValueError, match='overlap on side 1'):
        softdtw.require_disjoint('t', [0, 4], [5, 6], [11, 20], [7, 4])
    with pytest.raises(ValueError, match='overlap on side 2'):
        softdtw.require_disjoint('t', [0, 5], [5, 6], [11, 11], [7, 4])
    with pytest.raises(ValueError, match='overlap on side 1'):
        softdtw.require_disjoint('t', [3, 3], [1, 1], [11, 20], [7, 4])
    with pytest.raises(ValueError, match='one length'):
        softdtw.require_disjoint('t', [0, 5], [5], [11, 20], [7, 4])
    with pytest.raises(ValueError, match='1-d'):
        softdtw.require_disjoint('t', [[0, 5]], [[5, 6]], [[11, 20]], [[7, 4]])
    rows = softdtw._block_rows(np.array([10, 3], dtype=np.int64), np.array([2, 3], dtype=np.int32))
    assert rows.tolist() == [10, 11, 3, 4, 5]
    import torch
    e = torch.zeros(4, 3)
    with pytest.raises(ValueError, match='overlap'):
        softdtw.soft_dtw(e, [0, 1], [2, 2], [0, 2], [1, 1], 0.1)                    # refused before the device is asked for
    with pytest.raises(Exception) as err:
        softdtw.soft_dtw_batch(e, [0], [2], [2], [2], 0.1)                          # a host tensor: no CPU path
    assert 'HIP' in str(err.value) or 'device' in str(err.value)
    with pytest.raises(ValueError, match='gamma'):
        softdtw._check_gamma('t', 0.0)
    from abnet3_amd.loss import LossBuilder, SoftDTWLoss
    f = SoftDTWLoss()
    assert isinstance(f, LossBuilder) and (f.gamma, f.margin, f.normalize, f.divergence, f.avg) == (0.1, 0.5, True, False, True)
    assert SoftDTWLoss(gamma=1.0, divergence=True).whoami()['class_name'] == 'SoftDTWLoss'
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='gamma'):
            SoftDTWLoss(gamma=bad)
    assert 'untuned' in SoftDTWLoss.__doc__.lower() and 'nothing has been measured on speech' in SoftDTWLoss.__doc__


class HostCorpus(object):
    """dataloader.DeviceCorpus with the table left on the host: the token lookup is DeviceCorpus's own."""

    def __new__(cls, features, times):
        import torch
        from abnet3_amd.dataloader import DeviceCorpus
        self = DeviceCorpus.__new__(DeviceCorpus)
        self.names = list(features)
        self.offset, self.length, self.times, o = {}, {}, {}, 0
        for k in self.names:
            self.offset[k], self.length[k], self.times[k] = o, len(features[k]), np.asarray(times[k])
            o += len(features[k])
        self.dim, self.total = features[self.names[0]].shape[1], o
        self.table = torch.from_numpy(np.concatenate([features[k] for k in self.names]).astype(np.float32))
        self._init_lookup()
        return self


def test_word_pair_loader_batches(tmp_path, monkeypatch):
    import fake_h5features
    import abnet3_amd.dataloader as DL
    from abnet3_amd.utils import read_dataset, write_dataset
    cap = 256
    rng = np.random.default_rng(23)
    lens = {'u0': 300, 'u1': 120, 'u2': 400}
    feats = {k: rng.standard_normal((n, 5)).astype(np.float32) for k, n in lens.items()}
    times = {k: np.arange(n) * 0.01 + 0.005 for k, n in lens.items()}
    fake_h5features.write(str(tmp_path / 'f.h5f'), 'features', list(feats), [times[k] for k in feats], [feats[k] for k in feats])
    pairs = [('u0', 0.10, 0.29, 'u1', 0.50, 0.61, 'same'),              # 19 x 11 frames ...
             ('u0', 0.50, 0.53, 'u2', 1.00, 1.40, 'diff'),
             ('u1', 0.00, 0.05, 'u2', 2.00, 2.02, 'same'),
             ('u0', 1.00, 1.30, 'u1', 0.700, 0.701, 'same'),            # side 2 holds no frame: dropped
             ('u2', 0.00, 3.50, 'u0', 0.10, 0.20, 'diff'),              # 350 frames > max_len: dropped
             ('u2', 3.00, 3.10, 'u0', 2.00, 2.50, 'diff'),
             ('u1', 1.00, 1.10, 'u1', 1.00, 1.10, 'same')]              # a token against itself
    for sub in ('train_pairs', 'dev_pairs'):
        os.makedirs(str(tmp_path / sub))
        write_dataset(str(tmp_path / sub / 'dataset'), pairs if sub == 'train_pairs' else pairs[:2])
    got = fake_h5features.Reader(str(tmp_path / 'f.h5f'), 'features').read()
    monkeypatch.setattr(DL, 'gather_rows', lambda table, idx: table[idx])
    monkeypatch.setattr('abnet3_amd.softdtw.max_len', lambda: cap)
    dl = DL.WordPairDataLoader(str(tmp_path), str(tmp_path / 'f.h5f'), batch_size=4, seed=0)
    assert not hasattr(dl, 'plan') and dl.whoami()['class_name'] == 'WordPairDataLoader'
    dl.features = HostCorpus(got.dict_features(), got.dict_labels())
    dl.pairs['train'] = read_dataset(str(tmp_path / 'train_pairs' / 'dataset'))
    dl.pairs['dev'] = read_dataset(str(tmp_path / 'dev_pairs' / 'dataset'))
    np.random.seed(0)
    batches = list(dl.batch_iterator(True))
    assert len(batches) == 2 and sorted(len(b[5]) for b in batches) == [2, 3]
    table = dl.features.table.numpy()
    seen = []
    for X, off1, n1, off2, n2, y in batches:
        assert off1.dtype == np.int64 and off2.dtype == np.int64 and n1.dtype == np.int32 and n2.dtype == np.int32
        assert X.shape == (int(n1.sum() + n2.sum()), 5) and str(y.dtype) == 'torch.int64'
        # side 1's tokens end to end from row 0, then side 2's: no two ranges overlap
        assert off1.tolist() == (np.cumsum(n1) - n1).tolist() and off2.tolist() == (n1.sum() + np.cumsum(n2) - n2).tolist()
        for p in range(len(n1)):
            seen.append((X[off1[p]:off1[p] + n1[p]].numpy(), X[off2[p]:off2[p] + n2[p]].numpy(), int(y[p])))
    kept = [pr for k, pr in enumerate(pairs) if k not in (3, 4)]
    assert len(seen) == len(kept)
    for f1, s1, e1, f2, s2, e2, kind in kept:
        (a, na), (b, nb) = dl.features.token(f1, s1, e1), dl.features.token(f2, s2, e2)
        assert 1 <= na <= cap and 1 <= nb <= cap
        hit = [s for s in seen if s[0].shape[0] == na and s[1].shape[0] == nb and np.array_equal(s[0], table[a:a + na]) and
               np.array_equal(s[1], table[b:b + nb])]
        assert len(hit) == 1 and hit[0][2] == (1 if kind == 'same' else -1), (f1, s1, kind)
    st = dl.statistics_training
    assert (st['DroppedEmpty'], st['DroppedLong'], st['SameType'], st['DiffType']) == (1, 1, 3, 2)
    dev = list(dl.batch_iterator(False))
    assert len(dev) == 1 and dev[0][5].tolist() == [1, -1]
    with pytest.raises(AssertionError):
        DL.WordPairDataLoader(str(tmp_path), str(tmp_path / 'f.h5f'), tcl=0.1)


def test_gridsearch_resolves_the_three_classes():
    """A gridsearch YAML names classes and looks them up with getattr on their modules."""
    import abnet3_amd.dataloader
    import abnet3_amd.loss
    import abnet3_amd.trainer
    cls = getattr(abnet3_amd.trainer, 'TrainerSequencePairs')
    assert issubclass(cls, abnet3_amd.trainer.TrainerSiamese)
    assert cls.give_batch_to_network is not abnet3_amd.trainer.TrainerSiamese.give_batch_to_network      # what keeps _direct_ok() false
    assert 'BatchNorm' in cls.__doc__ and 'both' in cls.__doc__.lower()
    assert issubclass(getattr(abnet3_amd.dataloader, 'WordPairDataLoader'), abnet3_amd.dataloader.OriginalDataLoader)
    assert issubclass(getattr(abnet3_amd.loss, 'SoftDTWLoss'), abnet3_amd.loss.LossBuilder)
    assert 'plan' not in vars(abnet3_amd.dataloader.WordPairDataLoader) or isinstance(vars(abnet3_amd.dataloader.WordPairDataLoader)['plan'], property)
