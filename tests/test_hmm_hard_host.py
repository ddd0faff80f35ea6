"""Viterbi training of the full-transition HMM on the host: the numpy restatement of the hard statistics
(tests/hmm_hard_np.py) against hmm.bigram_counts and against the score they are meant to maximise, the float64 training
loop on the planted corpus, the Python layer's checks, the abnv_ ledger of include/abnet3_hip_next.h, and the refusals that
need no launch.  No kernel runs here."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_dense_dur_np as dd  # noqa: E402
import hmm_hard_np as hh  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abnv_hmm_hard_stats_ws_bytes', 'abnv_hmm_hard_stats'}


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_counts_without_a_minimum_duration_are_the_bigram_counts():
    from abnet3_amd import hmm
    rng = np.random.default_rng(1)
    for K in (1, 2, 5, 17):
        seqs = []
        for L in (0, 1, 2, 9, 60):
            a = rng.integers(0, K, size=L).astype(np.int32)
            a[rng.random(L) < 0.2] = -1
            seqs.append(a)
        total = np.zeros((K + 1, K), dtype=np.int64)
        for a in seqs:
            c, n = hh.counts_one(a, K, 1)
            assert n == int((a >= 0).sum())
            total += c
        assert np.array_equal(total[:K], hmm.bigram_counts(seqs, K))
        assert total[K].sum() == sum(1 for a in seqs if (a >= 0).any())
        x = np.zeros((sum(len(a) for a in seqs), 1), dtype=np.float32)
        lens = [len(a) for a in seqs]
        off = np.cumsum(lens) - lens
        counts, sums, ng = hh.hard_stats(x, off, lens, np.zeros(1), np.concatenate(seqs), K, 1)
        assert np.array_equal(counts, total) and ng.tolist() == [int((a >= 0).sum()) for a in seqs]
        assert np.array_equal(sums[:, 2], np.bincount(np.concatenate(seqs)[np.concatenate(seqs) >= 0], minlength=K))


def test_a_run_gives_its_frames_beyond_the_minimum_as_stays_and_bad_frames_do_not_break_it():
    for S in (1, 2, 3, 8):
        for L in range(0, 13):
            c, n = hh.counts_one([1] * L, 3, S)
            assert n == L and c[1, 1] == max(L - S, 0) and c.sum() == (L > 0) + max(L - S, 0) and (L == 0 or c[3, 1] == 1)
        # a BAD frame and an id outside 0 .. K - 1 inside a run: the run continues over them
        c, n = hh.counts_one([-1, 2, 2, -1, 2, 7, 2, -5, 2, 0, 0, -1], 3, S)
        assert n == 7 and c[2, 2] == max(5 - S, 0) and c[2, 0] == 1 and c[0, 0] == max(2 - S, 0) and c[3, 2] == 1


def normalised(counts):
    K = counts.shape[1]
    c = counts.astype(np.float64)
    tot = c.sum(axis=1, keepdims=True)
    return np.where(tot > 0, c / np.where(tot > 0, tot, 1.0), 1.0 / K)


def test_normalised_counts_maximise_the_score_of_their_path():
    """Every id sequence over K = 3 of length <= 7, S = 1, 2, 3: with the emissions at 0 the float64 score J_runs of the path
    under (init, trans) = the normalised counts is not raised by moving any one row towards another distribution."""
    K = 3
    rng = np.random.default_rng(2)
    others = rng.dirichlet(np.ones(K), size=8)
    n, moved = 0, 0
    with np.errstate(divide='ignore'):
        for L in range(1, 8):
            s = np.zeros((L, K))
            good = np.ones(L, dtype=bool)
            for path in itertools.product(range(K), repeat=L):
                for S in (1, 2, 3):
                    counts, _ = hh.counts_one(path, K, S)
                    p = normalised(counts)
                    best = dd.J_runs(s, path, good, np.log(p[K]), np.log(p[:K]), S)
                    assert np.isfinite(best)
                    for row in range(K + 1):
                        if not counts[row].sum():
                            continue
                        q = p.copy()
                        q[row] = 0.7 * p[row] + 0.3 * others[(n + row) % 8]
                        other = dd.J_runs(s, path, good, np.log(q[K]), np.log(q[:K]), S)
                        assert other <= best + 1e-12, (path, S, row)
                        moved += other < best - 1e-9
                    n += 1
    assert n == 3 * sum(3 ** L for L in range(1, 8)) and moved >= n // 2          # (the moves did cost something)


@pytest.mark.parametrize('S', [1, 3])
def test_float64_training_loop_is_monotone_on_the_planted_corpus(S):
    from abnet3_amd import hmm
    for seed in (0, 1, 2):
        x, lens, means, trans, _ = hh.planted_corpus(seed)
        shift = np.nanmean(x, axis=0).astype(np.float32)
        gv = np.nanvar(x.astype(np.float64), axis=0)
        m0, v0, t0, i0 = hh.planted_start(means, seed)
        lps, m, v, tr, ini, ids, _ = hh.fit_viterbi(hmm, x, lens, shift, m0 - shift.astype(np.float64), v0, gv, t0, i0, S=S, n_iter=10,
                                                    tol=-np.inf)
        assert len(lps) >= 3 and (np.diff(lps) >= -1e-12).all(), (seed, lps)
        assert (v > 1.5 * 0.01 * gv).all()                                       # the variance floor never bound
        off_diag = np.where(np.eye(4, dtype=bool), -1.0, tr)
        assert [int(np.argmax(off_diag[k])) for k in range(4)] == [1, 2, 3, 0]  # the planted successor
        if S == 1:
            assert np.abs(np.diag(tr) - 0.8).max() <= 0.07 and np.abs(m + shift - means).max() <= 0.11


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_on_the_host(lib, tmp_path):
    from abnet3_amd import hmm
    from test_hmm_host import fitted_mixture
    K, D, T = 3, 2, 6
    z = lambda *s: torch.zeros(*s)
    ids = torch.zeros(T, dtype=torch.int32)
    ok = dict(table=z(T, D), off=[0, 3], lens=[3, 3], shift=z(D), ids=ids, K=K)
    call = lambda **kw: hmm.hard_stats(**dict(ok, **kw))
    for bad in (0, 9, 2.5, True, '2'):
        with pytest.raises(ValueError, match='min_duration'):
            call(min_duration=bad)
    for bad in (-1, 257, 1.5, True, None):
        with pytest.raises(ValueError, match='n_ranges'):
            call(n_ranges=bad)
    with pytest.raises(ValueError, match='float32'):
        call(table=z(T, D).double())
    with pytest.raises(ValueError, match='shift'):
        call(shift=z(D + 1))
    for bad in (ids.long(), ids[:5], torch.zeros(T, 1, dtype=torch.int32), np.zeros(T, dtype=np.int32)):
        with pytest.raises(ValueError, match='ids'):
            call(ids=bad)
    for bad in (0, hmm.dense_max_k() + 1, 2.0, True):
        with pytest.raises(ValueError, match='K = '):
            call(K=bad)
    with pytest.raises(ValueError, match='D = '):
        call(table=z(T, 128), shift=z(128))
    with pytest.raises(ValueError, match='outside'):
        call(off=[0, 4])
    with pytest.raises(ValueError, match='overlap'):
        call(off=[0, 2])
    with pytest.raises(ValueError, match='offsets'):
        call(lens=[3])

    h = hmm.TransitionHmmPosteriorgram(fitted_mixture(), stay=0.75)
    assert h.viterbi_log_probs == [] and h.last_n_changed_ is None
    before = (h.trans_.copy(), h.init_.copy(), h.gmm)
    for bad in ('', 'mm', 'w', 'mvs', None, 3):
        with pytest.raises(ValueError, match='params'):
            h.fit_viterbi(torch.zeros(5, 2), params=bad)
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match='min_duration'):
            h.fit_viterbi(torch.zeros(5, 2), min_duration=bad)
    for bad in (-1, 257, 0.5):
        with pytest.raises(ValueError, match='n_ranges'):
            h.fit_viterbi(torch.zeros(5, 2), n_ranges=bad)
    with pytest.raises(ValueError, match='D = 4'):
        h.fit_viterbi(torch.zeros(5, 4))
    assert np.array_equal(h.trans_, before[0]) and np.array_equal(h.init_, before[1]) and h.gmm is before[2]
    assert h.viterbi_log_probs == []
    # files: the new key travels, a file without it loads as before
    h.viterbi_log_probs = [-3.5, -3.25]
    path = str(tmp_path / 'm.npz')
    h.save(path)
    assert hmm.TransitionHmmPosteriorgram.load(path).viterbi_log_probs == [-3.5, -3.25]
    with np.load(path) as f:
        old = {k: f[k] for k in f.files if k != 'viterbi_log_probs'}
    np.savez(str(tmp_path / 'old.npz'), **old)
    g = hmm.TransitionHmmPosteriorgram.load(str(tmp_path / 'old.npz'))
    assert g.viterbi_log_probs == [] and np.array_equal(g.trans_, h.trans_)
    # the command line
    with pytest.raises(SystemExit):
        hmm.main(['fit-trans', 'a', 'b', 'c', '--viterbi', '--min-duration', 'x'])
    text = open(os.path.join(ROOT, 'abnet3_amd', 'hmm.py')).read()
    assert 'abnv_hmm_hard_stats' in text and 'Left out: hard-EM' not in text and '--viterbi' in text
    example = open(os.path.join(ROOT, 'examples', 'zero_resource.py')).read()
    assert '--hmm-trans-viterbi' in example


# ---- the library -----------------------------------------------------------------------------------------------------------
def declared(prefix='abnv_'):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, text))


def test_next5_symbols_are_the_headers_fifth_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib
    assert declared() == set(_lib.NEXT5_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS) | set(_lib.NEXT4_SYMBOLS)
    assert not set(_lib.NEXT5_SYMBOLS) & others
    assert declared('abnx_') == set(_lib.NEXT_SYMBOLS) and declared('abny_') == set(_lib.NEXT2_SYMBOLS)      # the older sections stay
    assert declared('abnz_') == set(_lib.NEXT3_SYMBOLS) and declared('abnw_') == set(_lib.NEXT4_SYMBOLS)
    assert len(_lib.NEXT_SYMBOLS) == 3 and len(_lib.NEXT2_SYMBOLS) == 3 and len(_lib.NEXT3_SYMBOLS) == 2 and len(_lib.NEXT4_SYMBOLS) == 2
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abnv_')}
    assert exported == declared()
    for name, (res, args) in _lib.NEXT5_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert len(_lib.NEXT5_SYMBOLS['abnv_hmm_hard_stats'][1]) == 17 and len(_lib.NEXT5_SYMBOLS['abnv_hmm_hard_stats_ws_bytes'][1]) == 5
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20                     # not part of the numbered ABI
    head = open(HEADER).read()
    top = head[:head.index('#ifndef')]
    assert all(word in top for word in ('abnw_', 'NEXT4_SYMBOLS', 'abnv_', 'NEXT5_SYMBOLS'))


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 40
    #       x  T    D  off len n  sh ids K  S  nr counts sums ng ws bytes stream
    good = [p, 100, 4, p, p, 2, p, p, 8, 3, 0, p, p, p, p, big, None]
    call = lib.abnv_hmm_hard_stats
    name = b'abnv_hmm_hard_stats'

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 11, 12, 13):
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error() and name in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=(1 << 31) - 128) == _lib.E_ARG
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a8=0) == _lib.E_ARG
    max_k, max_d, smax = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d(), lib.abnx_viterbi_dur_max()
    assert with_(a8=max_k + 1) == _lib.E_UNSUPPORTED and b'abny_hmm_dense_max_k' in lib.abn_last_error()
    assert with_(a2=max_d + 1) == _lib.E_UNSUPPORTED and b'abn_gmm_max_d' in lib.abn_last_error()
    for S in (0, smax + 1, -1, 1 << 20):
        assert with_(a9=S) == _lib.E_ARG, S
        assert b'min_duration' in lib.abn_last_error() and b'abnx_viterbi_dur_max' in lib.abn_last_error()
    for nr in (-1, 257, 1 << 20):
        assert with_(a10=nr) == _lib.E_ARG and b'n_ranges' in lib.abn_last_error()
    need = lib.abnv_hmm_hard_stats_ws_bytes(100, 2, 8, 4, 0)
    assert need > 0
    assert with_(a14=None) == _lib.E_WORKSPACE and with_(a15=need - 1) == _lib.E_WORKSPACE
    assert b'abnv_hmm_hard_stats_ws_bytes' in lib.abn_last_error()
    assert with_(a14=ctypes.c_void_p(0x10004)) == _lib.E_ARG and b'aligned' in lib.abn_last_error()
    # the order: T, sizes and limits before the pointers, the pointers before min_duration and n_ranges, those before the workspace
    assert with_(a1=0, a8=max_k + 1) == _lib.E_ARG and b'T = 0' in lib.abn_last_error()
    assert with_(a8=max_k + 1, a0=None) == _lib.E_UNSUPPORTED and with_(a8=max_k + 1, a9=0) == _lib.E_UNSUPPORTED
    assert with_(a0=None, a9=0) == _lib.E_ARG and b'null pointer' in lib.abn_last_error()
    assert with_(a9=0, a14=None) == _lib.E_ARG and b'min_duration' in lib.abn_last_error()
    assert with_(a10=300, a14=None) == _lib.E_ARG and b'n_ranges' in lib.abn_last_error()
    assert with_(a14=ctypes.c_void_p(0x10004), a15=16) == _lib.E_WORKSPACE


def test_the_sizing_entry(lib):
    ws = lib.abnv_hmm_hard_stats_ws_bytes
    max_k, max_d = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d()
    up = lambda v: (v + 15) // 16 * 16
    # the header's geometry: the good ids [T] int32, then per range [K][2 D] fp32 and [K] int32; one range per 128-row block at most
    for T, K, D, nr, ranges in ((1, 1, 1, 0, 1), (128, 3, 2, 0, 1), (129, 3, 2, 0, 2), (1000, 8, 40, 0, 8), (1000, 8, 40, 3, 3),
                                (1 << 20, 128, 127, 0, 256), (1 << 20, 128, 127, 256, 256), (1 << 20, 64, 40, 7, 7)):
        assert ws(T, 2, K, D, nr) == up(up(up(4 * T) + ranges * K * 2 * D * 4) + ranges * K * 4), (T, K, D, nr)
        assert ws(T, 2, K, D, nr) == ws(T, 999, K, D, nr)
    for bad in ((0, 2, 8, 4, 0), ((1 << 31) - 128, 2, 8, 4, 0), (100, 0, 8, 4, 0), (100, 2, 0, 4, 0), (100, 2, max_k + 1, 4, 0),
                (100, 2, 8, 0, 0), (100, 2, 8, max_d + 1, 0), (100, 2, 8, 4, -1), (100, 2, 8, 4, 257)):
        assert ws(*bad) == -1 and b'abnv_hmm_hard_stats_ws_bytes' in lib.abn_last_error(), bad
