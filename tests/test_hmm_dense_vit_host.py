"""The max-product path of the full-transition HMM on the host: the numpy restatement (tests/hmm_dense_vit_np.py) against
enumeration of all paths, against the sticky restatement and against the frame-wise argmax, hmm.log_transitions, the Python
layer's checks, the abnz_ ledger of include/abnet3_hip_next.h, and the refusals that need no launch.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_vit_np  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abnz_hmm_dense_viterbi_ws_bytes', 'abnz_hmm_dense_viterbi'}


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def eighths(rng, lo, hi, size):
    """Multiples of 1/8 in [lo, hi]: sums of a few of them are exact in float32 and float64."""
    return rng.integers(int(8 * lo), int(8 * hi) + 1, size=size) / 8.0


def bad_patterns(L):
    """BAD frames anywhere: none, first, last, a middle one, two neighbours, all but one, all."""
    pats = [np.zeros(L, dtype=bool)]
    for rows in ([0], [L - 1], [L // 2], [L // 2, min(L - 1, L // 2 + 1)], list(range(1, L)), list(range(L))):
        b = np.zeros(L, dtype=bool)
        b[rows] = True
        pats.append(b)
    return pats


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_restatement_equals_the_brute_force_score_and_its_tie_rule_on_exact_inputs():
    rng = np.random.default_rng(11)
    n, with_ties = 0, 0
    for K in (1, 2, 3):
        for L in (1, 2, 3, 4, 5, 6):
            for bad in bad_patterns(L):
                # a coarse grid (halves, few values) so that many paths tie
                s = rng.integers(-2, 3, size=(L, K)) / 2.0
                li = -rng.integers(0, 3, size=K) / 2.0
                lt = -rng.integers(0, 3, size=(K, K)) / 2.0
                best, path = dv.brute_force(s, ~bad, li, lt)
                for dtype in (np.float32, np.float64):
                    ids, lp, nsw, ng, nt = dv.viterbi_one(s, ~bad, li, lt, dtype, count_ties=True)
                    assert lp == best, (K, L, bad, lp, best)
                    assert tuple(ids[~bad]) == tuple(path), (K, L, bad, ids, path)
                    assert (ids[bad] == -1).all() and ng == int((~bad).sum()) and nsw == dv.switches(ids)
                    assert ids.dtype == np.int32
                with_ties += nt > 0
                n += 1
    # the tie rule was exercised, not only the score (K = 1 and the cases with at most one good frame cannot tie on a path)
    assert n == 3 * 6 * 7 and with_ties >= n // 10


def test_float32_and_float64_restatements_agree_on_exact_inputs():
    rng = np.random.default_rng(12)
    for K, L in ((5, 40), (17, 64), (33, 20)):
        s = eighths(rng, -20, 4, (L, K))
        li, lt = eighths(rng, -5, 0, K), eighths(rng, -3, 0, (K, K))
        good = rng.random(L) > 0.15
        a = dv.viterbi_one(s, good, li, lt, np.float32, count_ties=True)
        b = dv.viterbi_one(s, good, li, lt, np.float64, count_ties=True)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        assert a[1] == dv.optimum_f64(s, good, li, lt) == dv.J(s, a[0], good, li, lt)
    off, lens = np.array([2, 9]), np.array([5, 3])
    s = eighths(rng, -6, 0, (14, 3))
    li, lt = eighths(rng, -5, 0, 3), eighths(rng, -3, 0, (3, 3))
    good = np.ones(14, dtype=bool)
    ids, lp, nsw, ng = dv.viterbi(s, good, off, lens, li, lt)
    assert (ids[[0, 1, 7, 8, 12, 13]] == -7).all() and ng.tolist() == [5, 3] and lp.dtype == np.float64
    assert np.array_equal(ids[2:7], dv.viterbi_one(s[2:7], good[2:7], li, lt)[0])
    assert dv.ties(s, good, off, lens, li, lt) >= 0


def test_sticky_matrix_gives_the_sticky_restatements_log_prob_bit_for_bit():
    rng = np.random.default_rng(13)
    for K, L, stay in ((2, 30, 0.5), (5, 80, 0.9), (9, 50, 0.0), (17, 40, 0.99)):
        w = rng.dirichlet(np.full(K, 3.0))
        s = (rng.normal(size=(L, K)) * 3.0).astype(np.float32)
        good = rng.random(L) > 0.1
        lw, ls, lr = hmm_vit_np.tables(w, stay)
        lt = dv.sticky_log_transitions(ls, lr)
        assert lt.dtype == np.float32 and np.array_equal(np.diag(lt), ls) and np.array_equal(lt[0, 1:], lr[1:])
        ref = hmm_vit_np.viterbi_one(s, good, lw, ls, lr)
        got = dv.viterbi_one(s, good, lw, lt, count_ties=True)
        assert np.float64(got[1]).tobytes() == np.float64(ref[1]).tobytes() and got[3] == ref[3]
        if got[4] == 0:                                           # without a tie the paths are the same path
            assert np.array_equal(got[0], ref[0]) and got[2] == ref[2]


def test_equal_rows_give_the_frame_wise_argmax():
    rng = np.random.default_rng(14)
    K, L = 7, 60
    s = (rng.normal(size=(L, K)) * 2.0).astype(np.float32)
    q = rng.dirichlet(np.full(K, 2.0)).astype(np.float32)
    lq, lt = dv.log_transitions(q, np.repeat(q[None, :], K, axis=0))
    good = rng.random(L) > 0.1
    ids, lp, _, ng = dv.viterbi_one(s, good, lq, lt)
    want = np.argmax((s + lq[None, :]).astype(np.float32), axis=1)
    assert np.array_equal(ids[good], want[good]) and (ids[~good] == -1).all() and ng == good.sum()
    assert lp == float(np.sum((s + lq[None, :]).astype(np.float32).max(axis=1)[good].astype(np.float64)))


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_log_transitions_round_once_from_float64_and_refuse_below_the_floor(lib):
    from abnet3_amd import hmm
    rng = np.random.default_rng(15)
    K = 6
    init = rng.dirichlet(np.ones(K))
    trans = rng.dirichlet(np.ones(K), size=K)
    li, lt = hmm.log_transitions(init, trans)
    assert li.dtype == np.float32 and lt.dtype == np.float32 and li.shape == (K,) and lt.shape == (K, K)
    i32, t32 = init.astype(np.float32), trans.astype(np.float32)
    assert np.array_equal(li, np.log(i32.astype(np.float64)).astype(np.float32))
    assert np.array_equal(lt, np.log(t32.astype(np.float64)).astype(np.float32))
    ri, rt = dv.log_transitions(init, trans)
    assert np.array_equal(li, ri) and np.array_equal(lt, rt)
    assert not np.array_equal(lt, np.log(t32))                                   # (a float32 logarithm is another number)
    li2, lt2 = hmm.log_transitions(torch.from_numpy(i32), torch.from_numpy(t32))   # tensors too
    assert np.array_equal(li2, li) and np.array_equal(lt2, lt)
    floor = np.full((3, 3), 1.0 / 3)
    floor[0] = [1.0 - 2.0 ** -99, 2.0 ** -100, 2.0 ** -100]
    a, b = hmm.log_transitions(np.full(3, 1.0 / 3), floor)                       # the floor itself is fine, and finite
    assert np.isfinite(a).all() and np.isfinite(b).all() and b[0, 1] == np.float32(-100.0 * np.log(2.0))
    low = floor.copy()
    low[0] = [1.0 - 2.0 ** -100, 2.0 ** -101, 2.0 ** -101]
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.log_transitions(np.full(3, 1.0 / 3), low)
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.log_transitions([1.0, 0.0, 0.0], floor)
    with pytest.raises(ValueError, match='sum to 1'):
        hmm.log_transitions(np.full(3, 1.0 / 3), np.full((3, 3), 0.5))
    with pytest.raises(ValueError):
        hmm.log_transitions(np.full(3, 1.0 / 3), np.full((2, 2), 0.5))


def test_dense_viterbi_refuses_on_the_host(lib):
    from abnet3_amd import hmm
    K, D = 3, 2
    z = lambda *s: torch.zeros(*s)
    li, lt = (torch.from_numpy(a) for a in hmm.log_transitions(np.full(K, 1.0 / K), np.full((K, K), 1.0 / K)))
    args = lambda **kw: dict(dict(table=z(6, D), off=[0, 3], lens=[3, 3], shift=z(D), A=z(K, D), B=z(K, D), c0=z(K), li=li, lt=lt), **kw)

    def at(t, value, *idx):
        t = t.clone()
        t[idx] = value
        return t
    cases = (
        (dict(table=z(6, D).double()), 'float32'), (dict(table=z(6)), 'float32 table'), (dict(A=z(K, D + 1)), 'A \\[K, D\\]'),
        (dict(shift=z(D).double()), 'float32'), (dict(li=li.double()), 'li \\[K\\]'), (dict(lt=lt[:2]), 'li \\[K\\]'),
        (dict(li=li.numpy()), 'li \\[K\\]'), (dict(lt=z(K)), 'li \\[K\\]'),
        (dict(li=at(li, float('nan'), 0)), 'NaN'), (dict(li=at(li, float('inf'), 1)), 'NaN'), (dict(li=at(li, float('-inf'), 2)), '-inf'),
        (dict(lt=at(lt, float('nan'), 0, 1)), 'NaN'), (dict(lt=at(lt, float('inf'), 2, 2)), 'NaN'), (dict(lt=at(lt, float('-inf'), 1, 0)), '-inf'),
        (dict(lens=[3]), 'offsets'), (dict(lens=[3, 4]), 'outside'), (dict(off=[-1, 3]), 'outside'), (dict(off=[0, 2]), 'overlap'),
        (dict(ids=torch.zeros(6, dtype=torch.int64)), 'ids'), (dict(ids=torch.zeros(5, dtype=torch.int32)), 'ids'),
        (dict(table=z(hmm.max_len() + 1, D), off=[0], lens=[hmm.max_len() + 1]), 'abn_hmm_max_len'),
    )
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            hmm.dense_viterbi(**args(**kw))
    Kbig = hmm.dense_max_k() + 1
    with pytest.raises(ValueError, match='abny_hmm_dense_max_k'):
        hmm.dense_viterbi(z(6, D), [0], [6], z(D), z(Kbig, D), z(Kbig, D), z(Kbig), z(Kbig), z(Kbig, Kbig))


def test_class_refuses_on_the_host_and_the_command_line_knows_the_route(lib, tmp_path):
    from abnet3_amd import hmm
    from test_hmm_host import fitted_mixture
    h = hmm.TransitionHmmPosteriorgram(fitted_mixture(), stay=0.75)
    assert h.last_log_prob_ is None and h.last_n_switch_ is None and h.last_n_good_ is None
    for call in (h.decode, h.quantize):
        with pytest.raises(ValueError, match='D = 4'):
            call(torch.zeros(5, 4))
        with pytest.raises(ValueError, match='float32'):
            call(torch.zeros(5, 2, dtype=torch.float64))
    # a file that holds `trans` is decoded by this model, and a minimum duration with it is an error that says why
    mpath, fpath = str(tmp_path / 'dense.npz'), str(tmp_path / 'feats.npz')
    h.save(mpath)
    np.savez(fpath, a=np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(ValueError, match='no minimum duration'):
        hmm.main(['decode', mpath, fpath, str(tmp_path / 'out.npz'), '--min-duration', '2'])
    assert not os.path.exists(str(tmp_path / 'out.npz'))
    text = open(os.path.join(ROOT, 'abnet3_amd', 'hmm.py')).read()
    assert 'not built yet' not in text and 'h.decode(feats)' in text and 'the max-product path of this model' not in text
    example = open(os.path.join(ROOT, 'examples', 'zero_resource.py')).read()
    assert 'TransitionHmmPosteriorgram.decode' in example and 'dense=None' in example and "'--hmm-decode'" in example
    for doc in ('README.md', 'INTEGRATION.md', os.path.join('include', 'abnet3_hip_next.h')):
        assert 'the max-product path of this model' not in open(os.path.join(ROOT, doc)).read(), doc


# ---- the library -----------------------------------------------------------------------------------------------------------
def declared(prefix='abnz_'):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, text))


def test_next3_symbols_are_the_headers_third_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib
    assert declared() == set(_lib.NEXT3_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS)
    assert not set(_lib.NEXT3_SYMBOLS) & others
    assert declared('abnx_') == set(_lib.NEXT_SYMBOLS) and declared('abny_') == set(_lib.NEXT2_SYMBOLS)      # the older sections stay
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abnz_')}
    assert exported == declared()
    for name, (res, args) in _lib.NEXT3_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # abn_hmm_viterbi's arguments with two tables in place of three
    assert len(_lib.NEXT3_SYMBOLS['abnz_hmm_dense_viterbi'][1]) == len(_lib.SYMBOLS['abn_hmm_viterbi'][1]) - 1
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20                     # not part of the numbered ABI
    head = open(HEADER).read()
    assert 'abnz_' in head[:head.index('#ifndef')] and 'NEXT3_SYMBOLS' in head[:head.index('#ifndef')]


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    #       x  T    D  off len n  sh A  B  c0 li lt K  ids lp nsw ng ws bytes stream
    good = [p, 100, 4, p, p, 2, p, p, p, p, p, p, 8, p, p, p, p, p, big, None]
    call = lib.abnz_hmm_dense_viterbi
    name = b'abnz_hmm_dense_viterbi'

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 8, 9, 10, 11, 13):
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error() and name in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a12=0) == _lib.E_ARG
    max_k, max_d = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d()
    assert with_(a12=max_k + 1) == _lib.E_UNSUPPORTED and b'abny_hmm_dense_max_k' in lib.abn_last_error()
    assert with_(a2=max_d + 1) == _lib.E_UNSUPPORTED and b'abn_gmm_max_d' in lib.abn_last_error()
    assert with_(a17=None) == _lib.E_WORKSPACE and with_(a18=1024) == _lib.E_WORKSPACE
    assert b'abnz_hmm_dense_viterbi_ws_bytes' in lib.abn_last_error()
    assert with_(a18=lib.abnz_hmm_dense_viterbi_ws_bytes(2, 1, 8, 4) - 256 * 2) == _lib.E_WORKSPACE    # (one frame short in both regions)
    assert with_(a17=ctypes.c_void_p(0x10004)) == _lib.E_ARG and b'aligned' in lib.abn_last_error()
    # the order: T before the sizes, the sizes and limits before the pointers, the pointers before the workspace
    assert with_(a1=0, a12=max_k + 1) == _lib.E_ARG and b'T = 0' in lib.abn_last_error()
    assert with_(a12=max_k + 1, a0=None) == _lib.E_UNSUPPORTED
    assert with_(a0=None, a17=None) == _lib.E_ARG and b'null pointer' in lib.abn_last_error()
    assert with_(a17=ctypes.c_void_p(0x10004), a18=1024) == _lib.E_WORKSPACE


def test_the_sizing_entry(lib):
    ws = lib.abnz_hmm_dense_viterbi_ws_bytes
    max_k, max_d = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d()
    assert ws(2, 100, 8, 4) > 0 and ws(2, 100, 8, 4) % 256 == 0 and ws(2, 101, 128, 4) >= ws(2, 100, 128, 4)
    assert ws(300, 10, 8, 4) == ws(256, 10, 8, 4) == 256 * ws(1, 10, 8, 4)          # min(n_utt, 256) workgroups
    # the slab of scores [128][128] fp32 and one backpointer byte per frame and state of the capacity K rounds up to
    up = lambda v: (v + 255) // 256 * 256
    for K, kc in ((1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)):
        for n in (0, 1, 64, 1000):
            assert ws(1, n, K, 4) == up(128 * 128 * 4 + n * kc), (K, n)
            assert ws(3, n, K, 4) == 3 * ws(1, n, K, 4)
    for bad in ((0, 10, 8, 4), (2, -1, 8, 4), (2, lib.abn_hmm_max_len() + 1, 8, 4), (2, 10, 0, 4), (2, 10, max_k + 1, 4),
                (2, 10, 8, 0), (2, 10, 8, max_d + 1)):
        assert ws(*bad) == -1 and b'abnz_hmm_dense_viterbi_ws_bytes' in lib.abn_last_error(), bad
