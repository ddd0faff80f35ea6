"""The minimum unit duration of the full-transition HMM's max-product path on the host: the numpy restatement
(tests/hmm_dense_dur_np.py) against enumeration of all segmentations, its S = 1, its run lengths, the Python layer's checks,
the abnw_ ledger of include/abnet3_hip_next.h, and the refusals that need no launch.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_dense_dur_np as dd  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abnw_hmm_dense_viterbi_dur_ws_bytes', 'abnw_hmm_dense_viterbi_dur'}


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def bad_patterns(L):
    """BAD frames anywhere: none, first, last, a middle one, two neighbours, all but one, all."""
    pats = [np.zeros(L, dtype=bool)]
    for rows in ([0], [L - 1], [L // 2], [L // 2, min(L - 1, L // 2 + 1)], list(range(1, L)), list(range(L))):
        b = np.zeros(L, dtype=bool)
        b[rows] = True
        pats.append(b)
    return pats


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_restatement_equals_the_brute_force_over_all_segmentations_on_exact_inputs():
    rng = np.random.default_rng(21)
    n, tied, switched = 0, 0, 0
    for K in (1, 2, 3):
        for L in (1, 2, 3, 4, 5, 6, 7, 8):
            for S in (2, 3, 4):
                pats = bad_patterns(L)
                for bad in (pats[0], pats[1 + (K + L + S) % 6]):
                    if (~bad).sum() > 7:
                        continue
                    # a coarse grid (halves, few values) so that many paths tie
                    s = rng.integers(-2, 3, size=(L, K)) / 2.0
                    li = -rng.integers(0, 3, size=K) / 2.0
                    lt = -rng.integers(0, 3, size=(K, K)) / 2.0
                    best, paths = dd.brute_force(s, ~bad, li, lt, S)
                    ids, lp, nsw, ng = dd.viterbi_one(s, ~bad, li, lt, S)
                    assert lp == best, (K, L, S, bad, lp, best)
                    assert tuple(ids[~bad]) in paths, (K, L, S, bad, ids, paths)
                    assert (ids[bad] == -1).all() and ng == int((~bad).sum()) and ids.dtype == np.int32
                    assert dd.run_lengths_ok(ids, S) and nsw == max(len(dd.runs(ids)) - 1, 0) == dv.switches(ids)
                    assert dd.optimum_f64(s, ~bad, li, lt, S) == best
                    assert dd.J_runs(s, ids, ~bad, li, lt, S) == best
                    tied += len(paths) > 1
                    switched += nsw > 0
                    n += 1
    assert n >= 120 and tied >= n // 10 and switched >= n // 10               # ties and switches were really exercised


def test_minimum_duration_one_is_the_restatement_without_it():
    rng = np.random.default_rng(22)
    for K, L in ((1, 9), (5, 40), (17, 64)):
        s = rng.integers(-160, 33, size=(L, K)) / 8.0
        li, lt = -rng.integers(0, 41, size=K) / 8.0, -rng.integers(0, 25, size=(K, K)) / 8.0
        good = rng.random(L) > 0.15
        a, b = dd.viterbi_one(s, good, li, lt, 1), dv.viterbi_one(s, good, li, lt)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        assert dd.optimum_f64(s, good, li, lt, 1) == dv.optimum_f64(s, good, li, lt)


def test_runs_are_long_enough_and_switches_are_runs_minus_one():
    rng = np.random.default_rng(23)
    shorter = 0
    for K, L, S in ((2, 50, 2), (5, 120, 3), (9, 90, 5), (17, 70, 8), (3, 5, 8)):
        s = (rng.normal(size=(L, K)) * 3.0).astype(np.float32)
        init, trans = rng.dirichlet(np.full(K, 2.0)), rng.dirichlet(np.full(K, 2.0), size=K)
        li, lt = dv.log_transitions(init, trans)
        good = rng.random(L) > 0.1
        ids, lp, nsw, ng = dd.viterbi_one(s, good, li, lt, S)
        assert dd.run_lengths_ok(ids, S) and nsw == len(dd.runs(ids)) - 1 == dv.switches(ids) and ng == good.sum()
        assert (ids[~good] == -1).all() and (ids[good] >= 0).all()
        free = dv.viterbi_one(s, good, li, lt)
        shorter += not dd.run_lengths_ok(free[0], S)
        # (the two optima are not ordered: a forced advance pays no lt[k][k], so the constrained score may be the larger)
        opt = dd.optimum_f64(s, good, li, lt, S)
        allow = 2.0 * ng * dd.delta(0.0, np.abs(s).max(), dd.table_max(li, lt), S)
        assert opt - allow <= dd.J_runs(s, ids, good, li, lt, S) <= opt + 1e-9 * (abs(opt) + 1.0) and abs(lp - opt) <= allow
    assert shorter >= 3                                                         # (without it the same data does flicker)
    off, lens = np.array([2, 9]), np.array([5, 3])
    s = rng.integers(-48, 1, size=(14, 3)) / 8.0
    li, lt = -rng.integers(0, 41, size=3) / 8.0, -rng.integers(0, 25, size=(3, 3)) / 8.0
    good = np.ones(14, dtype=bool)
    ids, lp, nsw, ng = dd.viterbi(s, good, off, lens, li, lt, 2)
    assert (ids[[0, 1, 7, 8, 12, 13]] == -7).all() and ng.tolist() == [5, 3] and lp.dtype == np.float64
    assert np.array_equal(ids[2:7], dd.viterbi_one(s[2:7], good[2:7], li, lt, 2)[0])


def test_delta_is_the_docstrings_formula():
    E, smax, lmax = 1e-5, 50.0, 7.0
    for S in (2, 5, 8):
        assert dd.delta(E, smax, lmax, S) == pytest.approx(E + 2.0 ** -24 * ((24 * S + 1) * smax + (24 * S + 3) * lmax), rel=1e-12)


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_a_bad_minimum_duration_on_the_host(lib):
    from abnet3_amd import hmm
    from test_hmm_host import fitted_mixture
    K, D = 3, 2
    z = lambda *s: torch.zeros(*s)
    li, lt = (torch.from_numpy(a) for a in hmm.log_transitions(np.full(K, 1.0 / K), np.full((K, K), 1.0 / K)))
    h = hmm.TransitionHmmPosteriorgram(fitted_mixture(), stay=0.75)
    for bad in (0, 9, 2.5, True, '2'):
        with pytest.raises(ValueError, match='min_duration'):
            hmm.dense_viterbi(z(6, D), [0, 3], [3, 3], z(D), z(K, D), z(K, D), z(K), li, lt, min_duration=bad)
        for call in (h.decode, h.quantize):
            with pytest.raises(ValueError, match='min_duration'):
                call(torch.zeros(5, 2), min_duration=bad)
    assert h.last_log_prob_ is None and h.last_n_switch_ is None and h.last_n_good_ is None
    # the other host checks still come with a good one
    with pytest.raises(ValueError, match='float32'):
        hmm.dense_viterbi(z(6, D).double(), [0, 3], [3, 3], z(D), z(K, D), z(K, D), z(K), li, lt, min_duration=3)
    with pytest.raises(ValueError, match='D = 4'):
        h.decode(torch.zeros(5, 4), min_duration=3)
    text = open(os.path.join(ROOT, 'abnet3_amd', 'hmm.py')).read()
    assert 'abnw_hmm_dense_viterbi_dur' in text and 'Left out: a minimum duration for this model' not in text
    example = open(os.path.join(ROOT, 'examples', 'zero_resource.py')).read()
    assert 'full-transition HMM Viterbi units, at least %d frames per unit' in example


# ---- the library -----------------------------------------------------------------------------------------------------------
def declared(prefix='abnw_'):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, text))


def test_next4_symbols_are_the_headers_fourth_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib
    assert declared() == set(_lib.NEXT4_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS)
    assert not set(_lib.NEXT4_SYMBOLS) & others
    assert declared('abnx_') == set(_lib.NEXT_SYMBOLS) and declared('abny_') == set(_lib.NEXT2_SYMBOLS)      # the older sections stay
    assert declared('abnz_') == set(_lib.NEXT3_SYMBOLS)
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abnw_')}
    assert exported == declared()
    for name, (res, args) in _lib.NEXT4_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # the twin's arguments and min_duration
    assert list(_lib.NEXT4_SYMBOLS['abnw_hmm_dense_viterbi_dur'][1]) == list(_lib.NEXT3_SYMBOLS['abnz_hmm_dense_viterbi'][1]) + [ctypes.c_int32]
    assert _lib.NEXT4_SYMBOLS['abnw_hmm_dense_viterbi_dur_ws_bytes'] == _lib.NEXT3_SYMBOLS['abnz_hmm_dense_viterbi_ws_bytes']
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20                     # not part of the numbered ABI
    head = open(HEADER).read()
    assert 'abnw_' in head[:head.index('#ifndef')] and 'NEXT4_SYMBOLS' in head[:head.index('#ifndef')]


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    #       x  T    D  off len n  sh A  B  c0 li lt K  ids lp nsw ng ws bytes stream S
    good = [p, 100, 4, p, p, 2, p, p, p, p, p, p, 8, p, p, p, p, p, big, None, 3]
    call = lib.abnw_hmm_dense_viterbi_dur
    name = b'abnw_hmm_dense_viterbi_dur'
    smax = lib.abnx_viterbi_dur_max()
    assert smax == 8

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for S in (1, 2, 3, 5, 8):                                                    # the twin's list at every kernel set
        for i in (0, 3, 4, 6, 7, 8, 9, 10, 11, 13):
            assert with_(**{'a%d' % i: None, 'a20': S}) == _lib.E_ARG, i
            assert b'null pointer' in lib.abn_last_error() and name in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a12=0) == _lib.E_ARG
    max_k, max_d = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d()
    assert with_(a12=max_k + 1) == _lib.E_UNSUPPORTED and b'abny_hmm_dense_max_k' in lib.abn_last_error()
    assert with_(a2=max_d + 1) == _lib.E_UNSUPPORTED and b'abn_gmm_max_d' in lib.abn_last_error()
    for S in (0, smax + 1, -1, 1 << 20):
        assert with_(a20=S) == _lib.E_ARG, S
        assert b'min_duration' in lib.abn_last_error() and b'abnx_viterbi_dur_max' in lib.abn_last_error()
    for S in (1, 2, smax):
        assert with_(a17=None, a20=S) == _lib.E_WORKSPACE and with_(a18=1024, a20=S) == _lib.E_WORKSPACE
        assert b'abnw_hmm_dense_viterbi_dur_ws_bytes' in lib.abn_last_error()
        assert with_(a18=lib.abnw_hmm_dense_viterbi_dur_ws_bytes(2, 1, 8, 4) - 256 * 2, a20=S) == _lib.E_WORKSPACE    # (one frame short in both regions)
        assert with_(a17=ctypes.c_void_p(0x10004), a20=S) == _lib.E_ARG and b'aligned' in lib.abn_last_error()
    # the order: T before the sizes, the sizes and limits before the pointers, the pointers before min_duration, that before the workspace
    assert with_(a1=0, a12=max_k + 1) == _lib.E_ARG and b'T = 0' in lib.abn_last_error()
    assert with_(a12=max_k + 1, a0=None) == _lib.E_UNSUPPORTED
    assert with_(a12=max_k + 1, a20=0) == _lib.E_UNSUPPORTED
    assert with_(a0=None, a20=0) == _lib.E_ARG and b'null pointer' in lib.abn_last_error()
    assert with_(a0=None, a17=None) == _lib.E_ARG and b'null pointer' in lib.abn_last_error()
    assert with_(a20=0, a17=None) == _lib.E_ARG and b'min_duration' in lib.abn_last_error()
    assert with_(a17=ctypes.c_void_p(0x10004), a18=1024) == _lib.E_WORKSPACE


def test_the_sizing_entry(lib):
    ws = lib.abnw_hmm_dense_viterbi_dur_ws_bytes
    max_k, max_d = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d()
    assert ws(2, 100, 8, 4) > 0 and ws(2, 100, 8, 4) % 256 == 0 and ws(2, 101, 128, 4) >= ws(2, 100, 128, 4)
    assert ws(300, 10, 8, 4) == ws(256, 10, 8, 4) == 256 * ws(1, 10, 8, 4)          # min(n_utt, 256) workgroups
    # the header's geometry: the slab of scores [128][128] fp32, one byte per frame and state of the capacity K rounds up to,
    # and one byte per frame
    up = lambda v: (v + 255) // 256 * 256
    for K, kc in ((1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 128), (128, 128)):
        for n in (0, 1, 64, 1000):
            assert ws(1, n, K, 4) == up(128 * 128 * 4 + n * (kc + 1)), (K, n)
            assert ws(3, n, K, 4) == 3 * ws(1, n, K, 4)
            assert ws(1, n, K, 4) >= lib.abnz_hmm_dense_viterbi_ws_bytes(1, n, K, 4)
    for bad in ((0, 10, 8, 4), (2, -1, 8, 4), (2, lib.abn_hmm_max_len() + 1, 8, 4), (2, 10, 0, 4), (2, 10, max_k + 1, 4),
                (2, 10, 8, 0), (2, 10, 8, max_d + 1)):
        assert ws(*bad) == -1 and b'abnw_hmm_dense_viterbi_dur_ws_bytes' in lib.abn_last_error(), bad
