"""The minimum unit duration of the two max-product decoders on the host: the numpy restatement (tests/vit_dur_np.py)
against enumeration of all segmentations, its S = 1 case against the two existing restatements, the run-length property,
the wrappers' argument checks, the ledger of include/abnet3_hip_next.h, and the refusals that need no launch.  No kernel
runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_vit_np  # noqa: E402
import units_np  # noqa: E402
import vit_dur_np  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def dyadic_case(rng, K, L, kmeans):
    """Scores and tables in eighths (every fp32 operation exact, ties plentiful), a BAD frame in about one of six."""
    s = (rng.integers(-24, 25, size=(L, K)) / 8.0).astype(np.float32)
    good = rng.random(L) > 0.17
    if kmeans:
        tables = vit_dur_np.kmeans_tables(K, np.float32(rng.integers(0, 33) / 8.0))
    else:
        ls = (-rng.integers(0, 9, size=K) / 8.0).astype(np.float32)
        lr = (ls - rng.integers(0, 25, size=K) / 8.0).astype(np.float32)
        lw = (-rng.integers(0, 41, size=K) / 8.0).astype(np.float32)
        tables = (lw, ls, lr)
    return s, good, tables


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kmeans', [False, True])
def test_restatement_attains_the_brute_force_maximum(kmeans):
    rng = np.random.default_rng(23 + kmeans)
    n = 0
    for K in (1, 2, 3):
        for L in range(0, 9):
            for S in (1, 2, 3, 4):
                s, good, tables = dyadic_case(rng, K, L, kmeans)
                best, arg = vit_dur_np.brute_force(s, good, *tables, S)
                ids, lp, nsw, ng = vit_dur_np.viterbi_one(s, good, *tables, S)
                assert lp == best, (K, L, S, lp, best)
                assert tuple(ids[good]) in arg, (K, L, S, ids, sorted(arg)[:3])          # its path attains it
                assert vit_dur_np.optimum_f64(s, good, *tables, S) == best
                assert (ids[~good] == -1).all() and (ids[good] >= 0).all() and ng == int(good.sum())
                assert nsw == units_np.switches(ids)
                assert vit_dur_np.run_lengths_ok(ids, S), (K, L, S, ids)
                if (S * tables[1] >= tables[2]).all():                                  # then the runs are the best segmentation
                    assert vit_dur_np.J_runs(s, ids, good, *tables, S) == best
                n += 1
    assert n == 3 * 9 * 4


def test_one_frame_minimum_is_the_two_existing_restatements_exactly():
    rng = np.random.default_rng(5)
    for K, L in ((1, 7), (3, 40), (9, 130), (17, 64)):
        s = (rng.normal(size=(L, K)) * 3.0).astype(np.float32)
        good = rng.random(L) > 0.1
        for stay in (0.0, 0.5, 0.9):
            t32 = hmm_vit_np.tables(rng.dirichlet(np.ones(K)), stay)
            ref = hmm_vit_np.viterbi_one(s, good, *t32)
            got = vit_dur_np.viterbi_one(s, good, *t32, 1)
            assert np.array_equal(got[0], ref[0]) and got[1:] == ref[1:]
        for penalty in (0.0, 1.0, 7.5):
            p = units_np.score_penalty(penalty)
            ref = units_np.viterbi_one(s, good, p)
            got = vit_dur_np.viterbi_one(s, good, *vit_dur_np.kmeans_tables(K, p), 1)
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and got[2] == ref[2]


@pytest.mark.parametrize('kmeans', [False, True])
def test_runs_are_long_enough_and_the_objective_against_the_minimum(kmeans):
    rng = np.random.default_rng(7 + kmeans)
    for K, L in ((2, 30), (5, 70), (8, 25)):
        s = (rng.normal(size=(L, K)) * 2.0).astype(np.float32)
        good = rng.random(L) > 0.12
        tables = vit_dur_np.kmeans_tables(K, 0.75) if kmeans else hmm_vit_np.tables(rng.dirichlet(np.ones(K)), 0.8)
        before = None
        for S in range(1, 9):
            ids, lp, nsw, ng = vit_dur_np.viterbi_one(s, good, *tables, S)
            assert vit_dur_np.run_lengths_ok(ids, S), (K, L, S, ids)
            assert nsw == units_np.switches(ids) and ng == int(good.sum())
            # A segmentation that S allows is allowed by S - 1 too, where each of its segments longer than S - 1 pays one
            # stay more: opt(S - 1) >= opt(S) + sum of those segments' ls.  With ls = 0 (the k-means tables) the objective
            # therefore does not rise with S; with the HMM's ls < 0 it may rise, by at most max|ls| per segment, of which
            # there are at most n_good // S + 1.  (Up to the fp32 roundings of two runs of the recurrence.)
            slack = 2.0 * ng * vit_dur_np.delta(0.0, np.abs(s).max(), hmm_vit_np.table_max(*tables), S)
            rise = (ng // S + 1) * float(np.abs(tables[1]).max())
            assert kmeans == (rise == 0.0)
            assert before is None or lp <= before + rise + slack, (K, L, S, lp, before)
            opt = vit_dur_np.optimum_f64(s, good, *tables, S)
            assert abs(lp - opt) <= slack
            before = lp


def test_forced_frames_skip_bad_frames_and_the_end_may_cut_the_last_unit_short():
    # two units, S = 3: unit 1 is better only at frames 4 and 5; too short to enter and leave, unless it is the end
    s = np.zeros((8, 2), dtype=np.float32)
    s[:, 1] = -1.0
    s[4:6, 1] = 4.0
    z = np.zeros(2, dtype=np.float32)
    lr = np.full(2, -1.0, dtype=np.float32)
    good = np.ones(8, dtype=bool)
    ids, lp, nsw, _ = vit_dur_np.viterbi_one(s, good, z, z, lr, 3)
    assert ids.tolist() == [0, 0, 0, 1, 1, 1, 0, 0] or ids.tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    assert lp == 8.0 - 1.0 - 2.0 and nsw == 2                                    # a third frame of unit 1 and two entries
    ids, lp, nsw, _ = vit_dur_np.viterbi_one(s[:6], good[:6], z, z, lr, 3)       # the end cuts unit 1 short
    assert ids.tolist() == [0, 0, 0, 0, 1, 1] and lp == 7.0 and nsw == 1
    good[4] = False                                                              # durations count good frames
    ids, lp, nsw, ng = vit_dur_np.viterbi_one(s, good, z, z, lr, 3)
    assert ids[4] == -1 and ng == 7 and vit_dur_np.run_lengths_ok(ids, 3)
    assert vit_dur_np.brute_force(s, good, z, z, lr, 3)[0] == lp


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_wrappers_check_the_minimum_duration_on_the_host(lib):
    from abnet3_amd import _utt, hmm, kmeans
    from test_hmm_host import fitted_mixture
    assert _utt.viterbi_dur_max() == 8
    assert [_utt.check_min_duration('t', v) for v in (1, 8, np.int64(3))] == [1, 8, 3]
    for bad in (0, 9, -1, 2.0, '3', None, True):
        with pytest.raises(ValueError, match='min_duration'):
            _utt.check_min_duration('t', bad)
    K, D = 3, 2
    z = lambda *s: torch.zeros(*s)
    lw, ls, lr = (torch.from_numpy(a) for a in hmm.viterbi_tables(np.full(K, 1.0 / K), 0.5))
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match='min_duration'):
            hmm.viterbi(z(6, D), [0], [6], z(D), z(K, D), z(K, D), z(K), lw, ls, lr, min_duration=bad)
        with pytest.raises(ValueError, match='min_duration'):
            kmeans.viterbi(z(6, D), [0], [6], z(D), z(K, D), z(K), 1.0, min_duration=bad)
    h = hmm.StickyHmmPosteriorgram(fitted_mixture(), 0.75)
    q = kmeans.KMeansQuantizer(3)
    q.centroids_, q.counts_, q.shift_ = np.zeros((3, 2)), np.ones(3), np.zeros(2, dtype=np.float32)
    for call in (h.decode, h.quantize):
        with pytest.raises(ValueError, match='min_duration'):
            call(z(5, 2), min_duration=9)
    for call in (lambda **kw: q.segment(z(5, 2), 1.0, **kw), lambda **kw: q.predict(z(5, 2), penalty=1.0, **kw),
                 lambda **kw: q.quantize(z(5, 2), penalty=1.0, **kw), lambda **kw: q.predict(z(5, 2), **kw)):
        with pytest.raises(ValueError, match='min_duration'):
            call(min_duration=0)
    with pytest.raises(ValueError, match='needs a penalty'):
        q.predict(z(5, 2), min_duration=2)
    with pytest.raises(ValueError, match='needs a penalty'):
        q.quantize(z(5, 2), min_duration=2)
    # the command lines know the flag
    assert kmeans.parser().parse_args(['transform', 'm', 'f', 'o', '--penalty', '2', '--min-duration', '3']).min_duration == 3
    assert kmeans.parser().parse_args(['transform', 'm', 'f', 'o']).min_duration == 1
    text = open(os.path.join(ROOT, 'abnet3_amd', 'hmm.py')).read() + open(os.path.join(ROOT, 'examples', 'zero_resource.py')).read()
    assert "'--min-duration'" in text and "'--kmeans-min-duration'" in text and "'--hmm-min-duration'" in text


# ---- the library -----------------------------------------------------------------------------------------------------------
def declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(abnx_[a-z0-9_]+)\s*\(', text))


def test_next_symbols_are_the_new_header_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib
    assert declared() == set(_lib.NEXT_SYMBOLS) == {'abnx_viterbi_dur_max', 'abnx_kmeans_viterbi_dur', 'abnx_hmm_viterbi_dur'}
    assert not set(_lib.NEXT_SYMBOLS) & set(_lib.SYMBOLS)
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abnx_')}
    assert exported == declared()
    for name, (res, args) in _lib.NEXT_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # the twins' arguments plus int32 min_duration
    for new, old in (('abnx_kmeans_viterbi_dur', 'abn_kmeans_viterbi'), ('abnx_hmm_viterbi_dur', 'abn_hmm_viterbi')):
        assert _lib.NEXT_SYMBOLS[new][1] == _lib.SYMBOLS[old][1] + [ctypes.c_int32]
    assert lib.abnx_viterbi_dur_max() == 8
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20                     # not part of the numbered ABI yet


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    #          x  T    D  off len n  sh m  b  K  pen  ids obj  nsw   ws bytes stream S
    good_k = [p, 100, 4, p, p, 2, p, p, p, 8, 1.0, p, None, None, p, big, None, 3]
    #          x  T    D  off len n  sh A  B  c0 lw ls lr K  ids lp    nsw   ng    ws bytes stream S
    good_h = [p, 100, 4, p, p, 2, p, p, p, p, p, p, p, 8, p, None, None, None, p, big, None, 3]

    def with_(call, good, **kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for call, good, ptrs, i_k, i_ws, name, max_k, max_d in (
            (lib.abnx_kmeans_viterbi_dur, good_k, (0, 3, 4, 6, 7, 8, 11), 9, 14, b'abnx_kmeans_viterbi_dur',
             lib.abn_kmeans_viterbi_max_k(), lib.abn_kmeans_max_d()),
            (lib.abnx_hmm_viterbi_dur, good_h, (0, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14), 13, 18, b'abnx_hmm_viterbi_dur',
             lib.abn_hmm_max_k(), lib.abn_gmm_max_d())):
        S = len(good) - 1
        for i in ptrs:
            assert with_(call, good, **{'a%d' % i: None}) == _lib.E_ARG, i
            assert b'null pointer' in lib.abn_last_error() and name in lib.abn_last_error()
        assert with_(call, good, a1=0) == _lib.E_ARG and with_(call, good, a1=1 << 31) == _lib.E_ARG
        assert with_(call, good, a2=0) == _lib.E_ARG and with_(call, good, a5=0) == _lib.E_ARG
        assert with_(call, good, **{'a%d' % i_k: 0}) == _lib.E_ARG
        assert with_(call, good, a2=max_d + 1) == _lib.E_UNSUPPORTED and with_(call, good, **{'a%d' % i_k: max_k + 1}) == _lib.E_UNSUPPORTED
        for bad in (0, -1, 9, 1 << 20):
            assert with_(call, good, **{'a%d' % S: bad}) == _lib.E_ARG, bad
            assert b'min_duration' in lib.abn_last_error()
        assert with_(call, good, **{'a%d' % i_ws: None}) == _lib.E_WORKSPACE
        assert with_(call, good, **{'a%d' % (i_ws + 1): 1024}) == _lib.E_WORKSPACE
        assert b'_viterbi_ws_bytes' in lib.abn_last_error()                           # the twin's sizing entry
        assert with_(call, good, **{'a%d' % i_ws: ctypes.c_void_p(0x10004)}) == _lib.E_ARG
    assert with_(lib.abnx_kmeans_viterbi_dur, good_k, a10=-1.0) == _lib.E_ARG
    assert with_(lib.abnx_kmeans_viterbi_dur, good_k, a10=float('inf')) == _lib.E_ARG
