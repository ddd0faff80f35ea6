"""The MFCC front end's host side, without a GPU: the C ABI declares, binds and exports abn_mfcc, abn_mfcc_batched,
abn_deltas_batched and abn_mfcc_path; bad arguments are refused before any launch; the kernel choice is a pure query; the
host tables (mel bank, bands, the DCT) are what the definition says (tests/mfcc_np.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ('abn_mfcc', 'abn_mfcc_batched', 'abn_deltas_batched', 'abn_mfcc_path')


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def test_new_symbols_declared_bound_exported(lib):
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(abn_[a-z0-9_]+)\s*\(', text))
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    dyn = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
        assert re.search(r'\b%s\b' % name, dyn), name
    assert lib.abn_abi_version() == _lib.ABI_VERSION == 20


def test_bad_arguments_are_refused_before_any_launch(lib):
    p = ctypes.c_void_p(0x10000)          # never dereferenced: every call below fails its checks first

    def mfcc(nfft=512, nfilt=40, ncep=13, wlen=400, nframes=10, ld=13, samples=p, dct=p, band=p):
        return lib.abn_mfcc(samples, 1, 16000, wlen, 160.0, nfft, nfilt, ncep, 0.97, p, p, band, dct, nframes, p, ld, None)
    assert mfcc(nfft=500) == -1 and b'nfft' in lib.abn_last_error()
    assert mfcc(nfft=4096) == -1
    assert mfcc(ncep=0) == -1 and b'ncep' in lib.abn_last_error()
    assert mfcc(ncep=41) == -1
    assert mfcc(nfilt=0, ncep=0) == -1 and mfcc(nfilt=129) == -1
    assert mfcc(wlen=0) == -1
    assert mfcc(ld=12) == -1 and b'stride' in lib.abn_last_error()
    assert mfcc(nframes=-1) == -1
    assert mfcc(samples=None) == -1 and b'null' in lib.abn_last_error()
    assert mfcc(dct=None) == -1 and mfcc(band=None) == -1
    assert lib.abn_mfcc(p, 1, 16000, 400, 0.0, 512, 40, 13, 0.97, p, p, p, p, 10, p, 13, None) == -1      # frame shift
    assert lib.abn_mfcc_batched(p, 1, None, None, 0, 400, 160.0, 512, 40, 13, 0.97, p, p, p, p, 10, p, 13, None) == -1
    assert b'utterance tables' in lib.abn_last_error()
    assert lib.abn_mfcc_batched(p, 1, p, p, 2, 400, 160.0, 512, 40, 14 * 4, 0.97, p, p, p, p, 10, p, 56, None) == -1
    # deltas_batched: strides, utterance count, null pointers, an output slice on top of the input's columns
    q = ctypes.c_void_p(0x10000 + 4 * 13)
    assert lib.abn_deltas_batched(p, 12, p, 1, 10, 13, q, 39, None) == -1
    assert lib.abn_deltas_batched(p, 39, p, 0, 10, 13, q, 39, None) == -1
    assert lib.abn_deltas_batched(None, 39, p, 1, 10, 13, q, 39, None) == -1
    assert lib.abn_deltas_batched(p, 39, None, 1, 10, 13, q, 39, None) == -1
    assert lib.abn_deltas_batched(p, 39, p, 1, 10, 13, ctypes.c_void_p(0x10000 + 4 * 12), 39, None) == -1
    assert b'overlap' in lib.abn_last_error()
    assert lib.abn_deltas_batched(p, 39, p, 1, 10, 0, q, 39, None) == -1
    # nothing to do is not an error
    assert lib.abn_deltas_batched(p, 39, p, 1, 0, 13, q, 39, None) == 0
    assert mfcc(nframes=0, samples=None) == 0


def test_mfcc_path_is_a_pure_query(lib):
    from abnet3_amd import _lib
    # the reference's call (nfft 512, 13 cepstra) at its default and at a wide filter count: the wavefront kernel
    assert lib.abn_mfcc_path(512, 40, 13) == _lib.MFCC_WAVE512
    assert lib.abn_mfcc_path(512, 64, 13) == _lib.MFCC_WAVE512
    assert lib.abn_mfcc_path(512, 20, 13) == _lib.MFCC_WAVE512
    assert lib.abn_mfcc_path(512, 65, 13) == _lib.MFCC_GENERAL
    assert lib.abn_mfcc_path(1024, 40, 13) == _lib.MFCC_GENERAL
    assert lib.abn_mfcc_path(256, 40, 13) == _lib.MFCC_GENERAL
    for args in ((500, 40, 13), (512, 40, 0), (512, 40, 41), (512, 129, 13), (32, 40, 13)):
        assert lib.abn_mfcc_path(*args) == -1, args


def test_host_dct_table_is_the_formula():
    import mfcc_np
    from abnet3_amd.features import dct_table
    for nfilt in (20, 40, 64):
        C = dct_table(nfilt, 13)
        assert C.shape == (13, nfilt) and C.dtype == np.float64
        for i in range(13):
            for j in range(nfilt):
                want = np.cos(np.pi * i * (j + 0.5) / nfilt) * (0.5 if j == 0 else 1.0)
                assert abs(C[i, j] - want) < 1e-15, (nfilt, i, j)
        assert np.array_equal(C, mfcc_np.dct_matrix(nfilt, 13))
    assert (dct_table(40)[0, 1:] == 1.0).all() and dct_table(40)[0, 0] == 0.5        # c0: half the first log energy + the rest


@pytest.mark.parametrize('fs,nfilt,wl,empty', [(16000, 40, 400, 0), (16000, 64, 400, 0), (22050, 40, 551, 0), (44100, 40, 1102, 3)])
def test_mfcc_generator_builds_its_tables(fs, nfilt, wl, empty):
    from abnet3_amd.features import FeaturesGenerator, MFCC_LOWERF, MFCC_UPPERF, MFCC_NFFT, NCEP
    from oracle import features_np as F
    fg = FeaturesGenerator(method='mfcc', n_filters=nfilt)
    win, bank, band, dct = fg._table(fs, wl, MFCC_NFFT, 'cpu', MFCC_LOWERF, MFCC_UPPERF, NCEP)
    ref = F.mel_filterbank(fs, 512, nfilt, 100, 6855.4976)
    assert win.shape == (wl,) and np.allclose(win.numpy(), np.hamming(wl), atol=1e-7)     # the whole window: the kernel crops
    assert bank.shape == (257, nfilt) and np.abs(bank.numpy() - ref).max() < 1e-6 * ref.max()
    b = band.numpy()
    assert (b[:, 1] <= 256).all()
    assert int((b[:, 1] < b[:, 0]).sum()) == empty == int((ref.max(axis=0) == 0).sum())   # filters with no non-zero weight
    for f in range(nfilt):
        nz = np.nonzero(ref[:, f])[0]
        if len(nz):
            assert (b[f, 0], b[f, 1]) == (nz[0], nz[-1])
    assert dct.shape == (13, nfilt) and dct.dtype.is_floating_point
    import mfcc_np
    assert np.array_equal(dct.numpy(), (mfcc_np.dct_matrix(nfilt) / nfilt).astype(np.float32))
    # the filterbank's tables of the same generator are kept apart (other edges, nfft, no DCT)
    w2, bank2, _, dct2 = fg._table(fs, wl if wl <= 1024 else 1024, 1024, 'cpu')
    assert dct2 is None and bank2.shape == (513, nfilt)


def test_unknown_method_still_refused():
    from abnet3_amd.features import FeaturesGenerator
    with pytest.raises(ValueError, match='Method plp not authorized'):
        FeaturesGenerator(method='plp', files=[]).generate()
    with pytest.raises(ValueError, match='Method plp not authorized'):
        FeaturesGenerator(method='plp').features_batch([np.zeros(10, dtype=np.int16)], 16000)
