"""The MFCC front end on the MI355X (FeaturesGenerator.do_mfccs, abnet3/features.py:116-133): abn_mfcc / abn_mfcc_batched
against the float64 restatement of tests/mfcc_np.py, the one-launch deltas against abn_deltas, and method='mfcc' through
features_from_waves and generate() -> training -> embedding on files.  Needs an MI355X: run with -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

import mfcc_np

pytestmark = pytest.mark.gpu

BAR = 5e-5            # the filterbank's bar against its definition (tests/test_gpu_dtw_features.py)


def speech_like(n, fs, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (2000 * np.sin(2 * np.pi * 700 * t) + 900 * np.sin(2 * np.pi * 2300 * t + 1.0)
            + 200 * rng.standard_normal(n)).astype(np.int16)


def _path(nfft, nfilt, ncep=13):
    from abnet3_amd import _lib
    return _lib.load().abn_mfcc_path(nfft, nfilt, ncep)


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
@pytest.mark.parametrize('n', [1, 399, 400, 401, 16000, 48137])
def test_mfcc_matches_restatement_lengths(n, dtype):
    from abnet3_amd import _lib
    from abnet3_amd.features import FeaturesGenerator
    from oracle import features_np as F
    fs = 16000
    sig = speech_like(n, fs, n)
    x = sig if dtype == 'int16' else sig.astype(np.float32)
    assert _path(512, 40) == _lib.MFCC_WAVE512
    got = FeaturesGenerator(method='mfcc').mfcc_from_samples(x, fs).cpu().numpy()
    ref = mfcc_np.mfcc(sig, fs)
    assert got.shape == ref.shape == (F.frame_count(n, fs), 13) and got.dtype == np.float32
    assert np.abs(got - ref).max() < BAR, np.abs(got - ref).max()


@pytest.mark.parametrize('nfilt', [20, 40, 64])
def test_mfcc_filter_counts(nfilt):
    from abnet3_amd import _lib
    from abnet3_amd.features import FeaturesGenerator
    fs, n = 16000, 16000
    sig = speech_like(n, fs, nfilt)
    assert _path(512, nfilt) == _lib.MFCC_WAVE512
    got = FeaturesGenerator(method='mfcc', n_filters=nfilt).mfcc_from_samples(sig, fs).cpu().numpy()
    ref = mfcc_np.mfcc(sig, fs, nfilt=nfilt)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < BAR, np.abs(got - ref).max()


@pytest.mark.parametrize('fs', [22050, 44100])
def test_mfcc_window_longer_than_fft(fs):
    """25 ms is 551 / 1102 samples: rfft(frame, 512) keeps the first 512 of the pre-emphasised, windowed frame.  At 44.1 kHz
    three of the 40 filters have no non-zero weight: their log energy is log(1e-5) inside the cepstra."""
    from oracle import features_np as F
    from abnet3_amd.features import FeaturesGenerator
    n = 3 * fs // 2 + 77
    sig = speech_like(n, fs, fs)
    bank = F.mel_filterbank(fs, 512, 40, 100, 6855.4976)
    assert int((bank.max(axis=0) == 0).sum()) == (3 if fs == 44100 else 0)
    if fs == 44100:
        assert np.allclose(mfcc_np.logspec(sig[:4000], fs)[:, bank.max(axis=0) == 0], np.log(1e-5))
    for x in (sig, sig.astype(np.float32)):
        got = FeaturesGenerator(method='mfcc').mfcc_from_samples(x, fs).cpu().numpy()
        ref = mfcc_np.mfcc(sig, fs)
        assert got.shape == ref.shape == (F.frame_count(n, fs), 13)
        assert np.abs(got - ref).max() < BAR, np.abs(got - ref).max()


def test_mfcc_general_kernel():
    """Another nfft or more than 64 filters takes the workgroup-per-frame kernel (the general filterbank kernel's 2e-4 bar)."""
    from abnet3_amd import _lib
    from abnet3_amd.features import FeaturesGenerator
    fs, n = 16000, 12345
    sig = speech_like(n, fs, 3)
    for nfft, nfilt in ((1024, 40), (512, 80)):
        assert _path(nfft, nfilt) == _lib.MFCC_GENERAL
        got = FeaturesGenerator(method='mfcc', n_filters=nfilt).mfcc_from_samples(sig, fs, nfft=nfft).cpu().numpy()
        ref = mfcc_np.mfcc(sig, fs, nfilt=nfilt, nfft=nfft)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() < 2e-4, (nfft, nfilt, np.abs(got - ref).max())


def ragged(seed=11):
    rng = np.random.default_rng(seed)
    lens = [1, 150, 399, 400, 401, 16000, 23456] + list(rng.integers(300, 20000, 9))
    return [speech_like(int(m), 16000, 100 + i) for i, m in enumerate(lens)]


@pytest.mark.parametrize('d,dd', [(False, False), (True, True), (False, True)])
def test_mfcc_batch_is_the_per_utterance_calls(d, dd):
    from abnet3_amd.features import FeaturesGenerator
    waves = ragged()
    fg = FeaturesGenerator(method='mfcc', deltas=d, deltasdeltas=dd)
    table, nfr = fg.mfcc_batch(waves, 16000)
    assert table.shape == (int(nfr.sum()), 13 * (1 + d + dd))
    host = table.cpu().numpy()
    o = 0
    for w, m in zip(waves, nfr):
        one = fg.mfcc_from_samples(w, 16000).cpu().numpy()
        assert one.shape[0] == m
        assert np.array_equal(host[o:o + m], one)
        o += m


@pytest.mark.parametrize('d,dd', [(True, False), (True, True), (False, True)])
def test_mfcc_deltas_match_restatement(d, dd):
    from abnet3_amd.features import FeaturesGenerator
    fs = 16000
    fg = FeaturesGenerator(method='mfcc', deltas=d, deltasdeltas=dd)
    for n in (1, 170, 9000):
        sig = speech_like(n, fs, n + 1)
        got = fg.mfcc_from_samples(sig, fs).cpu().numpy()
        ref = mfcc_np.mfcc_with_deltas(sig, fs, do_deltas=d, do_deltasdeltas=dd)
        assert got.shape == ref.shape == (ref.shape[0], 13 * (1 + d + dd))
        assert np.abs(got - ref).max() < BAR, (n, np.abs(got - ref).max())


def test_deltas_batched_is_per_utterance_deltas():
    """abn_deltas_batched (one launch, column slices) against abn_deltas on every utterance alone, bit for bit, on MFCC and
    filterbank tables; and fbank_batch's delta columns are what its per-utterance form gave."""
    from abnet3_amd import _lib
    from abnet3_amd.features import FeaturesGenerator
    lib = _lib.load()
    waves = ragged(12)[:9] + [speech_like(170, 16000, 5), speech_like(330, 16000, 6)]        # 1- to 3-frame utterances too
    for fg, batch in ((FeaturesGenerator(method='mfcc'), 'mfcc_batch'), (FeaturesGenerator(), 'fbank_batch')):
        table, nfr = getattr(fg, batch)(waves, 16000)
        T, D = table.shape
        foff = np.concatenate(([0], np.cumsum(nfr))).astype(np.int64)
        foff_d = torch.from_numpy(foff).cuda()
        wide = torch.full((T, 3 * D + 5), float('nan'), device=table.device)
        wide[:, :D] = table
        _lib.check(lib.abn_deltas_batched(_lib.ptr(wide), wide.shape[1], _lib.ptr(foff_d), len(nfr), T, D,
                                          _lib.ptr(wide[:, 2 * D:]), wide.shape[1], _lib.stream()), 'abn_deltas_batched')
        got = wide.cpu().numpy()
        assert np.isnan(got[:, D:2 * D]).all() and np.isnan(got[:, 3 * D:]).all()           # only its own columns written
        ref = torch.cat([fg.deltas_of(table[foff[u]:foff[u + 1]]) for u in range(len(nfr))]).cpu().numpy()
        assert np.array_equal(got[:, 2 * D:3 * D], ref)
    # fbank_batch with deltas / deltasdeltas: the columns the per-utterance abn_deltas + torch.cat route gave, bit for bit
    base, nfr = FeaturesGenerator().fbank_batch(waves, 16000)
    foff = np.concatenate(([0], np.cumsum(nfr))).astype(np.int64)
    fg0 = FeaturesGenerator()
    d1 = torch.cat([fg0.deltas_of(base[foff[u]:foff[u + 1]]) for u in range(len(nfr))])
    d2 = torch.cat([fg0.deltas_of(d1[foff[u]:foff[u + 1]]) for u in range(len(nfr))])
    for d, dd, cols in ((True, False, [base, d1]), (True, True, [base, d1, d2]), (False, True, [base, d2])):
        got, _ = FeaturesGenerator(deltas=d, deltasdeltas=dd).fbank_batch(waves, 16000)
        assert torch.equal(got, torch.cat(cols, dim=1)), (d, dd)


@pytest.mark.parametrize('d', [False, True])
def test_features_from_waves_mfcc(d):
    """method='mfcc' -> mean / variance normalisation per channel -> 7-frame stacking: oracle.features_np.mvn and
    stack_fbanks on the restatement (91 or, with deltas and deltasdeltas, 273 columns)."""
    from abnet3_amd.features import FeaturesGenerator
    from oracle import features_np as F
    waves = ragged(13)[3:10]
    fg = FeaturesGenerator(method='mfcc', normalization=True, norm_per_channel=True, stack=True, nframes=7, deltas=d,
                           deltasdeltas=d)
    table, names, nfr, times = fg.features_from_waves(waves, 16000)
    width = 13 * (1 + 2 * d)
    assert table.shape == (int(nfr.sum()), 7 * width)
    raw = [mfcc_np.mfcc_with_deltas(w, 16000, do_deltas=d, do_deltasdeltas=d) for w in waves]
    normed, _, std = F.mvn(np.vstack(raw), per_channel=True)
    # the cepstra's bar, carried through the division by each channel's standard deviation
    tol = 2 * BAR / std.min() + 1e-5
    got, o = table.cpu().numpy(), 0
    for w, m in zip(waves, nfr):
        ref = F.stack_fbanks(normed[o:o + m].astype(np.float32), 7)
        assert np.abs(got[o:o + m] - ref).max() < tol, np.abs(got[o:o + m] - ref).max()
        o += m


@pytest.fixture()
def h5features(monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_h5features
    monkeypatch.setitem(sys.modules, 'h5features', fake_h5features)
    return fake_h5features


def test_generate_mfcc_train_embed_on_files(tmp_path, h5features):
    """generate() with method='mfcc' (the gridsearch's features: {method: 'mfcc'}) -> 91-d items -> OriginalDataLoader ->
    TrainerSiamese(input_dim=91) -> EmbedderSiamese, on files (tests/fake_h5features.py stands in for h5features)."""
    from scipy.io import wavfile
    import abnet3_amd.loss as L
    from abnet3_amd.features import FeaturesGenerator
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.dataloader import OriginalDataLoader
    from abnet3_amd.trainer import TrainerSiamese
    from abnet3_amd.embedder import EmbedderSiamese
    from abnet3_amd.utils import write_dataset
    rng = np.random.default_rng(6)
    wavdir = tmp_path / 'wav'
    wavdir.mkdir()
    waves = {}
    for u in range(5):
        n = 16000 * 3 + 211 * u
        waves['utt%d' % u] = (3000 * np.sin(2 * np.pi * (180 + 50 * u) * np.arange(n) / 16000) + 300 * rng.standard_normal(n)).astype(np.int16)
        wavfile.write(str(wavdir / ('utt%d.wav' % u)), 16000, waves['utt%d' % u])
    feat_path = str(tmp_path / 'exp' / 'mfcc_stacked7.features')
    fg = FeaturesGenerator(files=str(wavdir), output_path=feat_path, method='mfcc', normalization=True, norm_per_file=False,
                           norm_per_channel=True, stack=True, nframes=7, run='once')
    fg.generate()
    with h5features.Reader(feat_path, 'features') as fh:
        data = fh.read()
    names = list(data.items())
    assert sorted(names) == sorted(waves)
    table, _, nfr, _ = fg.features_from_waves([waves[k] for k in names], 16000, names)
    offs = np.concatenate(([0], np.cumsum(nfr)))
    for i, k in enumerate(names):
        f = data.dict_features()[k]
        assert f.dtype == np.float32 and f.shape == (int(nfr[i]), 91)
        assert np.array_equal(f, table[offs[i]:offs[i + 1]].cpu().numpy())
        assert np.allclose(data.dict_labels()[k], np.arange(int(nfr[i])) * 0.01 + 0.0025)
    # do_mfccs on one file: the cepstra before normalisation and stacking
    one = FeaturesGenerator(method='mfcc').do_mfccs(str(wavdir / 'utt0.wav'))
    assert one.shape == (int(nfr[names.index('utt0')]), 13)
    assert np.abs(one - mfcc_np.mfcc(waves['utt0'], 16000)).max() < BAR
    toks = [(k, round(0.2 + 0.25 * j, 2), round(0.2 + 0.25 * j + 0.18, 2)) for k in names for j in range(8)]

    def pairs(n):
        out = []
        for _ in range(n):
            a, b, c, d = (toks[i] for i in rng.choice(len(toks), 4, replace=False))
            out += [a + b + ('same',), c + d + ('diff',)]
        return out
    pairs_dir = tmp_path / 'exp' / 'pairs'
    for sub, n in (('train_pairs', 24), ('dev_pairs', 8)):
        (pairs_dir / sub).mkdir(parents=True)
        write_dataset(str(pairs_dir / sub / 'dataset'), pairs(n))
    net = SiameseNetwork(input_dim=91, num_hidden_layers=1, hidden_dim=64, output_dim=24, p_dropout=0.0,
                         activation_layer='sigmoid', output_path=str(tmp_path / 'exp' / 'network'))
    dl = OriginalDataLoader(pairs_path=str(pairs_dir), features_path=feat_path, batch_size=4, num_max_minibatches=100)
    tr = TrainerSiamese(network=net, loss=L.coscos2(avg=False), optimizer_type='adadelta', lr=0.1, num_epochs=2, patience=5,
                        dataloader=dl, log_dir=str(tmp_path / 'exp' / 'logs'))
    tr.train()
    assert len(tr.train_losses) == 3 and np.isfinite(tr.train_losses).all()
    out_path = str(tmp_path / 'exp' / 'embeddings.h5f')
    emb = EmbedderSiamese(network=net, network_path=net.output_path + '.pth', feature_path=feat_path, output_path=out_path)
    emb.embed()
    with h5features.Reader(out_path, 'features') as fh:
        e = fh.read()
    assert list(e.items()) == names
    for i, k in enumerate(names):
        assert e.dict_features()[k].shape == (int(nfr[i]), 24)
        assert np.isfinite(e.dict_features()[k]).all()
