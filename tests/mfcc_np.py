"""Float64 restatement of the MFCC front end (FeaturesGenerator.do_mfccs, abnet3/features.py:116-133) that the HIP kernels
are tested against.  A test helper, not a test module.

PARITY UNPINNED, like the filterbank (oracle/features_np.py header): the reference calls spectral.Spectral(nfilt, alpha=0.97,
fs, frate=100, wlen=0.025, nfft=512, ncep=13, lowerf=100, upperf=6855.4976, do_deltas, do_deltasdeltas) with do_dct left on,
and casts to float32; the package is absent.  This follows the same Sphinx-III `mfcc.py` lineage as the filterbank:
  1. framing, pre-emphasis, window, power spectrum, log mel: exactly oracle/features_np.fbank's, with nfft = 512,
     lowerf = 100, upperf = 6855.4976;
  2. a window longer than the FFT (fs > 20480 Hz at 25 ms) is cropped: rfft(frame, 512) keeps the first 512 samples of the
     pre-emphasised, windowed frame, the next frame's pre-emphasis history is still the frame's last sample;
  3. the cepstra (the lineage's "legacy" DCT, s2dctmat / logspec2s2mfc): C[i, j] = cos(pi i (j + 1/2) / nfilt) for
     i < ncep, j < nfilt, column 0 halved; mfcc = logspec . C^T / nfilt, c0 included;
  4. deltas: oracle/features_np.deltas on the cepstra, deltasdeltas = deltas(deltas).
"""
import numpy as np

from oracle.features_np import FLOOR, deltas, frame_count, frame_samples, mel_filterbank

NFFT = 512
LOWERF = 100.0
UPPERF = 6855.4976
NCEP = 13


def dct_matrix(nfilt, ncep=NCEP):
    C = np.zeros((ncep, nfilt), dtype=np.float64)
    for i in range(ncep):
        for j in range(nfilt):
            C[i, j] = np.cos(np.pi * i * (j + 0.5) / nfilt)
    C[:, 0] *= 0.5
    return C


def logspec(sig, fs, nfilt=40, alpha=0.97, frate=100, wlen=0.025, nfft=NFFT, lowerf=LOWERF, upperf=UPPERF):
    """float64 [nfr, nfilt] log mel energies on the MFCC spectrum (items 1-2 of the module docstring)."""
    sig = np.asarray(sig).astype(np.float64)
    fshift = float(fs) / frate
    wl = int(wlen * fs)
    win = np.hamming(wl)
    filt = mel_filterbank(fs, nfft, nfilt, lowerf, upperf)
    nfr = frame_count(len(sig), fs, frate)
    out = np.zeros((nfr, nfilt), dtype=np.float64)
    prior = 0.0
    for t in range(nfr):
        frame = frame_samples(sig, t, fshift, wl)
        prev = np.concatenate(([prior], frame[:-1]))
        prior = frame[-1]
        spec = np.fft.rfft((frame - alpha * prev) * win, nfft)          # crops a frame longer than nfft
        power = spec.real * spec.real + spec.imag * spec.imag
        out[t] = np.log(np.clip(np.dot(power, filt), FLOOR, np.inf))
    return out


def mfcc(sig, fs, nfilt=40, ncep=NCEP, **kw):
    """float32 [nfr, ncep]: the cepstra of do_mfccs (no deltas)."""
    ls = logspec(sig, fs, nfilt=nfilt, **kw)
    return (np.dot(ls, dct_matrix(nfilt, ncep).T) / nfilt).astype(np.float32)


def mfcc_with_deltas(sig, fs, do_deltas=True, do_deltasdeltas=True, **kw):
    """[T, ncep * (1 + deltas + deltasdeltas)]: cepstra, then the slopes."""
    c = mfcc(sig, fs, **kw)
    cols = [c]
    d1 = deltas(c)
    if do_deltas:
        cols.append(d1)
    if do_deltasdeltas:
        cols.append(deltas(d1))
    return np.hstack(cols).astype(np.float32)
