"""Times the MFCC front end on bench.py's filterbank input (3000 s of synthetic 16 kHz int16 audio, 300 001 frames, resident
in HBM), beside the routes it is compared with, in one process:
  mfcc512        abn_mfcc, nfft 512, 40 filters, 13 cepstra (mfcc512_kernel)
  mfcc512_d_dd   the same with deltas and deltasdeltas (+ two abn_deltas_batched launches): 39 columns
  fbank1024      abn_fbank, nfft 1024, 40 filters (fbank1024_kernel, bench.py's fbank leg)
  fallback       what a caller would write without abn_mfcc: abn_fbank at nfft 512 on the MFCC bank (the general
                 workgroup-per-frame kernel) + a torch matmul with the DCT table
Every route settles the clock (untimed calls for 0.3 s), then 15 calls are timed one by one with events; the median is
reported.  python tools/mfcc_time.py [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from abnet3_amd import _lib
from abnet3_amd.features import FeaturesGenerator, MFCC_LOWERF, MFCC_UPPERF, NCEP


def settle(fn, seconds=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            fn()
        torch.cuda.synchronize()


def median_ms(fn, calls=15):
    settle(fn)
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=int, default=3000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    fs = 16000
    rng = np.random.default_rng(7)                    # bench.py fbank_bench's signal
    n = a.seconds * fs
    t = np.arange(n) / fs
    sig = (2000 * np.sin(2 * np.pi * 440 * t) + 500 * rng.standard_normal(n)).astype(np.int16)
    d = torch.from_numpy(sig).cuda()
    lib = _lib.load()
    mf = FeaturesGenerator(method='mfcc')
    mfd = FeaturesGenerator(method='mfcc', deltas=True, deltasdeltas=True)
    fb = FeaturesGenerator()
    wl, fshift = int(0.025 * fs), fs / 100.0
    nfr = int(n / fshift + 1)
    win, bank, band, dct = mf._table(fs, wl, 512, d.device, MFCC_LOWERF, MFCC_UPPERF, NCEP)
    logspec = torch.empty(nfr, 40, dtype=torch.float32, device=d.device)
    dct_t = dct.t().contiguous()

    def fallback():
        _lib.check(lib.abn_fbank(_lib.ptr(d), 1, n, wl, fshift, 512, 40, 0.97, _lib.ptr(win), _lib.ptr(bank), _lib.ptr(band), nfr,
                                 _lib.ptr(logspec), _lib.stream()), 'abn_fbank')
        return logspec @ dct_t

    routes = {'mfcc512': lambda: mf.mfcc_from_samples(d, fs),
              'mfcc512_d_dd': lambda: mfd.mfcc_from_samples(d, fs),
              'fbank1024': lambda: fb.fbank_from_samples(d, fs),
              'fallback': fallback}
    res = {'input': '%d s of 16 kHz int16 audio in HBM (bench.py fbank_bench signal), %d frames' % (a.seconds, nfr),
           'path_mfcc512': lib.abn_mfcc_path(512, 40, 13), 'routes': {}}
    for name, fn in routes.items():
        out = fn()
        torch.cuda.synchronize()
        assert out.shape[0] == nfr, (name, out.shape)
        ms, all_ms = median_ms(fn)
        res['routes'][name] = {'median_ms': round(ms, 4), 'frames_per_s': round(nfr / (ms * 1e-3), 1), 'cols': int(out.shape[1]),
                               'calls_ms': all_ms}
    r = res['routes']
    res['mfcc512_over_fbank1024'] = round(r['mfcc512']['frames_per_s'] / r['fbank1024']['frames_per_s'], 3)
    res['mfcc512_over_fallback'] = round(r['mfcc512']['frames_per_s'] / r['fallback']['frames_per_s'], 3)
    res['max_abs_diff_mfcc512_vs_fallback'] = float((mf.mfcc_from_samples(d, fs) - fallback()).abs().max())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
