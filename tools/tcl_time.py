"""Times the temporal-coherence pairs (abnet3_amd/csrc/tcl.hip, TemporalCoherenceDataLoader).

  draw time   one default pass -- 1000 batches x 500 frame pairs = 100 000 draws -- on a synthetic corpus (--files
              utterances of 2-10 s of 280-d frames):
                fill          device events around ONE abn_tcl_pairs launch into the loader's persistent arrays (the
                              launch as a caller sees it: at this size the interval holds the host's issue as well)
                batches       wall time of a whole pass through batch_iterator(True): the fill and 1000 x two
                              abn_gather_rows launches, synchronised at the end
                host          wall time of the existing OriginalDataLoader.temporal_coherence_loss(500) called 1000
                              times in the same run: Python's `random`, two index uploads and the same two gathers per
                              batch -- what a tcl > 0 run without tcl_seed does per batch
  step time   ms per step of TrainerSiamese.train() on the loader (280-500-500-100 sigmoid tower, coscos2, Adadelta),
              planned passes against planned_passes=False, from the trainer's own per-pass clock (time_passes); the
              untrained pass and the first trained pass (warm-up, graph capture) are left out, the median of the rest
              is reported

The GPU routes settle the clock (untimed calls for 0.3 s) before their 15 timed calls; medians are reported.

python tools/tcl_time.py [--files 500] [--epochs 5] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.sampler_time import median_ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def corpus(n_files, dim, seed=0):
    """A DeviceCorpus of n_files utterances of 200 .. 1000 frames drawn on the device, and a few sampled word pairs."""
    import torch
    from abnet3_amd.dataloader import DeviceCorpus
    rng = np.random.default_rng(seed)
    lengths = rng.integers(200, 1001, n_files)
    names = ['utt%05d' % k for k in range(n_files)]
    g = torch.Generator(device='cuda').manual_seed(seed)
    table = torch.randn(int(lengths.sum()), dim, device='cuda', generator=g)
    times = {k: np.arange(n) * 0.01 + 0.0025 for k, n in zip(names, lengths)}

    def token():
        k = int(rng.integers(n_files))
        a = int(rng.integers(0, lengths[k] - 60))
        return names[k], a * 0.01, (a + int(rng.integers(20, 60))) * 0.01

    def pairs(n):
        return [token() + token() + ('same' if i % 2 == 0 else 'diff',) for i in range(n)]
    return DeviceCorpus.from_table(table, names, lengths, times), pairs(4 * n_files), pairs(64)


def loader(cls, dc, train, dev, **kw):
    dl = cls('unused', 'unused', **kw)
    dl.features = dc
    dl.pairs['train'], dl.pairs['dev'] = list(train), list(dev)
    dl.train_files = list({p[0] for p in train} | {p[3] for p in train})
    return dl


def wall_ms(fn, calls):
    import torch
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3), calls=calls)


def step_ms(dc, train, dev, planned, epochs, folder):
    import torch
    from abnet3_amd.dataloader import TemporalCoherenceDataLoader
    from abnet3_amd.loss import coscos2
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    dl = loader(TemporalCoherenceDataLoader, dc, train, dev)
    np.random.seed(0)
    torch.manual_seed(0)
    net = SiameseNetwork(input_dim=dc.dim, num_hidden_layers=1, hidden_dim=500, output_dim=100, p_dropout=0.0,
                         activation_layer='sigmoid', output_path=os.path.join(folder, 'net%d' % planned))
    tr = TrainerSiamese(network=net, loss=coscos2(avg=False), num_epochs=epochs, patience=epochs + 1, optimizer_type='adadelta',
                        lr=0.1, dataloader=dl, log_dir=os.path.join(folder, 'runs%d' % planned))
    tr.planned_passes = planned
    tr.time_passes = True
    tr.train()
    per_step = [1e3 * t / dl.num_max_minibatches for t, _ in tr.pass_seconds]
    return dict(ms_per_step=round(float(np.median(per_step[2:])), 4), per_pass_ms_per_step=[round(v, 4) for v in per_step],
                train_losses=[round(float(v), 4) for v in tr.train_losses])


def run(a):
    import torch
    from abnet3_amd.dataloader import OriginalDataLoader, TemporalCoherenceDataLoader
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'files': a.files, 'dim': a.dim}
    dc, train, dev = corpus(a.files, a.dim)
    res['frames'] = int(dc.total)
    dl = loader(TemporalCoherenceDataLoader, dc, train, dev)
    plan = dl.plan(True)
    n_iter = len(plan.idx1) // 5
    res['pairs_per_pass'] = int(len(plan.idx1))
    fill = median_ms(lambda: dl._tcl_fill(n_iter, 1, plan.idx1, plan.idx2, plan.labels))
    host = loader(OriginalDataLoader, dc, train, dev, tcl=0.3)

    def host_pass():
        for _ in range(dl.num_max_minibatches):
            host.temporal_coherence_loss(dl.batch_size)

    def device_pass():
        for _ in dl.batch_iterator(True):
            pass
    device_pass()
    res['draw'] = {'abn_tcl_pairs_fill_ms': dict(zip(('median', 'min', 'max'), fill)),
                   'draws_per_s': round(n_iter / (fill[0] * 1e-3), 0),
                   'device_pass_batches_wall_ms': wall_ms(device_pass, 5),
                   'host_temporal_coherence_loss_pass_wall_ms': wall_ms(host_pass, 3)}
    d = res['draw']
    d['host_pass_over_fill'] = round(d['host_temporal_coherence_loss_pass_wall_ms']['median'] / fill[0], 1)
    d['host_pass_over_device_pass'] = round(d['host_temporal_coherence_loss_pass_wall_ms']['median'] /
                                            d['device_pass_batches_wall_ms']['median'], 2)
    folder = tempfile.mkdtemp(prefix='tcl_time_')
    res['step'] = {'planned': step_ms(dc, train, dev, True, a.epochs, folder),
                   'iterator': step_ms(dc, train, dev, False, a.epochs, folder)}
    res['step']['iterator_over_planned'] = round(res['step']['iterator']['ms_per_step'] / res['step']['planned']['ms_per_step'], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=500)
    ap.add_argument('--dim', type=int, default=280)
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tcl_time.json'))
    a = ap.parse_args()
    res = run(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
