"""Times KLLoss (abnet3/loss.py:108-137) on the device, in one process:
  kernel routes at B = 4096 pairs, D = 100 (the C1 / C2 output width):
    kl_prob        KLLoss.value_and_grad on probability rows (kl_pair_loss_kernel, one launch)
    kl_logits      KLLoss.value_and_dz(..., 'softmax'): softmax, loss and d loss / d logits (one launch)
    coscos2        coscos2.value_and_grad (pair_loss_kernel), the cosine loss beside it
    torch_prob     the reference formula as torch GPU ops with autograd (sum(p log(p/q)), two HingeEmbeddingLoss)
    torch_logits   nn.Softmax() in front of the same
  train steps of a softmax SiameseNetwork with KLLoss: C1-shaped (40->100->50, 32 pairs) and C2-shaped
  (40->500x2->100, 4096 pairs, Adadelta 0.1), TrainerSiamese.train_step's direct path against direct_steps = False.
Every route settles the clock (untimed calls for 0.3 s), then 15 calls are timed one by one with events; the median is
reported; the kernel routes are also timed as 20 launches replayed from one hipGraph (the launch alone).
python tools/kl_time.py [--out FILE] [--only-step c1|c2] (the latter: two steps of that shape behind a marker launch, for a trace)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn as nn

from abnet3_amd.loss import KLLoss, coscos2


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


def torch_kl(p, q, y, margin=1.0):
    """abnet3/loss.py:127-137 as torch ops (size_average=True is reduction='mean')."""
    h = nn.HingeEmbeddingLoss(margin=margin, reduction='mean')
    return h(torch.sum(p * torch.log(p / q), 1), y) + h(torch.sum(q * torch.log(q / p), 1), y)


def kernel_routes(res, B=4096, D=100):
    g = torch.Generator(device='cuda').manual_seed(0)
    z1 = 3 * torch.randn(B, D, device='cuda', generator=g)
    z2 = 3 * torch.randn(B, D, device='cuda', generator=g)
    p, q = torch.softmax(z1, 1), torch.softmax(z2, 1)
    y = torch.randint(0, 2, (B,), device='cuda', generator=g) * 2 - 1
    kl = KLLoss()
    sm = nn.Softmax(dim=1)

    def torch_prob():
        a, b = p.detach().requires_grad_(True), q.detach().requires_grad_(True)
        lv = torch_kl(a, b, y)
        return torch.autograd.grad(lv, (a, b))

    def torch_logits():
        a, b = z1.detach().requires_grad_(True), z2.detach().requires_grad_(True)
        lv = torch_kl(sm(a), sm(b), y)
        return torch.autograd.grad(lv, (a, b))

    routes = {'kl_prob': lambda: kl.value_and_grad(p, q, y),
              'kl_logits': lambda: kl.value_and_dz(z1, z2, y, 'softmax'),
              'coscos2': lambda: coscos2().value_and_grad(z1, z2, y),
              'torch_prob': torch_prob, 'torch_logits': torch_logits}
    out = res['kernel'] = {'B': B, 'D': D, 'bytes_per_pair_hbm': 4 * D * 4 + 8,
                           'median_us_is': 'one call from Python (ctypes, output allocation, launch) timed with events',
                           'graph20_us_is': 'the launch ALONE: 20 calls captured into one hipGraph, the replay timed, / 20'}
    for name, fn in routes.items():
        ms, all_ms = median_ms(fn)
        out[name] = {'median_us': round(ms * 1e3, 2), 'calls_ms': all_ms}
        if name.startswith('torch'):
            continue
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(20):
                fn()
        ms, _ = median_ms(graph.replay)
        out[name]['graph20_us'] = round(ms * 1e3 / 20, 2)
    lv, dz = kl.value_and_dz(z1, z2, y, 'softmax')
    a, b = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    lv64 = torch_kl(torch.softmax(a, 1), torch.softmax(b, 1), y)
    ga, gb = torch.autograd.grad(lv64, (a, b))
    out['kl_logits_rel_err_vs_torch_f64'] = {'loss': abs(float(lv) - float(lv64.detach())) / abs(float(lv64.detach())),
                                             'dz': float(max((dz[0].double() - ga).abs().max(), (dz[1].double() - gb).abs().max())
                                                         / max(ga.abs().max(), gb.abs().max()))}
    for name in ('kl_prob', 'kl_logits', 'coscos2'):
        out[name]['GB_per_s_graph20'] = round(B * out['bytes_per_pair_hbm'] / (out[name]['graph20_us'] * 1e-6) / 1e9, 1)


SHAPES = {'c1': (dict(input_dim=40, num_hidden_layers=0, hidden_dim=100, output_dim=50), 32),
          'c2': (dict(input_dim=40, num_hidden_layers=2, hidden_dim=500, output_dim=100), 4096)}


def make_step(shape, direct, bn=False):
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    kw, B = SHAPES[shape]
    torch.manual_seed(2)
    net = SiameseNetwork(p_dropout=0.0, type_init='xavier_uni', activation_layer='sigmoid', batch_norm=bn,
                         last_non_linearity='softmax', output_path='/tmp/abn_kl_time', **kw).cuda()
    tr = TrainerSiamese(network=net, loss=KLLoss(), optimizer_type='adadelta', lr=0.1, dataloader=None, log_dir='/tmp/abn_runs')
    tr.direct_steps = direct
    assert tr._direct_ok() == direct
    g = torch.Generator(device='cuda').manual_seed(20)
    batch = (torch.randn(B, kw['input_dim'], device='cuda', generator=g), torch.randn(B, kw['input_dim'], device='cuda', generator=g),
             torch.randint(0, 2, (B,), device='cuda', generator=g) * 2 - 1)
    net.train()
    return lambda: tr.train_step(batch, True)


def step_routes(res):
    out = res['train_step'] = {}
    for shape in SHAPES:
        for bn in (False, True):
            r = out['%s%s' % (shape, '_bn' if bn else '')] = {'pairs': SHAPES[shape][1]}
            for direct in (True, False):
                ms, all_ms = median_ms(make_step(shape, direct, bn))
                r['direct' if direct else 'autograd'] = {'median_us': round(ms * 1e3, 2), 'calls_ms': all_ms}
            r['autograd_over_direct'] = round(r['autograd']['median_us'] / r['direct']['median_us'], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--only-step', default=None, choices=sorted(SHAPES))
    a = ap.parse_args()
    if a.only_step:
        step = make_step(a.only_step, True)
        step()                                  # the first step (one-time buffers: scratch, optimizer state)
        torch.cuda.synchronize()
        torch.arange(7, device='cuda')          # a marker launch: the trace's launches behind it are ONE steady step
        torch.cuda.synchronize()
        step()
        torch.cuda.synchronize()
        return
    res = {'device': torch.cuda.get_device_name()}
    kernel_routes(res)
    step_routes(res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
