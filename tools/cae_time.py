"""Times abnr_recon_loss (abnet3_amd/csrc/recon.hip, CorrespondenceLoss) and one TrainerCorrespondence step against the torch
routes on the same device, in the same process, on the same inputs.

Loss workloads: (B, D) = (486, 280) -- the mean batch of the word-pair loader over stacked filterbanks --, (4096, 280) and
(4096, 40); labels half 'same'; mode 'correspondence', symmetric, avg (the three-launch form: count, rows, sum).  Per workload:

  fused             CorrespondenceLoss.value_and_grad: loss and both gradients
  fused value       the loss alone, as the dev pass calls it
  torch route       tests/cae_np.py's torch_loss -- mse_loss over the masked rows -- and autograd's backward.  Never the kernel.
  torch value       torch_loss under no_grad

Each is timed two ways.  `call`: device events around ONE Python call (tools/gmm_time.py's median_ms: the clock settled by
0.3 s of untimed calls, then the median of 15) -- at these sizes mostly the host's time to enqueue.  `graph`: the fused routes
captured K times into one graph, each call on input tables of its own, replayed; the replay's time over K is the device's time
per call with the launches already enqueued.  K is chosen so that the K sets of tables exceed the 256 MiB Infinity Cache
where 64 sets can (`streams_from_hbm`); where they cannot the tables are served from the cache and the fraction of the HBM
bound says so (`cache_resident`) -- it is then no statement about HBM.  The HBM bound counts four input tables, two gradient
tables, the labels and the float64 row terms (written, then read) at 6.3 TB/s, about what streaming kernels sustain of the 8 TB/s peak.

Step workload: a CorrespondenceAutoencoder 280 -> 500 x 2 -> 100 -> 500 x 2 -> 280 (sigmoid, no BatchNorm, no dropout) at 4096
pairs through TrainerCorrespondence.train_step (Adadelta), against the same modules as plain torch on the GPU with
torch.optim.Adadelta and torch_loss.

python tools/cae_time.py [--out FILE]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np

from gmm_time import median_ms

HBM_ACHIEVABLE = 6.3e12
INFINITY_CACHE = 256 << 20
MAX_SETS = 64


def loss_bytes(B, D, grad):
    return (6 if grad else 4) * B * D * 4 + B * 8 + 2 * B * 8


def graph_us_per_call(fn, sets):
    """fn(set) captured once per set into one graph; the median replay over len(sets), in microseconds per call."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in sets:
            fn(s)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph, keep = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph):
        for s in sets:
            keep.append(fn(s))
    t = median_ms(graph.replay)
    return {k.replace('_ms', '_us_per_call'): round(v * 1e3 / len(sets), 3) for k, v in t.items()}


def loss_workload(B, D):
    import torch
    import cae_np
    from abnet3_amd.loss import CorrespondenceLoss
    n_sets = int(min(MAX_SETS, max(2, -(-int(1.2 * INFINITY_CACHE) // loss_bytes(B, D, True)))))
    sets = []
    for k in range(n_sets):
        r1, r2, x1, x2, y = cae_np.draw(np.random.default_rng(k), B, D, labels=(1, -1))
        sets.append(tuple(torch.from_numpy(a).cuda() for a in (r1, r2, x1, x2, y)))
    f = CorrespondenceLoss(avg=True, symmetric=True)
    hold, turn = {}, [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % n_sets]

    def fused():
        hold['f'] = f.value_and_grad(*nxt())

    def fused_value():
        with torch.no_grad():
            hold['fv'] = f(*nxt())

    leaves = [(s[0].clone().requires_grad_(True), s[1].clone().requires_grad_(True)) + s[2:] for s in sets]

    def torch_route():
        turn[0] += 1
        a, b, x1, x2, y = leaves[turn[0] % n_sets]
        a.grad = b.grad = None
        loss = cae_np.torch_loss(a, b, x1, x2, y, 'correspondence', True, True)
        loss.backward()
        hold['t'] = loss

    def torch_value():
        with torch.no_grad():
            hold['tv'] = cae_np.torch_loss(*nxt(), 'correspondence', True, True)

    res = {'B': B, 'D': D, 'input_sets': n_sets, 'bytes_value_and_gradients': loss_bytes(B, D, True), 'bytes_value_only': loss_bytes(B, D, False),
           'streams_from_hbm': bool(n_sets * loss_bytes(B, D, True) > INFINITY_CACHE)}
    res['cache_resident'] = not res['streams_from_hbm']
    res['call'] = {'fused': median_ms(fused), 'torch_route': median_ms(torch_route), 'fused_value': median_ms(fused_value),
                   'torch_value': median_ms(torch_value), 'fused_again': median_ms(fused)}
    res['call']['speedup_over_torch'] = round(res['call']['torch_route']['median_ms'] / res['call']['fused']['median_ms'], 3)
    res['call']['value_speedup_over_torch'] = round(res['call']['torch_value']['median_ms'] / res['call']['fused_value']['median_ms'], 3)
    g = res['graph'] = {'fused': graph_us_per_call(lambda s: f.value_and_grad(*s), sets)}
    with torch.no_grad():
        g['fused_value'] = graph_us_per_call(lambda s: f(*s), sets)
    for key, grad in (('fused', True), ('fused_value', False)):
        bound_us = loss_bytes(B, D, grad) / HBM_ACHIEVABLE * 1e6
        g[key]['hbm_bound_us'] = round(bound_us, 3)
        g[key]['fraction_of_hbm_bound'] = round(bound_us / g[key]['median_us_per_call'], 4)
    # agreement of the two routes on the first set
    val, dr = f.value_and_grad(*sets[0])
    a, b, x1, x2, y = leaves[0]
    a.grad = b.grad = None
    want = cae_np.torch_loss(a, b, x1, x2, y, 'correspondence', True, True)
    want.backward()
    res['agreement'] = {'loss_fused': float(val), 'loss_torch': float(want.detach()),
                        'max_abs_gradient_difference': float(max((dr[0] - a.grad).abs().max(), (dr[1] - b.grad).abs().max())),
                        'max_abs_gradient': float(max(a.grad.abs().max(), b.grad.abs().max()))}
    return res


def step_workload(B=4096):
    import torch
    import cae_np
    from abnet3_amd.loss import CorrespondenceLoss
    from abnet3_amd.model import CorrespondenceAutoencoder
    from abnet3_amd.trainer import TrainerCorrespondence
    torch.manual_seed(0)
    kw = dict(input_dim=280, num_hidden_layers=1, hidden_dim=500, output_dim=100, num_decoder_layers=2, p_dropout=0.0, activation_layer='sigmoid')
    net = CorrespondenceAutoencoder(output_path='/tmp/abn_cae_time', **kw)
    names = ('input_emb', 'hidden_layers', 'output_layer', 'decoder_layers', 'recon_layer')
    plain = torch.nn.Sequential(*[copy.deepcopy(getattr(net, n)) for n in names]).cuda()      # the same modules, torch's kernels
    plain.train()
    opt = torch.optim.Adadelta(plain.parameters(), lr=1.0)
    tr = TrainerCorrespondence(network=net, loss=CorrespondenceLoss(), optimizer_type='adadelta', lr=1.0, dataloader=None,
                               log_dir='/tmp/abn_cae_time_runs')
    net.train()
    rng = np.random.default_rng(0)
    x1 = rng.standard_normal((B, 280)).astype(np.float32)
    x2 = (x1 + 0.3 * rng.standard_normal(x1.shape)).astype(np.float32)
    batch = (torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda(), torch.from_numpy(np.where(np.arange(B) % 2, 1, -1).astype(np.int64)).cuda())
    hold = {}

    def hip_step():
        hold['h'] = tr.train_step(batch, True)

    def torch_step():
        a, b, y = batch
        loss = cae_np.torch_loss(plain(a), plain(b), a, b, y, 'correspondence', True, True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        hold['t'] = loss.detach()

    res = {'pairs': B, 'network': '280 -> 500 x 2 -> 100 -> 500 x 2 -> 280, sigmoid', 'optimizer': 'adadelta',
           'first_loss_hip': float(tr.train_step(batch, False)), 'precision': net.precision}
    with torch.no_grad():
        a, b, y = batch
        res['first_loss_torch'] = float(cae_np.torch_loss(plain(a), plain(b), a, b, y, 'correspondence', True, True))
    res['trainer_step'] = median_ms(hip_step)
    res['torch_step'] = median_ms(torch_step)
    res['trainer_step_again'] = median_ms(hip_step)
    res['speedup_over_torch'] = round(res['torch_step']['median_ms'] / res['trainer_step']['median_ms'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cae_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'hbm_achievable_bytes_per_s': HBM_ACHIEVABLE,
           'loss': [loss_workload(486, 280), loss_workload(4096, 280), loss_workload(4096, 40)], 'step': step_workload()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
