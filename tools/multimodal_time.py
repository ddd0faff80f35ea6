"""Times the multimodal network on the device, in one process:
  train step   MultimodalSiameseNetwork (pre-nets [280, (500, 2)] and [100, (500, 2)], BiWeightedDeepLearnt
               ([[500, 1], [500, 1]]) in sum mode, post-net [500, 100], sigmoid), 4096 frame pairs, coscos2(avg=False),
               Adadelta(0.1), through MultimodalTrainer.train_step; the same model as plain torch modules (the
               reference's forward_once twice, torch ops for the integration and the loss) with torch.optim.Adadelta;
  kernels      abn_integrate_forward / abn_integrate_backward alone at R = 8192 rows (both towers), D = 500, K = 1,
               against their bytes: the forward reads x1, x2 and writes out (~49 MB), the backward reads g, x1, x2
               and writes dx1, dx2 (~82 MB).  The working set fits in the 256 MiB Infinity Cache, so a launch
               replayed back to back can beat the HBM bound: the ratio reported is against HBM bandwidth (8.0 TB/s
               peak, 6.29 TB/s measured copy), i.e. what the launch would cost from cold caches.
Every route settles the clock (untimed calls for 0.3 s), then 15 calls are timed one by one with events; the median is
reported; the kernels are also timed as 20 launches replayed from one hipGraph (the launch alone).
python tools/multimodal_time.py [--out FILE] [--only-step] (the latter: two steps behind a marker launch, for a trace)
python tools/multimodal_time.py --summarize-trace KERNEL_TRACE_CSV [--out FILE]: the steady step of such a trace
(rocprofv3 --kernel-trace of --only-step), launch by launch, as text"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn as nn

PAIRS, DA, DB, H, OUT = 4096, 280, 100, 500, 100
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


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


def batch():
    g = torch.Generator(device='cuda').manual_seed(20)
    X1 = [torch.randn(PAIRS, DA, device='cuda', generator=g), torch.randn(PAIRS, DB, device='cuda', generator=g)]
    X2 = [torch.randn(PAIRS, DA, device='cuda', generator=g), torch.randn(PAIRS, DB, device='cuda', generator=g)]
    y = torch.randint(0, 2, (PAIRS,), device='cuda', generator=g) * 2 - 1
    return X1, X2, y


def make_net():
    from abnet3_amd.integration import BiWeightedDeepLearnt
    from abnet3_amd.model import MultimodalSiameseNetwork
    torch.manual_seed(2)
    np.random.seed(2)
    unit = BiWeightedDeepLearnt(net_params=[[H, 1], [H, 1]], integration_mode='sum')
    return MultimodalSiameseNetwork(integration_unit=unit, pre_integration_net_params=[[DA, (H, 2)], [DB, (H, 2)]],
                                    post_integration_net_params=[H, OUT], activation_layer='sigmoid',
                                    output_path='/tmp/abn_mm_time')


def port_step():
    from abnet3_amd.dataloader import MultimodalDataLoader
    from abnet3_amd.loss import coscos2
    from abnet3_amd.trainer import MultimodalTrainer
    net = make_net().cuda()
    tr = MultimodalTrainer(network=net, loss=coscos2(avg=False), optimizer_type='adadelta', lr=0.1,
                           dataloader=MultimodalDataLoader('unused', ['a', 'b']), log_dir='/tmp/abn_runs')
    b = batch()
    net.train()
    return lambda: tr.train_step(b, True)


class TorchModel(nn.Module):
    """The reference's arithmetic as plain torch modules on the GPU (abnet3/model.py:529-570, integration.py:432-442)."""

    def __init__(self, port):
        super().__init__()
        def seq(s):
            layers = []
            for m in s:
                if isinstance(m, nn.Linear):
                    layers.append(nn.Linear(m.in_features, m.out_features))
                elif isinstance(m, nn.Dropout):
                    layers.append(nn.Identity())          # (p_dropout = 0)
                else:
                    layers.append(type(m)())
            out = nn.Sequential(*layers)
            out.load_state_dict(s.state_dict())
            return out
        self.pre = nn.ModuleList([seq(p) for p in port.pre_nets])
        self.post = seq(port.post_net)
        self.att1, self.att2 = seq(port.integration_unit.linear1), seq(port.integration_unit.linear2)

    def forward_once(self, xs):
        h = [p(x) for p, x in zip(self.pre, xs)]
        w = torch.sigmoid(torch.add(self.att1(h[0]), self.att2(h[1])))
        wc = torch.add(torch.mul(w, -1), 1)
        return self.post(torch.add(torch.mul(h[0], w), torch.mul(h[1], wc)))


def torch_coscos2(e1, e2, y):
    cos = nn.functional.cosine_similarity(e1, e2, dim=1, eps=1e-6)
    return torch.where(y == 1, (1 - cos) / 2, cos * cos).sum()


def torch_step():
    model = TorchModel(make_net()).cuda()
    opt = torch.optim.Adadelta(model.parameters(), lr=0.1)
    X1, X2, y = batch()

    def step():
        e1, e2 = model.forward_once(X1), model.forward_once(X2)
        lv = torch_coscos2(e1, e2, y)
        opt.zero_grad()
        lv.backward()
        opt.step()
        return lv.detach()
    return step


def kernel_routes(res, R=2 * PAIRS, D=H):
    from abnet3_amd import _lib
    from abnet3_amd.loss import _scratch
    lib = _lib.load()
    g = torch.Generator(device='cuda').manual_seed(0)
    x1, x2 = torch.randn(R, D, device='cuda', generator=g), torch.randn(R, D, device='cuda', generator=g)
    z1, z2 = torch.randn(R, 1, device='cuda', generator=g), torch.randn(R, 1, device='cuda', generator=g)
    gr = torch.randn(R, D, device='cuda', generator=g)
    out, w = torch.empty(R, D, device='cuda'), torch.empty(R, 1, device='cuda')
    dx1, dx2, dz = torch.empty_like(x1), torch.empty_like(x2), torch.empty(R, 1, device='cuda')
    ws = _scratch(lib.abn_integrate_ws_bytes(R), x1.device)
    sig, att = _lib.ACT['sigmoid'], _lib.W_ATTENTION

    def fwd():
        _lib.check(lib.abn_integrate_forward(_lib.ptr(x1), D, _lib.ptr(x2), D, R, 0, att, 0.0, 0.0, None, _lib.ptr(z1),
                                             _lib.ptr(z2), 1, sig, _lib.ptr(out), _lib.ptr(w), _lib.stream()), 'fwd')

    def bwd():
        _lib.check(lib.abn_integrate_backward(_lib.ptr(x1), D, _lib.ptr(x2), D, R, 0, att, 0.0, 0.0, None, _lib.ptr(w), 1,
                                              sig, _lib.ptr(gr), _lib.ptr(dx1), _lib.ptr(dx2), _lib.ptr(dz), None,
                                              _lib.ptr(ws), _lib.stream()), 'bwd')
    fwd()
    bytes_ = {'forward': 3 * R * D * 4 + 3 * R * 4, 'backward': 5 * R * D * 4 + 2 * R * 4}
    out_ = res['kernel'] = {'R': R, 'D': D, 'K': 1, 'mode': 'sum', 'act': 'sigmoid',
                            'median_us_is': 'one call from Python (ctypes, launch) timed with events',
                            'graph20_us_is': 'the launch ALONE: 20 calls captured into one hipGraph, the replay timed, / 20',
                            'bound_is': 'bytes / HBM bandwidth (8.0 TB/s peak; 6.29 TB/s measured copy); the working set '
                                        'fits in the 256 MiB Infinity Cache, so replays back to back may beat it'}
    for name, fn in (('forward', fwd), ('backward', bwd)):
        ms, all_ms = median_ms(fn)
        r = out_[name] = {'bytes': bytes_[name], 'median_us': round(ms * 1e3, 2), 'calls_ms': all_ms}
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(20):
                fn()
        ms, _ = median_ms(graph.replay)
        r['graph20_us'] = round(ms * 1e3 / 20, 2)
        r['GB_per_s_graph20'] = round(bytes_[name] / (r['graph20_us'] * 1e-6) / 1e9, 1)
        r['hbm_peak_bound_us'] = round(bytes_[name] / HBM_PEAK * 1e6, 2)
        r['hbm_copy_bound_us'] = round(bytes_[name] / HBM_COPY * 1e6, 2)
        r['of_hbm_peak'] = round(r['hbm_peak_bound_us'] / r['graph20_us'], 3)


def summarize_trace(path):
    """The launches behind the last marker (arange) of a --only-step kernel trace: one steady train step."""
    import csv
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    marks = [i for i, r in enumerate(rows) if 'arange' in r['Kernel_Name']]
    step = rows[marks[-1] + 1:]
    t0, t1 = int(step[0]['Start_Timestamp']), max(int(r['End_Timestamp']) for r in step)
    busy = sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in step)
    lines = ['# One steady multimodal train step (MultimodalTrainer.train_step, Adadelta 0.1), rocprofv3 --kernel-trace',
             '# python tools/multimodal_time.py --only-step: a first step, a marker launch (arange), then the step listed here.',
             '# pre-nets [280,(500,2)] + [100,(500,2)], BiWeightedDeepLearnt([[500,1],[500,1]]) sum, post-net [500,100],',
             '# sigmoid, 4096 frame pairs, coscos2(avg=False), no BatchNorm, p_dropout 0.', '',
             '%d launches, first start to last end %.1f us, kernels busy %.1f us' % (len(step), (t1 - t0) / 1e3, busy / 1e3), '']
    for r in step:
        name = r['Kernel_Name']
        name = name if len(name) <= 110 else name[:107] + '...'
        lines.append('%9.1f us  %7.1f us  %s' % ((int(r['Start_Timestamp']) - t0) / 1e3,
                                                 (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3, name))
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--only-step', action='store_true')
    ap.add_argument('--summarize-trace', default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        text = summarize_trace(a.summarize_trace)
        print(text, end='')
        if a.out:
            with open(a.out, 'w') as f:
                f.write(text)
        return
    if a.only_step:
        step = port_step()
        step()                                  # the first step (one-time buffers: scratch, optimizer state)
        torch.cuda.synchronize()
        torch.arange(7, device='cuda')          # a marker launch: the trace's launches behind it are ONE steady step
        torch.cuda.synchronize()
        step()
        torch.cuda.synchronize()
        return
    res = {'device': torch.cuda.get_device_name(), 'pairs': PAIRS,
           'model': 'pre [280,(500,2)] + [100,(500,2)], BiWeightedDeepLearnt([[500,1],[500,1]]) sum, post [500,100], '
                    'sigmoid, coscos2(avg=False), Adadelta(0.1)'}
    kernel_routes(res)
    st = res['train_step'] = {}
    for name, make in (('port', port_step), ('torch', torch_step)):
        ms, all_ms = median_ms(make())
        st[name] = {'median_us': round(ms * 1e3, 2), 'calls_ms': all_ms}
    st['torch_over_port'] = round(st['torch']['median_us'] / st['port']['median_us'], 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
