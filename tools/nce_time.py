"""Times abnt_nce_loss (abnet3_amd/csrc/nce.hip, InfoNCELoss) against the torch route on the same device and inputs.

Workloads: (B, D) = (486, 100) -- the mean batch of the word-pair loader --, (4096, 100) and (4096, 128), tau = 0.07, inputs
drawn around 8 prototypes as in tests/nce_np.py.  Timed, per workload, alternating in one process:

  fused             InfoNCELoss.value_and_grad: loss and both gradients, nine launches
  fused forward     the loss alone (seven launches), as the dev pass calls it
  torch route       tests/nce_np.py's torch_loss itself -- normalise, mm, two logsumexp -- and autograd's backward; it
                    materialises the B x B logits several times.  Never the new kernel.
  torch forward     torch_loss under no_grad

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls (tools/gmm_time.py's median_ms: device
events, one call per pair of events); medians, minima and maxima are reported.  Also: the workspace bytes against the
B^2 x 4 bytes of ONE logit matrix, the fraction of the fp32 matrix-core roof counting six 2 B^2 D products (two lse sweeps,
two recomputed tiles, two gradient GEMMs), the largest difference between the two routes' outputs, and for scale the C2
train step of BENCH_r06.json.

python tools/nce_time.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np

from gmm_time import FP32_MFMA_FLOPS, median_ms

TAU = 0.07


def c2_step_ms():
    try:
        with open(os.path.join(ROOT, 'BENCH_r06.json')) as fh:
            return json.load(fh)['parsed']['ms_per_step']
    except (OSError, KeyError, ValueError):
        return None


def workload(B, D):
    import torch
    import nce_np
    from abnet3_amd import _lib
    from abnet3_amd.loss import InfoNCELoss
    e1, e2 = nce_np.make_case(B, D)
    e1, e2 = torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda()
    y = torch.ones(B, dtype=torch.int64, device='cuda')
    f = InfoNCELoss(temperature=TAU)
    hold = {}

    def fused():
        hold['f'] = f.value_and_grad(e1, e2, y)

    def fused_forward():
        with torch.no_grad():
            hold['ff'] = f(e1, e2, y)

    t1, t2 = e1.clone().requires_grad_(True), e2.clone().requires_grad_(True)

    def torch_route():
        t1.grad = t2.grad = None
        loss = nce_np.torch_loss(t1, t2, y, TAU)
        loss.backward()
        hold['t'] = loss

    def torch_forward():
        with torch.no_grad():
            hold['tf'] = nce_np.torch_loss(e1, e2, y, TAU)

    flop = 6 * 2.0 * B * B * D
    res = {'B': B, 'D': D, 'tau': TAU, 'workspace_bytes': int(_lib.load().abnt_nce_ws_bytes(B, D)), 'one_logit_matrix_bytes': B * B * 4,
           'flop_of_six_products': flop}
    res['fused'] = median_ms(fused)
    res['torch_route'] = median_ms(torch_route)
    res['fused_forward'] = median_ms(fused_forward)
    res['torch_forward'] = median_ms(torch_forward)
    res['fused_again'] = median_ms(fused)                      # (alternating: the kernel once more)
    res['fused']['fraction_of_fp32_mfma_roof'] = round(flop / (res['fused']['median_ms'] * 1e-3) / FP32_MFMA_FLOPS, 4)
    res['speedup_over_torch'] = round(res['torch_route']['median_ms'] / res['fused']['median_ms'], 3)
    res['forward_speedup_over_torch'] = round(res['torch_forward']['median_ms'] / res['fused_forward']['median_ms'], 3)
    loss, de = hold['f']
    res['agreement'] = {'loss_fused': float(loss), 'loss_torch': float(hold['t']),
                        'max_abs_gradient_difference': float(max((de[0] - t1.grad).abs().max(), (de[1] - t2.grad).abs().max())),
                        'max_abs_gradient': float(max(t1.grad.abs().max(), t2.grad.abs().max()))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nce_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'fp32_mfma_roof_flops': FP32_MFMA_FLOPS,
           'c2_train_step_ms_of_BENCH_r06': c2_step_ms(),
           'workloads': [workload(486, 100), workload(4096, 100), workload(4096, 128)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
