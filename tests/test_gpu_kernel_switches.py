"""The non-default side of the library's A/B switches (include/abnet3_hip.h: "kernel choice only, never results beyond
fp32 summation order"): the DTW kernels behind ABN_DTW_PC / ABN_DTW_F40 and behind a misaligned feature table, bit for
bit against the oracle, and the launch geometries of the operand-plane weight gradients (ABN_WGRAD_TILE128,
ABN_WGRAD_XCD, ABN_WGRAD_ROWS_PER_SLAB), of the layer-per-launch kernels (ABN_WIDE_MAXG, ABN_WIDE) and ABN_FUSED
against the numpy oracle at the bars of tests/test_gpu_edge_cases.py.  Needs an MI355X: -m gpu."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err, check_grads

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# DTW: dtw_gang_kernel (default), dtw_fused_kernel<true, true> (ABN_DTW_PC=0), <true, false> (... and ABN_DTW_F40=0),
# <false, false> (a table that is not 16-byte aligned)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dtw_case():
    """60 pairs of 40-value frames, token lengths 1 .. 90, and what the oracle says about each (computed once):
    (path1, path2, cost), or None for a pair the reference drops."""
    from oracle import dtw_oracle as O
    rng = np.random.default_rng(40)
    P, D = 60, 40
    n1 = rng.integers(1, 91, P).astype(np.int32)
    n2 = rng.integers(1, 91, P).astype(np.int32)
    n1[:6] = [1, 1, 90, 64, 33, 90]
    n2[:6] = [1, 90, 1, 64, 90, 90]
    n1[6:10], n2[6:10] = [30, 25, 17, 40], [25, 30, 17, 9]
    o1 = np.concatenate(([0], np.cumsum(n1)[:-1])).astype(np.int64)
    o2 = np.concatenate(([0], np.cumsum(n2)[:-1])).astype(np.int64)
    f1 = rng.standard_normal((int(n1.sum()), D)).astype(np.float32)
    f2 = rng.standard_normal((int(n2.sum()), D)).astype(np.float32)
    for p in range(10, P):      # second token = time-warped copy of the first + noise (long diagonal runs)
        src = np.rint(np.linspace(0, n1[p] - 1, n2[p])).astype(int)
        f2[o2[p]:o2[p] + n2[p]] = f1[o1[p] + src] + 0.1 * f2[o2[p]:o2[p] + n2[p]]
    # ties: a constant token against a random one (every row of the distance matrix is the same row) and constant
    # against constant (one value in every cell)
    f1[o1[6]:o1[6] + n1[6]] = f1[o1[6]]
    f1[o1[7]:o1[7] + n1[7]] = f1[o1[7]]
    f2[o2[7]:o2[7] + n2[7]] = f2[o2[7]]
    # a dropped pair: a token against itself -- the cosine of a frame with itself rounds above 1 for some frames, its
    # arccos is NaN and the reference drops the pair (abnet3/utils.py:59, abnet3/dataloader.py:188-191)
    f2[o2[8]:o2[8] + n2[8]] = f1[o1[8]:o1[8] + n1[8]]
    # a zero-norm frame in the middle of token 1 is NOT a drop: the reference sets those distances to 1
    # (abnet3/utils.py:55-56), which ties a whole row
    f1[o1[9] + 20] = 0.0
    ref = []
    for p in range(P):
        a, b = f1[o1[p]:o1[p] + n1[p]], f2[o2[p]:o2[p] + n2[p]]
        try:
            d = O.cosine_distance(a, b)
        except AssertionError:
            ref.append(None)
            continue
        ref.append(O.dtw_path(d) + (O.dtw_cost(d),))
    assert [p for p in range(P) if ref[p] is None] == [8]
    return f1, o1, n1, f2, o2, n2, ref


def off_a_16_byte_boundary(a):
    """The same [rows, D] table as a contiguous view that starts one float behind a 16-byte boundary."""
    big = torch.zeros(a.size + 8, dtype=torch.float32, device='cuda')
    view = big[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize('setting', ['default', 'pc0', 'pc0_f40_0', 'misaligned'])
def test_dtw_kernel_choice_is_bit_exact_vs_oracle(setting, monkeypatch):
    from abnet3_amd.utils import dtw_align_batch
    if setting in ('pc0', 'pc0_f40_0'):
        monkeypatch.setenv('ABN_DTW_PC', '0')
    if setting == 'pc0_f40_0':
        monkeypatch.setenv('ABN_DTW_F40', '0')
    f1, o1, n1, f2, o2, n2, ref = dtw_case()
    if setting == 'misaligned':
        d1, d2 = off_a_16_byte_boundary(f1), off_a_16_byte_boundary(f2)
    else:
        d1, d2 = dev(f1), dev(f2)
        assert d1.data_ptr() % 16 == 0 and d2.data_ptr() % 16 == 0
    res = dtw_align_batch(d1, o1, n1, d2, o2, n2)
    got = res.to_lists()
    plen = res.path_len.cpu().numpy()
    cost = res.total_cost.cpu().numpy()
    for p in range(len(n1)):
        if ref[p] is None:
            assert got[p] is None and plen[p] == 0 and cost[p] == 0.0, p
            continue
        p1, p2, c = ref[p]
        assert plen[p] == len(p1), p
        assert (got[p][0] == p1).all() and (got[p][1] == p2).all(), p
        assert cost[p] == c, p                              # float64 recurrence: bit-exact too


# ---------------------------------------------------------------------------------------------------------------------
# operand-plane launch geometry
# ---------------------------------------------------------------------------------------------------------------------
DIMS = (40, 96, 200, 32)
PATH_PER_LAYER, PATH_BN_LAYERS, PATH_WIDE = 0, 5, 6


def build_tower(batch_norm, precision, seed):
    """A sigmoid SiameseNetwork of 40 -> 96 -> 200 -> 32 (the class takes ONE hidden width: the second and third Linear
    are replaced before anything looks at them -- the HIP plumbing reads its layers from the modules), the oracle's
    description of it and its parameters."""
    from abnet3_amd.model import SiameseNetwork
    from oracle import siamese_np as O
    from torch import nn
    torch.manual_seed(seed)
    net = SiameseNetwork(input_dim=DIMS[0], num_hidden_layers=1, hidden_dim=DIMS[1], output_dim=DIMS[3], p_dropout=0.0,
                         batch_norm=batch_norm, activation_layer='sigmoid')
    net.hidden_layers[0] = nn.Linear(DIMS[1], DIMS[2])
    net.output_layer[0] = nn.Linear(DIMS[2], DIMS[3])
    if batch_norm:
        net.hidden_layers[2] = nn.BatchNorm1d(DIMS[2])
    net.apply(net.init_weight_method)
    with torch.no_grad():       # (the class zeroes its biases; BatchNorm starts at gamma = 1, beta = 0: make every term count)
        for k, q in net.named_parameters():
            if q.dim() == 1:
                q.add_(0.1 * torch.randn_like(q))
    net._init_hip_state()
    net = net.cuda()
    net.precision = precision
    spec = O.TowerSpec(DIMS[0], 1, DIMS[1], DIMS[3], 'sigmoid', batch_norm)
    spec.dims = list(DIMS)
    p = {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}
    assert [tuple(p[k + '.weight'].shape) for k in spec.lin_keys] == [(DIMS[l + 1], DIMS[l]) for l in range(3)]
    return net, spec, p


def run_tower(batch_norm, precision, B, seed, path, path_precision=None):
    """tests/test_gpu_edge_cases.py:run_case on the tower above: forward, loss and every gradient against the oracle
    (embeddings and loss 1e-5, check_grads at 1e-4), and the kernel family both directions took."""
    import abnet3_amd.loss as L
    from abnet3_amd import _lib
    from oracle import siamese_np as O
    tol = 1e-5
    net, spec, p = build_tower(batch_norm, precision, seed)
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal((B, DIMS[0])).astype(np.float32)
    x2 = rng.standard_normal((B, DIMS[0])).astype(np.float32)
    y = rng.choice([1, -1], B)
    net.train()
    e1, e2 = net(dev(x1), dev(x2))
    assert _lib.last_forward_path() == path, _lib.last_path
    if path_precision is not None:
        assert _lib.last_path['forward_precision'] == _lib.PRECISION[path_precision], _lib.last_path
    lv = L.coscos2(avg=False)(e1, e2, dev(y))
    lv.backward()
    assert _lib.last_backward_path() == path, _lib.last_path
    o1, c1 = O.tower_forward(p, x1, spec, True)
    o2, c2 = O.tower_forward(p, x2, spec, True)
    ol, d1, d2, _ = O.pair_loss(o1, o2, y, 'coscos2', 0.5, False)
    og = {}
    O.tower_backward(p, c1, d1, spec, og)
    O.tower_backward(p, c2, d2, spec, og)
    errs = (rel_err(e1.detach().cpu().numpy(), o1), rel_err(e2.detach().cpu().numpy(), o2))
    print('embeddings: rel_err %.3g %.3g, loss %.9g (oracle %.9g)' % (errs + (float(lv.detach()), ol)))
    assert errs[0] < tol and errs[1] < tol
    assert abs(float(lv.detach()) - ol) <= tol * abs(ol) + 1e-6
    grads = {k: q.grad.cpu().numpy() for k, q in net.named_parameters()}
    check_grads(grads, og, spec.param_keys(), spec.batch_norm, tol=1e-4)
    net.eval()
    with torch.no_grad():
        ev = net.forward_once(dev(x1))
    oe, _ = O.tower_forward(p, x1, spec, False)
    assert rel_err(ev.cpu().numpy(), oe) < tol


# 100 pairs = 200 tower rows: the layer-per-launch kernels (ABN_PATH_WIDE) by default; without them (ABN_WIDE=0) or
# without the operand planes' launches altogether (ABN_FUSED=0) a batch of fewer than 256 rows goes to the per-layer
# GEMMs, which compute 'f16x2' as bf16 x 3.
GEOMETRIES = [
    ({'ABN_WGRAD_TILE128': '1'}, PATH_WIDE),
    ({'ABN_WGRAD_TILE128': '0'}, PATH_WIDE),
    ({'ABN_WGRAD_XCD': '0'}, PATH_WIDE),
    ({'ABN_WGRAD_ROWS_PER_SLAB': '32'}, PATH_WIDE),
    ({'ABN_WIDE_MAXG': '1'}, PATH_WIDE),
    ({'ABN_WIDE_MAXG': '2'}, PATH_WIDE),
    ({'ABN_WIDE': '0'}, PATH_PER_LAYER),
    ({'ABN_FUSED': '0'}, PATH_PER_LAYER),
    ({'ABN_WGRAD_TILE128': '1', 'ABN_WGRAD_ROWS_PER_SLAB': '32', 'ABN_WGRAD_XCD': '0'}, PATH_WIDE),
]


def env_id(v):
    return '-'.join('%s=%s' % (k[4:], v[k]) for k in sorted(v)) if isinstance(v, dict) else str(v)


@pytest.mark.parametrize('env,path', GEOMETRIES, ids=env_id)
def test_tower_under_a_launch_geometry_switch(env, path, split, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_tower(False, split, B=100, seed=11, path=path, path_precision='bf16x3' if path == PATH_PER_LAYER else split)


@pytest.mark.parametrize('env', [{'ABN_WGRAD_TILE128': '1'}, {'ABN_WGRAD_ROWS_PER_SLAB': '32'}], ids=env_id)
def test_batch_norm_tower_under_a_weight_gradient_switch(env, split, monkeypatch):
    """300 pairs through the BatchNorm layer launches (ABN_BN_PERSIST=0 keeps the resident tower out)."""
    monkeypatch.setenv('ABN_BN_PERSIST', '0')
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_tower(True, split, B=300, seed=12, path=PATH_BN_LAYERS, path_precision=split)
