"""Every library entry on dirty memory.  Almost every call site of abnet3_amd/*.py hands the kernels memory from torch.empty
(outputs, split-K scratch, forward workspaces, chain workspaces, back-pointer workspaces) and assumes that the entry writes
everything it later reads or returns.  Here each case runs three times, with torch.empty / torch.empty_like returning memory
of 0x00, 0xFF (NaN / -1) and 0xC2 (a plausible -97.38 / a negative int) bytes (tests/dirty_memory.py), and

  * the window poisoned at least one allocation (a wrapper that caches a workspace builds it inside the window),
  * the entries the case claims were called (dirty_memory.recorded),
  * every output has the same bits in the three runs, where the header or DESIGN.md promises the same bits for the same
    call (`same_bits`; a case without that promise says so and holds each run to the oracle bar instead),
  * the family's existing oracle, at that family's existing bar, passes on the 0xFF run,
  * a tower case took the kernel family it names (_lib.last_forward_path() / last_backward_path()).

No new tolerance is introduced: every bar below is the one of the test module named beside it.

Module-level caches of torch.empty memory in abnet3_amd (grep "_cache|_WS|_UNIT|torch.empty" over abnet3_amd/*.py), cleared
before every window:
  utils._DtwScratch._cache      the grow-only DTW workspace + pinned staging buffer, per (device, stream)
(loss._WS and loss._UNIT are torch.zeros / torch.ones memory: the header wants the ticket word zero.  Per-object
workspaces -- kmeans.LloydState.ws, gmm.EMState.ws, FeaturesGenerator._tables, a network's descriptor and gradient
buffers -- live in objects the cases build afresh inside the window.)

The ledger of tests/test_dirty_memory_host.py holds every key of _lib.SYMBOLS to a case here, to QUERIES or to EXCLUDED.
Needs an MI355X: -m gpu.  Measured on an MI355X: the whole file, three patterns, takes 6 s (89 tests; no case above 1 s)."""
import ctypes

import numpy as np
import pytest

import dirty_memory
from dirty_memory import bits, dirty, recorded

pytestmark = pytest.mark.gpu

_BUILT = {}            # case name -> inputs (made once, outside the window, never written to)


class Case(object):
    """build() -> inputs (outside the window); run(inputs) -> {name: numpy array} through the wrapper the users call;
    oracle(inputs, outputs): the family's reference check; entries: what the case claims to reach; env: library switches;
    paths: (forward, backward) kernel family of a tower case; same_bits=False: no promise of equal bits between calls."""

    def __init__(self, name, entries, build, run, oracle, env=None, paths=None, same_bits=True):
        self.name, self.entries, self.build, self.run, self.oracle = name, tuple(entries), build, run, oracle
        self.env, self.paths, self.same_bits = dict(env or {}), paths, same_bits

    def inputs(self):
        if self.name not in _BUILT:
            _BUILT[self.name] = self.build()
        return _BUILT[self.name]


def dev(a, dt=None):
    import torch
    a = np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))
    return torch.from_numpy(a).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


def clear_caches():
    from abnet3_amd import utils
    utils.release_dtw_scratch()


def run_dirty(case, byte):
    """One run of the case inside a window of `byte`: (outputs, poisoned allocations, entries called)."""
    import torch
    from abnet3_amd import _lib
    clear_caches()
    assert not torch.cuda.is_current_stream_capturing()
    with recorded(_lib.load()) as calls:
        with dirty(byte) as count:
            out = case.run(case.inputs())
            torch.cuda.synchronize()
    return {k: np.asarray(v, order='C') for k, v in out.items()}, count, calls


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        same = bits(a[k]) == bits(b[k])
        assert same.all(), '%s: output %r differs in %d of %d elements (first at %s)' % (
            what, k, (~same).sum(), same.size, np.argwhere(~same)[0] if same.ndim else ())


# ======================================================================================================================
# the tower
# ======================================================================================================================
P_PER_LAYER, P_FUSED, P_PLANES, P_BN_LAYERS, P_WIDE, P_BN_TOWER = 0, 1, 2, 5, 6, 7


def tower_case(name, kw, B, seed, paths, env=None, precision=None, loss=('coscos2', False, 0.5), shape=None,
               tols=(1e-5, 1e-4, 1e-5), loss_mult=1, entries=()):
    """tests/test_gpu_edge_cases.py:run_case, with an SGD step at its end (tests/test_gpu_planned_steps.py's check_params at
    1e-5): both embeddings, loss, every gradient, eval embeddings, parameters after the step.  The network is rebuilt from
    the same seed in every run; dropout 0.  `shape` = tests/test_gpu_kernel_switches.py:DIMS replaces the hidden Linears."""
    tol, gtol, ptol = tols

    def make_net():
        import torch
        from abnet3_amd.model import SiameseNetwork
        if shape is not None:
            import test_gpu_kernel_switches as KS
            assert tuple(shape) == KS.DIMS
            net, _, _ = KS.build_tower(kw.get('batch_norm', False), precision, seed)
            return net
        torch.manual_seed(seed)
        net = SiameseNetwork(p_dropout=0.0, **kw).cuda()
        if precision is not None:
            net.precision = precision
        return net

    def spec_of():
        from oracle import siamese_np as O
        spec = O.TowerSpec(kw['input_dim'], kw['num_hidden_layers'], kw['hidden_dim'], kw['output_dim'], kw['activation_layer'],
                           kw.get('batch_norm', False), kw.get('last_non_linearity', 'default'))
        if shape is not None:
            spec.dims = list(shape)
        return spec

    def build():
        rng = np.random.default_rng(seed)
        d = kw['input_dim']
        return dict(x1=rng.standard_normal((B, d)).astype(np.float32), x2=rng.standard_normal((B, d)).astype(np.float32),
                    y=rng.choice([1, -1], B))

    def run(inp):
        import torch
        import abnet3_amd.loss as L
        from abnet3_amd import _lib
        from abnet3_amd.trainer import FlatOptimizer
        net = make_net()
        out = {'p0.' + k: host(v) for k, v in net.state_dict().items()}
        x1, x2, y = dev(inp['x1']), dev(inp['x2']), dev(inp['y'])
        net.train()
        e1, e2 = net(x1, x2)
        fwd = _lib.last_forward_path()
        lf = getattr(L, loss[0])(avg=loss[1], margin=loss[2]) if loss[0] == 'cosmargin' else getattr(L, loss[0])(avg=loss[1])
        lv = lf(e1, e2, y)
        lv.backward()
        bwd = _lib.last_backward_path()
        assert (fwd, bwd) == tuple(paths), (_lib.last_path, paths)
        out.update(e1=host(e1), e2=host(e2), loss=host(lv))
        for k, q in net.named_parameters():
            out['g.' + k] = host(q.grad)
        p1 = {k: host(v) for k, v in net.state_dict().items()}      # (a BatchNorm tower moved its running statistics)
        net.eval()
        with torch.no_grad():
            out['eval'] = host(net.forward_once(x1))
        net.train()
        FlatOptimizer(net, 'sgd', 0.01, 0.9).step()
        for k, v in net.state_dict().items():
            out['p1.' + k] = host(v)
        out.update({'pe.' + k: v for k, v in p1.items()})
        return out

    def oracle(inp, out):
        from conftest import check_grads, check_params, rel_err
        from oracle import siamese_np as O
        spec = spec_of()
        p = {k[3:]: v.copy() for k, v in out.items() if k.startswith('p0.')}
        x1, x2, y = inp['x1'], inp['x2'], inp['y']
        o1, c1 = O.tower_forward(p, x1, spec, True)
        o2, c2 = O.tower_forward(p, x2, spec, True)
        ol, d1, d2, _ = O.pair_loss(o1, o2, y, loss[0], loss[2], loss[1])
        og = {}
        O.tower_backward(p, c1, d1, spec, og)
        O.tower_backward(p, c2, d2, spec, og)
        assert rel_err(out['e1'], o1) < tol and rel_err(out['e2'], o2) < tol, (rel_err(out['e1'], o1), rel_err(out['e2'], o2))
        assert abs(float(out['loss']) - ol) <= loss_mult * tol * abs(ol) + 1e-6, (float(out['loss']), ol)
        keys = spec.param_keys()
        check_grads({k: out['g.' + k] for k in keys}, og, keys, spec.batch_norm, tol=gtol)
        oe, _ = O.tower_forward(p, x1, spec, False)                   # (p holds the running statistics after the two calls)
        assert rel_err(out['eval'], oe) < tol, rel_err(out['eval'], oe)
        O.Optimizer('sgd', 0.01).step(p, og, keys)
        check_params({k: out['p1.' + k] for k in keys}, p, keys, spec.batch_norm, ptol)

    ent = ('abn_tower_forward', 'abn_tower_backward', 'abn_tower_ws_floats', 'abn_tower_out_offset', 'abn_tower_bwd_scratch_floats',
           'abn_tower_path', 'abn_pair_loss', 'abn_optimizer_step') + tuple(entries)
    return Case(name, ent, build, run, oracle, env=env, paths=paths)


ODD = dict(input_dim=39, num_hidden_layers=1, hidden_dim=50, output_dim=7, activation_layer='sigmoid')
TANH = dict(input_dim=40, num_hidden_layers=1, hidden_dim=72, output_dim=36, activation_layer='tanh', batch_norm=False)
WIDE_KW = dict(input_dim=40, num_hidden_layers=1, hidden_dim=96, output_dim=32, activation_layer='sigmoid')
WIDE_DIMS = (40, 96, 200, 32)
PLANES_ENV = {'ABN_FUSED_MIN_ROWS': '0', 'ABN_PLANES': '1', 'ABN_WIDE': '0'}       # tests/test_gpu_planes.py:planes_forced

TOWER_CASES = [
    # tests/test_gpu_edge_cases.py:test_odd_widths_and_ragged_rows: nothing is a multiple of 4, 33 rows per tower
    tower_case('tower-per-layer', dict(ODD, batch_norm=False), 33, 1, (P_PER_LAYER, P_PER_LAYER)),
    tower_case('tower-per-layer-bn', dict(ODD, batch_norm=True), 33, 1, (P_PER_LAYER, P_PER_LAYER)),
]


def _add_tower_cases():
    # tests/test_gpu_edge_cases.py:test_row_counts_around_tile_edges[65-fused], in the exact-fp32 arithmetic (the fused
    # fp32 forward: the split arithmetics' fused forward is the operand planes' below)
    TOWER_CASES.append(tower_case('tower-fused-fp32', TANH, 65, 65, (P_FUSED, P_PER_LAYER), env={'ABN_FUSED_MIN_ROWS': '0', 'ABNET3_PRECISION': 'fp32'},
                                  loss=('cosmargin', True, 0.5)))
    for split in ('bf16x3', 'f16x2'):
        # tests/test_gpu_kernel_switches.py:test_tower_under_a_launch_geometry_switch (B = 100: 200 rows, ragged 32-row groups)
        TOWER_CASES.append(tower_case('tower-wide-' + split, WIDE_KW, 100, 11, (P_WIDE, P_WIDE), precision=split, shape=WIDE_DIMS))
        TOWER_CASES.append(tower_case('tower-wide-slab32-' + split, WIDE_KW, 100, 11, (P_WIDE, P_WIDE), precision=split, shape=WIDE_DIMS,
                                      env={'ABN_WGRAD_ROWS_PER_SLAB': '32'}))
        # tests/test_gpu_planes.py:SHAPES: (4, 0, 8, 4, B = 5), the smallest batch (and tower) that file sends down the operand
        # planes, and (32, 1, 64, 32, B = 33), its smallest with a ragged second workgroup; that file's bars (embeddings 1e-5,
        # loss 10 x 1e-5, gradients 1e-4)
        for d_in, nh, hid, d_out, B in ((4, 0, 8, 4, 5), (32, 1, 64, 32, 33)):
            TOWER_CASES.append(tower_case('tower-planes-B%d-%s' % (B, split), dict(input_dim=d_in, num_hidden_layers=nh, hidden_dim=hid,
                                                                                  output_dim=d_out, activation_layer='sigmoid', batch_norm=False),
                                          B, B, (P_PLANES, P_PLANES), env=PLANES_ENV, precision=split, loss_mult=10))
        # tests/test_gpu_kernel_switches.py:test_batch_norm_tower_under_a_weight_gradient_switch without its switch
        TOWER_CASES.append(tower_case('tower-bn-layers-' + split, dict(WIDE_KW, batch_norm=True), 300, 12, (P_BN_LAYERS, P_BN_LAYERS),
                                      precision=split, shape=WIDE_DIMS, env={'ABN_BN_PERSIST': '0'}))


_add_tower_cases()


def bn_tower_case(split):
    """tests/test_gpu_bn_tower.py:test_resident_tower_against_the_oracle on its smallest tower, (4, 0, 8, 4, B = 128), p_drop 0:
    the float64 yardstick of that test and its bars -- embeddings and loss max(1e-5, 2 x the float32 oracle's own error),
    running statistics 1e-5, gradients check_grads at max(2e-5, 2 x float32's)."""
    d_in, nh, hid, d_out, B = 4, 0, 8, 4, 128
    kw = dict(input_dim=d_in, num_hidden_layers=nh, hidden_dim=hid, output_dim=d_out, activation_layer='sigmoid', p_dropout=0.0,
              batch_norm=True)

    def build():
        rng = np.random.default_rng(B + nh)
        return dict(x1=rng.standard_normal((B, d_in)).astype(np.float32), x2=(rng.standard_normal((B, d_in)) * 2.0 + 1.0).astype(np.float32),
                    y=rng.choice([1, -1], B))

    def run(inp):
        import torch
        import abnet3_amd.loss as L
        import test_gpu_bn_tower as BT
        from abnet3_amd import _lib
        from abnet3_amd.trainer import FlatOptimizer
        net = BT.build(kw, seed=B + 3, precision=split)
        BT.shake(net, np.random.default_rng(B + nh + 1))
        out = {'p0.' + k: host(v) for k, v in net.state_dict().items()}
        net.train()
        e1, e2 = net(dev(inp['x1']), dev(inp['x2']))
        fwd = _lib.last_forward_path()
        lv = L.coscos2(avg=False)(e1, e2, dev(inp['y']))
        lv.backward()
        assert (fwd, _lib.last_backward_path()) == (P_BN_TOWER, P_BN_TOWER), _lib.last_path
        assert not net.resident_tower_failed()
        out.update(e1=host(e1), e2=host(e2), loss=host(lv))
        for k, q in net.named_parameters():
            out['g.' + k] = host(q.grad)
        for k, v in net.state_dict().items():
            out['p1.' + k] = host(v)
        net.eval()
        with torch.no_grad():
            out['eval'] = host(net.forward_once(dev(inp['x1'])))
        net.train()
        FlatOptimizer(net, 'sgd', 0.01, 0.9).step()
        for k, q in net.named_parameters():
            out['p2.' + k] = host(q)
        return out

    def oracle(inp, out):
        from conftest import check_grads, check_params, is_pre_bn_bias, rel_err
        from oracle import siamese_np as O
        spec = O.TowerSpec(d_in, nh, hid, d_out, 'sigmoid', True)
        p0 = {k[3:]: v for k, v in out.items() if k.startswith('p0.')}
        x1, x2, y = inp['x1'], inp['x2'], inp['y']

        def evaluate(dtype):
            keep = O.F32
            O.F32 = dtype
            try:
                pp = {k: v.astype(dtype) if v.dtype.kind == 'f' else v.copy() for k, v in p0.items()}
                o1, c1 = O.tower_forward(pp, x1.astype(dtype), spec, True, masks=None)
                o2, c2 = O.tower_forward(pp, x2.astype(dtype), spec, True, masks=None)
                ol, d1, d2, _ = O.pair_loss(o1, o2, y, 'coscos2', 0.5, False)
                og = {}
                O.tower_backward(pp, c1, d1.astype(dtype), spec, og)
                O.tower_backward(pp, c2, d2.astype(dtype), spec, og)
                oe, _ = O.tower_forward(pp, x1.astype(dtype), spec, False)          # (on the running statistics the two calls left)
                O.Optimizer('sgd', 0.01).step(pp, og, spec.param_keys())
                return o1, o2, ol, og, pp, oe
            finally:
                O.F32 = keep
        t1, t2, tl, tg, tp, te = evaluate(np.float64)
        o1, o2, ol, og, _, _ = evaluate(np.float32)
        assert np.isfinite(out['e1']).all()
        f32_emb = max(rel_err(o1, t1), rel_err(o2, t2))
        assert max(rel_err(out['e1'], t1), rel_err(out['e2'], t2)) < max(1e-5, 2 * f32_emb)
        f32_loss = abs(ol - tl) / abs(tl)
        assert abs(float(out['loss']) - tl) <= max(1e-5, 2 * f32_loss) * abs(tl) + 1e-9
        for k in p0:
            if 'running' in k:
                assert rel_err(out['p1.' + k], tp[k]) < 1e-5, k
            if 'num_batches' in k:
                assert int(out['p1.' + k]) == int(tp[k]) == 2, k
        keys = [k for k in spec.param_keys() if not is_pre_bn_bias(k, True)]
        gmax = max(np.abs(tg[k]).max() for k in spec.param_keys())
        f32_grad = max(rel_err(og[k], tg[k], floor=1e-2 * gmax) for k in keys)
        check_grads({k: out['g.' + k] for k in spec.param_keys()}, tg, spec.param_keys(), True, tol=max(2e-5, 2 * f32_grad))
        # the eval forward on the running statistics the two calls left, and an SGD step on these gradients: the embeddings' bar;
        # tests/conftest.py:check_params at 1e-5 (tests/test_gpu_planned_steps.py's bar for sgd)
        assert rel_err(out['eval'], te) < max(1e-5, 2 * f32_emb), rel_err(out['eval'], te)
        check_params({k: out['p2.' + k] for k in spec.param_keys()}, tp, spec.param_keys(), True, 1e-5)

    return Case('tower-bn-resident-' + split, ('abn_tower_forward', 'abn_tower_backward', 'abn_tower_sync_ws_bytes', 'abn_pair_loss', 'abn_optimizer_step'),
                build, run, oracle, env=PLANES_ENV, paths=(P_BN_TOWER, P_BN_TOWER))


TOWER_CASES += [bn_tower_case('bf16x3'), bn_tower_case('f16x2')]


def direct_step_case(oname, defer):
    """tests/test_gpu_planned_steps.py: KW_C5 at n = 96 (test_the_lent_workspace_outlives_the_forwards_state) through
    direct_forward / direct_backward_loss / FlatOptimizer.step(): the deferred reduction + step in one launch
    (abn_tower_reduce_step), or the backward's own reduction and abn_optimizer_step.  Bars of that file: embeddings 1e-5, loss
    LOSS_TOL, check_grads at 1e-4, check_params at PARAM_TOL."""
    n, D = 96, 280
    lr = {'sgd': 0.01, 'adam': 0.001}[oname]

    def build():
        rng = np.random.default_rng(21)
        return dict(x1=rng.standard_normal((n, D)).astype(np.float32), x2=rng.standard_normal((n, D)).astype(np.float32),
                    y=rng.choice([1.0, -1.0], n))

    def run(inp):
        import torch
        import test_gpu_planned_steps as PS
        from abnet3_amd import _lib
        from abnet3_amd.trainer import FlatOptimizer
        net = PS.cuda_net(PS.KW_C5, PS.params_of(PS.KW_C5))
        opt = FlatOptimizer(net, oname, lr, 0.9)
        emb, state = net.direct_forward(dev(inp['x1']), dev(inp['x2']))
        assert _lib.last_forward_path() == _lib.PATH_WIDE and net.can_defer_reduce(state)
        out = {'emb': host(emb)}
        net.eval()
        with torch.no_grad():
            out['eval'] = host(net.forward_once(dev(inp['x1'])))
        net.train()
        loss = net.direct_backward_loss(state, dev(inp['y']), 'coscos2', 0.5, False, defer_reduce=defer)
        assert loss is not None and _lib.last_backward_path() == _lib.PATH_WIDE
        assert (net._pending_reduce is not None) == defer
        out['loss'] = host(loss)
        del emb, state
        opt.step()
        for k, q in net.named_parameters():
            out['g.' + k] = host(q.grad)
            out['p1.' + k] = host(q)
        return out

    def oracle(inp, out):
        import test_gpu_planned_steps as PS
        from conftest import check_grads, check_params, rel_err
        from oracle import siamese_np as O
        spec, p = PS._spec(PS.KW_C5), PS.copy_of(PS.params_of(PS.KW_C5))
        oe, _ = O.tower_forward(p, inp['x1'], spec, False)
        assert rel_err(out['eval'], oe) < 1e-5, rel_err(out['eval'], oe)
        want, og, (o1, o2) = O.train_step(p, inp['x1'], inp['x2'], inp['y'], spec, O.Optimizer(oname, lr), 'coscos2', 0.5, False)
        assert rel_err(out['emb'][:n], o1) < 1e-5 and rel_err(out['emb'][n:], o2) < 1e-5
        assert abs(float(out['loss']) - want) <= PS.LOSS_TOL * abs(want), (float(out['loss']), want)
        keys = spec.param_keys()
        check_grads({k: out['g.' + k] for k in keys}, og, keys, False, tol=1e-4)
        check_params({k: out['p1.' + k] for k in keys}, p, keys, False, PS.PARAM_TOL[oname])

    entries = ('abn_tower_forward', 'abn_tower_backward_loss', 'abn_tower_backward_loss_ws_bytes', 'abn_tower_bwd_scratch_floats',
               'abn_tower_reduce_step' if defer else 'abn_optimizer_step')
    return Case('tower-step-%s-%s' % ('deferred' if defer else 'direct', oname), entries, build, run, oracle, paths=(P_WIDE, P_WIDE))


TOWER_CASES += [direct_step_case('sgd', True), direct_step_case('sgd', False), direct_step_case('adam', False)]


def backward_launch_case(split):
    """abn_tower_backward_launch -- ONE of the two launches of an operand-plane backward, for per-launch timing; no Python
    caller -- issued twice (data gradients, then weight gradients) where SiameseNetwork.direct_backward(defer_reduce=True)
    makes its one abn_tower_backward call, on the same descriptor and a torch.empty scratch; FlatOptimizer.step() then sums
    the slabs (abn_tower_reduce_step).  32 -> 64 -> 32, B = 33 on the operand planes, an arbitrary d_out; the bars of
    tests/test_gpu_planned_steps.py:test_the_lent_workspace_outlives_the_forwards_state and of tests/test_gpu_planes.py:
    embeddings 1e-5, check_grads at 1e-4, check_params at 1e-5."""
    kw = dict(input_dim=32, num_hidden_layers=1, hidden_dim=64, output_dim=32, activation_layer='sigmoid', p_dropout=0.0, batch_norm=False)
    B = 33

    def build():
        rng = np.random.default_rng(B)
        return dict(x1=rng.standard_normal((B, 32)).astype(np.float32), x2=rng.standard_normal((B, 32)).astype(np.float32),
                    d_out=rng.standard_normal((2 * B, 32)).astype(np.float32))

    def run(inp):
        import test_gpu_planes as TP
        from abnet3_amd import _lib
        from abnet3_amd.trainer import FlatOptimizer
        lib, C = _lib.load(), _lib.C
        net, _, _ = TP.build(kw, seed=B, precision=split)
        out = {'p0.' + k: host(v) for k, v in net.state_dict().items()}
        opt = FlatOptimizer(net, 'sgd', 0.01, 0.9)
        net.train()
        emb, (seg, sv, grad_pass) = net.direct_forward(dev(inp['x1']), dev(inp['x2']))
        assert _lib.last_forward_path() == P_PLANES, _lib.last_path
        d_out, rows = dev(inp['d_out']), 2 * B
        grad_buf, grads = grad_pass.views(seg)
        desc = seg.descriptor(with_grads=True, grad_buf=grad_buf, masks=sv.masks, defer_reduce=True)
        n_scratch = lib.abn_tower_bwd_scratch_floats(C.byref(desc), rows)
        import torch
        scratch = torch.empty(max(n_scratch, 1), dtype=torch.float32, device='cuda')
        for part in (1, 2):
            _lib.check(lib.abn_tower_backward_launch(C.byref(desc), _lib.ptr(sv.x1), _lib.ptr(sv.x2), _lib.ptr(d_out), rows, sv.n_calls,
                                                     _lib.ptr(sv.ws), _lib.ptr(scratch), n_scratch, part, _lib.stream()),
                       'abn_tower_backward_launch')
        net._pending_reduce = (desc, rows, scratch, n_scratch, grad_buf, seg, sv.ws)
        for q, g in zip(seg.params, grads):
            q.grad = g
        opt.step()
        out['emb'] = host(emb)
        for k, q in net.named_parameters():
            out['g.' + k], out['p1.' + k] = host(q.grad), host(q)
        return out

    def oracle(inp, out):
        from conftest import check_grads, check_params, rel_err
        from oracle import siamese_np as O
        spec = O.TowerSpec(32, 1, 64, 32, 'sigmoid', False)
        p = {k[3:]: v.copy() for k, v in out.items() if k.startswith('p0.')}
        og = {}
        for x, d, e in ((inp['x1'], inp['d_out'][:B], out['emb'][:B]), (inp['x2'], inp['d_out'][B:], out['emb'][B:])):
            o, cache = O.tower_forward(p, x, spec, True)
            assert rel_err(e, o) < 1e-5, rel_err(e, o)
            O.tower_backward(p, cache, d, spec, og)
        keys = spec.param_keys()
        check_grads({k: out['g.' + k] for k in keys}, og, keys, False, tol=1e-4)
        O.Optimizer('sgd', 0.01).step(p, og, keys)
        check_params({k: out['p1.' + k] for k in keys}, p, keys, False, 1e-5)

    return Case('tower-backward-launch-' + split, ('abn_tower_forward', 'abn_tower_backward_launch', 'abn_tower_reduce_step'), build, run, oracle,
                env=PLANES_ENV, paths=(P_PLANES, P_PLANES))


TOWER_CASES += [backward_launch_case('bf16x3'), backward_launch_case('f16x2')]


# ======================================================================================================================
# pair loss, softmax, integration
# ======================================================================================================================
def pair_loss_case(kind):
    """abn_pair_loss / abn_pair_loss_dz at B = 33 (D = 7: the odd tower's output).  coscos2 / cosmargin against
    oracle/siamese_np.py at tests/conftest.py:check_loss_grads' bars (loss 1e-5, gradient rows 2e-5 of their largest entry); KLLoss
    against tests/kl_np.py at tests/test_gpu_kl_loss.py's (the same two numbers)."""
    B, D, margin, NVALID = 33, 7, 0.5, 22

    def build():
        rng = np.random.default_rng(33)
        z1, z2 = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
        y = rng.choice([1, -1], B).astype(np.int64)
        if kind == 'KLLoss':
            import kl_np
            e1, e2 = np.exp(kl_np.log_softmax(z1)).astype(np.float32), np.exp(kl_np.log_softmax(z2)).astype(np.float32)
        else:
            e1, e2 = (1.0 / (1.0 + np.exp(-z1.astype(np.float64)))).astype(np.float32), (1.0 / (1.0 + np.exp(-z2.astype(np.float64)))).astype(np.float32)
        return dict(z1=z1, z2=z2, e1=e1, e2=e2, y=y)

    def make():
        import abnet3_amd.loss as L
        return {'coscos2': lambda: L.coscos2(avg=False), 'cosmargin': lambda: L.cosmargin(avg=True, margin=margin),
                'KLLoss': lambda: L.KLLoss(margin=1.0, avg=True)}[kind]()

    def run(inp):
        a, b = dev(inp['e1']).requires_grad_(True), dev(inp['e2']).requires_grad_(True)
        lv = make()(a, b, dev(inp['y']))
        lv.backward()
        out = dict(loss=host(lv), g1=host(a.grad), g2=host(b.grad))
        if kind == 'KLLoss':
            lz, dz = make().value_and_dz(dev(inp['z1']), dev(inp['z2']), dev(inp['y']), 'softmax', None)
        else:
            lz, dz = make().value_and_dz(dev(inp['e1']), dev(inp['e2']), dev(inp['y']), 'sigmoid', None)
        out.update(loss_dz=host(lz), dz=host(dz))
        # abn_pair_loss_padded (from Python only inside TrainerSiamese's captured evaluation steps): the call of
        # tests/test_gpu_kl_loss.py:_padded with the gradient from torch.empty -- the padded rows get zeros
        import torch
        from abnet3_amd import _lib
        from abnet3_amd.loss import _scratch
        lib = _lib.load()
        e1, e2, y = dev(inp['e1']), dev(inp['e2']), dev(inp['y'])
        nv = torch.tensor([NVALID], dtype=torch.int32, device='cuda')
        acc = torch.zeros((), dtype=torch.float64, device='cuda')
        lp = torch.empty((), dtype=torch.float32, device='cuda')
        de = torch.empty((2, B, D), dtype=torch.float32, device='cuda')
        ws = _scratch(lib.abn_pair_loss_ws_bytes(B), e1.device)
        lf = make()
        _lib.check(lib.abn_pair_loss_padded(_lib.ptr(e1), _lib.ptr(e2), _lib.ptr(y), _lib.Y_DTYPE[y.dtype], B, D, _lib.LOSS[kind],
                                            float(getattr(lf, 'margin', 0.0)), int(lf.avg), _lib.ptr(nv), _lib.ptr(lp), _lib.ptr(acc),
                                            _lib.ptr(de[0]), _lib.ptr(de[1]), _lib.ptr(ws), _lib.stream()), 'abn_pair_loss_padded')
        out.update(loss_padded=host(lp), de_padded=host(de), acc=host(acc))
        return out

    def oracle(inp, out):
        from test_gpu_kl_loss import check_rows
        if kind == 'KLLoss':
            import kl_np
            ol, g1, g2 = kl_np.kl_prob(inp['e1'], inp['e2'], inp['y'], 1.0, True)
            olz, dz1, dz2 = kl_np.kl_logits(inp['z1'], inp['z2'], inp['y'], 1.0, True)
        else:
            from oracle import siamese_np as O
            avg = kind == 'cosmargin'
            ol, g1, g2, _ = O.pair_loss(inp['e1'], inp['e2'], inp['y'], kind, margin, avg)
            olz = ol
            s1, s2 = inp['e1'].astype(np.float64), inp['e2'].astype(np.float64)
            dz1, dz2 = g1 * s1 * (1 - s1), g2 * s2 * (1 - s2)
        assert abs(float(out['loss']) - ol) <= 1e-5 * abs(ol), (float(out['loss']), ol)
        assert abs(float(out['loss_dz']) - olz) <= 1e-5 * abs(olz), (float(out['loss_dz']), olz)
        check_rows(out['g1'], np.asarray(g1), kind)
        check_rows(out['g2'], np.asarray(g2), kind)
        check_rows(out['dz'][0], np.asarray(dz1), kind + ' dz')
        check_rows(out['dz'][1], np.asarray(dz2), kind + ' dz')
        n = NVALID
        if kind == 'KLLoss':
            pl, p1, p2 = kl_np.kl_prob(inp['e1'][:n], inp['e2'][:n], inp['y'][:n], 1.0, True)
        else:
            pl, p1, p2, _ = O.pair_loss(inp['e1'][:n], inp['e2'][:n], inp['y'][:n], kind, margin, avg)
        assert abs(float(out['loss_padded']) - pl) <= 1e-5 * abs(pl) and float(out['acc']) == float(out['loss_padded'])
        assert not out['de_padded'][:, n:].any()
        check_rows(out['de_padded'][0, :n], np.asarray(p1), kind + ' padded')
        check_rows(out['de_padded'][1, :n], np.asarray(p2), kind + ' padded')

    return Case('pair-loss-' + kind, ('abn_pair_loss', 'abn_pair_loss_dz', 'abn_pair_loss_padded', 'abn_pair_loss_ws_bytes'), build, run, oracle)


def softmax_case():
    """abn_softmax_rows / abn_softmax_rows_backward at 33 x 7 against tests/kl_np.py:log_softmax in float64, at the tower's
    1e-5 of the tensor's largest entry (tests/conftest.py:rel_err)."""
    def build():
        rng = np.random.default_rng(7)
        return dict(z=(3 * rng.standard_normal((33, 7))).astype(np.float32), g=rng.standard_normal((33, 7)).astype(np.float32))

    def run(inp):
        from abnet3_amd.model import _SoftmaxRows
        z = dev(inp['z']).requires_grad_(True)
        a = _SoftmaxRows.apply(z)
        a.backward(dev(inp['g']))
        return dict(a=host(a), dz=host(z.grad))

    def oracle(inp, out):
        import kl_np
        from conftest import rel_err
        a = np.exp(kl_np.log_softmax(inp['z']))
        g = inp['g'].astype(np.float64)
        dz = a * (g - (a * g).sum(1, keepdims=True))
        assert rel_err(out['a'], a) < 1e-5 and rel_err(out['dz'], dz) < 1e-5, (rel_err(out['a'], a), rel_err(out['dz'], dz))

    return Case('softmax-rows', ('abn_softmax_rows', 'abn_softmax_rows_backward'), build, run, oracle)


def integrate_case(mode, kind):
    """abn_integrate_forward / _backward through integration._IntegrateFunction on tests/test_gpu_multimodal.py's
    (37, 13, 13) shape and its bars against tests/mm_np.py: 1e-5 of the tensor's largest entry, attention weights 1e-6,
    unweighted / fixed / scalar outputs bit for bit the float32 expression."""
    R, d = 37, 13
    K = {'attention_k1': 1, 'attention_kd': d}.get(kind, 1)
    wv = {'none': 1.0, 'fixed': 0.3, 'scalar': 0.6}.get(kind, 0.0)

    def build():
        rng = np.random.default_rng(R * 7 + 2 * d)
        inp = dict(x1=rng.standard_normal((R, d)).astype(np.float32), x2=rng.standard_normal((R, d)).astype(np.float32),
                   g=rng.standard_normal((R, d if mode == 'sum' else 2 * d)).astype(np.float32))
        if kind.startswith('attention'):
            inp.update(z1=rng.standard_normal((R, K)).astype(np.float32), z2=rng.standard_normal((R, K)).astype(np.float32))
        return inp

    def run(inp):
        from abnet3_amd import _lib
        from abnet3_amd.integration import _IntegrateFunction
        x1, x2 = dev(inp['x1']).requires_grad_(True), dev(inp['x2']).requires_grad_(True)
        z1 = z2 = wp = None
        holder = type('Holder', (), {})()
        if kind.startswith('attention'):
            z1, z2 = dev(inp['z1']).requires_grad_(True), dev(inp['z2']).requires_grad_(True)
            code, wf, wc = _lib.W_ATTENTION, 0.0, 0.0
        elif kind == 'scalar':
            wp = dev(np.array([wv], np.float32)).requires_grad_(True)
            code, wf, wc = _lib.W_SCALAR, 0.0, 0.0
        else:
            code = _lib.W_FIXED if kind == 'fixed' else _lib.W_NONE
            wf, wc = (float(wv), float(np.float32(1 - wv))) if kind == 'fixed' else (0.0, 0.0)
        y = _IntegrateFunction.apply((mode, code, wf, wc, K, _lib.ACT['sigmoid'], None, holder), x1, x2, z1, z2, wp)
        y.backward(dev(inp['g']))
        out = dict(out=host(y), dx1=host(x1.grad), dx2=host(x2.grad))
        if z1 is not None:
            out.update(w=host(holder.w), dz1=host(z1.grad), dz2=host(z2.grad))
        if wp is not None:
            out['dw'] = host(wp.grad)
        return out

    def oracle(inp, out):
        import mm_np
        from test_gpu_multimodal import rel
        x1, x2, g = inp['x1'], inp['x2'], inp['g']
        if kind.startswith('attention'):
            w, wc = mm_np.weights('attention', R, z=inp['z1'] + inp['z2'], act_name='sigmoid')
            assert rel(out['w'], w) <= 1e-6
            rdx1, rdx2, rdz, _ = mm_np.backward(mode, 'attention', x1, x2, g, w, wc, 'sigmoid')
            assert rel(out['out'], mm_np.forward(mode, x1, x2, w, wc)) <= 1e-5
            assert rel(out['dx1'], rdx1) <= 1e-5 and rel(out['dx2'], rdx2) <= 1e-5
            assert rel(out['dz1'], rdz) <= 1e-5 and np.array_equal(out['dz1'], out['dz2'])
            return
        w32 = np.float32(wv)
        wc32 = np.float32(np.float32(1 - wv)) if kind == 'fixed' else np.float32(np.float32(1) - w32)
        if kind == 'none':
            exact = x1 + x2 if mode == 'sum' else np.concatenate((x1, x2), 1)
        elif mode == 'sum':
            exact = w32 * x1 + wc32 * x2
        else:
            exact = np.concatenate((w32 * x1, wc32 * x2), 1)
        assert np.array_equal(out['out'], exact)
        w, wc = mm_np.weights(kind, R, w=float(w32)) if kind != 'none' else mm_np.weights('none', R)
        if kind == 'fixed':
            wc = np.full_like(w, float(wc32))
        rdx1, rdx2, _, rdw = mm_np.backward(mode, kind, x1, x2, g, w, wc)
        assert rel(out['dx1'], rdx1) <= 1e-5 and rel(out['dx2'], rdx2) <= 1e-5
        if kind == 'scalar':
            assert abs(float(out['dw'][0]) - rdw[0]) <= 1e-5 * max(abs(rdw[0]), np.abs(g).sum() * 1e-3)

    entries = ('abn_integrate_forward', 'abn_integrate_backward') + (('abn_integrate_ws_bytes',) if kind == 'scalar' else ())
    return Case('integrate-%s-%s' % (mode, kind), entries, build, run, oracle)


LOSS_CASES = [pair_loss_case(k) for k in ('coscos2', 'cosmargin', 'KLLoss')] + [softmax_case()] + [
    integrate_case(m, k) for m in ('sum', 'concat') for k in ('none', 'fixed', 'scalar', 'attention_k1', 'attention_kd')
    ]



# ======================================================================================================================
# the front end
# ======================================================================================================================
FS = 16000


def _waves():
    from test_gpu_mfcc import speech_like
    return [speech_like(12345, FS, 12345), speech_like(150, FS, 150)]


def frontend_case(method, batched):
    """fbank / mfcc with deltas and deltasdeltas, two utterances of 12345 and 150 samples (one launch, or one call each),
    against oracle/features_np.py / tests/mfcc_np.py at the bar of tests/test_gpu_dtw_features.py and tests/test_gpu_mfcc.py:
    5e-5 absolute."""
    def build():
        return dict(waves=_waves())

    def run(inp):
        from abnet3_amd.features import FeaturesGenerator
        fg = FeaturesGenerator(method='mfcc' if method == 'mfcc' else 'fbanks', deltas=True, deltasdeltas=True)
        if batched:
            table, nfr = (fg.mfcc_batch if method == 'mfcc' else fg.fbank_batch)(inp['waves'], FS)
            return dict(table=host(table), nfr=np.asarray(nfr))
        one = fg.mfcc_from_samples if method == 'mfcc' else fg.fbank_from_samples
        parts = [host(one(w, FS)) for w in inp['waves']]
        return dict(table=np.concatenate(parts), nfr=np.array([len(p) for p in parts], dtype=np.int64))

    def oracle(inp, out):
        import mfcc_np
        from oracle import features_np as F
        refs = []
        for w in inp['waves']:
            if method == 'mfcc':
                c = mfcc_np.mfcc(w, FS)
                d1 = F.deltas(c)
                refs.append(np.hstack([c, d1, F.deltas(d1)]))
            else:
                refs.append(F.fbank_with_deltas(w, FS, do_deltas=True, do_deltasdeltas=True))
        assert out['nfr'].tolist() == [len(r) for r in refs] == [F.frame_count(len(w), FS) for w in inp['waves']]
        ref = np.concatenate(refs)
        assert out['table'].shape == ref.shape and np.abs(out['table'] - ref).max() < 5e-5, np.abs(out['table'] - ref).max()

    if method == 'mfcc':
        entries = ('abn_mfcc_batched', 'abn_deltas_batched') if batched else ('abn_mfcc', 'abn_deltas_batched')
    else:
        entries = ('abn_fbank_batched', 'abn_deltas_batched') if batched else ('abn_fbank', 'abn_deltas')
    return Case('%s-%s' % (method, 'batched' if batched else 'single'), entries, build, run, oracle)


def stack_case(T, n):
    """stack_fbanks and stack_table against oracle/features_np.py:stack_fbanks, bit for bit (tests/test_gpu_dtw_features.py
    holds the kernel to the reference's fixtures bit for bit); the batched form on two utterances of T and 2 frames."""
    def build():
        return dict(x=np.random.default_rng(T).standard_normal((T + 2, 13)).astype(np.float32))

    def run(inp):
        from abnet3_amd.features import FeaturesGenerator
        fg = FeaturesGenerator(nframes=n)
        return dict(one=host(fg.stack_fbanks(dev(inp['x'][:T]), nframes=n)), table=host(fg.stack_table(dev(inp['x']), [T, 2])))

    def oracle(inp, out):
        from oracle import features_np as F
        x = inp['x']
        assert np.array_equal(out['one'], F.stack_fbanks(x[:T], n))
        assert np.array_equal(out['table'], np.concatenate([F.stack_fbanks(x[:T], n), F.stack_fbanks(x[T:], n)]))

    return Case('stack-T%d-n%d' % (T, n), ('abn_stack_frames', 'abn_stack_frames_batched'), build, run, oracle)


def mvn_case(per_channel):
    """abn_mvn_stats / abn_mvn_apply at T = 37, D = 13 against oracle/features_np.py:mvn at the bars of
    tests/test_gpu_dtw_features.py:test_mean_variance_normalisation (output 2e-5 x max(1, |ref|), statistics rtol 1e-5)."""
    def build():
        return dict(x=(np.random.default_rng(37).standard_normal((37, 13)) * 3 + 12).astype(np.float32))

    def run(inp):
        from abnet3_amd.features import FeaturesGenerator
        fg = FeaturesGenerator(norm_per_channel=per_channel)
        out, (mean, std) = fg.normalize_table(dev(inp['x']), [37])
        return dict(out=host(out), mean=host(mean), std=host(std))

    def oracle(inp, out):
        from oracle import features_np as F
        x = inp['x']
        ref, _, _ = F.mvn(x, per_channel)
        assert np.abs(out['out'] - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
        axis = 0 if per_channel else None
        assert np.allclose(out['mean'], np.mean(x, axis=axis), rtol=1e-5) and np.allclose(out['std'], np.std(x, axis=axis), rtol=1e-5)

    return Case('mvn-%s' % ('per-channel' if per_channel else 'whole'), ('abn_mvn_stats', 'abn_mvn_apply', 'abn_mvn_ws_bytes'), build, run, oracle)


def cosine_case(f64):
    """cosine_distance at 33 x 17 x 40: float32 inputs bit for bit the oracle's (tests/test_gpu_dtw_features.py), float64
    inputs within that file's 2e-15 of the float64 expression."""
    def build():
        rng = np.random.default_rng(17)
        dt = np.float64 if f64 else np.float32
        return dict(x=rng.standard_normal((33, 40)).astype(dt), y=rng.standard_normal((17, 40)).astype(dt))

    def run(inp):
        from abnet3_amd.utils import cosine_distance
        return dict(d=cosine_distance(inp['x'], inp['y']))

    def oracle(inp, out):
        x, y = inp['x'], inp['y']
        if f64:
            c = (x @ y.T) / np.outer(np.linalg.norm(x, axis=1), np.linalg.norm(y, axis=1))
            assert np.abs(out['d'] - np.arccos(c) / np.pi).max() < 2e-15
        else:
            from oracle import dtw_oracle as O
            assert (out['d'] == O.cosine_distance(x, y)).all()

    name = 'abn_cosine_distance_f64' if f64 else 'abn_cosine_distance'
    return Case('cosine-distance-%s' % ('f64' if f64 else 'f32'), (name,), build, run, oracle)


def arccos_case():
    """abn_arccos_f32 has no Python wrapper (tools and tests call the entry): the call of
    tests/test_gpu_dtw_features.py:test_device_arccos_equals_libm_acosf on every 997th float32 of [-1, 1] and arguments outside,
    bit for bit the oracle's restatement of glibc's acosf."""
    def build():
        b = np.concatenate([np.arange(0, 0x3f800100, 997 * 61, dtype=np.int64), np.arange(0x3f7fff00, 0x3f800100, dtype=np.int64)])
        return dict(x=np.concatenate([b, b + 0x80000000]).astype(np.uint32).view(np.float32))

    def run(inp):
        import torch
        from abnet3_amd import _lib
        lib, xd, out = _lib.load(), dev(inp['x']), {}
        for over_pi in (0, 1, 2, 3):
            o = torch.empty_like(xd)
            _lib.check(lib.abn_arccos_f32(_lib.ptr(xd), xd.numel(), over_pi, _lib.ptr(o), _lib.stream()), 'abn_arccos_f32')
            out['acos%d' % over_pi] = host(o)
        return out

    def oracle(inp, out):
        from oracle import dtw_oracle as O
        L, x = O.lib(), inp['x']
        L.abn_oracle_acosf_array.restype = None
        L.abn_oracle_acosf_array.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
        for over_pi in (0, 1, 2, 3):
            ref = np.empty_like(x)
            L.abn_oracle_acosf_array(x.ctypes.data_as(ctypes.c_void_p), len(x), over_pi & 1, ref.ctypes.data_as(ctypes.c_void_p))
            got, nan = out['acos%d' % over_pi], np.isnan(ref)
            assert (np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == ref.view(np.uint32)[~nan]).all()

    return Case('arccos', ('abn_arccos_f32',), build, run, oracle)


def gather_case():
    """dataloader.gather_rows against numpy indexing (bit for bit), and abn_gather_pairs -- reached from Python only inside
    the trainer's planned passes -- called as tests/test_gpu_planned_steps.py:test_gather_pairs_is_the_host_gather calls it,
    with x12 / y / n_valid from torch.empty: both towers' rows, zero rows up to the padded size, an index outside the table
    reads a zero row."""
    D, rows, first, n, npad = 39, 20, 5, 33, 64

    def build():
        import plan_np
        h = plan_np.host_plan(np.random.default_rng(D), D, [5, 33, 64, 1], np.float64, table_rows=rows, scatter=False)
        h['idx1'][7], h['idx2'][9], h['idx2'][37] = -1, rows, 1 << 40
        return h

    def run(h):
        import torch
        from abnet3_amd import _lib
        from abnet3_amd.dataloader import gather_rows
        lib = _lib.load()
        table, idx1, idx2, lab = dev(h['table']), dev(h['idx1']), dev(h['idx2']), dev(h['labels'])
        x12 = torch.empty(2 * npad, D, dtype=torch.float32, device='cuda')
        y = torch.empty(npad, dtype=lab.dtype, device='cuda')
        nv = torch.empty(1, dtype=torch.int32, device='cuda')
        _lib.check(lib.abn_gather_pairs(_lib.ptr(table), rows, D, _lib.ptr(idx1), _lib.ptr(idx2), first, n, npad, _lib.ptr(lab),
                                        lab.element_size(), _lib.ptr(x12), _lib.ptr(y), _lib.ptr(nv), _lib.stream()), 'abn_gather_pairs')
        good = torch.clamp(idx1[first:first + n], 0, rows - 1)
        return dict(x12=host(x12), y=host(y), nv=host(nv), rows=host(gather_rows(table, good)))

    def oracle(h, out):
        import plan_np
        x1, x2, labels = plan_np.gather_batch(h, 1)
        want = np.zeros((2 * npad, D), dtype=np.float32)
        want[:n], want[npad:npad + n] = x1, x2
        assert np.array_equal(out['x12'], want)
        assert np.array_equal(out['y'][:n], labels) and not out['y'][n:].any() and int(out['nv'][0]) == n
        assert np.array_equal(out['rows'], h['table'][np.clip(h['idx1'][first:first + n], 0, rows - 1)])

    return Case('gather', ('abn_gather_rows', 'abn_gather_pairs'), build, run, oracle)


FRONT_CASES = ([frontend_case(m, b) for m in ('fbank', 'mfcc') for b in (True, False)] + [stack_case(5, 7), stack_case(100, 3)]
               + [mvn_case(True), mvn_case(False), cosine_case(False), cosine_case(True), arccos_case(), gather_case()])


# ======================================================================================================================
# DTW with paths, DTW cost, ABX score
# ======================================================================================================================
def dtw_align_case(name, env=None):
    """dtw_align_batch (abn_dtw_batched_overlap: the package's only caller of the path DTW) on
    tests/test_gpu_kernel_switches.py:dtw_case() -- 60 pairs, one of them dropped --, bit for bit against the oracle as
    test_dtw_kernel_choice_is_bit_exact_vs_oracle holds it; the dropped pair's path_len and total_cost come back 0."""
    def build():
        from test_gpu_kernel_switches import dtw_case
        return dtw_case()

    def run(inp):
        from abnet3_amd.utils import dtw_align_batch
        f1, o1, n1, f2, o2, n2, _ = inp
        res = dtw_align_batch(dev(f1), o1, n1, dev(f2), o2, n2)
        got = res.to_lists()
        out = dict(plen=host(res.path_len), cost=host(res.total_cost))
        for p, g in enumerate(got):
            out['p1.%d' % p], out['p2.%d' % p] = (g if g is not None else (np.zeros(0, np.int32), np.zeros(0, np.int32)))
        return out

    def oracle(inp, out):
        ref = inp[6]
        for p in range(len(ref)):
            if ref[p] is None:
                assert out['plen'][p] == 0 and out['cost'][p] == 0.0 and len(out['p1.%d' % p]) == 0, p
                continue
            p1, p2, c = ref[p]
            assert out['plen'][p] == len(p1) and (out['p1.%d' % p] == p1).all() and (out['p2.%d' % p] == p2).all(), p
            assert out['cost'][p] == c, p

    def run_raw(inp):
        """abn_dtw_batched itself (one stream; no Python caller since dtw_align_batch took the overlapped entry): the
        wrapper's allocations, sized by the same queries."""
        import torch
        from abnet3_amd import _lib
        lib = _lib.load()
        f1, o1, n1, f2, o2, n2, _ = inp
        d1, d2 = dev(f1), dev(f2)
        o1, o2 = np.ascontiguousarray(o1, dtype=np.int64), np.ascontiguousarray(o2, dtype=np.int64)
        n1, n2 = np.ascontiguousarray(n1, dtype=np.int32), np.ascontiguousarray(n2, dtype=np.int32)
        P, stride = len(n1), int((n1.astype(np.int64) + n2).max()) - 1
        a = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        both = torch.empty(2, P, stride, dtype=torch.int32, device='cuda')
        plen = torch.empty(P, dtype=torch.int32, device='cuda')
        cost = torch.empty(P, dtype=torch.float64, device='cuda')
        ws = torch.empty(int(lib.abn_dtw_ws_bytes(a(n1), a(n2), P, d1.shape[0], d2.shape[0])), dtype=torch.uint8, device='cuda')
        stage = torch.empty(int(lib.abn_dtw_host_stage_bytes(a(n1), a(n2), P)) + 256, dtype=torch.uint8).pin_memory()
        _lib.check(lib.abn_dtw_batched(_lib.ptr(d1), d1.shape[0], _lib.ptr(d2), d2.shape[0], a(o1), a(n1), a(o2), a(n2), P, d1.shape[1],
                                       _lib.ptr(both[0]), _lib.ptr(both[1]), _lib.ptr(plen), stride, _lib.ptr(cost), _lib.ptr(ws), ws.numel(),
                                       ctypes.c_void_p(stage.data_ptr()), stage.numel(), _lib.stream()), 'abn_dtw_batched')
        torch.cuda.synchronize()
        ln, b = host(plen), host(both)
        out = dict(plen=ln, cost=host(cost))
        for p in range(P):
            out['p1.%d' % p], out['p2.%d' % p] = b[0, p, stride - ln[p]:], b[1, p, stride - ln[p]:]
        return out

    if name == 'dtw-batched-raw':
        return Case(name, ('abn_dtw_batched', 'abn_dtw_ws_bytes', 'abn_dtw_host_stage_bytes'), build, run_raw, oracle, env=env)
    return Case(name, ('abn_dtw_batched_overlap', 'abn_dtw_ws_bytes', 'abn_dtw_host_stage_bytes'), build, run, oracle, env=env)


def dtw_cost_case(how):
    """abx.dtw_cost_batch: 'cosine' and 'zero' on 60 pairs of 39-value frames (tests/test_gpu_abx.py:pair_table: every band and
    round edge; an empty token on either side, a NaN frame -- dropped -- under 'cosine'), bit for bit the oracle's cost and
    path length (test_cost_kernel_matches_the_oracle); 'kl' on tests/test_gpu_abx_kl.py:kl_pair_table with a BAD row, bit for
    bit tests/abx_kl_np.py on the device's own tables (test_kl_cost_kernel_matches_the_restatement)."""
    D = 39

    def build():
        rng = np.random.default_rng(100 + D)
        if how == 'kl':
            from test_gpu_abx_kl import kl_pair_table
            f1, o1, n1, f2, o2, n2 = kl_pair_table(rng, 60, D, False)
            f1[o1[-3] + n1[-3] // 2, D // 2] = np.nan
            f1[o1[-5] + n1[-5] - 1, 0] = 0.0
        else:
            from test_gpu_abx import pair_table
            f1, o1, n1, f2, o2, n2 = pair_table(rng, 60, D, False)
            if how == 'cosine':
                f1[o1[-3]] = np.nan
            f1[o1[-4] + n1[-4] - 1] = 0.0
        n1[-1] = 0
        n2[-2] = 0
        return f1, o1, n1, f2, o2, n2

    def run(inp):
        from abnet3_amd import abx
        f1, o1, n1, f2, o2, n2 = inp
        out = {}
        if how == 'kl':
            t1, t2 = abx.kl_tables(dev(f1)), abx.kl_tables(dev(f2))
            c, l = abx.dtw_cost_batch(t1, o1, n1, t2, o2, n2, distance='kl')
            ok1, ok2 = host(t1[2]) == 0, host(t2[2]) == 0
            out.update(bad1=host(t1[2]), bad2=host(t2[2]))
            for k, t, ok in (('1', t1, ok1), ('2', t2, ok2)):       # (what a BAD row's P and L hold is nobody's business)
                out['rawP' + k] = np.where(ok[:, None], host(t[0]), np.float32(0))
                out['rawL' + k] = np.where(ok[:, None], host(t[1]), np.float32(0))
        else:
            c, l = abx.dtw_cost_batch(dev(f1), o1, n1, dev(f2), o2, n2, parallel='zero' if how == 'zero' else 'drop')
        out.update(cost=host(c), plen=host(l))
        return out

    def oracle(inp, out):
        f1, o1, n1, f2, o2, n2 = inp
        if how == 'kl':
            import abx_kl_np
            from abnet3_amd import _lib
            t1 = (out['rawP1'], out['rawL1'], out['bad1'])
            t2 = (out['rawP2'], out['rawL2'], out['bad2'])
            ref_c, ref_l = abx_kl_np.dtw_cost_batch(t1, o1, n1, t2, o2, n2, cap=_lib.load().abn_dtw_cost_max_n2())
            assert np.array_equal(out['plen'], ref_l) and np.array_equal(bits(out['cost']), bits(ref_c))
            assert out['plen'][-3:].tolist() == [0, 0, 0] and (out['plen'][:-3] > 0).all()
            return
        from oracle import dtw_oracle as O
        for p in range(len(n1)):
            a, b = f1[o1[p]:o1[p] + n1[p]], f2[o2[p]:o2[p] + n2[p]]
            if len(a) == 0 or len(b) == 0 or not np.isfinite(a).all():
                assert out['plen'][p] == 0 and out['cost'][p] == 0.0, p
                continue
            d = O.cosine_distance(a, b)
            assert out['cost'][p] == O.dtw_cost(d) and out['plen'][p] == len(O.dtw_path(d)[0]), p

    entries = {'cosine': ('abn_dtw_cost_batched',), 'zero': ('abn_dtw_cost_parallel_batched',),
               'kl': ('abn_kl_tables', 'abn_dtw_cost_kl_batched')}[how] + ('abn_dtw_cost_max_n2',)
    return Case('dtw-cost-' + how, entries, build, run, oracle)


def abx_score_case():
    """abx.abx_score on tests/test_gpu_abx.py:test_score_kernel_matches_brute_force's 60 items ('within'), distances with many
    ties: exactly the brute-force triplet scores of tests/abx_np.py (integers)."""
    def build():
        import abx_np
        from abnet3_amd.abx import enumerate_cells
        from test_abx_host import random_items
        rng = np.random.default_rng(21)
        phones, contexts, speakers = random_items(rng, 60, n_phones=3, n_ctx=2, n_spk=3)
        plan = enumerate_cells(phones, contexts, speakers, 'within')
        pairs = list(zip(plan.P.tolist(), plan.Q.tolist()))
        dist = rng.integers(0, 5, len(pairs)).astype(np.float64)
        ref = abx_np.cell_scores(abx_np.triplets(phones, contexts, speakers, 'within'), dict(zip(pairs, dist)))
        return dict(plan=plan, dist=dist, ref=ref)

    def run(inp):
        from abnet3_amd.abx import abx_score
        s2, cnt = abx_score(dev(inp['dist']), inp['plan'])
        return dict(s2=np.asarray(s2), cnt=np.asarray(cnt))

    def oracle(inp, out):
        assert {k: (int(a), int(b)) for k, a, b in zip(inp['plan'].cells, out['s2'], out['cnt'])} == inp['ref']

    return Case('abx-score', ('abn_abx_score',), build, run, oracle)


DTW_CASES = [dtw_align_case('dtw-align'), dtw_align_case('dtw-align-pc0', env={'ABN_DTW_PC': '0'}), dtw_align_case('dtw-batched-raw')] + [
    dtw_cost_case(h) for h in ('cosine', 'zero', 'kl')] + [abx_score_case()]



# ======================================================================================================================
# query-by-example search, local alignment, LSH prefilter, edit distance
# ======================================================================================================================
def kl_host(t):
    """(P, L, bad) of abx.kl_tables on the host; what a BAD row's P and L hold is nobody's business (its pairs are dropped)."""
    bad = host(t[2])
    ok = (bad == 0)[:, None]
    return np.where(ok, host(t[0]), np.float32(0)), np.where(ok, host(t[1]), np.float32(0)), bad


def search_case(kl):
    """qbe.subsequence_dtw_batch with profiles on the pair table of tests/test_gpu_qbe.py (test_search_kernel_matches_the_
    restatement at D = 40 / test_kl_search_kernel_matches_the_restatement at D = 40, without the pairs the Python surface
    refuses before the launch): blocked frames, BAD rows, empty sides -- bit for bit tests/qbe_np.py, profile included."""
    D = 40

    def build():
        import test_gpu_qbe as Q
        rng = np.random.default_rng((400 if kl else 300) + D)
        un, qn = Q.lengths(rng, 40 if kl else 60)
        if kl:
            un[-1] = 50
            uo, qo = Q.offsets(un), Q.offsets(qn)
            fu = rng.dirichlet(np.full(D, 0.5), int(un.sum())).astype(np.float32)
            fq = rng.dirichlet(np.full(D, 0.5), int(qn.sum())).astype(np.float32)
            fq[qo[3]:qo[3] + qn[3]] = fu[uo[3] + 10:uo[3] + 10 + qn[3]]
            fu[uo[-1] + un[-1] // 2, 0] = -0.25
            fq[qo[-2], D // 2] = np.nan
            fu[uo[-3], 1] = 0.0
            un[-4] = 0
        else:
            un[-1], un[-3] = 50, 40
            fu, fq = Q.frames(rng, int(un.sum()), D, False), Q.frames(rng, int(qn.sum()), D, False)
            uo, qo = Q.offsets(un), Q.offsets(qn)
            fu[uo[-1] + un[-1] // 2] = np.nan
            fq[qo[-2] + qn[-2] // 2, D // 2] = np.nan
            fu[uo[-3], 0] = np.inf
            fu[uo[-4] + un[-4] - 1] = 0.0
            fq[qo[-5]] = 0.0
            un[-6] = 0
            qn[-7] = 0
        return dict(fu=fu, uo=uo, un=un, fq=fq, qo=qo, qn=qn)

    def run(inp):
        from abnet3_amd.abx import kl_tables
        from abnet3_amd.qbe import subsequence_dtw_batch
        out = {}
        if kl:
            tu, tq = kl_tables(dev(inp['fu'])), kl_tables(dev(inp['fq']))
            for k, t in (('u', tu), ('q', tq)):
                out['P' + k], out['L' + k], out['bad' + k] = kl_host(t)
            res = subsequence_dtw_batch(tq, inp['qo'], inp['qn'], tu, inp['uo'], inp['un'], distance='kl', profile=True)
        else:
            res = subsequence_dtw_batch(dev(inp['fq']), inp['qo'], inp['qn'], dev(inp['fu']), inp['uo'], inp['un'], profile=True)
        out.update(cost=host(res[0]), plen=host(res[1]), start=host(res[2]), end=host(res[3]),
                   prof_cost=host(res[4].cost), prof_len=host(res[4].len), prof_start=host(res[4].start))
        return out

    def oracle(inp, out):
        import qbe_np
        from test_gpu_qbe import assert_same
        got = (out['cost'], out['plen'], out['start'], out['end'], (out['prof_cost'], out['prof_len'], out['prof_start']))
        if kl:
            ref = qbe_np.search_kl_batch((out['Pq'], out['Lq'], out['badq']), inp['qo'], inp['qn'],
                                         (out['Pu'], out['Lu'], out['badu']), inp['uo'], inp['un'])
        else:
            ref = qbe_np.search_cosine_batch(inp['fq'], inp['qo'], inp['qn'], inp['fu'], inp['uo'], inp['un'])
        assert_same(got, ref, 'kl' if kl else 'cosine')

    entries = ('abn_dtw_search_kl_batched', 'abn_kl_tables') if kl else ('abn_dtw_search_batched',)
    return Case('search-' + ('kl' if kl else 'cosine'), entries + ('abn_dtw_search_max_query',), build, run, oracle)


def local_case(kl):
    """terms.local_dtw_batch on the pair table of tests/test_gpu_terms.py (test_local_kernel_matches_the_restatement /
    test_kl_local_kernel_matches_the_restatement at D = 40, without the pairs the Python surface refuses): bit for bit
    tests/terms_np.py."""
    D = 40

    def build():
        import test_gpu_terms as T
        rng = np.random.default_rng((700 if kl else 500) + D)
        n1, n2 = T.lengths(rng, 40 if kl else 60)
        if kl:
            n1[-1] = 50
            o1, o2 = T.offsets(n1), T.offsets(n2)
            f1 = rng.dirichlet(np.full(D, 0.5), int(n1.sum())).astype(np.float32)
            f2 = rng.dirichlet(np.full(D, 0.5), int(n2.sum())).astype(np.float32)
            f2[o2[3] + 5:o2[3] + 25] = f1[o1[3] + 10:o1[3] + 30]
            f1[o1[-1] + n1[-1] // 2, 0] = -0.25
            f2[o2[-2], D // 2] = np.nan
            f1[o1[-3], 1] = 0.0
            n1[-4] = 0
        else:
            n1[-1], n1[-3] = 50, 40
            f1, f2 = T.frames(rng, int(n1.sum()), D, False), T.frames(rng, int(n2.sum()), D, False)
            o1, o2 = T.offsets(n1), T.offsets(n2)
            f1[o1[-1] + n1[-1] // 2] = np.nan
            f2[o2[-2] + n2[-2] // 2, D // 2] = np.nan
            f1[o1[-3], 0] = np.inf
            f1[o1[-4] + n1[-4] - 1] = 0.0
            f2[o2[-5]] = 0.0
            n1[-6] = 0
            n2[-7] = 0
        return dict(f1=f1, o1=o1, n1=n1, f2=f2, o2=o2, n2=n2)

    def theta_of(t1, t2):
        import terms_np
        if not kl:
            from test_gpu_terms import THETA
            return THETA
        return float(np.quantile(terms_np.kl_cells([a[:200] for a in t1], [a[:200] for a in t2]), 0.25))

    def run(inp):
        from abnet3_amd.abx import kl_tables
        from abnet3_amd.terms import local_dtw_batch
        out = {}
        if kl:
            t1, t2 = kl_tables(dev(inp['f1'])), kl_tables(dev(inp['f2']))
            for k, t in (('1', t1), ('2', t2)):
                out['P' + k], out['L' + k], out['bad' + k] = kl_host(t)
            theta = theta_of((out['P1'], out['L1'], out['bad1']), (out['P2'], out['L2'], out['bad2']))
            res = local_dtw_batch(t1, inp['o1'], inp['n1'], t2, inp['o2'], inp['n2'], theta, distance='kl')
        else:
            res = local_dtw_batch(dev(inp['f1']), inp['o1'], inp['n1'], dev(inp['f2']), inp['o2'], inp['n2'], theta_of(None, None))
        from test_gpu_terms import NAMES
        out.update({k: host(t) for k, t in zip(NAMES, res)})
        return out

    def oracle(inp, out):
        import terms_np
        from test_gpu_terms import NAMES, assert_same
        got = tuple(out[k] for k in NAMES)
        if kl:
            t1, t2 = (out['P1'], out['L1'], out['bad1']), (out['P2'], out['L2'], out['bad2'])
            ref = terms_np.local_kl_batch(t1, inp['o1'], inp['n1'], t2, inp['o2'], inp['n2'], theta_of(t1, t2))
        else:
            ref = terms_np.local_cosine_batch(inp['f1'], inp['o1'], inp['n1'], inp['f2'], inp['o2'], inp['n2'], theta_of(None, None))
        assert_same(got, ref, 'kl' if kl else 'cosine')
        assert (out['path_len'] > 0).sum() >= 30

    entries = ('abn_dtw_local_kl_batched', 'abn_kl_tables') if kl else ('abn_dtw_local_batched',)
    return Case('local-' + ('kl' if kl else 'cosine'), entries + ('abn_dtw_local_max_n2',), build, run, oracle)


def lsh_case():
    """prefilter.lsh_signatures on 130 x 40 frames with dead rows (tests/test_gpu_prefilter.py: live flags equal, dead rows'
    words zero, every bit the float32 bound decides equal to tests/prefilter_np.py) and prefilter.diag_hits_batch on that
    file's edge pair table over pool signatures (exactly tests/prefilter_np.py:diag_hits)."""
    words, mh, span, dilate = 2, 16, 32, 1

    def build():
        import prefilter_np
        import test_gpu_prefilter as TP
        rng = np.random.default_rng(100 * words + dilate)
        table = rng.standard_normal((130, 40)).astype(np.float32)
        table[3] = 0.0
        table[7, 20] = np.nan
        table[20, 0] = np.inf
        table[129, 13] = -np.inf
        n1 = np.repeat(TP.N1_EDGES, len(TP.N2_EDGES)).astype(np.int32)
        n2 = np.tile(TP.N2_EDGES, len(TP.N1_EDGES)).astype(np.int32)
        sig1, live1 = TP.pool_table(rng, int(n1.sum()), words)
        sig2, live2 = TP.pool_table(rng, int(n2.sum()), words)
        sig2[:] = sig1[rng.integers(0, len(sig1), len(sig2))]
        return dict(table=table, planes=prefilter_np.planes(40, 64, seed=40), n1=n1, n2=n2, o1=TP.offsets(n1), o2=TP.offsets(n2),
                    sig1=sig1, live1=live1, sig2=sig2, live2=live2)

    def run(inp):
        from abnet3_amd.prefilter import diag_hits_batch, lsh_signatures
        from test_gpu_prefilter import dev_sig
        sig, live = lsh_signatures(dev(inp['table']), inp['planes'])
        best, diag, end1 = diag_hits_batch(dev_sig(inp['sig1']), dev(inp['live1'], np.uint8), inp['o1'], inp['n1'],
                                           dev_sig(inp['sig2']), dev(inp['live2'], np.uint8), inp['o2'], inp['n2'], mh, span, dilate)
        return dict(sig=host(sig).view(np.uint32), live=host(live), best=host(best), diag=host(diag), end1=host(end1))

    def oracle(inp, out):
        import prefilter_np
        from test_gpu_prefilter import assert_same
        ref_sig, ref_live, decided = prefilter_np.signatures(inp['table'], inp['planes'])
        alive = ref_live != 0
        assert np.array_equal(out['live'], ref_live) and not out['sig'][~alive].any() and (~alive).sum() == 4
        got, want = prefilter_np.unpack(out['sig'], 64)[alive], prefilter_np.unpack(ref_sig, 64)[alive]
        assert np.array_equal(got[decided[alive]], want[decided[alive]])
        ref = prefilter_np.diag_hits(inp['sig1'], inp['live1'], inp['o1'], inp['n1'], inp['sig2'], inp['live2'], inp['o2'], inp['n2'],
                                     mh, span, dilate, 0)
        assert_same((out['best'], out['diag'], out['end1']), ref)
        assert (out['best'] > 0).any()

    return Case('lsh', ('abn_lsh_signatures', 'abn_lsh_diag_hits_batched'), build, run, oracle)


def edit_case():
    """tde.edit_distance_batch on the short-side edges up to 64 of tests/test_gpu_tde.py:test_length_edges (the long side the
    same length, one more, 300) plus one pair beyond max_short (refused: -1), exactly tests/tde_np.py's Levenshtein rows."""
    max_short = 64

    def build():
        from test_gpu_tde import SHORT, tables
        rng = np.random.default_rng(max_short)
        seqs1, seqs2 = [], []
        for s in SHORT:
            if s <= max_short:
                for n in (s, s + 1, 300):
                    seqs1.append(rng.integers(0, 4, s))
                    seqs2.append(rng.integers(0, 4, n))
        seqs1.append(rng.integers(0, 4, 65))
        seqs2.append(rng.integers(0, 4, 70))
        return tables(seqs1) + tables(seqs2)

    def run(inp):
        from abnet3_amd.tde import edit_distance_batch
        f1, o1, n1, f2, o2, n2 = inp
        return dict(dist=host(edit_distance_batch(f1, o1, n1, f2, o2, n2, max_short=max_short)))

    def oracle(inp, out):
        import tde_np
        f1, o1, n1, f2, o2, n2 = inp
        ref = tde_np.edit_batch(f1, o1, n1, f2, o2, n2, max_short, distance=tde_np.levenshtein_rows)
        assert np.array_equal(out['dist'], ref) and out['dist'][-1] == -1 and (out['dist'][:-1] >= 0).all()

    return Case('edit-distance', ('abn_edit_distance_batched', 'abn_edit_max_short'), build, run, oracle)


SEARCH_CASES = [search_case(False), search_case(True), local_case(False), local_case(True), lsh_case(), edit_case()]



# ======================================================================================================================
# pair mining, samplers, same-different, ES-KMeans
# ======================================================================================================================
def knn_case():
    """discovery.knn_topk at nq = 33, nc = 257, d = 40, k = 10 with the overlap exclusion -- several candidate ranges, so the
    call has a workspace -- against tests/knn_np.py:check_topk (tests/test_gpu_knn.py:test_shapes_around_the_tile_edges)."""
    nq, nc, d, k = 33, 257, 40, 10

    def build():
        from test_gpu_knn import random_meta, unit_rows
        rng = np.random.default_rng(nq * 1009 + nc * 13 + d + k)
        C, basis = unit_rows(rng, nc, d)
        x = rng.standard_normal((nq, basis.shape[1])) @ basis.T
        Q = (x / np.sqrt((x * x).sum(1))[:, None]).astype(np.float32)
        return dict(Q=Q, C=C, qm=random_meta(rng, nq), cm=random_meta(rng, nc))

    def run(inp):
        from abnet3_amd import _lib
        from abnet3_amd.discovery import knn_topk
        assert _lib.load().abn_knn_ws_bytes(nq, nc, k) > 0
        idx, sim = knn_topk(dev(inp['Q']), dev(inp['C']), k, dev(inp['qm']), dev(inp['cm']))
        return dict(idx=host(idx), sim=host(sim))

    def oracle(inp, out):
        import knn_np
        S = inp['Q'].astype(np.float64) @ inp['C'].astype(np.float64).T
        knn_np.check_topk(out['idx'], out['sim'], S, k, knn_np.excluded(inp['qm'], inp['cm']), knn_np.delta(d))

    return Case('knn-topk', ('abn_knn_topk', 'abn_knn_ws_bytes'), build, run, oracle)


def segment_vectors_case():
    """discovery.segment_vectors on tests/test_gpu_knn.py:test_segment_vectors_bit_equal_gather's +-1 frames (K D = 1024: the
    gathered frames / 32 bit for bit), one file all zero: its segments are flagged and their rows are zero."""
    def build():
        import knn_np
        rng = np.random.default_rng(1)
        feats = [rng.choice([-1.0, 1.0], (int(n), 64)).astype(np.float32) for n in (90, 17, 64)]
        feats.append(np.zeros((50, 64), dtype=np.float32))
        segs = knn_np.segments([len(f) for f in feats], (16, 17, 40, 63), 3)
        off = np.concatenate(([0], np.cumsum([len(f) for f in feats])))
        return dict(feats=feats, segs=segs, row0=np.array([off[f] + s for f, s, L in segs], dtype=np.int64),
                    L=np.array([L for _, _, L in segs], dtype=np.int32))

    def run(inp):
        from abnet3_amd.discovery import segment_vectors
        vec, keep = segment_vectors(dev(np.concatenate(inp['feats'])), inp['row0'], inp['L'], 16)
        return dict(vec=host(vec), keep=host(keep))

    def oracle(inp, out):
        import knn_np
        g = knn_np.gather(inp['feats'], inp['segs'], 16)
        zero = np.array([f == 3 for f, _, _ in inp['segs']])
        assert np.array_equal(out['keep'], ~zero) and zero.any()
        assert np.array_equal(out['vec'][~zero], g[~zero] / np.float32(32.0)) and not out['vec'][zero].any()

    return Case('segment-vectors', ('abn_segment_vectors',), build, run, oracle)


def tcl_case():
    """abn_tcl_pairs, packed, 65 iterations over three files (31, 32 and 100000 frames) -- the entry as
    TemporalCoherenceDataLoader._tcl_fill calls it (its arrays belong to a loader's plan; here they come from torch.empty, 5 x 65
    entries exactly): bit for bit tests/tcl_np.py (tests/test_gpu_tcl.py:test_kernel_equals_the_restatement)."""
    n_iter, seed, epoch = 65, (7 << 32) + 5, 3

    def build():
        from test_gpu_tcl import _files
        row0, lens = _files(3, np.random.default_rng(3))
        return dict(row0=row0, lens=lens)

    def run(inp):
        import torch
        import tcl_np
        from abnet3_amd import _lib
        lens_h = np.ascontiguousarray(inp['lens'], dtype=np.int64)
        d_row0, d_len = dev(inp['row0'], np.int64), dev(lens_h)
        dl = np.asarray(tcl_np.DELTAS, dtype=np.int32)
        n = 5 * n_iter
        i1, i2 = torch.empty(n, dtype=torch.int64, device='cuda'), torch.empty(n, dtype=torch.int64, device='cuda')
        y = torch.empty(n, dtype=torch.float64, device='cuda')
        _lib.check(_lib.load().abn_tcl_pairs(_lib.ptr(d_row0), _lib.ptr(d_len), lens_h.ctypes.data, len(lens_h), dl.ctypes.data, len(dl), 1,
                                             n_iter, 0, seed, epoch, None, _lib.ptr(i1), _lib.ptr(i2), _lib.ptr(y), 1, n, _lib.stream()),
                   'abn_tcl_pairs')
        return dict(i1=host(i1), i2=host(i2), y=host(y))

    def oracle(inp, out):
        import tcl_np
        r1, r2, ry = tcl_np.tcl_pairs(inp['row0'], inp['lens'], n_iter, 0, seed, epoch, 5 * n_iter, label_dtype=np.float64)
        assert (out['i1'] == r1).all() and (out['i2'] == r2).all() and (out['y'] == ry).all()

    return Case('tcl-pairs', ('abn_tcl_pairs',), build, run, oracle)


def sample_pairs_case():
    """sampler.sample_pairs_device on the 'small' cluster fixture, counts around one wavefront: bit for bit
    tests/sampler_np.py (tests/test_gpu_sampler.py:test_kernel_equals_the_restatement_bit_for_bit)."""
    counts, seed, mode = (63, 64, 65, 1), (3 << 32) + 1, 'log'

    def build():
        import sampler_np
        from abnet3_amd import sampler as S
        from test_gpu_sampler import describe
        descr = describe('small')
        return dict(tables=S.build_tables(descr, mode, mode), want=sampler_np.sample_pairs(sampler_np.build_tables(descr, mode, mode), counts, seed))

    def run(inp):
        from abnet3_amd import sampler as S
        tok1, tok2, key = S.sample_pairs_device(S.DeviceTables(inp['tables']), counts, seed)
        return dict(tok1=host(tok1), tok2=host(tok2), key=host(key))

    def oracle(inp, out):
        from test_gpu_sampler import assert_same_bits
        assert_same_bits((out['tok1'], out['tok2'], out['key']), inp['want'], 'small')

    return Case('sample-pairs', ('abn_sample_pairs',), build, run, oracle)


def samediff_case():
    """samediff.collect and vector_histogram (abn_sd_collect, abn_sd_count) at n = 129, d = 36 on integer rows
    (tests/test_gpu_samediff.py:test_exact_arithmetic_inputs): the collected similarities EQUAL the integer dot products, the
    histogram and n_bad tests/samediff_np.py's."""
    n, d, condition = 129, 36, 'swdp'

    def build():
        from test_gpu_samediff import integer_rows, type_ranges
        rng = np.random.default_rng(1000 * n + d)
        X = integer_rows(rng, n, d)
        cbeg, cend = type_ranges(rng, n)
        return dict(X=X, cbeg=cbeg, cend=cend, spk=rng.integers(0, 2, n).astype(np.int32))

    def run(inp):
        from abnet3_amd import samediff
        X = dev(inp['X'])
        pos_sim, _ = samediff.collect(X, inp['cbeg'], inp['cend'])
        thr, hist, n_bad = samediff.vector_histogram(X, inp['cbeg'], inp['cend'], inp['spk'], condition)
        return dict(pos_sim=host(pos_sim), thr=host(thr), hist=host(hist), n_bad=np.array([n_bad]))

    def oracle(inp, out):
        import samediff_np
        X, cbeg, cend = inp['X'], inp['cbeg'], inp['cend']
        i, j = np.triu_indices(n, 1)
        S = (X.astype(np.float64) @ X.astype(np.float64).T).astype(np.float32)
        same = j < cend[i]
        assert np.array_equal(out['pos_sim'], S[i, j][same])
        ref_thr, ref_hist, ref_bad = samediff_np.buckets_hist(S[i, j], i, j, cbeg, cend, inp['spk'], condition)
        assert np.array_equal(out['thr'], ref_thr) and np.array_equal(out['hist'], np.array(ref_hist, dtype=np.int64))
        assert int(out['n_bad'][0]) == ref_bad == 0

    return Case('same-different', ('abn_sd_collect', 'abn_sd_count'), build, run, oracle)


def esk_score_case():
    """eskmeans.candidate_scores on tests/test_gpu_esk.py's layout (3, (40, 2, 7)) with the special rows (an all-zero
    segment, a NaN row, an infinite value), K = 129, 10 frames x D = 4, max_frames 15: ids and scores bit for bit the
    unfused route's (segment_vectors + kmeans.assign), that file's reference (check_fused)."""
    S, counts, K, frames, D, max_frames, seed = 3, (40, 2, 7), 129, 10, 4, 15, 10

    def build():
        import test_gpu_esk as E
        table, lm, lm_off = E.corpus(counts, D, seed)
        m, b = E.tables(K, frames * D, seed + 1)
        return dict(table=table, lm=lm, lm_off=lm_off, m=m, b=b)

    def run(inp):
        from abnet3_amd import eskmeans
        best, ids = eskmeans.candidate_scores(dev(inp['table']), inp['lm'], inp['lm_off'], dev(inp['m']), dev(inp['b']), frames, S, max_frames)
        return dict(best=host(best), ids=host(ids))

    def oracle(inp, out):
        import test_gpu_esk as E
        want_best, want_id, _, keep = E.unfused(inp['table'], inp['lm'], inp['lm_off'], inp['m'], inp['b'], frames, S, max_frames)
        assert np.array_equal(out['ids'], want_id) and E.same_bits(out['best'], want_best)
        assert np.array_equal(np.isnan(out['best']), out['ids'] < 0) and not keep.all()
        assert out['ids'][3 * S] == -1 and out['ids'][9 * S] == -1 and out['ids'][17 * S] == -1

    return Case('esk-score', ('abn_esk_score',), build, run, oracle)


def esk_segment_case():
    """eskmeans.segment_dp on tests/test_gpu_esk.py:exact_dp_case (utterances of 40, 2, 7 and 65 landmarks, S = 3, one
    utterance blocked: objective NaN, n_seg -1): every output equals tests/esk_np.py:dp."""
    S, counts = 3, (40, 2, 7, 65)

    def build():
        import test_gpu_esk as E
        return E.exact_dp_case(counts, S, seed=23, block=(2,))

    def run(inp):
        from abnet3_amd import eskmeans
        best, ids, lm, lm_off = inp
        out = eskmeans.segment_dp(dev(best), dev(ids, np.int32), lm, lm_off, S)
        return dict(zip(('cut', 'word', 'span', 'objective', 'n_seg'), (host(t) for t in out)))

    def oracle(inp, out):
        import esk_np
        best, ids, lm, lm_off = inp
        want = esk_np.dp(best, ids, lm, lm_off, S)
        for name, w in zip(('cut', 'word', 'span', 'objective', 'n_seg'), want):
            assert np.array_equal(out[name], w, equal_nan=True), name
        assert np.isnan(out['objective'][2]) and out['n_seg'][2] == -1

    return Case('esk-segment', ('abn_esk_segment',), build, run, oracle)


MINING_CASES = [knn_case(), segment_vectors_case(), tcl_case(), sample_pairs_case(), samediff_case(), esk_score_case(), esk_segment_case()]


# ======================================================================================================================
# mixtures, k-means, Baum-Welch statistics
# ======================================================================================================================
def gmm_case():
    """gmm.posteriors and gmm.em_iteration (abn_gmm_posteriors, _accumulate, _mstep) at T = 300, K = 130, D = 13, two frame
    ranges, a NaN row: tests/test_gpu_gmm.py's run_kernels (a fresh EMState: its workspace is allocated inside the window),
    check_case and check_mstep."""
    T, K, D, n_ranges = 300, 130, 13, 2

    def build():
        import test_gpu_gmm as G
        x, shift, gv, w, m, v = G.make_case(T, K, D, seed=T * 1000 + K)
        x[7, 3] = np.nan
        return dict(x=x, shift=shift, gv=gv, w=w, m=m, v=v)

    def run(inp):
        import test_gpu_gmm as G
        return G.run_kernels(inp['x'], inp['shift'], inp['gv'], inp['w'], inp['m'], inp['v'], n_ranges)

    def oracle(inp, out):
        import test_gpu_gmm as G
        G.check_case(out, G.reference(inp['x'], inp['shift'], inp['w'], inp['m'], inp['v']), K, D, 'dirty memory')
        G.check_mstep(out, inp['gv'], inp['m'], inp['v'])
        assert out['stats'][1] == 1

    return Case('gmm', ('abn_gmm_posteriors', 'abn_gmm_accumulate', 'abn_gmm_mstep', 'abn_gmm_ws_bytes'), build, run, oracle)


def kmeans_case():
    """kmeans.assign and kmeans.accumulate (abn_kmeans_assign, _accumulate, _update) at T = 300, K = 129, D = 33, three
    frame ranges, a NaN row: tests/test_gpu_kmeans.py:check_iteration.  That file's run_kernels hands the kernels a zeroed
    workspace; here LloydState's is the torch.empty one kmeans.accumulate allocates (the partials themselves, whose padding
    nobody reads, are not an output)."""
    T, K, D, n_ranges = 300, 129, 33, 3

    def build():
        import test_gpu_kmeans as KM
        x, _, shift, mu = KM.make_case(T, K, D, seed=T * 1000 + K + D)
        x[11, 2] = np.nan
        return dict(x=x, shift=shift, mu=mu)

    def run(inp):
        from abnet3_amd import kmeans
        table, dshift = dev(inp['x']), dev(inp['shift'])
        st = kmeans.LloydState(inp['mu'], T, table.device, 'euclidean')
        m0, b0 = host(st.m), host(st.b)
        _, best = kmeans.assign(table, dshift, st.m, st.b, ids=st.ids, want_best=True)
        kmeans.accumulate(table, dshift, st, n_ranges)
        return dict(ids=host(st.ids), best=host(best), sums=host(st.sums), stats=host(st.stats), mu=host(st.mu), m=host(st.m),
                    b=host(st.b), m0=m0, b0=b0)

    def oracle(inp, out):
        import test_gpu_kmeans as KM
        KM.check_iteration(inp['x'], inp['shift'], inp['mu'], out)
        assert out['ids'][11] == -1 and out['stats'][1] == 1

    return Case('kmeans', ('abn_kmeans_assign', 'abn_kmeans_accumulate', 'abn_kmeans_update', 'abn_kmeans_ws_bytes'), build, run, oracle)


def hmm_accumulate_case():
    """hmm.accumulate at T = 129, K = 130, D = 5, three frame ranges on exact arithmetic
    (tests/test_gpu_hmm_bw.py:test_accumulate_is_exact_on_exact_arithmetic), one non-finite entry (it contributes 0): exact."""
    T, K, D, n_ranges = 129, 130, 5, 3

    def build():
        rng = np.random.default_rng(T)
        post = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(T, K))
        x = rng.integers(-8, 9, size=(T, D)).astype(np.float32)
        x[5, 0] = np.nan
        return dict(post=post, x=x, shift=rng.integers(-3, 4, size=D).astype(np.float32))

    def run(inp):
        from abnet3_amd import hmm
        return dict(sums=host(hmm.accumulate(dev(inp['x']), dev(inp['post']), dev(inp['shift']), n_ranges)))

    def oracle(inp, out):
        from test_gpu_hmm_bw import augment_elementwise
        want = inp['post'].astype(np.float64).T @ augment_elementwise(inp['x'], inp['shift'])
        assert out['sums'].shape == (K, 2 * D + 1) and np.array_equal(out['sums'], want)

    return Case('hmm-accumulate', ('abn_hmm_accumulate', 'abn_hmm_accumulate_ws_bytes'), build, run, oracle)


MODEL_CASES = [gmm_case(), kmeans_case(), hmm_accumulate_case()]


# ======================================================================================================================
# the per-utterance chain kernels
# ======================================================================================================================
CHAIN_LENS = np.array([1, 127, 129, 300])
CHAIN_D = 13
CHAIN_KS = (5, 130, 300)            # the LDS slab, the workspace slab with ks = 256, NQ = 2


def chain_layout():
    """(off, T): the utterances end to end, with 5 rows nobody owns between the second and the third, and 3 behind the last."""
    off = np.array([0, 1, 1 + 127 + 5, 1 + 127 + 5 + 129], dtype=np.int64)
    return off, int(off[-1] + CHAIN_LENS[-1] + 3)


CHAIN_BAD = 1 + 127 + 5 + 64        # a BAD frame in the middle of the 129-frame utterance


def inside_rows(off, lens, T):
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    return inside


def kmeans_viterbi_inputs(K):
    import units_np
    off, T = chain_layout()
    x, m, b, s = units_np.exact_case(T, K, CHAIN_D, seed=100 * K + CHAIN_D)
    good = np.ones(T, dtype=bool)
    x[CHAIN_BAD, CHAIN_D // 2] = np.nan
    good[CHAIN_BAD] = False
    return dict(x=x, m=m, b=b, s=s, good=good, off=off, T=T)


def kmeans_viterbi_run(inp, ids=None, penalty=3.0):
    from abnet3_amd import kmeans
    shift = dev(np.zeros(CHAIN_D, dtype=np.float32))
    got = kmeans.viterbi(dev(inp['x']), inp['off'], CHAIN_LENS, shift, dev(inp['m']), dev(inp['b']), penalty, ids=ids, want_objective=True)
    return dict(ids=host(got[0]), objective=host(got[1]), n_switch=host(got[2]))


def kmeans_viterbi_case(K):
    """kmeans.viterbi on tests/units_np.py:exact_case, penalty 3: ids, objective and n_switch EQUAL tests/units_np.py:viterbi
    (tests/test_gpu_units.py:check_exact); the BAD frame gets -1, rows outside every utterance keep the fresh ids' -1."""
    def oracle(inp, out):
        import units_np
        ref = units_np.viterbi(inp['s'], inp['good'], inp['off'], CHAIN_LENS, units_np.score_penalty(3.0), ids=np.full(inp['T'], -1, dtype=np.int32))
        assert np.array_equal(out['ids'], ref[0]) and np.array_equal(out['objective'], ref[1]) and np.array_equal(out['n_switch'], ref[2])
        assert out['ids'][CHAIN_BAD] == -1

    return Case('chain-kmeans-viterbi-K%d' % K, ('abn_kmeans_viterbi', 'abn_kmeans_viterbi_ws_bytes'), lambda: kmeans_viterbi_inputs(K),
                kmeans_viterbi_run, oracle)


def hmm_viterbi_inputs(K):
    from test_gpu_hmm_vit import exact_case
    off, T = chain_layout()
    c = exact_case(T, K, CHAIN_D, seed=100 * K + CHAIN_D)
    good = np.ones(T, dtype=bool)
    c['x'][CHAIN_BAD, CHAIN_D // 2] = np.nan
    good[CHAIN_BAD] = False
    c.update(good=good, off=off, T=T)
    return c


def hmm_viterbi_run(c, ids=None):
    from abnet3_amd import hmm
    shift = dev(np.zeros(CHAIN_D, dtype=np.float32))
    got = hmm.viterbi(dev(c['x']), c['off'], CHAIN_LENS, shift, dev(c['A']), dev(c['B']), dev(c['c0']), dev(c['lw']), dev(c['ls']),
                      dev(c['lr']), ids=ids)
    return dict(ids=host(got[0]), log_prob=host(got[1]), n_switch=host(got[2]), n_good=host(got[3]))


def hmm_viterbi_case(K):
    """hmm.viterbi on tests/test_gpu_hmm_vit.py:exact_case: ids, log_prob, n_switch and n_good EQUAL tests/hmm_vit_np.py:viterbi
    (check_exact of that file)."""
    def oracle(c, out):
        import hmm_vit_np
        ref = hmm_vit_np.viterbi(c['s'], c['good'], c['off'], CHAIN_LENS, c['lw'], c['ls'], c['lr'])
        inside = inside_rows(c['off'], CHAIN_LENS, c['T'])
        assert np.array_equal(out['ids'][inside], ref[0][inside]) and (out['ids'][~inside] == -1).all() and out['ids'][CHAIN_BAD] == -1
        assert np.array_equal(out['log_prob'], ref[1]) and np.array_equal(out['n_switch'], ref[2]) and np.array_equal(out['n_good'], ref[3])
        assert out['n_good'].tolist() == [1, 127, 128, 300]

    return Case('chain-hmm-viterbi-K%d' % K, ('abn_hmm_viterbi', 'abn_hmm_viterbi_ws_bytes'), lambda: hmm_viterbi_inputs(K), hmm_viterbi_run, oracle)


CHAIN_RHO = 0.9


def hmm_fb_inputs(K):
    """A model and a corpus of tests/test_gpu_hmm.py (make_model): `case` is that file's Case over the utterances laid end to
    end (its references index rows that way); `x` is the same frames in chain_layout(), the rows nobody owns filled with noise."""
    from test_gpu_hmm import Case as HmmCase, make_model
    off, T = chain_layout()
    n = int(CHAIN_LENS.sum())
    xs, shift, w, m, v = make_model(n, K, CHAIN_D, seed=1000 * K + CHAIN_D)
    compact_off = np.cumsum(CHAIN_LENS) - CHAIN_LENS
    xs[compact_off[2] + 64, 0] = np.nan
    x = np.random.default_rng(K).standard_normal((T, CHAIN_D)).astype(np.float32)
    for o, co, ln in zip(off, compact_off, CHAIN_LENS):
        x[o:o + ln] = xs[co:co + ln]
    assert np.isnan(x[CHAIN_BAD, 0])
    return dict(case=HmmCase(xs, shift, w, m, v, CHAIN_LENS), x=x, off=off, T=T, compact_off=compact_off, K=K)


def hmm_fb_run(inp, mode='smooth', want_stay_k=False, out=None):
    from abnet3_amd import hmm
    d = inp['case'].d
    got = hmm.forward_backward(dev(inp['x']), inp['off'], CHAIN_LENS, d['shift'], d['A'], d['B'], d['c0'], d['w'], CHAIN_RHO, mode,
                               out=out, want_stay_k=want_stay_k)
    res = dict(post=host(got[0]), loglik=host(got[1]), stays=host(got[2]), n_good=host(got[3]))
    if want_stay_k:
        res['stay_k'] = host(got[4])
    return res


def hmm_fb_case(K, stats):
    """hmm.forward_backward (modes 0 and 1; `stats`: with stay_k, abn_hmm_forward_backward_stats) under rho = 0.9 against the
    float64 restatement at the bars of tests/test_gpu_hmm.py:check_against_reference; stay_k at the bar of
    tests/test_gpu_hmm_bw.py (n_good expm1(2 S)); rows nobody owns keep the fresh table's zeros.  (Float data: the restatement of
    this recursion is held to derived bars, not to equality; the kernel's own bits are held equal across the runs.)"""
    def run(inp):
        out = {}
        for mode in ('smooth', 'filter'):
            out.update({mode + '.' + k: v for k, v in hmm_fb_run(inp, mode, stats).items()})
        return out

    def oracle(inp, out):
        from test_gpu_hmm import check_against_reference
        case, off = inp['case'], inp['off']
        inside = inside_rows(off, CHAIN_LENS, inp['T'])
        for mode in ('smooth', 'filter'):
            got = {k: out[mode + '.' + k] for k in ('post', 'loglik', 'stays', 'n_good')}
            assert not got['post'][~inside].any()
            got['post'] = np.concatenate([got['post'][o:o + n] for o, n in zip(off, CHAIN_LENS)])
            check_against_reference(case, got, CHAIN_RHO, mode == 'smooth', 'dirty memory K%d %s' % (K, mode))
            assert got['n_good'].tolist() == [1, 127, 128, 300]
        if stats:
            import hmm_bw_np
            r = case.scores()
            S = case.per_utterance(r['eps'] + r['delta'])
            bar = out['smooth.n_good'] * np.expm1(2.0 * S)
            ref = np.array([hmm_bw_np.forward_backward(r['s64'][o:o + n], case.bad[o:o + n], case.w32, CHAIN_RHO)['stay_k']
                            for o, n in zip(case.off, case.lens)])
            sk = out['smooth.stay_k']
            assert np.isfinite(sk).all() and (sk >= 0).all() and (np.abs(sk - ref) <= bar[:, None]).all()
            assert (np.abs(sk.sum(axis=1) - out['smooth.stays']) <= bar).all() and not out['filter.stay_k'].any()

    entries = ('abn_hmm_forward_backward_stats' if stats else 'abn_hmm_forward_backward', 'abn_hmm_ws_bytes')
    return Case('chain-hmm-fb-%sK%d' % ('stats-' if stats else '', K), entries, lambda: hmm_fb_inputs(K), run, oracle)


CHAIN_CASES = [f(K) for K in CHAIN_KS for f in (kmeans_viterbi_case, hmm_viterbi_case, lambda K: hmm_fb_case(K, False),
                                                lambda K: hmm_fb_case(K, True))]

CASES = TOWER_CASES + LOSS_CASES + FRONT_CASES + DTW_CASES + SEARCH_CASES + MINING_CASES + MODEL_CASES + CHAIN_CASES
assert len({c.name for c in CASES}) == len(CASES)


# ======================================================================================================================
# the tests
# ======================================================================================================================
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_entry_on_dirty_memory(case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    runs = {}
    for byte in dirty_memory.PATTERNS:
        out, count, calls = run_dirty(case, byte)
        assert int(count) > 0, 'no allocation of this case went through torch.empty: the window is vacuous'
        missing = set(case.entries) - set(calls)
        assert not missing, 'the case claims entries it did not reach: %s (called: %s)' % (sorted(missing), sorted(set(calls)))
        runs[byte] = out
    anchor = runs.get(0xFF, runs[dirty_memory.PATTERNS[-1]])
    case.oracle(case.inputs(), anchor)                               # anchored to the reference, not to the library's own clean run
    if case.same_bits:
        first = dirty_memory.PATTERNS[0]
        for byte in dirty_memory.PATTERNS[1:]:
            assert_same_bits(runs[first], runs[byte], '%s: 0x%02X against 0x%02X memory' % (case.name, first, byte))
    else:
        for byte, out in runs.items():
            case.oracle(case.inputs(), out)


# ======================================================================================================================
# caller-supplied and wrapper-zeroed outputs of the chain entries (K = 130)
# ======================================================================================================================
# The wrappers torch.zeros / torch.full their own per-row and per-utterance outputs: the window cannot reach them, and the
# zeros hide whether the kernel writes them.  (a) ids= / out= filled with 0xC2 bytes: rows inside the utterances equal the
# clean run, rows outside keep the pattern bit for bit.  (b) the raw entries, the way
# tests/test_gpu_hmm_vit.py:test_refused_utterances_and_refusals_at_the_raw_entry calls one, every per-utterance output filled
# with 0xC2, one utterance outside the table and one longer than the workspace was sized for: valid utterances equal the
# clean run, refused ones hold exactly what the header states (NaN / -1), no pattern byte survives.
PATTERN = 0xC2
K4 = 130


def filled(shape, dtype):
    import torch
    return dirty_memory.fill_bytes(torch.empty(shape, dtype=dtype, device='cuda'), PATTERN)


def pattern_of(a):
    return np.frombuffer(bytes([PATTERN]) * a.dtype.itemsize, dtype=bits(a).dtype)[0]


def holds_pattern(a):
    return bits(a) == pattern_of(a)


def check_rows_kept(got, clean, inside, what):
    assert np.array_equal(bits(got[inside]), bits(clean[inside])), what
    assert holds_pattern(got[~inside]).all(), what + ': a row outside every utterance was written'


@pytest.mark.parametrize('entry', ['kmeans_viterbi', 'hmm_viterbi', 'hmm_forward_backward', 'hmm_forward_backward_stats'])
def test_caller_supplied_rows_outside_the_utterances_keep_their_bytes(entry):
    import torch
    off, T = chain_layout()
    inside = inside_rows(off, CHAIN_LENS, T)
    if entry == 'kmeans_viterbi':
        inp = kmeans_viterbi_inputs(K4)
        clean, got = kmeans_viterbi_run(inp), kmeans_viterbi_run(inp, ids=filled((T,), torch.int32))
        check_rows_kept(got['ids'], clean['ids'], inside, entry)
        rest = ('objective', 'n_switch')
    elif entry == 'hmm_viterbi':
        inp = hmm_viterbi_inputs(K4)
        clean, got = hmm_viterbi_run(inp), hmm_viterbi_run(inp, ids=filled((T,), torch.int32))
        check_rows_kept(got['ids'], clean['ids'], inside, entry)
        rest = ('log_prob', 'n_switch', 'n_good')
    else:
        inp, stats = hmm_fb_inputs(K4), entry.endswith('stats')
        rest = ('loglik', 'stays', 'n_good') + (('stay_k',) if stats else ())
        for mode in ('smooth', 'filter'):
            clean, got = hmm_fb_run(inp, mode, stats), hmm_fb_run(inp, mode, stats, out=filled((T, K4), torch.float32))
            check_rows_kept(got['post'], clean['post'], inside, entry + ' ' + mode)
            for k in rest:
                assert np.array_equal(bits(got[k]), bits(clean[k])), (entry, mode, k)
        return
    for k in rest:
        assert np.array_equal(bits(got[k]), bits(clean[k])), (entry, k)


@pytest.mark.parametrize('entry', ['kmeans_viterbi', 'hmm_viterbi', 'hmm_forward_backward', 'hmm_forward_backward_stats'])
def test_raw_entry_overwrites_every_per_utterance_output(entry):
    import torch
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    off, T = chain_layout()
    D, K, n_ok = CHAIN_D, K4, len(CHAIN_LENS)
    # utterances 0 .. 3 as in the cases; 4: past the table's end; 5: inside the table, longer than the workspace holds
    offs = np.concatenate([off, [T - 3, 0]]).astype(np.int64)
    lens = np.concatenate([CHAIN_LENS, [4, 400]]).astype(np.int32)
    n_utt, sized_for = len(lens), int(CHAIN_LENS.max())
    assert 400 <= T
    off_d, len_d = dev(offs), dev(lens)
    shift = dev(np.zeros(D, dtype=np.float32))
    f64 = lambda *shape: filled(shape, torch.float64)
    i32 = lambda *shape: filled(shape, torch.int32)

    def workspace(fn):
        need = int(fn(n_utt, sized_for, K, D))
        assert need > 0
        return torch.empty(need, dtype=torch.uint8, device='cuda'), need

    if entry == 'kmeans_viterbi':
        inp = kmeans_viterbi_inputs(K)
        clean = kmeans_viterbi_run(inp)
        ids, out = torch.full((T,), -1, dtype=torch.int32, device='cuda'), dict(objective=f64(n_utt), n_switch=i32(n_utt))
        ws, need = workspace(lib.abn_kmeans_viterbi_ws_bytes)
        x, m, b = dev(inp['x']), dev(inp['m']), dev(inp['b'])                # (named: alive until the call has run)
        rc = lib.abn_kmeans_viterbi(p(x), T, D, p(off_d), p(len_d), n_utt, p(shift), p(m), p(b), K,
                                    float(np.float32(1.5)), p(ids), p(out['objective']), p(out['n_switch']), p(ws), need, _lib.stream())
        rows, refused = ('ids', ids), dict(objective=np.nan, n_switch=-1)
    elif entry == 'hmm_viterbi':
        c = hmm_viterbi_inputs(K)
        clean = hmm_viterbi_run(c)
        ids, out = torch.full((T,), -1, dtype=torch.int32, device='cuda'), dict(log_prob=f64(n_utt), n_switch=i32(n_utt), n_good=i32(n_utt))
        ws, need = workspace(lib.abn_hmm_viterbi_ws_bytes)
        t = {k: dev(c[k]) for k in ('x', 'A', 'B', 'c0', 'lw', 'ls', 'lr')}    # (named: alive until the call has run)
        rc = lib.abn_hmm_viterbi(p(t['x']), T, D, p(off_d), p(len_d), n_utt, p(shift), p(t['A']), p(t['B']), p(t['c0']),
                                 p(t['lw']), p(t['ls']), p(t['lr']), K, p(ids), p(out['log_prob']), p(out['n_switch']),
                                 p(out['n_good']), p(ws), need, _lib.stream())
        rows, refused = ('ids', ids), dict(log_prob=np.nan, n_switch=-1, n_good=-1)
    else:
        stats = entry.endswith('stats')
        inp = hmm_fb_inputs(K)
        d = inp['case'].d
        clean = hmm_fb_run(inp, 'smooth', stats)
        post = torch.zeros((T, K), dtype=torch.float32, device='cuda')
        out = dict(loglik=f64(n_utt), stays=f64(n_utt), n_good=i32(n_utt))
        refused = dict(loglik=np.nan, stays=np.nan, n_good=-1)
        if stats:
            out['stay_k'], refused['stay_k'] = f64(n_utt, K), np.nan
        ws, need = workspace(lib.abn_hmm_ws_bytes)
        x = dev(inp['x'])
        head = [p(x), T, D, p(off_d), p(len_d), n_utt, p(d['shift']), p(d['A']), p(d['B']), p(d['c0']), p(d['w']), K, CHAIN_RHO, 0,
                p(post), p(out['loglik']), p(out['stays']), p(out['n_good'])]
        tail = [p(ws), need, _lib.stream()]
        rc = lib.abn_hmm_forward_backward_stats(*(head + [p(out['stay_k'])] + tail)) if stats else lib.abn_hmm_forward_backward(*(head + tail))
        rows = ('post', post)
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(rows[1])), bits(clean[rows[0]])), 'the refused utterances touched rows'
    for k, t in out.items():
        got = host(t)
        assert np.array_equal(bits(got[:n_ok]), bits(clean[k])), (entry, k, got[:n_ok], clean[k])
        want = refused[k]
        assert (np.isnan(got[n_ok:]).all() if isinstance(want, float) else (got[n_ok:] == want).all()), (entry, k, got[n_ok:])
        assert not holds_pattern(got).any(), (entry, k, 'a byte pattern survived the call')
