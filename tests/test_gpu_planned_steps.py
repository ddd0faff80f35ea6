"""Planned training passes (TrainerSiamese._run_planned: ragged batches in 32-pair buckets, a captured step per bucket, the
batch read from the pass's plan through an abn_step_source) held step by step against the numpy oracle on host-gathered
batches (tests/plan_np.py): every step trains on ITS batch, labels and pair count, under every documented switch; the
sourced kernels alone at the bucket edges; the lifetime of the forward workspace a deferred backward lends to the
optimizer's launch.  Needs an MI355X: -m gpu."""
import gc
import weakref

import numpy as np
import pytest
import torch

import plan_np
from conftest import check_grads, check_params, rel_err

pytestmark = pytest.mark.gpu

KW = dict(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=32, activation_layer='sigmoid', p_dropout=0.0)
KW_C5 = dict(input_dim=280, num_hidden_layers=2, hidden_dim=500, output_dim=100, activation_layer='sigmoid', p_dropout=0.0)
LOSS_TOL = 2e-5          # per-step loss against the oracle (the bar test_planned_passes_train_like_the_iterator holds losses to)
NP_DTYPE = {'float64': np.float64, 'float32': np.float32, 'int64': np.int64, 'int8': np.int8}
_CACHE = {}              # references are computed once and shared (never written to afterwards)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _spec(kw):
    from oracle import siamese_np as O
    return O.TowerSpec(kw['input_dim'], kw['num_hidden_layers'], kw['hidden_dim'], kw['output_dim'], kw['activation_layer'],
                       kw.get('batch_norm', False))


def host_params(kw, seed=0, gain=4.0):
    """A state_dict in numpy.  Sigmoid towers at torch's default initialisation map every frame to nearly the same
    embedding (cosines of 0.999: a lone 'same' pair's loss (1 - cos) / 2 is then a cancelled 1e-4 no fp32 kernel holds to
    2e-5 of itself); wider weights, centred on the sigmoid's mean output, spread the cosines over 0.7 .. 0.97."""
    spec, rng, p = _spec(kw), np.random.default_rng(seed), {}
    for l in range(spec.n_layers):
        W = (gain * rng.standard_normal((spec.dims[l + 1], spec.dims[l])) / np.sqrt(spec.dims[l])).astype(np.float32)
        b = (0.3 * rng.standard_normal(spec.dims[l + 1])).astype(np.float32)
        if l > 0:
            b = (b - 0.5 * W.sum(axis=1)).astype(np.float32)
        p[spec.lin_keys[l] + '.weight'], p[spec.lin_keys[l] + '.bias'] = W, b
        if spec.batch_norm:
            w = spec.dims[l + 1]
            k = spec.bn_keys[l]
            p[k + '.weight'], p[k + '.bias'] = np.ones(w, np.float32), np.zeros(w, np.float32)
            p[k + '.running_mean'], p[k + '.running_var'] = np.zeros(w, np.float32), np.ones(w, np.float32)
            p[k + '.num_batches_tracked'] = np.array(0, dtype=np.int64)
    return p


def cuda_net(kw, params):
    from abnet3_amd.model import SiameseNetwork
    net = SiameseNetwork(**kw)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return net.cuda().train()


def copy_of(params):
    return {k: np.array(v) for k, v in params.items()}


def state_np(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def make_trainer(net, plan, oname, lr, loss, momentum=0.9):
    from abnet3_amd.trainer import TrainerSiamese
    tr = TrainerSiamese(network=net, loss=loss, optimizer_type=oname, lr=lr, momentum=momentum, dataloader=plan_np.PlanLoader(plan),
                        log_dir='/tmp/abn_runs')
    net.train()
    return tr


def run_pass(tr, plan):
    """tr._run_planned(plan) with the pass's loss accumulator read before every step and once after the pass: the
    differences are the steps' losses.  Returns (losses, the forward path noted after each step)."""
    from abnet3_amd import _lib
    reads, paths, state = [], [], {'depth': 0, 'refused': False}
    planned, stepped = tr._planned_step, tr.train_step

    def planned_step(*a, **k):
        reads.append(float(tr._loss_acc))
        state['depth'] += 1
        try:
            done = planned(*a, **k)
        finally:
            state['depth'] -= 1
        state['refused'] = not done
        if done:
            paths.append(_lib.last_forward_path())
        return done

    def train_step(*a, **k):
        if state['depth'] == 0:                  # the iterator's step on a batch the padded form was refused for
            if not state['refused']:
                reads.append(float(tr._loss_acc))
            state['refused'] = False
            out = stepped(*a, **k)
            paths.append(_lib.last_forward_path())
            return out
        return stepped(*a, **k)
    tr._planned_step, tr.train_step = planned_step, train_step
    try:
        total = torch.zeros((), dtype=torch.float64, device='cuda')
        tr.network.train()
        assert tr._run_planned(plan, True, total) == len(plan.order)
    finally:
        del tr._planned_step, tr.train_step
    reads.append(float(tr._loss_acc))
    assert float(total) == reads[-1] and len(reads) == len(plan.order) + 1
    return np.diff(reads), paths


def run_iterator(tr):
    """The same plan through the plain iterator (planned_passes = False): the step the goldens pin."""
    tr.planned_passes = False
    assert tr._planned(True) is None
    tr.network.train()
    return np.array([float(tr.train_step_auto(batch)) for batch in tr._batches(True)])


def check_losses(got, want, tag):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    nan, zero = np.isnan(want), want == 0                       # (a batch of no pairs: a mean of nothing, a sum of nothing)
    assert np.isnan(got[nan]).all() and (got[zero] == 0).all(), (tag, got[nan | zero])
    real = ~(nan | zero)
    err = np.abs(got[real] - want[real]) / np.abs(want[real])
    print('%s: per-step loss, worst relative error %.3g over %d steps' % (tag, err.max(), real.sum()))
    assert (err <= LOSS_TOL).all(), (tag, int(np.argmax(err)), err.max(), got[real][:6], want[real][:6])


def frozen_reference(name, kw, sizes, dtype='float64', seed=1, **plan_kw):
    """(host plan, oracle loss of every step) for a pass that leaves the parameters alone."""
    def make():
        host = plan_np.host_plan(np.random.default_rng(seed), kw['input_dim'], sizes, NP_DTYPE[dtype], **plan_kw)
        losses, _ = plan_np.oracle_pass(copy_of(_cached(('params', str(kw)), lambda: host_params(kw))), host, _spec(kw), None,
                                        'coscos2', 0.5, False)
        return host, losses
    return _cached(('frozen', name, str(kw), dtype, seed), make)


def params_of(kw):
    return _cached(('params', str(kw)), lambda: host_params(kw))


def graphs_of(tr):
    return {k: b['graph'][0] for k, b in tr._buckets.items() if b['graph'] is not None}


# ---- (a) batch identity with frozen parameters ---------------------------------------------------------------------------------
SIZES_A = [1, 31, 32, 33, 64, 65, 33, 96, 1, 64, 200, 32, 31, 65]
SWITCHES = [None, 'ABN_FUSED_STEP', 'ABN_WGRAD_STEP', 'ABN_STEP_SOURCE', 'ABN_LOSS_IN_BACKWARD', 'ABN_WIDE']
# 0 here and the padded step is refused on the pass's first batch: the whole pass takes the iterator's step (_plan_refused)
REFUSED_UNDER = ('ABN_LOSS_IN_BACKWARD', 'ABN_WIDE')


@pytest.mark.parametrize('dtype', ['float64', 'float32', 'int64', 'int8'])
@pytest.mark.parametrize('switch', SWITCHES)
def test_every_step_sees_its_own_batch(switch, dtype, monkeypatch):
    """lr = 0: the parameters never move, so step k's loss is the oracle's forward loss of batch k and of no other --
    a step that read another entry of the step table, another label offset or another pair count shows at once.  The
    sizes straddle every 32-pair bucket edge; the first pass runs each bucket eagerly, captures it and replays it, the
    second pass on the same plan replays from step 0 again, the third pass reads a NEW plan's arrays."""
    from abnet3_amd import _lib
    from abnet3_amd.loss import coscos2
    if switch:
        monkeypatch.setenv(switch, '0')
    host, want = frozen_reference('a', KW, SIZES_A, dtype)
    host3, want3 = frozen_reference('a', KW, SIZES_A, dtype, seed=7)
    net = cuda_net(KW, params_of(KW))
    plan = plan_np.upload(host)
    tr = make_trainer(net, plan, 'sgd', 0.0, coscos2(avg=False), momentum=0.0)
    before = net.flat_parameters().clone()
    refused, sourced = switch in REFUSED_UNDER, switch not in REFUSED_UNDER + ('ABN_STEP_SOURCE',)
    for rep in range(2):
        losses, paths = run_pass(tr, plan)
        check_losses(losses, want, 'pass %d, %s=0, %s labels' % (rep, switch, dtype))
        assert bool(getattr(tr, '_plan_refused', False)) == refused
        if refused:
            assert not graphs_of(tr)
            continue
        assert len(graphs_of(tr)) == len(tr._buckets) == 4
        assert all((b['source'] is not None) == sourced for b in tr._buckets.values())
        assert all(p == _lib.PATH_WIDE for p in paths)
        if sourced:
            assert int(tr._src['ctr']) == len(SIZES_A)          # moved once per step, whichever launch ended the step
    old = None if refused else graphs_of(tr)
    plan3 = plan_np.upload(host3)
    losses, _ = run_pass(tr, plan3)
    check_losses(losses, want3, 'new plan, %s=0, %s labels' % (switch, dtype))
    if sourced:                                                  # captured steps held the old arrays' addresses: all recaptured
        new = graphs_of(tr)
        assert len(new) == 4 and all(new[k] is not old[k] for k in new)
        assert int(tr._src['ctr']) == len(SIZES_A)
    assert torch.equal(net.flat_parameters(), before)
    del plan                                                     # (alive until here: the new plan's arrays are other addresses)


# ---- (b) the optimizer matrix with live parameters -----------------------------------------------------------------------------
SIZES_B = [33, 64, 31, 96, 33, 64, 1, 96, 65, 32, 33, 64]
LR = {'sgd': 0.01, 'adadelta': 0.1, 'adagrad': 0.001, 'RMSprop': 0.001, 'adam': 0.001}
STEPS_B = {'sgd': 12, 'adadelta': 12, 'adagrad': 12, 'RMSprop': 12, 'adam': 12}
PARAM_TOL = {'sgd': 1e-5, 'adadelta': 1e-5, 'adagrad': 3e-4, 'RMSprop': 3e-4, 'adam': 3e-4}      # tests/test_gpu_timed_path.py, against the reference
PLAIN = ('coscos2', False, 0.5)
CASES_B = ([(o, s, PLAIN) for o in LR for s in (None, 'ABN_FUSED_STEP')]
           + [(o, s, PLAIN) for o in ('sgd', 'adadelta') for s in ('ABN_WGRAD_STEP', 'ABN_STEP_SOURCE')]
           + [(o, s, l) for o in ('sgd', 'adadelta') for s in (None, 'ABN_FUSED_STEP')
              for l in (('coscos2', True, 0.5), ('cosmargin', True, 0.3))])


def live_reference(kw, sizes, oname, loss, seed=3):
    def make():
        from oracle import siamese_np as O
        host = plan_np.host_plan(np.random.default_rng(seed), kw['input_dim'], sizes)
        losses, after = plan_np.oracle_pass(copy_of(params_of(kw)), host, _spec(kw), O.Optimizer(oname, LR[oname]), loss[0], loss[2], loss[1])
        return host, losses, after
    return _cached(('live', str(kw), tuple(sizes), oname, loss, seed), make)


@pytest.mark.parametrize('oname,switch,loss', CASES_B, ids=lambda v: str(v).replace(' ', ''))
def test_a_planned_pass_trains_like_the_oracle(oname, switch, loss, monkeypatch):
    """Live parameters: per-step losses and the parameters after the pass against the oracle's pass over the same plan,
    for every update rule; a mean loss on a sourced step divides by the real pair count of the step table.  The iterator's
    pass over the same plan is held to the same oracle at the same bars in the same test: the bars are the ones the
    iterator's step meets against the reference's goldens, not ones fitted to the planned pass."""
    import abnet3_amd.loss as L
    if switch:
        monkeypatch.setenv(switch, '0')
    sizes = SIZES_B[:STEPS_B[oname]]
    host, want, after = live_reference(KW, sizes, oname, loss)
    keys = _spec(KW).param_keys()
    make_loss = lambda: getattr(L, loss[0])(avg=loss[1], margin=loss[2]) if loss[0] == 'cosmargin' else getattr(L, loss[0])(avg=loss[1])
    # the iterator first: it validates the bars
    plan = plan_np.upload(host)
    net = cuda_net(KW, params_of(KW))
    tr = make_trainer(net, plan, oname, LR[oname], make_loss())
    check_losses(run_iterator(tr), want, 'iterator, %s' % oname)
    mine = state_np(net)
    print('iterator, %s: worst parameter error %.3g' % (oname, max(rel_err(mine[k], after[k]) for k in keys)))
    check_params(mine, after, keys, False, PARAM_TOL[oname])
    # the planned pass
    net = cuda_net(KW, params_of(KW))
    tr = make_trainer(net, plan, oname, LR[oname], make_loss())
    losses, _ = run_pass(tr, plan)
    check_losses(losses, want, 'planned, %s, %s=0, %s' % (oname, switch, loss))
    assert not getattr(tr, '_plan_refused', False) and len(graphs_of(tr)) == 3
    sourced = oname != 'adam' and switch != 'ABN_STEP_SOURCE'
    assert all((b['source'] is not None) == sourced for b in tr._buckets.values())
    if sourced:
        assert int(tr._src['ctr']) == len(sizes)
    assert tr.optimizer.step_count == len(sizes)
    mine = state_np(net)
    print('planned, %s, %s=0: worst parameter error %.3g' % (oname, switch, max(rel_err(mine[k], after[k]) for k in keys)))
    check_params(mine, after, keys, False, PARAM_TOL[oname])


# ---- (c) mixed buckets and odd cases ---------------------------------------------------------------------------------------------
SIZES_C = [33, 1570, 31, 0, 64, 33, 1570, 64, 32]


def test_sourced_and_gathered_buckets_share_one_pass():
    """A 1570-pair batch (3140 rows: over the layer-per-launch kernels' 3072) runs on the chains and is gathered, the small
    buckets around it read the plan: the pass's step counter moves for every step, whoever ran it -- and for a batch of
    zero frames (has_arrays: the reference yields an empty batch there), which takes the iterator's step: no launch, a loss
    of exactly 0."""
    from abnet3_amd import _lib
    from abnet3_amd.loss import coscos2
    host, want = frozen_reference('c', KW, SIZES_C, has_arrays=[True] * len(SIZES_C))
    plan = plan_np.upload(host)
    net = cuda_net(KW, params_of(KW))
    tr = make_trainer(net, plan, 'sgd', 0.0, coscos2(avg=False), momentum=0.0)
    before = net.flat_parameters().clone()
    for rep in range(2):
        losses, paths = run_pass(tr, plan)
        check_losses(losses, want, 'mixed buckets, pass %d' % rep)
        if rep == 0:
            assert paths[1] != _lib.PATH_WIDE and paths[0] == paths[2] == _lib.PATH_WIDE
        assert int(tr._src['ctr']) == len(SIZES_C)
        assert not getattr(tr, '_plan_refused', False)
        big = [b for b in tr._buckets.values() if b['npad'] == 1600]
        assert len(big) == 1 and big[0]['source'] is None and big[0]['graph'] is not None
        assert all(b['source'] is not None for b in tr._buckets.values() if b['npad'] != 1600)
    assert torch.equal(net.flat_parameters(), before)
    # the empty batch's step: what the iterator makes of it
    it = run_iterator(make_trainer(cuda_net(KW, params_of(KW)), plan, 'sgd', 0.0, coscos2(avg=False), momentum=0.0))
    assert want[3] == 0 and losses[3] == it[3] == 0
    check_losses(it, want, 'mixed buckets, iterator')


@pytest.mark.parametrize('oname,loss', [('sgd', ('coscos2', False, 0.5)), ('adadelta', ('coscos2', False, 0.5))])
def test_an_empty_batch_still_steps_the_optimizer(oname, loss):
    """The reference's loop on a batch of no frame pairs: a loss of 0 (as a mean: 0 / 0), all-zero gradients and an
    optimizer step on them -- SGD's momentum carries the parameters on, Adadelta's averages decay.  Planned pass and
    iterator against the oracle's pass, which steps on explicit zeros."""
    import abnet3_amd.loss as L
    sizes = [33, 0, 31, 64, 0, 33]
    def make():
        from oracle import siamese_np as O
        host = plan_np.host_plan(np.random.default_rng(9), 40, sizes, has_arrays=[True] * len(sizes))
        return (host,) + plan_np.oracle_pass(copy_of(params_of(KW)), host, _spec(KW), O.Optimizer(oname, LR[oname]), loss[0], loss[2], loss[1])
    host, want, after = _cached(('empty', oname, loss), make)
    keys = _spec(KW).param_keys()
    plan = plan_np.upload(host)
    for planned in (False, True):
        net = cuda_net(KW, params_of(KW))
        tr = make_trainer(net, plan, oname, LR[oname], getattr(L, loss[0])(avg=loss[1]))
        losses = run_pass(tr, plan)[0] if planned else run_iterator(tr)
        check_losses(losses, want, 'an empty batch, %s, planned %s' % (oname, planned))
        assert tr.optimizer.step_count == len(sizes)
        if planned:
            assert int(tr._src['ctr']) == len(sizes)
        check_params(state_np(net), after, keys, False, PARAM_TOL[oname])
    # (a MEAN over no pairs is 0 / 0, as in the reference; a pass's running sum is not a number from there on)
    tr = make_trainer(cuda_net(KW, params_of(KW)), plan, oname, LR[oname], L.coscos2(avg=True))
    assert np.isnan(float(tr.train_step(plan.materialise(host['order'][1]), True)))
    assert all(np.isfinite(v).all() for v in state_np(tr.network).values())


def test_a_table_width_that_is_no_multiple_of_four():
    """D = 39: the operand-plane kernels take widths that are multiples of 4 only, so the padded step is refused on the
    first batch and the whole pass takes the iterator's step on the plan's batches -- the right ones, in order (the
    element-wise gather such a table needs: test_gather_pairs_is_the_host_gather)."""
    from abnet3_amd.loss import coscos2
    kw = dict(KW, input_dim=39)
    sizes = [33, 1, 64, 31, 33, 64, 32]
    host, want = frozen_reference('c39', kw, sizes)
    plan = plan_np.upload(host)
    net = cuda_net(kw, params_of(kw))
    tr = make_trainer(net, plan, 'sgd', 0.0, coscos2(avg=False), momentum=0.0)
    before = net.flat_parameters().clone()
    for rep in range(2):
        losses, _ = run_pass(tr, plan)
        check_losses(losses, want, 'D = 39, pass %d' % rep)
        assert all(b.get('source') is None for b in tr._buckets.values())
        assert tr._plan_refused and not graphs_of(tr)
    assert torch.equal(net.flat_parameters(), before)


@pytest.mark.parametrize('dtype', ['float64', 'int8'])
@pytest.mark.parametrize('D', [39, 40])
def test_gather_pairs_is_the_host_gather(D, dtype):
    """abn_gather_pairs, element-wise (D = 39) and in 16-byte pieces (D = 40), against plain numpy indexing: both towers'
    rows, zero rows up to the padded size, an index outside the table on either side reads a zero row, the labels and the
    real-pair count."""
    from abnet3_amd import _lib
    lib = _lib.load()
    host = plan_np.host_plan(np.random.default_rng(D), D, [5, 33, 64, 1], NP_DTYPE[dtype], table_rows=20, scatter=False)
    host['idx1'][7], host['idx2'][9], host['idx2'][37] = -1, 20, 1 << 40
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table, idx1, idx2, lab = dev(host['table']), dev(host['idx1']), dev(host['idx2']), dev(host['labels'])
    for b in range(4):
        first, n = int(host['offsets'][b]), int(host['offsets'][b + 1] - host['offsets'][b])
        for npad in ((n + 31) // 32 * 32, (n + 31) // 32 * 32 + 32):
            x12 = torch.full((2 * npad, D), float('nan'), device='cuda')
            y = torch.full((npad,), 1, dtype=lab.dtype, device='cuda')
            nv = torch.full((1,), -7, dtype=torch.int32, device='cuda')
            _lib.check(lib.abn_gather_pairs(_ptr(table), 20, D, _ptr(idx1), _ptr(idx2), first, n, npad, _ptr(lab), lab.element_size(),
                                            _ptr(x12), _ptr(y), _ptr(nv), _lib.stream()), 'abn_gather_pairs')
            x1, x2, labels = plan_np.gather_batch(host, b)
            want = np.zeros((2 * npad, D), dtype=np.float32)
            want[:n], want[npad:npad + n] = x1, x2
            assert np.array_equal(x12.cpu().numpy(), want)
            assert np.array_equal(y.cpu().numpy()[:n], labels) and not y.cpu().numpy()[n:].any() and int(nv) == n


def test_the_step_table_grows_past_its_first_size():
    """Eight steps, then 1100 steps over the same device arrays: the step table outgrows the 1024 rows it was given, and
    the steps captured against the old table's address are dropped with it."""
    from abnet3_amd.dataloader import BatchPlan
    from abnet3_amd.loss import coscos2
    n_steps = 1100
    host, want = frozen_reference('grow', KW, [32] * n_steps, table_rows=512)
    short = plan_np.upload(host, order=host['order'][:8])
    full = BatchPlan(short.table, short.idx1, short.idx2, short.labels, host['offsets'], host['order'])
    net = cuda_net(KW, params_of(KW))
    tr = make_trainer(net, short, 'sgd', 0.0, coscos2(avg=False), momentum=0.0)
    losses, _ = run_pass(tr, short)
    check_losses(losses, want[:8], 'the short pass')
    table, (graph,) = tr._src['steps'], graphs_of(tr).values()
    assert table.shape[0] == 1024 and int(tr._src['ctr']) == 8
    losses, _ = run_pass(tr, full)
    check_losses(losses, want, 'the long pass')
    assert tr._src['steps'].shape[0] >= n_steps and tr._src['steps'].data_ptr() != table.data_ptr()
    assert int(tr._src['ctr']) == n_steps
    (regraph,) = graphs_of(tr).values()
    assert regraph is not graph and all(b['source'] is tr._src for b in tr._buckets.values())


# ---- (d) the dev pass ------------------------------------------------------------------------------------------------------------
def test_the_dev_pass_sums_the_oracles_losses():
    from abnet3_amd.loss import coscos2
    host, want = frozen_reference('a', KW, SIZES_A)          # (no dropout, no BatchNorm: the eval-mode loss is the training-mode one)
    plan = plan_np.upload(host)
    net = cuda_net(KW, params_of(KW))
    tr = make_trainer(net, plan, 'sgd', 0.0, coscos2(avg=False), momentum=0.0)
    net.eval()
    for rep in ('first use', 'replay'):
        total = torch.zeros((), dtype=torch.float64, device='cuda')
        with torch.no_grad():
            assert tr._run_planned_eval(plan, total) == len(SIZES_A)
        err = abs(float(total) - want.sum()) / want.sum()
        print('dev pass, %s: relative error of the summed loss %.3g' % (rep, err))
        assert err <= LOSS_TOL
        assert sum(1 for b in tr._buckets.values() if b.get('eval') is not None) == 4


# ---- (e) BatchNorm ---------------------------------------------------------------------------------------------------------------
def test_a_batch_norm_pass_counts_its_real_rows():
    """A padded batch through BatchNorm (abn_tower_desc.n_valid: batch and running statistics over the real rows) against
    the oracle on the unpadded batches: losses, parameters, running statistics, num_batches_tracked."""
    from abnet3_amd.loss import coscos2
    from oracle import siamese_np as O
    kw = dict(KW, batch_norm=True)
    sizes = [129, 160, 97, 200, 130, 222, 100, 128]      # (the BatchNorm layer launches take calls of 256 rows and more: 128-pair buckets and up)
    spec = _spec(kw)
    host = plan_np.host_plan(np.random.default_rng(5), 40, sizes)
    want, after = plan_np.oracle_pass(copy_of(params_of(kw)), host, spec, O.Optimizer('adadelta', 0.1), 'coscos2', 0.5, False)
    plan = plan_np.upload(host)
    net = cuda_net(kw, params_of(kw))
    tr = make_trainer(net, plan, 'adadelta', 0.1, coscos2(avg=False))
    losses, _ = run_pass(tr, plan)
    check_losses(losses, want, 'BatchNorm')
    assert not getattr(tr, '_plan_refused', False) and len(graphs_of(tr)) == 3
    mine = state_np(net)
    check_params(mine, after, spec.param_keys(), True, 2e-5)
    for k in after:
        if k.endswith('num_batches_tracked'):
            assert int(mine[k]) == int(after[k]) == 2 * len(sizes), k
        elif 'running' in k:
            assert rel_err(mine[k], after[k]) < 2e-5, (k, rel_err(mine[k], after[k]))


# ---- (f) the sourced kernels alone -----------------------------------------------------------------------------------------------
SPANS = [(0, 1), (1, 31), (32, 32), (64, 33), (97, 64)]
ENDINGS = {'wgrad_step': (True, None), 'slab_step': (True, 'ABN_WGRAD_STEP'), 'undeferred': (False, None)}


def _ptr(t):
    from abnet3_amd import _lib
    return _lib.ptr(t)


@pytest.mark.parametrize('avg', [False, True])
@pytest.mark.parametrize('ending', list(ENDINGS))
@pytest.mark.parametrize('k', range(len(SPANS)))
def test_a_sourced_step_is_the_gathered_step(k, ending, avg, monkeypatch):
    """direct_forward(source=...) / direct_backward_loss / FlatOptimizer.step() on a hand-built abn_step_source with the
    counter at entry k: embeddings, loss and gradients of the host-gathered batch (oracle), bit for bit those of the same
    step fed through abn_gather_pairs.  The padded x1 / x2 hold NaN (unused, says the header), every label outside the
    step's span is -1 (a padded pair's two rows are equal: cos = 1, and only a 'different' label makes that count), one
    idx1 entry is negative and one idx2 entry equals table_rows (both read as zero rows).  The counter: untouched by the
    forward and the backward, + 1 by abn_tower_reduce_step's launch -- either of its kernels -- and untouched by a step
    whose reduction was not deferred (abn_optimizer_step: the caller moves it, TrainerSiamese._run_planned).
    (No entry point hands out a padded row's own gradient: what such rows would add shows in the bias gradients, which
    are held to the oracle's on the unpadded batch and, bit for bit, to the gathered step's.)"""
    from abnet3_amd import _lib
    from abnet3_amd.trainer import FlatOptimizer
    from oracle import siamese_np as O
    defer, switch = ENDINGS[ending]
    if switch:
        monkeypatch.setenv(switch, '0')
    lib = _lib.load()
    first, n = SPANS[k]
    npad = (n + 31) // 32 * 32
    rng = np.random.default_rng(10 + k)
    total, rows, D = 161, 50, 40
    host = plan_np.host_plan(rng, D, [total], table_rows=rows, scatter=False)
    labels = -np.ones(total)
    labels[first:first + n] = host['labels'][first:first + n]
    host['labels'] = labels
    host['idx1'][first] = -1
    if n > 1:             # (a lone pair of two zero rows has cos = 1 and, labelled 'same', a loss of exactly 0: nothing to be relative to)
        host['idx2'][first + n - 1] = rows
    host['offsets'] = np.array([0, first, first + n, total], dtype=np.int64)       # (batch 1 = the step's span)
    x1, x2, y = plan_np.gather_batch(host, 1)
    spec, p = _spec(KW), copy_of(params_of(KW))
    want_loss, og, (o1, o2) = O.train_step(p, x1, x2, y, spec, O.Optimizer('sgd', 0.01), 'coscos2', 0.5, avg)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table, idx1, idx2, lab = dev(host['table']), dev(host['idx1']), dev(host['idx2']), dev(host['labels'])
    steps = dev(np.array(SPANS, dtype=np.int64))
    ctr = torch.full((1,), k, dtype=torch.int32, device='cuda')
    src = _lib.StepSource()
    src.table, src.table_rows, src.idx1, src.idx2, src.labels = table.data_ptr(), rows, idx1.data_ptr(), idx2.data_ptr(), lab.data_ptr()
    src.steps, src.step_ctr = steps.data_ptr(), ctr.data_ptr()
    res = []
    for sourced in (True, False):
        net = cuda_net(KW, params_of(KW))
        opt = FlatOptimizer(net, 'sgd', 0.01, 0.9)
        if sourced:
            x12 = torch.full((2 * npad, D), float('nan'), device='cuda')
            emb, state = net.direct_forward(x12[:npad], x12[npad:], source=src)
            assert _lib.last_forward_path() == _lib.PATH_WIDE
            emb = emb.clone()
            loss = net.direct_backward_loss(state, lab, 'coscos2', 0.5, avg, defer_reduce=defer)
            assert loss is not None and int(ctr) == k
            opt.step()
            assert int(ctr) == (k + 1 if defer else k)
        else:
            x12 = torch.zeros(2 * npad, D, device='cuda')
            yb, nv = torch.zeros(npad, dtype=lab.dtype, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
            _lib.check(lib.abn_gather_pairs(_ptr(table), rows, D, _ptr(idx1), _ptr(idx2), first, n, npad, _ptr(lab), lab.element_size(),
                                            _ptr(x12), _ptr(yb), _ptr(nv), _lib.stream()), 'abn_gather_pairs')
            emb, state = net.direct_forward(x12[:npad], x12[npad:])
            emb = emb.clone()
            loss = net.direct_backward_loss(state, yb, 'coscos2', 0.5, avg, defer_reduce=defer, n_valid=nv)
            opt.step()
        res.append((emb, loss.clone(), {q: v.grad.clone() for q, v in net.named_parameters()},
                    {q: v.detach().clone() for q, v in net.named_parameters()}))
    (emb, loss, grads, params), (emb_g, loss_g, grads_g, params_g) = res
    assert torch.equal(emb[:n], emb_g[:n]) and torch.equal(emb[npad:npad + n], emb_g[npad:npad + n]) and torch.equal(loss, loss_g)
    for q in grads:
        assert torch.equal(grads[q], grads_g[q]) and torch.equal(params[q], params_g[q]), q
    e = emb.cpu().numpy()
    assert rel_err(e[:n], o1) < 1e-5 and rel_err(e[npad:npad + n], o2) < 1e-5
    assert np.isfinite(e).all()
    assert abs(float(loss) - want_loss) <= LOSS_TOL * abs(want_loss), (float(loss), want_loss)
    check_grads({q: v.cpu().numpy() for q, v in grads.items()}, og, spec.param_keys(), False, tol=1e-4)
    check_params({q: v.cpu().numpy() for q, v in params.items()}, p, spec.param_keys(), False, 1e-5)


# ---- (g) the lent forward workspace ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['direct_backward_loss', 'direct_backward'])
def test_the_lent_workspace_outlives_the_forwards_state(entry):
    """A deferred backward on the layer-per-launch kernels leaves the weight gradients to the optimizer's launch, which
    reads the forward's activation images from the forward's workspace (abn_tower_desc.fwd_ws: a bare address).  Whoever
    drops the forward's state before step() -- the trainer's bucket body does -- must not free that memory: the pending
    reduction owns it, a NaN-filled allocation of its size in between changes nothing, and the step releases it."""
    from abnet3_amd import _lib
    from abnet3_amd.trainer import FlatOptimizer
    from oracle import siamese_np as O
    n, D = 96, 280
    spec, p = _spec(KW_C5), copy_of(params_of(KW_C5))
    rng = np.random.default_rng(21)
    x1, x2 = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((n, D)).astype(np.float32)
    y = rng.choice([1.0, -1.0], n)
    d_out = rng.standard_normal((2 * n, 100)).astype(np.float32)
    if entry == 'direct_backward_loss':
        O.train_step(p, x1, x2, y, spec, O.Optimizer('sgd', 0.01), 'coscos2', 0.5, False)
    else:
        og = {}
        for x, d in ((x1, d_out[:n]), (x2, d_out[n:])):
            _, cache = O.tower_forward(p, x, spec, True)
            O.tower_backward(p, cache, d, spec, og)
        O.Optimizer('sgd', 0.01).step(p, og, spec.param_keys())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    net = cuda_net(KW_C5, params_of(KW_C5))
    opt = FlatOptimizer(net, 'sgd', 0.01, 0.9)
    emb, state = net.direct_forward(dev(x1), dev(x2))
    assert _lib.last_forward_path() == _lib.PATH_WIDE and net.can_defer_reduce(state)
    if entry == 'direct_backward_loss':
        assert net.direct_backward_loss(state, dev(y), 'coscos2', 0.5, False, defer_reduce=True) is not None
    else:
        net.direct_backward(state, dev(d_out), defer_reduce=True)
    assert net._pending_reduce[0].fwd_ws == state[1].ws.data_ptr()          # the workspace IS lent on this shape
    ws = weakref.ref(state[1].ws)
    nbytes = state[1].ws.numel() * 4
    del emb, state
    gc.collect()
    assert ws() is not None, 'the forward workspace was freed while the reduction that reads it is pending'
    poison = torch.full((nbytes // 4,), float('nan'), device='cuda')
    opt.step()
    torch.cuda.synchronize()
    del poison
    mine = {k: v.detach().cpu().numpy() for k, v in net.named_parameters()}
    assert all(np.isfinite(v).all() for v in mine.values())
    check_params(mine, p, spec.param_keys(), False, 1e-5)
    gc.collect()
    assert ws() is None, 'the step did not release the forward workspace'
