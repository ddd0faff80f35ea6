"""What the tower entry points refuse, and that they refuse it before any launch (csrc/tower.hip: abn_tower_forward,
abn_tower_backward, abn_tower_backward_loss, abn_tower_backward_launch, abn_tower_reduce_step).

Every case builds the smallest descriptor that triggers one refusal -- a 40 -> 64 -> 16 sigmoid tower, 64 rows unless a
path needs more -- and asserts the exact return code, the exact abn_last_error() text, and that the workspace, the
backward scratch and the flat gradient buffer, filled with a sentinel beforehand, are bit-unchanged afterwards: nothing
was launched.  One doubly-bad call per entry point pins which message wins.  The one refusal that sits behind launches
(cross-replica statistics with n_valid, inside the BatchNorm layer loop) is held to code and text only.

The texts are the library's as of ABI 20; no kernel runs in any sentinel case.  Needs an MI355X: -m gpu."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
SENTINEL = 12345.0
DIMS = (40, 64, 16)
ROWS = 64
F32, F16X2 = 0, 3
SGD, ADAM = 0, 2
COSCOS2, KL = 0, 2
Y_F32 = 3


def lib_():
    from abnet3_amd import _lib
    return _lib, _lib.load()


@pytest.fixture
def switches(monkeypatch):
    """set(NAME=value, ...): environment switches for this test, read by the library at once; read again without them after."""
    _lib, _ = lib_()
    names = []

    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setenv(k, str(v))
            names.append(k)
        _lib.reload_switches()
    yield set_
    for k in names:
        monkeypatch.delenv(k, raising=False)
    _lib.reload_switches()


def sentinel(n):
    return torch.full((int(n),), SENTINEL, dtype=torch.float32, device='cuda')


class Tower:
    """A descriptor over zero-initialised parameters, every gradient tensor a slice of ONE flat sentinel buffer, plus a
    sentinel workspace and backward scratch of the sizes the library asks for."""

    def __init__(self, precision=F32, batch_norm=False, rows=ROWS, n_calls=1):
        _lib, lib = lib_()
        self._lib, self.lib = _lib, lib
        self.rows, self.n_calls = rows, n_calls
        self.keep = []
        d = _lib.TowerDesc()
        d.n_layers, d.act, d.last_act, d.batch_norm, d.precision = len(DIMS) - 1, 1, 1, int(batch_norm), precision
        for i, w in enumerate(DIMS):
            d.dims[i] = w
        sizes = []
        for l in range(d.n_layers):
            sizes += [DIMS[l + 1] * DIMS[l], DIMS[l + 1]] + ([DIMS[l + 1]] * 2 if batch_norm else [])
        self.n_flat = sum(sizes)
        self.grads = sentinel(self.n_flat)
        self.params = torch.zeros(self.n_flat, device='cuda')
        o = 0
        for l in range(d.n_layers):
            names = [('W', 'dW'), ('b', 'db')] + ([('bn_w', 'dbn_w'), ('bn_b', 'dbn_b')] if batch_norm else [])
            for (p, g), n in zip(names, sizes[(4 if batch_norm else 2) * l:]):
                assert o % 4 == 0                      # (every tensor 16-byte aligned: the operand-plane kernels take the tower)
                getattr(d, p)[l] = self.params[o:].data_ptr()
                getattr(d, g)[l] = self.grads[o:].data_ptr()
                o += n
            if batch_norm:
                for name in ('bn_rm', 'bn_rv'):
                    s = torch.ones(DIMS[l + 1], device='cuda')
                    self.keep.append(s)
                    getattr(d, name)[l] = s.data_ptr()
        self.d = d
        self.x = torch.zeros(rows * DIMS[0] + 4, device='cuda')
        self.d_out = torch.zeros(rows * DIMS[-1] + 4, device='cuda')
        n_ws = lib.abn_tower_ws_floats(C.byref(d), rows, n_calls)
        self.n_scratch = lib.abn_tower_bwd_scratch_floats(C.byref(d), rows)
        assert n_ws > 0 and self.n_scratch > 0
        self.ws, self.scratch = sentinel(n_ws), sentinel(self.n_scratch)

    def x2(self):
        return self.x[(self.rows // 2) * DIMS[0]:] if self.n_calls == 2 else None

    def refused(self, rc, code, text, untouched=True):
        msg = self.lib.abn_last_error().decode()
        assert (rc, msg) == (code, text)
        if untouched:
            torch.cuda.synchronize()
            for name in ('ws', 'scratch', 'grads'):
                assert bool((getattr(self, name) == SENTINEL).all()), name

    # the entry points, every argument valid unless a case overrides it
    def forward(self, train=1, x2='auto', n_calls=None, rows=None):
        p = self._lib.ptr
        return self.lib.abn_tower_forward(C.byref(self.d), p(self.x), p(self.x2() if isinstance(x2, str) else x2),
                                          self.rows if rows is None else rows, n_calls or self.n_calls, train, p(self.ws), None)

    def backward(self, d_out='auto', scratch_floats=None):
        p = self._lib.ptr
        return self.lib.abn_tower_backward(C.byref(self.d), p(self.x), p(self.x2()), p(self.d_out if isinstance(d_out, str) else d_out),
                                           self.rows, self.n_calls, p(self.ws), p(self.scratch),
                                           self.n_scratch if scratch_floats is None else scratch_floats, None, None)

    def backward_launch(self, part=1, scratch_floats=None):
        p = self._lib.ptr
        return self.lib.abn_tower_backward_launch(C.byref(self.d), p(self.x), p(self.x2()), p(self.d_out), self.rows, self.n_calls,
                                                  p(self.ws), p(self.scratch),
                                                  self.n_scratch if scratch_floats is None else scratch_floats, part, None)

    def backward_loss(self, kind=COSCOS2, y_dtype=Y_F32, margin=0.5, scratch_floats=None, y='auto'):
        p = self._lib.ptr
        self.y = torch.ones(self.rows // 2, device='cuda')
        self.loss_out = torch.zeros(1, device='cuda')
        self.loss_ws = torch.zeros(self.lib.abn_tower_backward_loss_ws_bytes(self.rows) // 4 + 4, device='cuda')
        return self.lib.abn_tower_backward_loss(C.byref(self.d), p(self.x), p(self.x2()), p(self.y if isinstance(y, str) else y), y_dtype,
                                                kind, margin, 0, self.rows, p(self.ws), p(self.scratch),
                                                self.n_scratch if scratch_floats is None else scratch_floats, p(self.loss_out),
                                                p(self.loss_ws), None, None, None)

    def reduce_step(self, kind=SGD, state2=True, n=None, step=1, scratch_floats=None, params='auto'):
        p = self._lib.ptr
        self.s1, self.s2 = torch.zeros(self.n_flat, device='cuda'), torch.zeros(self.n_flat, device='cuda')
        return self.lib.abn_tower_reduce_step(C.byref(self.d), self.rows, p(self.scratch),
                                              self.n_scratch if scratch_floats is None else scratch_floats, kind,
                                              p(self.params if isinstance(params, str) else params), p(self.grads), p(self.s1),
                                              p(self.s2 if state2 else None), self.n_flat if n is None else n, 0.1, 0.9, 0.999,
                                              1e-8, step, 1.0, None)


def noop_allreduce():
    """An abn_allreduce_fn that must never be called (the refusals come first)."""
    _lib, _ = lib_()

    def fn(ctx, buf, n, stream):
        raise AssertionError('bn_sync_fn called')
    return _lib.ALLREDUCE_FN(fn)


def step_source(t, labels=False, table=True):
    """An abn_step_source over small real arrays (never read: every case is refused first)."""
    s = t._lib.StepSource()
    arrays = {k: torch.zeros(256, dtype=torch.int32, device='cuda') for k in ('idx1', 'idx2', 'steps', 'step_ctr', 'labels')}
    arrays['table'] = torch.zeros(4 * DIMS[0], device='cuda')
    t.keep += list(arrays.values())
    s.table = arrays['table'].data_ptr() if table else None
    s.table_rows = 4
    for k in ('idx1', 'idx2', 'steps', 'step_ctr'):
        setattr(s, k, arrays[k].data_ptr())
    s.labels = arrays['labels'].data_ptr() if labels else None
    t.keep.append(s)
    t.d.source = C.addressof(s)
    return s


def path_of(t, train=1, backward=0):
    p = t._lib.ptr
    return t.lib.abn_tower_path(C.byref(t.d), p(t.x), p(t.x2()), t.rows, t.n_calls, train, p(t.ws), backward, None)


# ---------------------------------------------------------------------------------------------------------------------
# abn_tower_forward
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_refuses_x2_without_two_calls():
    t = Tower()
    t.refused(t.forward(x2=t.x), E_ARG, 'tower_forward: x2 given but n_calls=1')


def test_forward_refuses_more_than_eight_calls():
    t = Tower(rows=72, n_calls=9)
    t.refused(t.forward(x2=None), E_ARG, 'tower_forward: at most 8 calls per launch')


def test_forward_refuses_null_workspace():
    t = Tower()
    p = t._lib.ptr
    rc = t.lib.abn_tower_forward(C.byref(t.d), p(t.x), None, t.rows, 1, 1, None, None)
    t.refused(rc, E_ARG, 'tower_forward: null input/workspace')


def test_forward_refuses_cross_replica_statistics_off_the_plane_launches():
    t = Tower(batch_norm=True)                  # fp32: the per-layer kernels
    fn = noop_allreduce()
    t.d.bn_sync_fn, t.d.bn_sync_world = C.cast(fn, C.c_void_p), 2
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: cross-replica BatchNorm statistics (bn_sync_world) need the operand-plane launches')


def test_forward_refuses_cross_replica_statistics_with_the_plane_launches_switched_off(switches):
    t = Tower(precision=F16X2, batch_norm=True, rows=256)
    assert path_of(t) in (t._lib.PATH_BN_LAYERS, t._lib.PATH_BN_TOWER)
    switches(ABN_BN_PLANES=0)
    assert path_of(t) == t._lib.PATH_PER_LAYER
    fn = noop_allreduce()
    t.d.bn_sync_fn, t.d.bn_sync_world = C.cast(fn, C.c_void_p), 2
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: cross-replica BatchNorm statistics (bn_sync_world) need the operand-plane launches')


def test_forward_refuses_n_valid_off_the_batch_norm_layer_launches():
    t = Tower(batch_norm=True)
    nv = torch.full((1,), 60, dtype=torch.int32, device='cuda')
    t.d.n_valid = nv.data_ptr()
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: a padded batch (n_valid) through a BatchNorm tower in training needs the BatchNorm layer launches')


def test_forward_refuses_a_step_source_outside_wide_training():
    t = Tower(precision=F16X2, n_calls=2)
    assert path_of(t) == t._lib.PATH_WIDE
    step_source(t)
    t.refused(t.forward(train=0), E_UNSUPPORTED,
              'tower_forward: a step source (abn_tower_desc.source) needs the layer-per-launch kernels in training, two calls')


def test_forward_refuses_a_step_source_with_a_null_array():
    t = Tower(precision=F16X2, n_calls=2)
    assert path_of(t) == t._lib.PATH_WIDE
    step_source(t, table=False)
    t.refused(t.forward(), E_ARG, 'tower_forward: abn_step_source: null or misaligned array')


def test_forward_refuses_in_kernel_dropout_without_masks_off_the_planes():
    t = Tower()
    seed = torch.zeros(2, dtype=torch.int64, device='cuda')
    t.d.drop_seed, t.d.drop_p = seed.data_ptr(), 0.1
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: in-kernel dropout (drop_seed) needs the operand-plane kernels: pass drop_mask tensors')


@pytest.mark.parametrize('rows, env, path', [(64, {}, 6), (256, {'ABN_WIDE': 0}, 2)])
def test_forward_refuses_a_misaligned_wpack(rows, env, path, switches):
    switches(**env)
    t = Tower(precision=F16X2, rows=rows)
    assert path_of(t) == path
    n = t.lib.abn_tower_wpack_floats(C.byref(t.d))
    wpack = sentinel(n + 4)
    t.d.wpack = wpack.data_ptr() + 4
    t.refused(t.forward(), E_ARG, 'tower_forward: wpack must be 16-byte aligned')
    assert bool((wpack == SENTINEL).all())


def test_forward_doubly_bad_sync_wins_over_n_valid_and_source():
    t = Tower(batch_norm=True)
    fn = noop_allreduce()
    t.d.bn_sync_fn, t.d.bn_sync_world = C.cast(fn, C.c_void_p), 2
    nv = torch.full((1,), 60, dtype=torch.int32, device='cuda')
    t.d.n_valid = nv.data_ptr()
    step_source(t)
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: cross-replica BatchNorm statistics (bn_sync_world) need the operand-plane launches')
    t.d.bn_sync_fn = None                       # ... then n_valid over the source
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: a padded batch (n_valid) through a BatchNorm tower in training needs the BatchNorm layer launches')


def test_forward_doubly_bad_source_wins_over_dropout_and_x2_over_all():
    t = Tower()
    seed = torch.zeros(2, dtype=torch.int64, device='cuda')
    t.d.drop_seed, t.d.drop_p = seed.data_ptr(), 0.1
    step_source(t)
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: a step source (abn_tower_desc.source) needs the layer-per-launch kernels in training, two calls')
    t.refused(t.forward(x2=t.x), E_ARG, 'tower_forward: x2 given but n_calls=1')


def test_forward_sync_with_n_valid_is_refused_inside_the_layer_loop(switches):
    """Behind the weight pack and the first layer's launch (the workspace is NOT untouched): code and text only."""
    switches(ABN_BN_PERSIST=0)
    t = Tower(precision=F16X2, batch_norm=True, rows=256)
    assert path_of(t) == t._lib.PATH_BN_LAYERS
    t.ws.zero_()
    fn = noop_allreduce()
    t.d.bn_sync_fn, t.d.bn_sync_world = C.cast(fn, C.c_void_p), 1
    nv = torch.full((1,), 250, dtype=torch.int32, device='cuda')
    t.d.n_valid = nv.data_ptr()
    t.refused(t.forward(), E_UNSUPPORTED,
              'tower_forward: n_valid (a padded batch) cannot be combined with cross-replica BatchNorm statistics', untouched=False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# abn_tower_backward
# ---------------------------------------------------------------------------------------------------------------------
def test_backward_refuses_null_pointer_and_null_gradients():
    t = Tower()
    t.refused(t.backward(d_out=None), E_ARG, 'tower_backward: null pointer')
    t.d.db[1] = None
    t.refused(t.backward(), E_ARG, 'tower_backward: layer 1 has null gradient buffers')


def test_backward_refuses_a_small_scratch():
    t = Tower()
    t.refused(t.backward(scratch_floats=t.n_scratch - 1), E_WORKSPACE,
              'tower_backward: scratch too small (%d < %d floats)' % (t.n_scratch - 1, t.n_scratch))


def test_backward_refuses_a_step_source():
    t = Tower(precision=F16X2, n_calls=2)
    step_source(t, labels=True)
    t.refused(t.backward(), E_ARG,
              'tower_backward: a step source (abn_tower_desc.source) goes with abn_tower_backward_loss (the labels are the plan\'s)')


def test_backward_refuses_wgrad_part_off_the_planes():
    t = Tower()
    t.d.wgrad_part, t.d.wgrad_split = 1, 1
    t.refused(t.backward(), E_UNSUPPORTED, 'tower_backward: wgrad_part needs the operand-plane launches of a tower without BatchNorm')


def test_backward_refuses_cross_replica_statistics_and_n_valid_off_the_plane_launches():
    t = Tower(batch_norm=True)
    nv = torch.full((1,), 60, dtype=torch.int32, device='cuda')
    t.d.n_valid = nv.data_ptr()
    t.refused(t.backward(), E_UNSUPPORTED,
              'tower_backward: a padded batch (n_valid) through a BatchNorm tower needs the BatchNorm layer launches')
    fn = noop_allreduce()                       # both: the statistics' message wins
    t.d.bn_sync_fn, t.d.bn_sync_world = C.cast(fn, C.c_void_p), 2
    t.refused(t.backward(), E_UNSUPPORTED,
              'tower_backward: cross-replica BatchNorm statistics (bn_sync_world) need the operand-plane launches')


def test_backward_refuses_d_out_is_dz_with_batch_norm():
    t = Tower(batch_norm=True)
    t.d.d_out_is_dz = 1
    t.refused(t.backward(), E_ARG, 'tower_backward: d_out_is_dz cannot be combined with batch_norm')


@pytest.mark.parametrize('rows, env, path', [(64, {}, 6), (256, {'ABN_WIDE': 0}, 2)])
def test_backward_refuses_misaligned_d_out_and_bad_wgrad_part_on_the_planes(rows, env, path, switches):
    switches(**env)
    t = Tower(precision=F16X2, rows=rows)
    assert path_of(t, backward=1) == path
    t.refused(t.backward(d_out=t.d_out[1:]), E_ARG, 'tower_backward: d_out / scratch / dx must be 16-byte aligned')
    t.d.wgrad_part = 3
    t.refused(t.backward(), E_ARG, 'tower_backward: wgrad_part=3')
    t.d.wgrad_part, t.d.wgrad_split = 1, 5
    t.refused(t.backward(), E_ARG, 'tower_backward: wgrad_split=5')
    t.d.wgrad_split, t.d.defer_reduce = 1, 1
    t.refused(t.backward(), E_ARG, 'tower_backward: wgrad_part cannot be combined with defer_reduce')
    t.refused(t.backward(d_out=t.d_out[1:]), E_ARG, 'tower_backward: d_out / scratch / dx must be 16-byte aligned')


def test_backward_doubly_bad_scratch_wins_over_source_and_wgrad_part():
    t = Tower()
    step_source(t, labels=True)
    t.d.wgrad_part, t.d.wgrad_split = 1, 1
    t.refused(t.backward(scratch_floats=8), E_WORKSPACE, 'tower_backward: scratch too small (8 < %d floats)' % t.n_scratch)
    t.refused(t.backward(), E_ARG,
              'tower_backward: a step source (abn_tower_desc.source) goes with abn_tower_backward_loss (the labels are the plan\'s)')


# ---------------------------------------------------------------------------------------------------------------------
# abn_tower_backward_loss
# ---------------------------------------------------------------------------------------------------------------------
def test_backward_loss_refuses_kl_and_unknown_kinds():
    t = Tower(precision=F16X2, n_calls=2)
    t.refused(t.backward_loss(kind=KL), E_UNSUPPORTED,
              'tower_backward_loss: ABN_LOSS_KL is not computed inside the backward: use abn_pair_loss_dz + abn_tower_backward')
    t.refused(t.backward_loss(kind=7), E_ARG, 'tower_backward_loss: unknown loss kind 7')
    t.refused(t.backward_loss(y_dtype=9), E_ARG, 'tower_backward_loss: unknown label dtype 9')
    t.refused(t.backward_loss(kind=1, margin=1.5), E_ARG, 'tower_backward_loss: margin outside [0,1]')
    t.refused(t.backward_loss(y=None), E_ARG, 'tower_backward_loss: null pointer')
    t.d.dW[0] = None
    t.refused(t.backward_loss(), E_ARG, 'tower_backward_loss: layer 0 has null gradient buffers')


UNSUPPORTED_LOSS = ('tower_backward_loss: only for towers the operand-plane kernels take (the split arithmetics, '
                    'widths <= 512 and multiples of 4, enough rows; BatchNorm without cross-replica statistics): use abn_pair_loss_dz + abn_tower_backward')


def test_backward_loss_refuses_towers_off_the_planes():
    t = Tower(n_calls=2)                        # fp32
    t.refused(t.backward_loss(), E_UNSUPPORTED, UNSUPPORTED_LOSS)


def test_backward_loss_refuses_batch_norm_with_cross_replica_statistics():
    t = Tower(precision=F16X2, batch_norm=True, rows=256, n_calls=2)
    fn = noop_allreduce()
    t.d.bn_sync_fn, t.d.bn_sync_world = C.cast(fn, C.c_void_p), 2
    t.refused(t.backward_loss(), E_UNSUPPORTED, UNSUPPORTED_LOSS)


def test_backward_loss_refuses_a_step_source_without_labels_or_off_the_wide_kernels(switches):
    t = Tower(precision=F16X2, n_calls=2)
    step_source(t, labels=False)
    text = 'tower_backward_loss: a step source (abn_tower_desc.source) needs the layer-per-launch kernels and its labels'
    t.refused(t.backward_loss(), E_UNSUPPORTED, text)
    switches(ABN_WIDE=0)
    t = Tower(precision=F16X2, rows=256, n_calls=2)
    assert path_of(t, backward=1) == t._lib.PATH_PLANES
    step_source(t, labels=True)
    t.refused(t.backward_loss(), E_UNSUPPORTED, text)


@pytest.mark.parametrize('rows, env, batch_norm', [(64, {}, False), (256, {'ABN_WIDE': 0}, False), (256, {}, True)])
def test_backward_loss_refuses_a_small_scratch(rows, env, batch_norm, switches):
    switches(**env)
    t = Tower(precision=F16X2, batch_norm=batch_norm, rows=rows, n_calls=2)
    t.refused(t.backward_loss(scratch_floats=t.n_scratch - 1), E_WORKSPACE, 'tower_backward_loss: scratch too small')


def test_backward_loss_refuses_two_different_n_valid():
    t = Tower(precision=F16X2, batch_norm=True, rows=256, n_calls=2)
    nv = torch.full((8,), 100, dtype=torch.int32, device='cuda')
    t.d.n_valid = nv.data_ptr()
    p = t._lib.ptr
    t.backward_loss(scratch_floats=0)           # (allocates y / loss_out / loss_ws)
    rc = t.lib.abn_tower_backward_loss(C.byref(t.d), p(t.x), p(t.x2()), p(t.y), Y_F32, COSCOS2, 0.5, 0, t.rows, p(t.ws), p(t.scratch),
                                       t.n_scratch, p(t.loss_out), p(t.loss_ws), p(nv[4:]), None, None)
    t.refused(rc, E_ARG, 'tower_backward_loss: two different n_valid')


def test_backward_loss_doubly_bad_kl_wins_over_null_then_path_over_scratch():
    t = Tower(n_calls=2)                        # fp32: no operand planes
    t.refused(t.backward_loss(kind=KL, y=None, scratch_floats=0), E_UNSUPPORTED,
              'tower_backward_loss: ABN_LOSS_KL is not computed inside the backward: use abn_pair_loss_dz + abn_tower_backward')
    t.refused(t.backward_loss(scratch_floats=0), E_UNSUPPORTED, UNSUPPORTED_LOSS)
    t = Tower(precision=F16X2, n_calls=2)       # ... the source's message over the scratch's
    step_source(t, labels=False)
    t.refused(t.backward_loss(scratch_floats=0), E_UNSUPPORTED,
              'tower_backward_loss: a step source (abn_tower_desc.source) needs the layer-per-launch kernels and its labels')


# ---------------------------------------------------------------------------------------------------------------------
# abn_tower_backward_launch
# ---------------------------------------------------------------------------------------------------------------------
def test_backward_launch_refusals(switches):
    t = Tower(precision=F16X2)
    assert path_of(t, backward=1) == t._lib.PATH_WIDE
    t.refused(t.backward_launch(part=1), E_UNSUPPORTED, 'tower_backward_launch: single-launch operand-plane towers only')
    t.refused(t.backward_launch(part=0), E_ARG, 'tower_backward_launch: bad argument')      # doubly bad: the argument first
    t.refused(Tower().backward_launch(part=2), E_UNSUPPORTED, 'tower_backward_launch: single-launch operand-plane towers only')
    switches(ABN_WIDE=0)
    t = Tower(precision=F16X2, rows=256)
    assert path_of(t, backward=1) == t._lib.PATH_PLANES
    t.refused(t.backward_launch(part=2, scratch_floats=t.n_scratch - 1), E_WORKSPACE, 'tower_backward_launch: scratch too small')
    t.refused(t.backward_launch(part=3, scratch_floats=0), E_ARG, 'tower_backward_launch: bad argument')
    t.d.wgrad_part = 3                          # (refused by the launcher itself, ahead of its launches)
    t.refused(t.backward_launch(part=1), E_ARG, 'tower_backward: wgrad_part=3')


# ---------------------------------------------------------------------------------------------------------------------
# abn_tower_reduce_step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision, batch_norm', [(F32, False), (F16X2, False), (F32, True)])
def test_reduce_step_refusals(precision, batch_norm):
    t = Tower(precision=precision, batch_norm=batch_norm)
    t.refused(t.reduce_step(kind=9), E_ARG, 'tower_reduce_step: unknown optimizer 9')
    t.refused(t.reduce_step(kind=-1, params=None), E_ARG, 'tower_reduce_step: unknown optimizer -1')      # doubly bad
    t.refused(t.reduce_step(params=None), E_ARG, 'tower_reduce_step: null pointer')
    t.refused(t.reduce_step(kind=ADAM, state2=False), E_ARG, 'tower_reduce_step: state2 required')
    t.refused(t.reduce_step(kind=1, state2=False), E_ARG, 'tower_reduce_step: state2 required')
    assert t.reduce_step(kind=SGD, state2=False, scratch_floats=0) == E_WORKSPACE            # (sgd needs none: on to the next check)
    t.refused(t.reduce_step(step=0), E_ARG, 'tower_reduce_step: bad n/step')
    t.refused(t.reduce_step(n=0), E_ARG, 'tower_reduce_step: bad n/step')
    t.refused(t.reduce_step(scratch_floats=t.n_scratch - 1), E_WORKSPACE, 'tower_reduce_step: scratch too small')
    t.refused(t.reduce_step(kind=ADAM, state2=False, scratch_floats=0), E_ARG, 'tower_reduce_step: state2 required')   # doubly bad
    # the flat buffer ends one float short of the last gradient tensor
    last = "tower_reduce_step: layer 1's %sgradients are not inside the flat buffer" % ('BatchNorm ' if batch_norm else '')
    t.refused(t.reduce_step(n=t.n_flat - 1), E_ARG, last)
    elsewhere = sentinel(DIMS[1] * DIMS[0])
    t.d.dW[0] = elsewhere.data_ptr()
    t.refused(t.reduce_step(), E_ARG, "tower_reduce_step: layer 0's gradients are not inside the flat buffer")
    assert bool((elsewhere == SENTINEL).all())


def test_reduce_step_refuses_gradients_outside_the_flat_buffer_on_the_one_launch_step():
    """defer_reduce + fwd_ws on a small fp16 x 2 batch: the weight gradients and the rule are ONE launch of this entry."""
    t = Tower(precision=F16X2, n_calls=2)
    t.d.defer_reduce, t.d.fwd_ws, t.d.fwd_calls = 1, t.ws.data_ptr(), 2
    t.refused(t.reduce_step(n=t.n_flat - 1), E_ARG, "tower_reduce_step: layer 1's gradients are not inside the flat buffer")
    t.d.fwd_calls = 1                           # (one call: the same text)
    t.refused(t.reduce_step(n=t.n_flat - 1), E_ARG, "tower_reduce_step: layer 1's gradients are not inside the flat buffer")


# ---------------------------------------------------------------------------------------------------------------------
# the descriptor checks every entry shares
# ---------------------------------------------------------------------------------------------------------------------
def test_every_entry_checks_the_descriptor_first():
    t = Tower(precision=F16X2, n_calls=2)
    t.d.precision = 4
    text = 'tower: precision=4 (0 = fp32, 1 = bf16 operands, 2 = bf16 x 3, 3 = fp16 x 2)'
    for call in (lambda: t.forward(x2=t.x, n_calls=1), lambda: t.backward(scratch_floats=0), lambda: t.backward_launch(part=0),
                 lambda: t.backward_loss(kind=7), lambda: t.reduce_step(kind=9)):
        t.refused(call(), E_ARG, text)
    t.d.precision = F16X2
    t.refused(t.forward(rows=63), E_ARG, 'tower: rows=63 not divisible by n_calls=2')
    t.d.act = 7
    t.refused(t.forward(), E_UNSUPPORTED, 'tower: unsupported activation 7')
