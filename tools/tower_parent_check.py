"""Bit-identity of the tower and single-Linear entry points against another build of the library (the parent commit's).

For every ABN_PATH_* value one small seeded tower runs forward and backward (abn_tower_reduce_step where the backward
leaves it the job), abn_tower_path confirming the path, and every abn_linear_* entry runs on two shapes; each library
does so in a fresh child process (ABNET3_HIP_LIB) under its own time limit, the run stops at the first child that fails,
and the dumped outputs are compared byte for byte.  Host-side refactors of csrc/tower.hip must leave every one identical.

python tools/tower_parent_check.py --parent-lib FILE [--keep DIR]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (40, 96, 200, 32)
# name: (forward path, backward path or None, precision, batch_norm, rows, n_calls, train, descriptor extras, switches)
CASES = {
    'per_layer_fp32': (0, 0, 0, 0, 300, 2, 1, {}, {}),
    'per_layer_bf16': (0, 0, 1, 0, 300, 2, 1, {}, {'ABN_PLANES': 0}),
    'per_layer_bf16x3_pair_grid': (0, 0, 2, 0, 512, 1, 1, {}, {'ABN_PLANES': 0, 'ABN_GEMM_TILE': 1}),
    'per_layer_batch_norm': (0, 0, 0, 1, 300, 2, 1, {}, {}),
    'fused_fp32': (1, 0, 0, 0, 320, 2, 1, {}, {'ABN_FUSED_MIN_ROWS': 256}),
    'planes': (2, 2, 3, 0, 512, 2, 1, {}, {'ABN_WIDE': 0}),
    'planes_bf16x3_deferred': (2, 2, 2, 0, 384, 1, 1, {'defer_reduce': 1}, {'ABN_WIDE': 0}),
    'planes_infer': (3, None, 3, 0, 512, 1, 0, {'forward_only': 1}, {'ABN_WIDE': 0}),
    'planes_infer_bn': (4, None, 3, 1, 512, 1, 0, {'forward_only': 1}, {}),
    'bn_layers': (5, 5, 3, 1, 512, 2, 1, {}, {}),
    'bn_tower': (7, 7, 3, 1, 512, 2, 1, {'sync_ws': True}, {}),
    'wide': (6, 6, 3, 0, 256, 2, 1, {}, {}),
    'wide_bf16': (6, 6, 1, 0, 192, 1, 1, {}, {}),
    'wide_step': (6, 6, 3, 0, 256, 2, 1, {'defer_reduce': 1, 'fwd_ws': True}, {}),
}
LINEAR_SHAPES = [(300, 72, 136), (130, 37, 67)]


def tower_case(name, out):
    import numpy as np
    import torch
    from abnet3_amd import _lib
    fpath, bpath, precision, bn, rows, n_calls, train, extra, env = CASES[name]
    for k, v in env.items():
        os.environ[k] = str(v)
    _lib.reload_switches()
    lib, p = _lib.load(), _lib.ptr
    g = torch.Generator().manual_seed(len(name) + 17 * rows)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()
    nl = len(DIMS) - 1
    d = _lib.TowerDesc()
    d.n_layers, d.act, d.last_act, d.batch_norm, d.precision = nl, 1, 3, bn, precision
    for i, w in enumerate(DIMS):
        d.dims[i] = w
    sizes = []
    for l in range(nl):
        sizes += [DIMS[l + 1] * DIMS[l], DIMS[l + 1]] + ([DIMS[l + 1]] * 2 if bn else [])
    n = sum(sizes)
    params, grads = 0.2 * rnd(n), torch.full((n,), float('nan'), device='cuda')
    keep, o, k = [], 0, 0
    for l in range(nl):
        for pn, gn in [('W', 'dW'), ('b', 'db')] + ([('bn_w', 'dbn_w'), ('bn_b', 'dbn_b')] if bn else []):
            getattr(d, pn)[l], getattr(d, gn)[l] = params[o:].data_ptr(), grads[o:].data_ptr()
            if pn == 'bn_w':
                params[o:o + sizes[k]] += 1.0
            o += sizes[k]
            k += 1
        if bn:
            rm, rv, nbt = 0.1 * rnd(DIMS[l + 1]), 1.0 + 0.1 * rnd(DIMS[l + 1]).abs(), torch.zeros(1, dtype=torch.int64, device='cuda')
            keep += [rm, rv, nbt]
            d.bn_rm[l], d.bn_rv[l], d.bn_nbt[l] = rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()
    for key, v in extra.items():
        if key not in ('sync_ws', 'fwd_ws'):
            setattr(d, key, v)
    ws = torch.zeros(lib.abn_tower_ws_floats(C.byref(d), rows, n_calls), device='cuda')
    scratch = torch.zeros(lib.abn_tower_bwd_scratch_floats(C.byref(d), rows), device='cuda')
    if extra.get('sync_ws'):
        sync = torch.zeros(lib.abn_tower_sync_ws_bytes() // 4 + 4, device='cuda')
        keep.append(sync)
        d.sync_ws = sync.data_ptr()
    if extra.get('fwd_ws'):
        d.fwd_ws, d.fwd_calls = ws.data_ptr(), n_calls
    x = rnd(rows, DIMS[0])
    x1, x2 = (x[:rows // 2], x[rows // 2:]) if n_calls == 2 else (x, None)
    d_out, dx = rnd(rows, DIMS[-1]), torch.full((rows, DIMS[0]), float('nan'), device='cuda')
    want_dx = n_calls == 1                  # (d loss / d input: one forward_once call's rows are contiguous)

    def path(backward):
        return lib.abn_tower_path(C.byref(d), p(x1), p(x2), rows, n_calls, train, p(ws), backward, None)
    assert path(0) == fpath, (name, 'forward path', path(0))
    _lib.check(lib.abn_tower_forward(C.byref(d), p(x1), p(x2), rows, n_calls, train, p(ws), None), name + ' forward')
    o_out = lib.abn_tower_out_offset(C.byref(d), rows, n_calls)
    out[name + '/embeddings'] = ws[o_out:o_out + rows * DIMS[-1]]
    if bn:
        out[name + '/bn_state'] = torch.cat([t.float().flatten() for t in keep[:3 * nl]])
    if bpath is not None:
        assert path(1) == bpath, (name, 'backward path', path(1))
        _lib.check(lib.abn_tower_backward(C.byref(d), p(x1), p(x2), p(d_out), rows, n_calls, p(ws), p(scratch), scratch.numel(),
                                          p(dx) if want_dx else None, None), name + ' backward')
        if d.defer_reduce:
            s1, s2 = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
            _lib.check(lib.abn_tower_reduce_step(C.byref(d), rows, p(scratch), scratch.numel(), 1, p(params), p(grads), p(s1), p(s2),
                                                 n, 0.1, 0.9, 0.0, 1e-6, 1, 1.0, None), name + ' reduce_step')
            out[name + '/params'], out[name + '/state1'], out[name + '/state2'] = params, s1, s2
        out[name + '/grads'] = grads
        if want_dx:
            out[name + '/dx'] = dx
    torch.cuda.synchronize()
    for k in list(out):
        if not isinstance(out[k], np.ndarray):
            out[k] = out[k].detach().cpu().numpy().copy()
    for k in env:
        del os.environ[k]
    _lib.reload_switches()


def linear_cases(out):
    import torch
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')
    for tile in (None, 1):                  # (ABN_GEMM_TILE=1: wgrad and dgrad of a layer go out as one grid)
        if tile is not None:
            os.environ['ABN_GEMM_TILE'] = str(tile)
        _lib.reload_switches()
        for rows, k, n in LINEAR_SHAPES:
            g = torch.Generator().manual_seed(rows + k + n)
            x, W, b, dz = [torch.randn(*s, generator=g).cuda() for s in ((rows, k), (n, k), (n,), (rows, n))]
            a = torch.sigmoid(x)
            tag = 'linear_%dx%dx%d_tile%s/' % (rows, k, n, tile)
            y, dx = nan(rows, n), nan(rows, k)
            _lib.check(lib.abn_linear_forward(p(x), p(W), p(b), rows, k, n, 1, p(y), None), 'linear_forward')
            _lib.check(lib.abn_linear_dgrad(p(dz), p(W), rows, k, n, p(a), 1, p(dx), None), 'linear_dgrad')
            nsc = lib.abn_linear_wgrad_scratch_floats(rows, k, n)
            out[tag + 'wgrad_scratch_floats'] = torch.tensor([nsc])
            sc, dW, db = nan(nsc), nan(n, k), nan(n)
            _lib.check(lib.abn_linear_wgrad(p(dz), p(a), rows, k, n, p(dW), p(db), p(sc), nsc, None), 'linear_wgrad')
            out.update({tag + 'forward': y, tag + 'dgrad': dx, tag + 'wgrad_dW': dW, tag + 'wgrad_db': db})
            sc, dW, db, dx = nan(nsc), nan(n, k), nan(n), nan(rows, k)
            _lib.check(lib.abn_linear_backward(p(dz), p(W), p(a), rows, k, n, 1, p(dW), p(db), p(dx), p(sc), nsc, None), 'linear_backward')
            out.update({tag + 'backward_dW': dW, tag + 'backward_db': db, tag + 'backward_dx': dx})
            for prec in range(4):
                for act in (0, 1):
                    sc, dW, db, dx = nan(nsc), nan(n, k), nan(n), nan(rows, k)
                    _lib.check(lib.abn_linear_backward_prec(p(dz), p(W), p(a), rows, k, n, act, prec, p(dW), p(db), p(dx), p(sc), nsc,
                                                            None), 'linear_backward_prec')
                    out.update({tag + 'prec%d_act%d_%s' % (prec, act, nm): v for nm, v in (('dW', dW), ('db', db), ('dx', dx))})
    os.environ.pop('ABN_GEMM_TILE', None)
    _lib.reload_switches()
    torch.cuda.synchronize()
    for k in list(out):
        if hasattr(out[k], 'cpu'):
            out[k] = out[k].detach().cpu().numpy().copy()


def dump(path):
    import numpy as np
    out = {}
    for name in CASES:
        tower_case(name, out)
    linear_cases(out)
    np.savez(path, **{k.replace('/', '.'): v for k, v in out.items()})
    print('%d outputs from %s' % (len(out), os.environ.get('ABNET3_HIP_LIB', "the tree's library")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', help="the parent commit's build of the library")
    ap.add_argument('--keep', default=None, help='directory to keep the two dumps in')
    ap.add_argument('--dump', default=None, help='(child) run every case with the library in ABNET3_HIP_LIB and write FILE')
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child')
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump)
    if not a.parent_lib:
        ap.error('--parent-lib is required')
    import numpy as np
    from abnet3_amd import build
    work = a.keep or tempfile.mkdtemp(prefix='abn_parent_check_')
    os.makedirs(work, exist_ok=True)
    files = {}
    for side, lib in (('parent', os.path.abspath(a.parent_lib)), ('this', build.LIB)):
        files[side] = os.path.join(work, side + '.npz')
        env = dict(os.environ, ABNET3_HIP_LIB=lib)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--dump', files[side]], env=env, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                         # nothing more is started after a child that failed
            print('FAILED: the %s build exited with %d' % (side, rc))
            return 1
    A, B = np.load(files['parent']), np.load(files['this'])
    assert sorted(A.files) == sorted(B.files)
    differ = [k for k in A.files if A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    nonfinite = [k for k in A.files if A[k].dtype.kind == 'f' and not np.isfinite(A[k]).all()]
    print('%d outputs compared, %d differ, %d hold a non-finite value' % (len(A.files), len(differ), len(nonfinite)))
    for k in differ:
        print('  differs:', k)
    for k in nonfinite:
        print('  non-finite (an output the entry did not write?):', k)
    return 1 if differ or nonfinite else 0


if __name__ == '__main__':
    sys.exit(main())
