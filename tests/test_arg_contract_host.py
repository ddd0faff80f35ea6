"""tests/arg_contract.py on a fake library object and on CPU tensors, and the ledger of tests/test_gpu_arg_contract.py: every
entry include/abnet3_hip.h declares (abnet3_amd._lib.SYMBOLS) is in exactly one of SURFACE (a row holds the Python entry in
front of it to the argument contract), QUERIES (tests/test_dirty_memory_host.py: it touches no device memory) or EXCLUDED (no
caller-supplied array reaches it; the reason names the call site).  A new C entry without a row fails here.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import arg_contract as AC
from arg_contract import LeakedPointer, ReachedLibrary, guarded
from test_dirty_memory_host import QUERIES

NO_WRAPPER = 'it has no Python wrapper: abnet3_amd/*.py never calls it (tests and tools under tests/ and tools/ call the entry itself)'
LINEAR = NO_WRAPPER + '; tests/test_gpu_linear_entries.py holds it'
MAILBOX = 'a mailbox between the processes of a data-parallel job (parallel.OneShotAllReduce.all_reduce on the flat gradient buffer of the job): not a single-process call'
EXCLUDED = {
    'abn_linear_forward': LINEAR,
    'abn_linear_dgrad': LINEAR,
    'abn_linear_wgrad': LINEAR,
    'abn_linear_backward': LINEAR,
    'abn_linear_backward_prec': LINEAR,
    'abn_tower_backward_launch': NO_WRAPPER,
    'abn_dtw_batched': NO_WRAPPER + ' since utils.dtw_align_batch took abn_dtw_batched_overlap',
    'abn_arccos_f32': NO_WRAPPER,
    'abn_allreduce_oneshot': MAILBOX,
    'abn_rccl_allreduce_f64': MAILBOX + '; the library calls it back through abn_tower_desc.bn_sync_fn with its own statistics',
    'abn_optimizer_step': 'trainer.FlatOptimizer.step calls it on the network\'s flat parameter, gradient and state buffers, which '
                          'model._HipNetwork.flatten_parameters and the optimizer allocated',
    'abn_tower_reduce_step': 'trainer.FlatOptimizer.step calls it on the slabs and the descriptor model.SiameseNetwork.direct_backward left in '
                             '_pending_reduce and on the network\'s own flat buffers',
    'abn_tower_backward_loss': 'model.SiameseNetwork.direct_backward_loss, the trainer\'s autograd-free step: x1 / x2 are the copies '
                               'model._segment_forward checked and kept (the tower row holds that check), and labels it does not take make it '
                               'return None, after which the trainer goes through loss.value_and_dz (the pair-loss row)',
    'abn_pair_loss_padded': 'trainer.TrainerSiamese._planned_eval calls it inside a captured evaluation step on the padded batch and the counters '
                            'the trainer allocated',
    'abn_gather_pairs': 'trainer.TrainerSiamese._planned_step / _planned_eval and dataloader.MultimodalDataLoader.load_batch call it on the table and the index '
                        'columns of a plan the loaders built and uploaded themselves',
    'abn_tcl_pairs': 'dataloader.OriginalDataLoader._tcl_fill calls it on the row table and the plan columns the loader built and uploaded itself',
}


# ----------------------------------------------------------------------------------------------------------------------
# the guard on a fake library
# ----------------------------------------------------------------------------------------------------------------------
class Lib(object):
    pass


def fake_lib():
    lib = Lib()
    for name in AC.all_symbols():
        setattr(lib, name, (lambda name: lambda *a: (name, len(a)))(name))
    return lib, {name: getattr(lib, name) for name in AC.all_symbols()}


def vp(p):
    return ctypes.c_void_p(p)


def test_exceptions_are_not_refusals():
    from abnet3_amd._lib import HipLibraryError
    for e in (ReachedLibrary, LeakedPointer):
        assert e.__bases__ == (Exception,) and not issubclass(e, (ValueError, TypeError, AssertionError, HipLibraryError))


def test_range_detection_at_both_ends_of_a_span():
    lib, _ = fake_lib()
    b, e = 0x10000, 0x10040
    with guarded(lib, forbidden=[(b, e)]) as log:
        assert lib.abn_gather_rows(vp(b - 1), vp(e), 3, 4, None, None) == ('abn_gather_rows', 6)       # just outside, both ends
        for inside, index in ((b, 0), (e - 1, 1), (b + 7, 4)):
            args = [vp(0x500), vp(0x600), 3, 4, vp(0x700), None]
            args[index] = vp(inside)
            with pytest.raises(LeakedPointer) as info:
                lib.abn_gather_rows(*args)
            assert (info.value.name, info.value.index) == ('abn_gather_rows', index)
        # an integer passed for a size is no pointer, whatever its value; a plain int passed for a pointer is one
        assert lib.abn_gather_rows(vp(0x500), vp(0x600), b + 1, b + 2, None, None)
        with pytest.raises(LeakedPointer):
            lib.abn_gather_rows(b + 8, vp(0x600), 3, 4, None, None)
        # a numpy array handed over by ctypes.data / data_as
        a = np.zeros(16, dtype=np.int64)
    with guarded(lib, forbidden=[AC.span(a)]) as log2:
        with pytest.raises(LeakedPointer):
            lib.abn_gather_rows(a[3:].ctypes.data_as(ctypes.c_void_p), None, 1, 1, None, None)          # (a view: its base is the span)
        with pytest.raises(LeakedPointer):
            lib.abn_tcl_pairs(None, None, a.ctypes.data, 3, None, 0, 1, 1, 0, 0, 0, None, None, None, None, 1, 1, None)
    assert log.launched == ['abn_gather_rows', 'abn_gather_rows'] and log.blocked == ['abn_gather_rows'] * 4
    assert log2.launched == [] and len(log2.blocked) == 2


def test_pointers_inside_a_structure():
    from abnet3_amd import _lib
    lib, _ = fake_lib()
    desc = _lib.TowerDesc()
    desc.W[2] = 0x20010
    tabs = _lib.SamplerTables()
    tabs.toks = 0x30000
    with guarded(lib, forbidden=[(0x20000, 0x20020)]):
        with pytest.raises(LeakedPointer) as info:
            lib.abn_tower_forward(ctypes.byref(desc), vp(1), vp(2), 4, 2, 1, vp(3), None)
        assert info.value.index == 0
        with pytest.raises(LeakedPointer):
            lib.abn_tower_forward(ctypes.pointer(desc), vp(1), vp(2), 4, 2, 1, vp(3), None)
        with pytest.raises(LeakedPointer):
            lib.abn_tower_forward(desc, vp(1), vp(2), 4, 2, 1, vp(3), None)                               # by value
        desc.W[2], desc.fwd_ws = 0x20020, 0x1FFFF                                                         # one past the end, one before
        assert lib.abn_tower_forward(ctypes.byref(desc), vp(1), vp(2), 4, 2, 1, vp(3), None)
        desc.fwd_ws = 0x2001F                                                                             # a plain pointer field
        with pytest.raises(LeakedPointer):
            lib.abn_tower_forward(ctypes.byref(desc), vp(1), vp(2), 4, 2, 1, vp(3), None)
    with guarded(lib, forbidden=[(0x30000, 0x30001)]):
        with pytest.raises(LeakedPointer):
            lib.abn_sample_pairs(ctypes.byref(tabs), None, 0, None, None, None, 64, None)


def test_queries_pass_and_block_all_stops_the_rest():
    lib, _ = fake_lib()
    with guarded(lib, block_all=True) as log:
        assert lib.abn_abi_version() == ('abn_abi_version', 0) and lib.abn_knn_ws_bytes(1, 2, 3) == ('abn_knn_ws_bytes', 3)
        assert lib.abnu_hmm_hsmm_max_duration() == ('abnu_hmm_hsmm_max_duration', 0)
        for name in ('abn_knn_topk', 'abnt_nce_loss'):
            with pytest.raises(ReachedLibrary) as info:
                getattr(lib, name)(None)
            assert info.value.name == name
    assert log.calls == ['abn_abi_version', 'abn_knn_ws_bytes', 'abnu_hmm_hsmm_max_duration'] and not log.launched
    assert log.blocked == ['abn_knn_topk', 'abnt_nce_loss']
    # a query is a query under a forbidden range too: abn_dtw_ws_bytes reads the host columns the wrapper made
    a = np.zeros(4, dtype=np.int32)
    with guarded(lib, forbidden=[AC.span(a)]) as log:
        assert lib.abn_dtw_ws_bytes(a.ctypes.data_as(ctypes.c_void_p), None, 4, 1, 1)
    assert log.calls == ['abn_dtw_ws_bytes'] and not log.launched
    assert AC.NEXT_QUERIES <= set(AC.all_symbols()) and not AC.NEXT_QUERIES & set(QUERIES)


def test_the_entries_come_back_also_after_an_exception():
    lib, before = fake_lib()
    with guarded(lib):
        assert all(getattr(lib, name) is not before[name] for name in before)
    assert all(getattr(lib, name) is before[name] for name in before)
    for exc, kw in ((KeyError, {}), (ReachedLibrary, dict(block_all=True)), (LeakedPointer, dict(forbidden=[(8, 16)]))):
        with pytest.raises(exc):
            with guarded(lib, **kw):
                lib.abn_gather_rows(vp(8), None, 1, 1, None, None)
                raise KeyError('x')
        assert all(getattr(lib, name) is before[name] for name in before)


@pytest.mark.parametrize('as_numpy', [False, True])
def test_view_builders_keep_values_and_are_not_contiguous(as_numpy):
    t = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    t[1, 1] = float('nan')
    t = t.numpy() if as_numpy else t
    contiguous = lambda v: v.flags['C_CONTIGUOUS'] if as_numpy else v.is_contiguous()
    nbytes = 60
    for build in (AC.strided_cols, AC.transposed, AC.strided_rows):
        v = build(t)
        assert tuple(v.shape) == (5, 3) and v.dtype == t.dtype and not contiguous(v) and AC.same_values(v, t)
        lo, hi = AC.span(v)
        assert hi - lo >= 2 * nbytes or build is AC.transposed and hi - lo >= nbytes
        first = v.ctypes.data if as_numpy else v.data_ptr()
        assert lo <= first < hi
    one = t[:, 0].copy() if as_numpy else t[:, 0].clone()
    v = AC.strided_rows(one)
    assert tuple(v.shape) == (5,) and not contiguous(v) and AC.same_values(v, one)
    with pytest.raises(AssertionError):
        AC.strided_rows(one[:1])                            # one row: every view of it is contiguous
    with pytest.raises(AssertionError):
        AC.transposed(t[:, :1])


def test_wider_never_narrows():
    pairs = ((torch.float32, torch.float64), (torch.int32, torch.int64), (torch.uint8, torch.int32), (torch.int64, torch.float64))
    for frm, to in pairs:
        t = torch.tensor([3, 0, 200, 7]).to(frm)
        w = AC.wider(t)
        assert w.dtype == to and w.element_size() >= t.element_size() and w.is_contiguous() and (w.to(frm) == t).all()
        wn = AC.wider(t.numpy())
        assert str(wn.dtype) == str(to).replace('torch.', '') and (wn.astype(t.numpy().dtype) == t.numpy()).all()
    assert AC.wider(torch.zeros(2, dtype=torch.float64)) is None and AC.wider(np.zeros(2, dtype=np.int16)) is None
    lo, hi = AC.span(AC.wider(torch.zeros(7, dtype=torch.float32)))
    assert hi - lo >= 56


def test_span_covers_the_whole_allocation():
    base = torch.zeros(10, 6)
    v = base[2:5, ::2]
    assert AC.span(v) == (base.data_ptr(), base.data_ptr() + 240)
    nb = np.zeros((10, 6), dtype=np.float32)
    assert AC.span(nb[2:5, ::2][1:]) == (nb.ctypes.data, nb.ctypes.data + 240)


# ----------------------------------------------------------------------------------------------------------------------
# the ledger
# ----------------------------------------------------------------------------------------------------------------------
def test_every_entry_is_accounted_for():
    from abnet3_amd import _lib
    import test_gpu_arg_contract as G
    claimed = {}
    for row in G.SURFACE:
        for e in row.entries:
            claimed.setdefault(e, []).append(row.name)
    symbols = set(_lib.SYMBOLS)
    later = set(AC.all_symbols()) - symbols            # (include/abnet3_hip_next.h: rows claim them, the ledger is the numbered ABI's)
    assert not set(claimed) - symbols - later, 'a row claims an entry no header declares: %s' % sorted(set(claimed) - symbols - later)
    assert not later - AC.NEXT_QUERIES - set(claimed), 'no row for: %s' % sorted(later - AC.NEXT_QUERIES - set(claimed))
    assert not (QUERIES | set(EXCLUDED)) - symbols, sorted((QUERIES | set(EXCLUDED)) - symbols)
    rows = (set(claimed) & symbols) - QUERIES                      # (a row may also prove that it asked a query: the query stays a query)
    assert not rows & set(EXCLUDED), sorted(rows & set(EXCLUDED))
    assert not QUERIES & set(EXCLUDED)
    missing = symbols - rows - QUERIES - set(EXCLUDED)
    assert not missing, 'no row (tests/test_gpu_arg_contract.py), query or exclusion for: %s' % sorted(missing)
    # a reason is a sentence that names the call site
    assert all(isinstance(r, str) and len(r) > 40 and ('.' in r or 'abnet3_amd' in r) for r in EXCLUDED.values())
    # five single-Linear entries, three more without a Python caller, two mailboxes, and six the trainer and the loaders
    # call on memory they allocated themselves: the list does not grow silently
    assert len(EXCLUDED) == 16


def test_the_table_is_well_formed():
    import test_gpu_arg_contract as G
    for row in G.SURFACE:
        names = set(row.args)
        assert names, row.name
        for group in row.widths + row.lengths:
            assert set(group) <= names, (row.name, group)
        for name in (n for g in row.widths for n in g):
            assert row.args[name].rank == 2, (row.name, name)
        for a in row.args.values():
            assert a.where in ('device', 'host', 'any') and a.rank in (1, 2) and not (a.out and a.where == 'host')
        assert G.value_mutations(row) and row.same_bits
    # every row mutates something of every kind the contract names
    kinds = {k for _, _, k in G.VALUE_CASES} | {k for _, _, k in G.SHAPE_CASES}
    assert kinds == {'strided_cols', 'transposed', 'strided_rows', 'wider', 'list', 'other_int', 'rank_up', 'rank_down', 'cpu', 'narrower',
                     'broader', 'shorter'}
