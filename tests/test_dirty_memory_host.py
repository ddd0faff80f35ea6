"""tests/dirty_memory.py on CPU tensors, and the coverage ledger of tests/test_gpu_dirty_memory.py: every entry
include/abnet3_hip.h declares (abnet3_amd._lib.SYMBOLS) is in exactly one of CASES (a dirty-memory case reaches it), QUERIES
(a size / limit / version / error getter that touches no device memory) or EXCLUDED (with the reason).  A new C entry
without a dirty-memory case fails here.  No GPU needed."""
import numpy as np
import pytest
import torch

import dirty_memory
from dirty_memory import dirty

# pure host functions: sizes, limits, the version, the last error, the path a call would take, the switches
QUERIES = {
    'abn_abi_version', 'abn_last_error', 'abn_reload_switches',
    'abn_tower_ws_floats', 'abn_tower_out_offset', 'abn_tower_bwd_scratch_floats', 'abn_tower_wpack_floats', 'abn_tower_uses_planes',
    'abn_tower_path', 'abn_tower_image_offset', 'abn_tower_backward_loss_ws_bytes', 'abn_tower_sync_ws_bytes',
    'abn_linear_wgrad_scratch_floats', 'abn_pair_loss_ws_bytes', 'abn_oneshot_mail_bytes',
    'abn_dtw_ws_bytes', 'abn_dtw_host_stage_bytes', 'abn_dtw_cost_max_n2', 'abn_dtw_search_max_query', 'abn_dtw_local_max_n2',
    'abn_edit_max_short', 'abn_mvn_ws_bytes', 'abn_mfcc_path', 'abn_integrate_ws_bytes', 'abn_knn_ws_bytes',
    'abn_gmm_max_d', 'abn_gmm_max_k', 'abn_gmm_ws_bytes', 'abn_kmeans_max_d', 'abn_kmeans_max_k', 'abn_kmeans_ws_bytes',
    'abn_kmeans_viterbi_max_len', 'abn_kmeans_viterbi_max_k', 'abn_kmeans_viterbi_ws_bytes',
    'abn_hmm_max_len', 'abn_hmm_max_k', 'abn_hmm_ws_bytes', 'abn_hmm_accumulate_ws_bytes', 'abn_hmm_viterbi_ws_bytes',
    'abn_esk_max_span', 'abn_sd_grid_runs',
}

LINEAR = ('tests/test_gpu_linear_entries.py runs it on NaN-filled outputs and scratch between guard bands')
MAILBOX = 'a mailbox between the processes of a data-parallel job (tests/test_gpu_dp.py, tests/rccl_worker.py): not a single-process call'
EXCLUDED = {
    'abn_linear_forward': LINEAR,
    'abn_linear_dgrad': LINEAR,
    'abn_linear_wgrad': LINEAR,
    'abn_linear_backward': LINEAR,
    'abn_linear_backward_prec': LINEAR,
    'abn_allreduce_oneshot': MAILBOX,
    'abn_rccl_allreduce_f64': MAILBOX + '; it forwards to the caller\'s ncclAllReduce and owns no memory',
}


def test_patterns_per_dtype():
    with dirty(0xFF) as n:
        f32, f64 = torch.empty(5, 3), torch.empty(7, dtype=torch.float64)
        i32, i64 = torch.empty(4, dtype=torch.int32), torch.empty(2, 2, dtype=torch.int64)
        u8 = torch.empty_like(torch.zeros(9, dtype=torch.uint8))
    assert int(n) == 5 and n.nbytes == 60 + 56 + 16 + 32 + 9
    assert torch.isnan(f32).all() and torch.isnan(f64).all() and (i32 == -1).all() and (i64 == -1).all() and (u8 == 255).all()
    with dirty(0xC2):
        f32, f64, i32 = torch.empty(6), torch.empty(3, dtype=torch.float64), torch.empty(3, dtype=torch.int32)
    assert (f32.numpy().view(np.uint32) == 0xC2C2C2C2).all() and abs(float(f32[0]) + 97.38) < 0.01
    assert torch.isfinite(f64).all() and (i32 < 0).all() and (i32.numpy().view(np.uint32) == 0xC2C2C2C2).all()
    with dirty(0x00):
        z = torch.empty(1000)
    assert not z.any()


def test_shapes_the_hook_must_survive():
    with dirty(0xFF) as n:
        scalar = torch.empty((), dtype=torch.float32)                   # 0-dim
        nothing = torch.empty(0, 7)                                     # zero-size: skipped, not counted
        like = torch.empty_like(torch.zeros(3, 4).t())                  # dense, not contiguous
        kw = torch.empty(size=(2, 3), dtype=torch.float64, device='cpu')
        assert torch.zeros(3).sum() == 0 and (torch.full((3,), 2.0) == 2).all() and (torch.ones(2) == 1).all()      # left alone
    assert int(n) == 3 and torch.isnan(scalar) and nothing.numel() == 0 and torch.isnan(like).all() and like.shape == (4, 3)
    assert torch.isnan(kw).all()
    if torch.cuda.is_available():                                       # (pinned memory needs a device runtime)
        with dirty(0xC2):
            pinned = torch.empty(16, dtype=torch.uint8).pin_memory()
        assert (pinned == 0xC2).all()


def test_both_functions_come_back_also_after_an_exception():
    empty, empty_like = torch.empty, torch.empty_like
    with dirty(0xFF):
        assert torch.empty is not empty and torch.empty_like is not empty_like
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(ZeroDivisionError):
        with dirty(0xFF):
            1 / 0
    assert torch.empty is empty and torch.empty_like is empty_like
    with dirty(0xFF) as outer:                                          # nested windows unwind in order
        with dirty(0x00) as inner:
            assert not torch.empty(4).any()
        assert torch.isnan(torch.empty(4)).all()
    assert torch.empty is empty and int(inner) == 1 and int(outer) == 2


def test_recorded_wraps_and_restores_the_entries():
    class Lib(object):
        pass
    from abnet3_amd import _lib
    lib = Lib()
    for name in _lib.SYMBOLS:
        setattr(lib, name, (lambda name: lambda *a: (name, a))(name))
    before = {name: getattr(lib, name) for name in _lib.SYMBOLS}
    with dirty_memory.recorded(lib) as calls:
        assert lib.abn_abi_version() == ('abn_abi_version', ()) and lib.abn_gather_rows(1, 2) == ('abn_gather_rows', (1, 2))
    assert calls == ['abn_abi_version', 'abn_gather_rows']
    assert all(getattr(lib, name) is before[name] for name in _lib.SYMBOLS)
    with pytest.raises(KeyError):
        with dirty_memory.recorded(lib):
            raise KeyError('x')
    assert all(getattr(lib, name) is before[name] for name in _lib.SYMBOLS)


def test_bits_compares_nan_with_nan():
    a = np.array([np.nan, 1.0, -0.0], dtype=np.float32)
    assert (dirty_memory.bits(a) == dirty_memory.bits(a.copy())).all()
    assert not (dirty_memory.bits(a) == dirty_memory.bits(np.array([np.nan, 1.0, 0.0], dtype=np.float32))).all()
    assert dirty_memory.bits(np.float64(3.0)).dtype == np.uint64 and dirty_memory.bits(np.arange(3)).dtype == np.arange(3).dtype


def test_every_entry_is_accounted_for():
    from abnet3_amd import _lib
    import test_gpu_dirty_memory as G
    claimed = {}
    for case in G.CASES:
        for e in case.entries:
            claimed.setdefault(e, []).append(case.name)
    symbols = set(_lib.SYMBOLS)
    assert not set(claimed) - symbols, 'a case claims an entry the header does not declare: %s' % sorted(set(claimed) - symbols)
    assert not (QUERIES | set(EXCLUDED)) - symbols, sorted((QUERIES | set(EXCLUDED)) - symbols)
    cases = set(claimed) - QUERIES                     # (a case may also prove that it asked a query: the query stays a query)
    assert not cases & set(EXCLUDED), sorted(cases & set(EXCLUDED))
    assert not QUERIES & set(EXCLUDED)
    missing = symbols - cases - QUERIES - set(EXCLUDED)
    assert not missing, 'no dirty-memory case (tests/test_gpu_dirty_memory.py), query or exclusion for: %s' % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 20 for r in EXCLUDED.values())
    # the five single-Linear entries and the multi-process mailboxes: the list does not grow silently
    assert len(EXCLUDED) == 7
