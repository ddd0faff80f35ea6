"""tests/side_stream.py on CPU tensors and a fake library object (a counting delay in place of the GPU's), and the coverage
ledger of tests/test_gpu_side_stream.py: every key of every *_SYMBOLS dictionary of abnet3_amd/_lib.py is in exactly one of
the side-stream cases (a case reaches it on the lagging stream), QUERIES (a host-only getter) or EXCLUDED (with the reason).
A new entry without a side-stream case fails here.  No GPU needed."""
import numpy as np
import pytest
import torch

import side_stream
from dirty_memory import dirty
from side_stream import lagging
from test_dirty_memory_host import MAILBOX, QUERIES as MAIN_QUERIES

# the host-only getters: those of the main ledger, and the other sections' limits, workspace sizes and path queries
SECTION_QUERIES = {
    'abnx_viterbi_dur_max',
    'abny_hmm_dense_max_k', 'abny_hmm_dense_ws_bytes',
    'abnz_hmm_dense_viterbi_ws_bytes',
    'abnw_hmm_dense_viterbi_dur_ws_bytes',
    'abnv_hmm_hard_stats_ws_bytes',
    'abnu_hmm_hsmm_max_duration', 'abnu_hmm_hsmm_viterbi_ws_bytes',
    'abnt_nce_max_d', 'abnt_nce_ws_bytes',
    'abns_edit_hist_max_len', 'abns_edit_cluster_hist_ws_bytes',
    'abnr_recon_max_d', 'abnr_recon_ws_bytes',
    'abnq_softdtw_max_len', 'abnq_softdtw_max_d', 'abnq_softdtw_ws_bytes',
}
QUERIES = MAIN_QUERIES | SECTION_QUERIES

EXCLUDED = {
    'abn_allreduce_oneshot': MAILBOX,
    'abn_rccl_allreduce_f64': MAILBOX + '; it forwards to the caller\'s ncclAllReduce and owns no memory',
}


class Lib(object):
    """Every entry of every ledger as a function that logs its call and returns its name and arguments."""

    def __init__(self, log):
        for name in side_stream.all_symbols():
            setattr(self, name, (lambda name: lambda *a: (log.append(name), (name, a))[1])(name))


def counter(log):
    return lambda: log.append('delay')


def snapshot(lib):
    return {name: getattr(lib, name) for name in side_stream.all_symbols()}, {name: getattr(torch, name) for name in side_stream.ALLOCATORS}


def restored(lib, before):
    entries, allocators = before
    return all(getattr(lib, n) is f for n, f in entries.items()) and all(getattr(torch, n) is f for n, f in allocators.items())


def test_all_symbols_is_every_ledger_of_the_binding():
    from abnet3_amd import _lib
    ledgers = [k for k in vars(_lib) if k.endswith('SYMBOLS') and isinstance(getattr(_lib, k), dict)]
    assert sorted(ledgers) == sorted(side_stream.LEDGERS)
    assert len(side_stream.all_symbols()) == sum(len(getattr(_lib, k)) for k in ledgers)


def test_a_delay_in_front_of_every_entry_and_every_allocation():
    log = []
    lib = Lib(log)
    before = snapshot(lib)
    with lagging(lib, counter(log)) as lag:
        assert lag.side is None                                     # (no device here: the stream is the GPU file's business)
        assert lib.abn_gather_rows(1, 2) == ('abn_gather_rows', (1, 2))
        assert lib.abnq_softdtw_backward() == ('abnq_softdtw_backward', ()) and lib.abns_edit_hist_max_len() == ('abns_edit_hist_max_len', ())
        assert log == ['delay', 'abn_gather_rows', 'delay', 'abnq_softdtw_backward', 'delay', 'abns_edit_hist_max_len']
        del log[:]
        f32, i32 = torch.empty(5, 3), torch.empty_like(torch.tensor([1, 2], dtype=torch.int32))       # poisoned behind a delay
        assert torch.isnan(f32).all() and (i32 == -1).all()
        z, zl, fu, on = torch.zeros(3), torch.zeros_like(f32), torch.full((2,), 2.0), torch.ones(2)   # delayed, not poisoned
        assert not z.any() and not zl.any() and (fu == 2).all() and (on == 1).all()
        assert log == ['delay'] * 6
    assert lag.calls == ['abn_gather_rows', 'abnq_softdtw_backward', 'abns_edit_hist_max_len'] and lag.entry_delays == 3
    assert lag.alloc_delays == 6 and int(lag.poisoned) == 2 and lag.poisoned.nbytes == 60 + 8
    assert restored(lib, before)
    del log[:]
    assert not torch.isnan(torch.zeros(2)).any() and lib.abn_abi_version() == ('abn_abi_version', ()) and log == ['abn_abi_version']


def test_everything_comes_back_after_an_exception():
    log = []
    lib = Lib(log)
    before = snapshot(lib)
    with pytest.raises(ZeroDivisionError):
        with lagging(lib, counter(log)):
            assert not restored(lib, before)
            1 / 0
    assert restored(lib, before)

    def failing():
        raise KeyError('the delay itself fails')
    with pytest.raises(KeyError):
        with lagging(lib, failing):
            torch.empty(3)
    assert restored(lib, before)


def test_nested_with_dirty_and_with_itself():
    log = []
    lib = Lib(log)
    before = snapshot(lib)
    with dirty(0x00) as outer:                                          # lagging inside dirty: its own 0xFF window wins while it is open
        with lagging(lib, counter(log)) as lag:
            assert torch.isnan(torch.empty(4)).all()
        assert not torch.empty(4).any() and log == ['delay']
    assert int(outer) == 2 and int(lag.poisoned) == 1 and restored(lib, before)
    del log[:]
    with lagging(lib, counter(log)) as a:                               # dirty inside lagging: the inner pattern wins, the delay stays
        with dirty(0xC2) as inner:
            t = torch.empty(6)
        assert (t.numpy().view(np.uint32) == 0xC2C2C2C2).all() and log == ['delay'] and int(inner) == 1
        with lagging(lib, counter(log)) as b:                           # two windows: two delays in front of everything
            lib.abn_last_error()
            assert torch.isnan(torch.empty(2)).all()
        assert b.calls == ['abn_last_error'] and b.entry_delays == 1 and b.alloc_delays == 1
        assert log == ['delay', 'delay', 'delay', 'abn_last_error', 'delay', 'delay']
        lib.abn_last_error()
    assert a.calls == ['abn_last_error', 'abn_last_error'] and a.entry_delays == 2 and a.alloc_delays == 2 and int(a.poisoned) == 2
    assert restored(lib, before)


def test_the_delay_rule():
    """The delay is a condition, not a measurement of the code under test: at least 20 empty-launch latencies, never below 0.5 ms."""
    assert side_stream.MIN_DELAY_MS == 0.5 and side_stream.MIN_LATENCIES == 20


def test_every_entry_of_every_ledger_is_accounted_for():
    import test_gpu_side_stream as G
    import test_gpu_dirty_memory as D
    claimed = {}
    for case in G.CASES:
        for e in case.entries:
            claimed.setdefault(e, []).append(case.name)
    symbols = set(side_stream.all_symbols())
    assert not set(claimed) - symbols, 'a case claims an entry no ledger declares: %s' % sorted(set(claimed) - symbols)
    assert not (QUERIES | set(EXCLUDED)) - symbols, sorted((QUERIES | set(EXCLUDED)) - symbols)
    cases = set(claimed) - QUERIES                     # (a case may also prove that it asked a query: the query stays a query)
    assert not cases & set(EXCLUDED), sorted(cases & set(EXCLUDED))
    assert not QUERIES & set(EXCLUDED)
    missing = symbols - cases - QUERIES - set(EXCLUDED)
    assert not missing, 'no side-stream case (tests/test_gpu_side_stream.py), query or exclusion for: %s' % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 20 for r in EXCLUDED.values())
    assert len(EXCLUDED) == 2                          # the multi-process mailboxes: the list does not grow silently
    # the whole dirty-memory ledger is swept, imported and not copied; the sections and the single-Linear entries are new
    assert all(c in G.CASES for c in D.CASES) and len(G.CASES) == len(D.CASES) + len(G.SECTION_CASES) and not G.CAPTURING
    new = {e for c in G.SECTION_CASES for e in c.entries}
    assert {e for e in new if e.startswith('abn_')} == {'abn_linear_forward', 'abn_linear_dgrad', 'abn_linear_wgrad', 'abn_linear_backward',
                                                         'abn_linear_backward_prec'}
    assert new - QUERIES == symbols - {e for c in D.CASES for e in c.entries} - QUERIES - set(EXCLUDED)
    # a section getter is named like one
    assert all(n.endswith(('_ws_bytes', '_max', '_max_k', '_max_d', '_max_len', '_max_duration', '_path')) for n in SECTION_QUERIES)
