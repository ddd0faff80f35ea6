"""tests/test_gpu_arg_contract.py's argument contract for the entries of abnet3_amd._lib.EVAL_SYMBOLS (prefix abns_, the
pair-free histogram behind the full term scores): the same Row / A table, the same guard, the same mutants and the same three
tests, for tde.cluster_histogram and TermEvaluator.evaluate_full.  The section is no NEXT<n>_SYMBOLS because the main ledger
(tests/test_arg_contract_host.py) demands a row in tests/test_gpu_arg_contract.py for every entry of those; until a change
that may edit those files folds it in, this file is its ledger: every key of EVAL_SYMBOLS is a query or claimed by a row here.

The guard wraps what arg_contract.all_symbols() lists, so the tests put EVAL_SYMBOLS into it for their duration and pass
the section's two pure host queries through `allow=`.

Needs an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arg_contract as AC  # noqa: E402
import tde_full_np as full_np  # noqa: E402
import test_gpu_arg_contract as G  # noqa: E402
from test_dirty_memory_host import QUERIES  # noqa: E402
from test_gpu_dirty_memory import dev  # noqa: E402

pytestmark = pytest.mark.gpu

A, Row = G.A, G.Row
EVAL_QUERIES = {'abns_edit_hist_max_len', 'abns_edit_cluster_hist_ws_bytes'}


@pytest.fixture(autouse=True)
def eval_symbols_under_the_guard(monkeypatch):
    """arg_contract.guarded wraps all_symbols() and lets `allow` through unchecked: both get the new section."""
    from abnet3_amd import _lib
    plain, guarded = AC.all_symbols, AC.guarded

    def all_symbols():
        out = plain()
        out.update(_lib.EVAL_SYMBOLS)
        return out

    def guarded_with_queries(lib, forbidden=(), block_all=False, allow=QUERIES):
        return guarded(lib, forbidden=forbidden, block_all=block_all, allow=set(allow) | EVAL_QUERIES)
    monkeypatch.setattr(AC, 'all_symbols', all_symbols)
    monkeypatch.setattr(AC, 'guarded', guarded_with_queries)


def histogram_row():
    def build():
        t = full_np.token_table(G.rng_of('cluster-histogram'), [3, 1, 5, 0, 2], [0, 1, 2, 5, 9], 4)
        return dict(table=dev(np.concatenate([t['table'], np.zeros(4, np.int32)])), tok_off=t['tok_off'], tok_n=t['tok_n'], tok_file=t['tok_file'],
                    tok_on=t['tok_on'], tok_end=t['tok_end'], cl_first=t['cl_first'], groups=dev(t['groups']))

    def run(a):
        from abnet3_amd import tde
        hist, n_pairs, n_skipped = tde.cluster_histogram(a['table'], a['tok_off'], a['tok_n'], a['tok_file'], a['tok_on'], a['tok_end'],
                                                         a['cl_first'], a['groups'])
        return dict(hist=hist, counts=np.array([n_pairs, n_skipped]))

    return Row('cluster-histogram', ('abns_edit_cluster_hist', 'abns_edit_cluster_hist_ws_bytes', 'abns_edit_hist_max_len'), build, run,
               dict(table=A('int32', 1), tok_off=A('int64', 1, 'host'), tok_n=A('int32', 1, 'host'), tok_file=A('int32', 1, 'host'),
                    tok_on=A('float64', 1, 'host'), tok_end=A('float64', 1, 'host'), cl_first=A('int64', 1, 'host'), groups=A('int32', 1)),
               lengths=[('tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end', 'groups'), ('cl_first',)])


def device_columns_row():
    """The same call with every token column on the device, as a caller that already holds them there makes it."""
    def build():
        t = full_np.token_table(G.rng_of('cluster-histogram-device'), [4, 2, 6], [0, 1, 3, 8], 3)
        out = {k: dev(t[k]) for k in ('table', 'tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end')}
        out['cl_first'] = t['cl_first']
        return out

    def run(a):
        from abnet3_amd import tde
        hist, n_pairs, n_skipped = tde.cluster_histogram(a['table'], a['tok_off'], a['tok_n'], a['tok_file'], a['tok_on'], a['tok_end'], a['cl_first'])
        return dict(hist=hist, counts=np.array([n_pairs, n_skipped]))

    return Row('cluster-histogram-device', ('abns_edit_cluster_hist',), build, run,
               dict(table=A('int32', 1), tok_off=A('int64', 1), tok_n=A('int32', 1), tok_file=A('int32', 1), tok_on=A('float64', 1),
                    tok_end=A('float64', 1), cl_first=A('int64', 1, 'host')),
               lengths=[('tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end'), ('cl_first',)])


SURFACE = [histogram_row(), device_columns_row()]


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_canonical_call(row):
    assert not set(row.entries) - set(AC.all_symbols())
    out, log = G.canonical(row)
    missing = set(row.entries) - set(log.calls)
    assert not missing, 'the row claims entries it did not reach: %s (called: %s)' % (sorted(missing), sorted(set(log.calls)))
    assert not log.blocked and out and log.launched == ['abns_edit_cluster_hist']
    again, _ = G.run_guarded(row, dict(row.inputs()))
    G.assert_same_bits(out, again, '%s: two valid calls' % row.name)
    t = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in row.inputs().items()}
    hist, n_pairs, n_skipped = full_np.table_histogram(t, use_groups='groups' in t)
    assert np.array_equal(out['hist'], hist) and out['counts'].tolist() == [n_pairs, n_skipped]


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_value_preserving_mutations(row):
    G.every_mutant(row, G.value_mutations(row), G.check_value_mutant)


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_shape_mutations_are_refused(row):
    G.every_mutant(row, G.shape_mutations(row), G.check_shape_mutant)


def test_every_entry_of_the_section_is_a_query_or_claimed_by_a_row():
    from abnet3_amd import _lib
    claimed = {e for row in SURFACE for e in row.entries}
    assert claimed <= set(_lib.EVAL_SYMBOLS)
    assert not set(_lib.EVAL_SYMBOLS) - EVAL_QUERIES - claimed, sorted(set(_lib.EVAL_SYMBOLS) - EVAL_QUERIES - claimed)
    assert EVAL_QUERIES <= set(_lib.EVAL_SYMBOLS) and not EVAL_QUERIES & (set(QUERIES) | AC.NEXT_QUERIES)
    assert set(_lib.EVAL_SYMBOLS) <= set(AC.all_symbols())                    # the fixture put them under the guard
    for row in SURFACE:
        names = set(row.args)
        assert all(set(group) <= names for group in row.widths + row.lengths) and G.value_mutations(row) and G.shape_mutations(row)


def test_the_queries_pass_and_the_entry_is_stopped_under_block_all():
    from abnet3_amd import _lib
    lib = _lib.load()
    with AC.guarded(lib, block_all=True) as log:
        assert lib.abns_edit_hist_max_len() == 256 and lib.abns_edit_cluster_hist_ws_bytes(5, 3, 4) > 0
        with pytest.raises(AC.ReachedLibrary):
            lib.abns_edit_cluster_hist(None)
    assert log.calls == ['abns_edit_hist_max_len', 'abns_edit_cluster_hist_ws_bytes'] and log.blocked == ['abns_edit_cluster_hist'] and not log.launched
