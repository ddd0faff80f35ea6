"""tests/test_gpu_arg_contract.py's argument contract for the entries of abnet3_amd._lib.SDTW_SYMBOLS (prefix abnq_, batched
soft-DTW and its gradient): the same Row / A table, the same guard, the same mutants and the same three tests, for the raw
calls of abnet3_amd/softdtw.py and for SoftDTWLoss behind a network as TrainerSequencePairs calls it.  The section is no
NEXT<n>_SYMBOLS because the main ledger (tests/test_arg_contract_host.py) demands a row in tests/test_gpu_arg_contract.py for
every entry of those; until a change that may edit those files folds it in, this file is its ledger: every key of SDTW_SYMBOLS
is a query or claimed by a row here.

The guard wraps what arg_contract.all_symbols() lists, so the tests put SDTW_SYMBOLS into it for their duration and pass the
section's three pure host queries through `allow=`.

Needs an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arg_contract as AC  # noqa: E402
import sdtw_np as S  # noqa: E402
import test_gpu_arg_contract as G  # noqa: E402
from test_dirty_memory_host import QUERIES  # noqa: E402
from test_gpu_dirty_memory import dev, host  # noqa: E402

pytestmark = pytest.mark.gpu

A, Row = G.A, G.Row
SDTW_QUERIES = {'abnq_softdtw_max_len', 'abnq_softdtw_max_d', 'abnq_softdtw_ws_bytes'}
EPS = 2.0 ** -24
N1, N2 = np.array([5, 9, 1, 12], dtype=np.int32), np.array([6, 4, 7, 3], dtype=np.int32)
OFF1 = (np.cumsum(N1) - N1).astype(np.int64)
OFF2 = (N1.sum() + np.cumsum(N2) - N2).astype(np.int64)               # the table's last row belongs to the last pair
ROWS = int(N1.sum() + N2.sum())
COLS = dict(o1=A('int64', 1, 'host'), n1=A('int32', 1, 'host'), o2=A('int64', 1, 'host'), n2=A('int32', 1, 'host'))


@pytest.fixture(autouse=True)
def sdtw_symbols_under_the_guard(monkeypatch):
    """arg_contract.guarded wraps all_symbols() and lets `allow` through unchecked: both get the new section."""
    from abnet3_amd import _lib
    plain, guarded = AC.all_symbols, AC.guarded

    def all_symbols():
        out = plain()
        out.update(_lib.SDTW_SYMBOLS)
        return out

    def guarded_with_queries(lib, forbidden=(), block_all=False, allow=QUERIES):
        return guarded(lib, forbidden=forbidden, block_all=block_all, allow=set(allow) | SDTW_QUERIES)
    monkeypatch.setattr(AC, 'all_symbols', all_symbols)
    monkeypatch.setattr(AC, 'guarded', guarded_with_queries)


def table(name, D):
    rng = G.rng_of(name)
    rows = []
    for a, b in zip(N1, N2):
        rows.append(S.draw(rng, int(a), int(b), D))
    return np.concatenate([x for x, _ in rows] + [y for _, y in rows]).astype(np.float32)


def raw_row():
    """soft_dtw_batch and soft_dtw_backward.  The weights reach the second entry only (late): a view or a wider dtype of them
    is converted.  w is in no lengths group and has no shape mutant here: a short w is refused by soft_dtw_backward, which can
    only happen after the forward has launched -- what Row's `late` rule permits and the shape test (nothing launched before
    a refusal) cannot hold it to; test_w_of_another_shape_is_refused_by_the_backward holds it to the refusal itself."""
    def build():
        return dict(e=dev(table('sdtw-raw', 8)), o1=OFF1.copy(), n1=N1.copy(), o2=OFF2.copy(), n2=N2.copy(),
                    w=dev(G.f32([1.0, -0.5, 0.0, 2.0])))

    def run(a):
        from abnet3_amd import softdtw
        value, handle = softdtw.soft_dtw_batch(a['e'], a['o1'], a['n1'], a['o2'], a['n2'], 0.1, keep=True)
        g1, g2 = softdtw.soft_dtw_backward(handle, a['w'])
        v0, _ = softdtw.soft_dtw_batch(a['e'], a['o1'], a['n1'], a['o2'], a['n2'], 0.1, keep=False)
        return dict(value=host(value), g1=host(g1), g2=host(g2), value0=host(v0))

    return Row('sdtw-raw', ('abnq_softdtw_forward', 'abnq_softdtw_backward', 'abnq_softdtw_ws_bytes', 'abnq_softdtw_max_len',
                            'abnq_softdtw_max_d'), build, run, dict(COLS, e=A('float32', 2), w=A('float32', 1)),
               lengths=[('o1', 'n1', 'o2', 'n2'), ('e',)], late=('w',))


def loss_network_row():
    """The loss behind the network, as TrainerSequencePairs.give_batch_to_network calls it: the batch is checked, the rows go
    through ONE tower call, the embeddings and the row ranges reach the loss.  check_batch looks at the labels before the tower
    launches, so y is not `late`: a y on the host is refused before any launch too."""
    kw = dict(input_dim=8, num_hidden_layers=1, hidden_dim=16, output_dim=4, activation_layer='sigmoid', batch_norm=False, p_dropout=0.0)

    def build():
        return dict(X=dev(table('sdtw-network', 8)), o1=OFF1.copy(), n1=N1.copy(), o2=OFF2.copy(), n2=N2.copy(),
                    y=dev(np.array([1, -1, 1, -1], dtype=np.int64)))

    def run(a):
        import torch
        import abnet3_amd.loss as L
        from abnet3_amd.model import SiameseNetwork
        torch.manual_seed(5)
        net = SiameseNetwork(**kw).cuda()
        net.train()
        out = {}
        for tag, f in (('', L.SoftDTWLoss(margin=0.25)), ('_div', L.SoftDTWLoss(divergence=True, normalize=False, avg=False, margin=3.0))):
            cols = f.check_batch(a['X'].shape[0], a['o1'], a['n1'], a['o2'], a['n2'], a['y'])
            emb = net.forward_once(a['X'])
            lv = f(emb, *cols, a['y'], checked=True)
            net.zero_grad()
            lv.backward()
            out['loss' + tag] = host(lv)
            out['emb'] = host(emb)
            out.update({'g%s.%s' % (tag, k): host(q.grad) for k, q in net.named_parameters()})
            with torch.no_grad():
                out['value_and_grad' + tag] = host(f.value_and_grad(emb.detach(), *cols, a['y'])[1])
        return out

    return Row('sdtw-network', ('abn_tower_forward', 'abn_tower_backward', 'abnq_softdtw_forward', 'abnq_softdtw_backward'), build, run,
               dict(COLS, X=A('float32', 2), y=A('int64', 1, takes=G.LABEL_DTYPES)),
               widths=[('X',)], lengths=[('o1', 'n1', 'o2', 'n2', 'y'), ('X',)])


SURFACE = [raw_row(), loss_network_row()]


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_canonical_call(row):
    assert not set(row.entries) - set(AC.all_symbols())
    out, log = G.canonical(row)
    missing = set(row.entries) - set(log.calls)
    assert not missing, 'the row claims entries it did not reach: %s (called: %s)' % (sorted(missing), sorted(set(log.calls)))
    assert not log.blocked and out and 'abnq_softdtw_forward' in log.launched and 'abnq_softdtw_backward' in log.launched
    again, _ = G.run_guarded(row, dict(row.inputs()))
    G.assert_same_bits(out, again, '%s: two valid calls' % row.name)
    if row.name == 'sdtw-raw':
        t = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in row.inputs().items()}
        s1, s2 = np.cumsum(N1) - N1, np.cumsum(N2) - N2
        assert np.array_equal(out['value'], out['value0'])
        for p in range(len(N1)):
            x, y = t['e'][OFF1[p]:OFF1[p] + N1[p]], t['e'][OFF2[p]:OFF2[p] + N2[p]]
            ref, yard = S.problem(x, y, 0.1, float(t['w'][p])), S.problem(x, y, 0.1, float(t['w'][p]), cell_dtype=np.float32)
            assert abs(float(out['value'][p]) - ref['value']) <= (N1[p] + N2[p] - 1) * 24 * EPS + 2 * EPS * abs(ref['value'])
            for got, key, s, n in ((out['g1'], 'g1', s1, N1), (out['g2'], 'g2', s2, N2)):
                bar = 16 * np.abs(yard[key] - ref[key]).max() + 4 * EPS * np.abs(ref[key]).max()
                assert np.abs(got[s[p]:s[p] + n[p]] - ref[key]).max() <= bar, (p, key)


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_value_preserving_mutations(row):
    G.every_mutant(row, G.value_mutations(row), G.check_value_mutant)


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_shape_mutations_are_refused(row):
    G.every_mutant(row, G.shape_mutations(row), G.check_shape_mutant)


def test_w_of_another_shape_is_refused_by_the_backward():
    import torch
    from abnet3_amd import _lib, softdtw
    a = SURFACE[0].inputs()
    value, handle = softdtw.soft_dtw_batch(a['e'], a['o1'], a['n1'], a['o2'], a['n2'], 0.1, keep=True)
    lib = _lib.load()
    with AC.guarded(lib, block_all=True) as log:
        for bad in (a['w'][:-1].clone(), a['w'][None], a['w'].long()):
            with pytest.raises(ValueError):
                softdtw.soft_dtw_backward(handle, bad)
        with pytest.raises(_lib.HipLibraryError):
            softdtw.soft_dtw_backward(handle, a['w'].cpu())
    assert not log.blocked and not log.launched
    torch.cuda.synchronize()


def test_every_entry_of_the_section_is_a_query_or_claimed_by_a_row():
    from abnet3_amd import _lib
    claimed = {e for row in SURFACE for e in row.entries} & set(_lib.SDTW_SYMBOLS)
    assert not set(_lib.SDTW_SYMBOLS) - SDTW_QUERIES - claimed, sorted(set(_lib.SDTW_SYMBOLS) - SDTW_QUERIES - claimed)
    assert SDTW_QUERIES <= set(_lib.SDTW_SYMBOLS) and not SDTW_QUERIES & (set(QUERIES) | AC.NEXT_QUERIES)
    assert set(_lib.SDTW_SYMBOLS) <= set(AC.all_symbols())                    # the fixture put them under the guard
    for row in SURFACE:
        names = set(row.args)
        assert all(set(group) <= names for group in row.widths + row.lengths) and G.value_mutations(row) and G.shape_mutations(row)


def test_the_queries_pass_and_the_entries_are_stopped_under_block_all():
    import ctypes
    from abnet3_amd import _lib
    lib = _lib.load()
    n = np.array([3], dtype=np.int32)
    with AC.guarded(lib, block_all=True) as log:
        assert lib.abnq_softdtw_max_len() >= 256 and lib.abnq_softdtw_max_d() >= 1024
        assert lib.abnq_softdtw_ws_bytes(n.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(ctypes.c_void_p), 1, 4, 0) > 0
        for name in ('abnq_softdtw_forward', 'abnq_softdtw_backward'):
            with pytest.raises(AC.ReachedLibrary):
                getattr(lib, name)(None)
    assert log.calls == ['abnq_softdtw_max_len', 'abnq_softdtw_max_d', 'abnq_softdtw_ws_bytes']
    assert log.blocked == ['abnq_softdtw_forward', 'abnq_softdtw_backward'] and not log.launched
