"""tests/test_gpu_arg_contract.py's argument contract for the entries of abnet3_amd._lib.CAE_SYMBOLS (prefix abnr_, the
reconstruction loss of the correspondence autoencoder): the same Row / A table, the same guard, the same mutants and the same
three tests, for CorrespondenceLoss on its own and behind a CorrespondenceAutoencoder.  The section is no NEXT<n>_SYMBOLS
because the main ledger (tests/test_arg_contract_host.py) demands a row in tests/test_gpu_arg_contract.py for every entry of
those; until a change that may edit those files folds it in, this file is its ledger: every key of CAE_SYMBOLS is a query or
claimed by a row here.

The guard wraps what arg_contract.all_symbols() lists, so the tests put CAE_SYMBOLS into it for their duration and pass the
section's two pure host queries through `allow=`.

Needs an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arg_contract as AC  # noqa: E402
import cae_np  # noqa: E402
import test_gpu_arg_contract as G  # noqa: E402
from test_dirty_memory_host import QUERIES  # noqa: E402
from test_gpu_dirty_memory import dev, host  # noqa: E402

pytestmark = pytest.mark.gpu

A, Row = G.A, G.Row
CAE_QUERIES = {'abnr_recon_max_d', 'abnr_recon_ws_bytes'}
EPS = 2.0 ** -24


@pytest.fixture(autouse=True)
def cae_symbols_under_the_guard(monkeypatch):
    """arg_contract.guarded wraps all_symbols() and lets `allow` through unchecked: both get the new section."""
    from abnet3_amd import _lib
    plain, guarded = AC.all_symbols, AC.guarded

    def all_symbols():
        out = plain()
        out.update(_lib.CAE_SYMBOLS)
        return out

    def guarded_with_queries(lib, forbidden=(), block_all=False, allow=QUERIES):
        return guarded(lib, forbidden=forbidden, block_all=block_all, allow=set(allow) | CAE_QUERIES)
    monkeypatch.setattr(AC, 'all_symbols', all_symbols)
    monkeypatch.setattr(AC, 'guarded', guarded_with_queries)


def recon_loss_row():
    B, D = 9, 8

    def build():
        r1, r2, x1, x2, y = cae_np.draw(G.rng_of('recon-loss'), B, D, labels=(1, -1))
        y[:2] = (1, -1)
        return dict(r1=dev(r1), r2=dev(r2), x1=dev(x1), x2=dev(x2), y=dev(y))

    def run(a):
        import abnet3_amd.loss as L
        lv, dr = L.CorrespondenceLoss(avg=True, symmetric=True).value_and_grad(a['r1'], a['r2'], a['x1'], a['x2'], a['y'])
        la, da = L.CorrespondenceLoss(avg=False, symmetric=False, mode='autoencoder').value_and_grad(a['r1'], a['r2'], a['x1'], a['x2'], a['y'])
        return dict(loss=host(lv), dr=host(dr), loss_ae=host(la), dr_ae=host(da))

    return Row('recon-loss', ('abnr_recon_loss', 'abnr_recon_ws_bytes', 'abnr_recon_max_d'), build, run,
               dict(r1=A('float32', 2), r2=A('float32', 2), x1=A('float32', 2), x2=A('float32', 2), y=A('int64', 1, takes=G.LABEL_DTYPES)),
               widths=[('r1', 'r2', 'x1', 'x2')], lengths=[('r1', 'r2', 'x1', 'x2', 'y')])


def cae_network_row():
    """The loss behind the network, as TrainerCorrespondence.give_batch_to_network calls it: the inputs reach the towers
    AND the loss."""
    kw = dict(input_dim=8, num_hidden_layers=1, hidden_dim=16, output_dim=4, activation_layer='sigmoid', batch_norm=False, p_dropout=0.0)
    B = 9

    def build():
        rng = G.rng_of('cae-network')
        y = rng.choice([1, -1], B).astype(np.int64)
        y[:2] = (1, -1)
        return dict(x1=dev(G.f32(rng.standard_normal((B, 8)))), x2=dev(G.f32(rng.standard_normal((B, 8)))), y=dev(y))

    def run(a):
        import torch
        import abnet3_amd.loss as L
        from abnet3_amd.model import CorrespondenceAutoencoder
        torch.manual_seed(5)
        net = CorrespondenceAutoencoder(**kw).cuda()
        net.train()
        r1, r2 = net(a['x1'], a['x2'])
        lv = L.CorrespondenceLoss()(r1, r2, a['x1'], a['x2'], a['y'])
        lv.backward()
        out = dict(r1=host(r1), r2=host(r2), loss=host(lv))
        out.update({'g.' + k: host(q.grad) for k, q in net.named_parameters()})
        net.eval()
        with torch.no_grad():
            out['code'] = host(net.forward_once(a['x1']))
            out['rec'] = host(net.reconstruct(a['x1']))
        return out

    return Row('cae-network', ('abn_tower_forward', 'abn_tower_backward', 'abnr_recon_loss'), build, run,
               dict(x1=A('float32', 2), x2=A('float32', 2), y=A('int64', 1, takes=G.LABEL_DTYPES)),
               widths=[('x1', 'x2')], lengths=[('x1', 'x2')], late=('y',))


SURFACE = [recon_loss_row(), cae_network_row()]


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_canonical_call(row):
    assert not set(row.entries) - set(AC.all_symbols())
    out, log = G.canonical(row)
    missing = set(row.entries) - set(log.calls)
    assert not missing, 'the row claims entries it did not reach: %s (called: %s)' % (sorted(missing), sorted(set(log.calls)))
    assert not log.blocked and out and 'abnr_recon_loss' in log.launched
    again, _ = G.run_guarded(row, dict(row.inputs()))
    G.assert_same_bits(out, again, '%s: two valid calls' % row.name)
    if row.name == 'recon-loss':
        t = {k: v.cpu().numpy() for k, v in row.inputs().items()}
        for tag, v in (('', ('correspondence', True, True)), ('_ae', ('autoencoder', False, False))):
            lv, _, g1, g2 = cae_np.recon_loss(t['r1'], t['r2'], t['x1'], t['x2'], t['y'], *v)
            assert abs(float(out['loss' + tag]) - lv) <= 4 * EPS * abs(lv)
            assert (np.abs(out['dr' + tag].astype(np.float64) - np.stack([g1, g2])) <= 3 * EPS * np.abs(np.stack([g1, g2]))).all()


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_value_preserving_mutations(row):
    G.every_mutant(row, G.value_mutations(row), G.check_value_mutant)


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_shape_mutations_are_refused(row):
    G.every_mutant(row, G.shape_mutations(row), G.check_shape_mutant)


def test_every_entry_of_the_section_is_a_query_or_claimed_by_a_row():
    from abnet3_amd import _lib
    claimed = {e for row in SURFACE for e in row.entries} & set(_lib.CAE_SYMBOLS)
    assert not set(_lib.CAE_SYMBOLS) - CAE_QUERIES - claimed, sorted(set(_lib.CAE_SYMBOLS) - CAE_QUERIES - claimed)
    assert CAE_QUERIES <= set(_lib.CAE_SYMBOLS) and not CAE_QUERIES & (set(QUERIES) | AC.NEXT_QUERIES)
    assert set(_lib.CAE_SYMBOLS) <= set(AC.all_symbols())                     # the fixture put them under the guard
    for row in SURFACE:
        names = set(row.args)
        assert all(set(group) <= names for group in row.widths + row.lengths) and G.value_mutations(row) and G.shape_mutations(row)


def test_the_queries_pass_and_the_entry_is_stopped_under_block_all():
    from abnet3_amd import _lib
    lib = _lib.load()
    with AC.guarded(lib, block_all=True) as log:
        assert lib.abnr_recon_max_d() >= 2048 and lib.abnr_recon_ws_bytes(5, 3) == 16 + 8 * 5
        with pytest.raises(AC.ReachedLibrary):
            lib.abnr_recon_loss(None)
    assert log.calls == ['abnr_recon_max_d', 'abnr_recon_ws_bytes'] and log.blocked == ['abnr_recon_loss'] and not log.launched
