"""The host side of the correspondence autoencoder without a GPU: the float64 restatement of CorrespondenceLoss
(tests/cae_np.py) against brute force and against torch's mse_loss + autograd, the abnr_ ledger of
include/abnet3_hip_next.h, the network's state-dict keys and constructor assertions, the class lookup a gridsearch
experiment does, and the refusals of abnr_recon_loss that need no launch.  No kernel runs here."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cae_np  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abnr_recon_max_d', 'abnr_recon_ws_bytes', 'abnr_recon_loss'}
VARIANTS = list(itertools.product(cae_np.MODES, (True, False), (True, False)))          # mode, symmetric, avg
KW = dict(input_dim=40, num_hidden_layers=2, hidden_dim=24, output_dim=8, activation_layer='sigmoid', batch_norm=True, p_dropout=0.0)


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,symmetric,avg', VARIANTS)
def test_restatement_against_brute_force(mode, symmetric, avg):
    rng = np.random.default_rng(3)
    for B, D in ((1, 1), (3, 2), (5, 4)):
        r1, r2, x1, x2, y = cae_np.draw(rng, B, D)
        y[0] = 1
        lv, terms, dr1, dr2 = cae_np.recon_loss(r1, r2, x1, x2, y, mode, symmetric, avg)
        want = cae_np.brute_loss(r1, r2, x1, x2, y, mode, symmetric, avg)
        assert abs(lv - want) <= 1e-14 * max(abs(want), 1.0)
        counted = cae_np.counted_rows(y, mode, B)
        assert np.all(terms[~counted] == 0) and np.all(dr1[~counted] == 0) and np.all(dr2[~counted] == 0)
        assert abs(cae_np.scale_of(int(counted.sum()), D, symmetric, avg) * terms.sum() - lv) <= 1e-14 * max(abs(lv), 1.0)
        if not symmetric:
            assert np.all(dr2 == 0)
        # the gradient by central differences of the brute-force loss (a quadratic: exact up to rounding)
        h = 1e-4
        for tab, grad in ((r1, dr1), (r2, dr2)):
            i, d = B - 1, D - 1
            up, dn = tab.astype(np.float64).copy(), tab.astype(np.float64).copy()
            up[i, d] += h
            dn[i, d] -= h
            args = lambda t: (t, r2, x1, x2) if tab is r1 else (r1, t, x1, x2)
            fd = (cae_np.brute_loss(*args(up), y, mode, symmetric, avg) - cae_np.brute_loss(*args(dn), y, mode, symmetric, avg)) / (2 * h)
            assert abs(fd - grad[i, d]) <= 1e-8 * max(1.0, abs(fd))


@pytest.mark.parametrize('mode,symmetric,avg', VARIANTS)
def test_restatement_against_torch_mse_and_autograd(mode, symmetric, avg):
    import torch
    rng = np.random.default_rng(5)
    r1, r2, x1, x2, y = cae_np.draw(rng, 11, 7)
    lv, terms, dr1, dr2 = cae_np.recon_loss(r1, r2, x1, x2, y, mode, symmetric, avg)
    t = [torch.from_numpy(a.astype(np.float64)) for a in (r1, r2, x1, x2)]
    t[0].requires_grad_(True)
    t[1].requires_grad_(True)
    out = cae_np.torch_loss(t[0], t[1], t[2], t[3], torch.from_numpy(y), mode, symmetric, avg)
    out.backward()
    assert abs(float(out.detach()) - lv) <= 1e-13 * max(abs(lv), 1.0)
    g2 = t[1].grad.numpy() if t[1].grad is not None else np.zeros_like(dr2)          # (not symmetric: r2 is not in the graph)
    assert (t[1].grad is None) == (not symmetric)
    assert np.abs(t[0].grad.numpy() - dr1).max() <= 1e-13 and np.abs(g2 - dr2).max() <= 1e-13


def test_no_same_row_and_labels_of_every_dtype():
    rng = np.random.default_rng(7)
    r1, r2, x1, x2, _ = cae_np.draw(rng, 6, 5)
    for avg in (True, False):
        lv, terms, dr1, dr2 = cae_np.recon_loss(r1, r2, x1, x2, -np.ones(6), 'correspondence', True, avg)
        assert lv == 0.0 and not terms.any() and not dr1.any() and not dr2.any()
        lv, _, dr1, _ = cae_np.recon_loss(r1, r2, x1, x2, -np.ones(6), 'autoencoder', True, avg)
        assert lv > 0 and dr1.all()                                                   # the labels are ignored there
    base = np.array([1, -1, 0, 2, 1, -1])
    want = cae_np.recon_loss(r1, r2, x1, x2, base, 'correspondence', True, True)
    for dt in (np.int8, np.int32, np.int64, np.float32, np.float64):
        got = cae_np.recon_loss(r1, r2, x1, x2, base.astype(dt), 'correspondence', True, True)
        assert got[0] == want[0] and np.array_equal(got[2], want[2])
    frac = cae_np.counted_rows(np.array([1.0, 1.5, 0.999, 1.0 + 1e-7, -1.0]), 'correspondence', 5)
    assert frac.tolist() == [True, False, False, False, False]


# ---- the ledger ---------------------------------------------------------------------------------------------------------
def declared(prefix='abnr_'):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, text))


def test_cae_symbols_are_the_headers_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib, build
    assert declared() == set(_lib.CAE_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS) | set(_lib.EVAL_SYMBOLS)
    for k in vars(_lib):
        if k.startswith('NEXT') and k.endswith('_SYMBOLS'):
            others |= set(getattr(_lib, k))
    assert not NAMES & others and not [k for k in vars(_lib) if k.startswith('NEXT8')]
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abnr_')}
    assert exported == NAMES
    for name, (res, args) in _lib.CAE_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert len(_lib.CAE_SYMBOLS['abnr_recon_loss'][1]) == 17
    assert lib.abn_abi_version() == 20 and _lib.ABI_VERSION == 20
    head = open(HEADER).read()
    top = head[:head.index('#ifndef')]
    assert 'abnr_' in top and 'CAE_SYMBOLS' in top
    assert 'recon.hip' in build.SOURCES and 'recon.hip' not in build.STRICT_FP


def test_queries_and_refusals_before_any_launch(lib):
    from abnet3_amd import _lib
    assert lib.abnr_recon_max_d() >= 2048
    ws = lib.abnr_recon_ws_bytes
    assert ws(4096, 280) == 16 + 8 * 4096 and ws(1, 1) == 24 and ws(7, lib.abnr_recon_max_d()) > 0
    for B, D in ((0, 4), (4, 0), (-1, 4)):
        assert ws(B, D) == -1 and b'abnr_recon_ws_bytes' in lib.abn_last_error()
    assert ws(4, lib.abnr_recon_max_d() + 1) == -1 and ws((1 << 22) + 1, 4) == -1
    p = 256                                                                          # a non-null, aligned address that is never read
    ok = dict(r1=p, r2=p, x1=p, x2=p, y=p, y_dtype=2, B=5, D=4, mode=0, symmetric=1, avg=1, loss=p, terms=0, dr1=p, dr2=p, ws=p, stream=0)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.abnr_recon_loss(*[a[k] for k in ok])
    for kw in (dict(B=0), dict(D=0), dict(B=-3)):
        assert call(**kw) == _lib.E_ARG and b'out of range' in lib.abn_last_error(), kw
    assert call(D=lib.abnr_recon_max_d() + 1) == _lib.E_UNSUPPORTED and b'abnr_recon_max_d' in lib.abn_last_error()
    assert call(B=(1 << 22) + 1) == _lib.E_UNSUPPORTED
    for name in ('r1', 'r2', 'x1', 'x2', 'y', 'loss', 'ws'):
        assert call(**{name: 0}) == _lib.E_ARG and b'null' in lib.abn_last_error(), name
    for y_dtype in (-1, 5):
        assert call(y_dtype=y_dtype) == _lib.E_ARG and b'y_dtype' in lib.abn_last_error()
    for mode in (-1, 2):
        assert call(mode=mode) == _lib.E_ARG and b'mode' in lib.abn_last_error()
    assert call(dr1=0) == _lib.E_ARG and call(dr2=0) == _lib.E_ARG and b'go together' in lib.abn_last_error()
    assert call(ws=p + 8) == _lib.E_ARG and b'aligned' in lib.abn_last_error()


# ---- the classes --------------------------------------------------------------------------------------------------------
def test_encoder_keys_are_the_siamese_networks():
    from abnet3_amd.model import CorrespondenceAutoencoder, SiameseNetwork
    for kw in (KW, dict(KW, batch_norm=False, num_hidden_layers=0), dict(KW, last_non_linearity=None), dict(KW, num_decoder_layers=1)):
        cae, sia = CorrespondenceAutoencoder(**kw), SiameseNetwork(**{k: v for k, v in kw.items() if k != 'num_decoder_layers'})
        enc = cae.encoder_state_dict()
        assert list(enc) == list(sia.state_dict()) == [k for k in cae.state_dict() if not k.startswith(('decoder_layers.', 'recon_layer.'))]
        assert all(enc[k].shape == v.shape and enc[k].dtype == v.dtype for k, v in sia.state_dict().items())
        sia.load_state_dict(enc)                                                      # strict: the keys as they are
        rest = [k for k in cae.state_dict() if k not in enc]
        assert rest[-2:] == ['recon_layer.weight', 'recon_layer.bias'] and all(k.startswith('decoder_layers.') for k in rest[:-2])
        n_dec = kw.get('num_decoder_layers', kw['num_hidden_layers'] + 1)
        assert cae.num_decoder_layers == n_dec and sum(k.endswith('.weight') and v.dim() == 2 for k, v in cae.decoder_layers.state_dict().items()) == n_dec
        assert tuple(cae.recon_layer.weight.shape) == (kw['input_dim'], kw['hidden_dim'])
        assert tuple(cae.decoder_layers[0].weight.shape) == (kw['hidden_dim'], kw['output_dim'])
        segs = cae._segment_list()
        assert [s.last_act for s in segs][1:] == ['sigmoid', 'none'] and segs[-1].batch_norm is False
        assert [s.first_block for s in segs] == [0, kw['num_hidden_layers'] + 2, kw['num_hidden_layers'] + 2 + n_dec]
        assert sum(len(s.params) for s in segs) == len(list(cae.parameters()))
    who = CorrespondenceAutoencoder(**KW).whoami()
    assert who['class_name'] == 'CorrespondenceAutoencoder' and who['params']['num_decoder_layers'] == 3 and '_flat' not in who['params']


def test_save_encoder_file_loads_into_a_siamese_network(tmp_path):
    import torch
    from abnet3_amd.model import CorrespondenceAutoencoder, SiameseNetwork
    cae = CorrespondenceAutoencoder(output_path=str(tmp_path / 'cae'), **KW)
    cae.save_encoder(str(tmp_path / 'enc.pth'))
    sia = SiameseNetwork(**KW)
    sia.load_network(str(tmp_path / 'enc.pth'))
    assert all(torch.equal(v, cae.state_dict()[k]) for k, v in sia.state_dict().items())
    cae.save_network()
    other = CorrespondenceAutoencoder(**KW)
    other.load_network(str(tmp_path / 'cae.pth'))
    assert all(torch.equal(v, cae.state_dict()[k]) for k, v in other.state_dict().items())


def test_constructor_assertions():
    from abnet3_amd import _lib
    from abnet3_amd.loss import CorrespondenceLoss, LossBuilder
    from abnet3_amd.model import CorrespondenceAutoencoder
    for bad in (dict(activation_layer='softmax'), dict(type_init='he'), dict(input_dim=40.0), dict(hidden_dim=None), dict(output_dim='8'),
                dict(num_hidden_layers=None), dict(num_hidden_layers=_lib.MAX_LAYERS - 1), dict(num_decoder_layers=0),
                dict(num_decoder_layers=_lib.MAX_LAYERS + 1), dict(num_decoder_layers=2.0), dict(last_non_linearity='softmax')):
        with pytest.raises(AssertionError):
            CorrespondenceAutoencoder(**dict(KW, **bad))
    f = CorrespondenceLoss()
    assert isinstance(f, LossBuilder) and (f.avg, f.symmetric, f.mode) == (True, True, 'correspondence')
    who = CorrespondenceLoss(avg=False, symmetric=False, mode='autoencoder').whoami()
    assert who['class_name'] == 'CorrespondenceLoss' and (who['params']['avg'], who['params']['symmetric'], who['params']['mode']) == (False, False, 'autoencoder')
    with pytest.raises(ValueError, match='mode'):
        CorrespondenceLoss(mode='denoising')
    f.mode = 'autoencoder'                                                            # reassigned between passes
    assert f.mode == 'autoencoder'


def test_gridsearch_resolves_the_three_classes(tmp_path):
    """`model: {class: CorrespondenceAutoencoder}`, `loss: {class: CorrespondenceLoss}`, `trainer: {class: TrainerCorrespondence}`
    built the way the reference's gridsearch builds them (tests/test_gridsearch_boundary.py: build_experiment)."""
    import copy
    import abnet3_amd.trainer
    from test_gridsearch_boundary import build_experiment, load
    d = load()
    params = copy.deepcopy(d['default_params'])
    params['model']['class'] = 'CorrespondenceAutoencoder'
    params['model']['arguments']['num_decoder_layers'] = 2
    params['loss'] = {'class': 'CorrespondenceLoss', 'arguments': {'avg': True, 'symmetric': False}}
    _, model, loss, _, _, embedder = build_experiment(tmp_path, params, d['reference'], False)
    assert type(model).__name__ == 'CorrespondenceAutoencoder' and model.num_decoder_layers == 2
    assert model.output_path == os.path.join(str(tmp_path), 'network')               # the injected argument
    assert type(loss).__name__ == 'CorrespondenceLoss' and loss.symmetric is False and loss.mode == 'correspondence'
    assert embedder.network is model
    cls = getattr(abnet3_amd.trainer, 'TrainerCorrespondence')
    assert issubclass(cls, abnet3_amd.trainer.TrainerSiamese)
    assert cls.give_batch_to_network is not abnet3_amd.trainer.TrainerSiamese.give_batch_to_network      # what keeps _direct_ok() false
