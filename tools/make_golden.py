#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by IMPORTING the reference.

Runs only in the build container (needs /root/reference); never on the GPU box.
The reference's modules import five third-party packages that are absent here
(h5features, dtw, spectral, h5py, tensorboardX); they are registered as empty
stub modules in THIS process only, so that abnet3.model / abnet3.loss /
abnet3.utils.cosine_distance / FeaturesGenerator.stack_fbanks can be imported
and executed unmodified on torch-CPU.  Nothing of the reference is copied: the
fixtures are inputs + the outputs the reference produced for them.

Fixture sets:
  G1 tower_*      SiameseNetwork forward, eval + train mode, BN on/off
  G2 train_c1_*   loss scalar + every parameter gradient + params after 3 steps
  G3 loss_edge    pair losses on edge-case rows (label 0, tiny norms, margin)
  G4 train_mid / train_c2   reduced-width C2 with full tensors; true C2 scalars
  G5 cosdist      abnet3.utils.cosine_distance
  G6 stack        FeaturesGenerator.stack_fbanks
  G7 frames       OriginalDataLoader.load_frames_from_pairs (needs the oracle DTW
                  monkey-patched in as get_dtw_alignment; third-party dtw absent)
  G8 multitask_*  SiameseMultitaskNetwork + weighted_loss_multi: forward (eval,
                  train), every gradient, params after 3 steps; and the speaker
                  labels of load_frames_from_pairs(fid2spk=...)
  G5L cosdist_libm  abnet3.utils.cosine_distance with numpy on its plain-libm path
                  (NPY_DISABLE_CPU_FEATURES drops numpy's AVX512/SVML arccos; the
                  generator re-runs itself in a child process with that variable) on
                  matrices large enough for OpenBLAS's regular sgemm kernel: what the
                  oracle and the HIP kernel reproduce bit for bit, plus the per-pair
                  drop decisions (AssertionError) for near-duplicate tokens
  G10 mvn        the four normalisation cases of the reference's own test/test_features.py:37-281
                  (global / per file, with and without a VAD, per channel and over the whole spectrum),
                  re-enacted in memory: the inputs are that test's literals, the VAD file is read and
                  applied by the reference's read_vad_file / filter_vad_* (pure numpy, importable), the
                  expected statistics and outputs are the expressions that test asserts
  G11 gridsearch  the `default_params` of the reference's test/data/buckeye.yaml as a dictionary, and what
                  the reference's own classes make of it when built the way gridsearch.py:145-202 builds them
                  (which keyword arguments they accept, parameter count, state_dict keys, optimizer class)
  G12 kl_loss    KLLoss (abnet3/loss.py:108-137): on probability rows, behind nn.Softmax() from logits (with the
                  reference's own float64 evaluation, a near-uniform case among them), and a softmax SiameseNetwork
                  trained 3 steps with it (BatchNorm off / on, SGD / Adadelta; the float64 run's losses beside)
  G13 multimodal  MultimodalSiameseNetwork (abnet3/model.py:379-621) with each integration unit of
                  abnet3/integration.py (BiWeightedDeepLearnt with K = 1 and K = width, sum and concat, asynchronous
                  index 0 and 1, BatchNorm, attention_lr): initial tensors (pre-nets included), e1 / e2, coscos2
                  loss and gradients, parameters after 3 SGD and 3 Adadelta steps; the integration units alone
                  (inputs, output, every gradient); two headstart schedules; MultimodalDataLoader batches
  G9 frames_loader  FramesDataLoader.load_all_frames / load_batch / batch_iterator
                  (shuffles, batch slicing, max_batches_per_epoch wrap-around) and
                  OriginalDataLoader.add_tcl_to_batch / temporal_coherence_loss
  G14 pairs_loader  PairsDataLoader.load_pairs (abnet3/dataloader.py:439-474) on the reference's own test files
                  (test/data/dataloader/pairs_knn.txt, id_to_file.txt, copied to tests/golden/pairs_loader/ as data):
                  the train / test pair lists for both split methods at ratios 0.5 and 0.7, with and without the
                  id_to_file map.  split_method='files' calls random.sample on a SET (dataloader.py:484), a TypeError
                  from Python 3.11 on: for those cases only, random.sample is given sorted(set) instead (the
                  population abnet3_amd's class samples from), after random.seed(seed); the seed is recorded
  G15 sampler     SamplerClusterSiamese (abnet3/sampler.py) on three cluster files under tests/golden/sampler/: the
                  reference's own test/data/english.test.classes and english.split.test.classes (copied as data, with
                  the speaker map of its test/test_sampler.py written as a spkid file) and a hand-made one (6 speakers,
                  12 types, 60 tokens, no two speakers sharing two types: asserted) and a second hand-made one with exactly one
                  colliding quadruple beside collision-free keys.  Recorded per file: the outputs of
                  parse_input_file, split_each_file, analyze_clusters, generate_token_dict; the keys and probabilities
                  of type_speaker_sampling_p in four mode pairs; the four per-configuration counts of sample_batch for
                  several num_samples and ratios (observed as the lengths of what it returns, on the hand-made file);
                  and the sampler section of test/data/buckeye.yaml

usage: python tools/make_golden.py [--only G1,G3]
"""
import argparse
import os
import sys
import types
import warnings

import numpy as np

REF = '/root/reference'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden')


def import_reference():
    for name in ['h5features', 'dtw', 'spectral', 'h5py', 'tensorboardX']:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['dtw'].DTW = None
    sys.modules['spectral'].Spectral = None
    sys.modules['tensorboardX'].SummaryWriter = None
    sys.path.insert(0, REF)
    import scipy
    if not hasattr(scipy, 'arccos'):
        scipy.arccos = np.arccos      # removed from scipy >= 1.12 (utils.py:50,53)
    warnings.simplefilter('ignore')
    import torch  # noqa
    import abnet3.model
    import abnet3.loss
    import abnet3.utils
    import abnet3.features
    import abnet3.dataloader
    import abnet3.integration
    return abnet3


def sd_to_np(net, prefix='p.'):
    return {prefix + k: v.detach().cpu().numpy().copy()
            for k, v in net.state_dict().items()}


def make_inputs(B, D, seed):
    import torch
    torch.manual_seed(seed)
    x1 = torch.randn(B, D)
    x2 = torch.randn(B, D)
    np.random.seed(seed)
    y = np.random.choice([1, -1], B)
    return x1, x2, y


def build_net(abnet3, seed, **kw):
    import torch
    torch.manual_seed(seed)
    return abnet3.model.SiameseNetwork(**kw)


OPTIMS = {
    'sgd': lambda torch, p: torch.optim.SGD(p, lr=0.001, momentum=0.9),
    'adadelta': lambda torch, p: torch.optim.Adadelta(p, lr=0.1),
    'adam': lambda torch, p: torch.optim.Adam(p, lr=0.001),
    'adagrad': lambda torch, p: torch.optim.Adagrad(p, lr=0.001),
    'RMSprop': lambda torch, p: torch.optim.RMSprop(p, lr=0.001),
}


def g1_tower(abnet3):
    """G1: tower forward in eval and train mode (model.py:179-196)."""
    import torch
    cases = {
        'sig': dict(activation_layer='sigmoid', batch_norm=False),
        'sig_bn': dict(activation_layer='sigmoid', batch_norm=True),
        'relu_bn': dict(activation_layer='relu', batch_norm=True),
        'tanh': dict(activation_layer='tanh', batch_norm=False),
        'sig_lin': dict(activation_layer='sigmoid', batch_norm=False,
                        last_non_linearity=None),
        'relu_h2': dict(activation_layer='relu', batch_norm=False,
                        num_hidden_layers=2),
        'tanh_softmax': dict(activation_layer='tanh', batch_norm=False,
                             last_non_linearity='softmax'),
        'relu_bn_softmax': dict(activation_layer='relu', batch_norm=True,
                                last_non_linearity='softmax'),
    }
    for name, extra in cases.items():
        kw = dict(input_dim=40, num_hidden_layers=0, hidden_dim=100,
                  output_dim=50, p_dropout=0.0, type_init='xavier_uni')
        kw.update(extra)
        net = build_net(abnet3, 0, **kw)
        x1, x2, y = make_inputs(32, 40, 0)
        out = sd_to_np(net)
        out['x1'], out['x2'], out['y'] = x1.numpy(), x2.numpy(), y
        net.eval()
        with torch.no_grad():
            e1, e2 = net(x1, x2)
        out['eval_e1'], out['eval_e2'] = e1.numpy(), e2.numpy()
        net.train()
        with torch.no_grad():
            e1, e2 = net(x1, x2)
        out['train_e1'], out['train_e2'] = e1.numpy(), e2.numpy()
        out.update(sd_to_np(net, 'after.'))   # BN running stats after 2 calls
        if 'softmax' in name:                 # + one backward through the softmax head
            net = build_net(abnet3, 0, **kw)
            net.train()
            e1, e2 = net(x1, x2)
            lv = abnet3.loss.cosmargin(avg=True)(e1, e2, torch.from_numpy(y))
            lv.backward()
            out['loss'] = np.float64(lv.detach())
            for k, p in net.named_parameters():
                out['grad.' + k] = p.grad.detach().numpy().copy()
        out['kw'] = np.array(repr(kw))
        np.savez_compressed(os.path.join(OUT, 'tower_%s.npz' % name), **out)


def run_steps(abnet3, net, loss_mod, optim_name, batches, nsteps, out, tag):
    """Re-enacts trainer.py:236-242 (optimize_model's five statements)."""
    import torch
    opt = OPTIMS[optim_name](torch, net.parameters())
    net.train()
    losses = []
    for s in range(nsteps):
        x1, x2, y = batches[s % len(batches)]
        e1, e2 = net(x1, x2)
        lv = loss_mod(e1, e2, torch.from_numpy(y))
        opt.zero_grad()
        lv.backward()
        if s == 0:
            for k, p in net.named_parameters():
                out['%s.grad0.%s' % (tag, k)] = p.grad.detach().numpy().copy()
            out['%s.e1_0' % tag] = e1.detach().numpy().copy()
            out['%s.e2_0' % tag] = e2.detach().numpy().copy()
        opt.step()
        losses.append(float(lv.detach()))
    out['%s.losses' % tag] = np.array(losses, dtype=np.float64)
    for k, v in net.state_dict().items():
        out['%s.after.%s' % (tag, k)] = v.detach().numpy().copy()


def g2_train_c1(abnet3):
    """G2: C1 = 40->100->50, B=32. Loss, all grads, params after 3 steps."""
    for bn in (False, True):
        out = {}
        kw = dict(input_dim=40, num_hidden_layers=0, hidden_dim=100,
                  output_dim=50, p_dropout=0.0, type_init='xavier_uni',
                  activation_layer='sigmoid', batch_norm=bn)
        x1, x2, y = make_inputs(32, 40, 0)
        out['x1'], out['x2'], out['y'] = x1.numpy(), x2.numpy(), y
        net0 = build_net(abnet3, 0, **kw)
        out.update(sd_to_np(net0))
        for lname in ('coscos2', 'cosmargin'):
            for avg in (True, False):
                for oname in OPTIMS:
                    if oname not in ('sgd', 'adadelta') and not (
                            lname == 'coscos2' and avg is False):
                        continue
                    net = build_net(abnet3, 0, **kw)
                    loss_mod = getattr(abnet3.loss, lname)(avg=avg)
                    tag = '%s.avg%d.%s' % (lname, int(avg), oname)
                    run_steps(abnet3, net, loss_mod, oname, [(x1, x2, y)], 3,
                              out, tag)
        out['kw'] = np.array(repr(kw))
        np.savez_compressed(
            os.path.join(OUT, 'train_c1_bn%d.npz' % int(bn)), **out)


def g3_loss_edge(abnet3):
    """G3: pair losses + autograd gradients on edge-case rows (loss.py:46-105)."""
    import torch
    torch.manual_seed(3)
    B, D = 32, 50
    e1 = torch.randn(B, D)
    e2 = torch.randn(B, D)
    np.random.seed(3)
    y = np.random.choice([1, -1], B).astype(np.int64)
    y[0] = 0            # any other label leaves raw cos (loss.py:60-63)
    y[1] = 2
    e2[2] = e1[2]       # identical rows, same
    y[2] = 1
    e2[3] = e1[3]       # identical rows, diff
    y[3] = -1
    e2[4] = -e1[4]      # opposite rows
    y[4] = -1
    e1[5] = e1[5] * 1e-8   # tiny norm -> eps clamp on one side
    y[5] = 1
    e1[6] = e1[6] * 1e-8
    e2[6] = e2[6] * 1e-8   # both below eps
    y[6] = -1
    e1[7] = 0.0            # exact zero row
    y[7] = 1
    e1[8] = e1[8] * 1e-7   # around eps=1e-6 (norm ~ 7e-7)
    y[8] = -1
    # cos just above / below the default margin 0.5 for cosmargin
    v = torch.randn(D)
    w = torch.randn(D)
    w = w - (w @ v) / (v @ v) * v
    v = v / v.norm()
    w = w / w.norm()
    for row, c in ((9, 0.5005), (10, 0.4995), (11, 0.5)):
        e1[row] = 2.0 * v
        e2[row] = 3.0 * (c * v + float(np.sqrt(1 - c * c)) * w)
        y[row] = -1
    out = {'e1': e1.numpy().copy(), 'e2': e2.numpy().copy(), 'y': y}
    label_sets = {
        'mixed': y,
        'allsame': np.ones(B, dtype=np.int64),
        'alldiff': -np.ones(B, dtype=np.int64),
        'f64': y.astype(np.float64),
    }
    for lsname, yy in label_sets.items():
        out['y.' + lsname] = yy
        for lname, kwargs in (('coscos2', {}), ('cosmargin', {}),
                              ('cosmargin', {'margin': 0.2})):
            for avg in (True, False):
                a = e1.clone().requires_grad_(True)
                b = e2.clone().requires_grad_(True)
                mod = getattr(abnet3.loss, lname)(avg=avg, **kwargs)
                lv = mod(a, b, torch.from_numpy(yy))
                lv.backward()
                tag = '%s.%s%s.avg%d' % (
                    lsname, lname,
                    '' if not kwargs else '_m%g' % kwargs['margin'], int(avg))
                out[tag + '.loss'] = np.array(float(lv.detach()),
                                              dtype=np.float64)
                out[tag + '.de1'] = a.grad.numpy().copy()
                out[tag + '.de2'] = b.grad.numpy().copy()
    np.savez_compressed(os.path.join(OUT, 'loss_edge.npz'), **out)


def g4_train_mid(abnet3):
    """G4: reduced-width C2 with full tensors; true C2 with scalars only."""
    import torch
    # reduced width, odd sizes on purpose (tile tails): 40 -> 72 x2 -> 36, B=96
    for bn in (False, True):
        out = {}
        kw = dict(input_dim=40, num_hidden_layers=2, hidden_dim=72,
                  output_dim=36, p_dropout=0.0, type_init='xavier_uni',
                  activation_layer='sigmoid', batch_norm=bn)
        batches = []
        for s in range(3):
            x1, x2, y = make_inputs(96, 40, 10 + s)
            batches.append((x1, x2, y))
            out['x1.%d' % s], out['x2.%d' % s], out['y.%d' % s] = \
                x1.numpy(), x2.numpy(), y
        net0 = build_net(abnet3, 1, **kw)
        out.update(sd_to_np(net0))
        for oname in ('sgd', 'adadelta'):
            net = build_net(abnet3, 1, **kw)
            run_steps(abnet3, net, abnet3.loss.coscos2(avg=False), oname,
                      batches, 5, out, 'coscos2.avg0.' + oname)
        out['kw'] = np.array(repr(kw))
        np.savez_compressed(
            os.path.join(OUT, 'train_mid_bn%d.npz' % int(bn)), **out)

    # true C2: 40 -> 500 x2 -> 100, B=4096; weights regenerated from the seed by
    # torch's own initialisers, so only checksums + scalars + a few rows travel.
    for bn in (False, True):
        out = {}
        kw = dict(input_dim=40, num_hidden_layers=2, hidden_dim=500,
                  output_dim=100, p_dropout=0.0, type_init='xavier_uni',
                  activation_layer='sigmoid', batch_norm=bn)
        net = build_net(abnet3, 2, **kw)
        for k, v in net.state_dict().items():
            out['chk.' + k] = np.array([float(v.double().sum()),
                                        float(v.double().abs().sum())])
        batches = [make_inputs(4096, 40, 20 + s) for s in range(2)]
        opt = torch.optim.Adadelta(net.parameters(), lr=0.1)
        loss_mod = abnet3.loss.coscos2(avg=False)
        net.train()
        losses = []
        for s in range(5):
            x1, x2, y = batches[s % 2]
            e1, e2 = net(x1, x2)
            lv = loss_mod(e1, e2, torch.from_numpy(y))
            opt.zero_grad()
            lv.backward()
            if s == 0:
                out['e1_rows'] = e1.detach().numpy()[:8].copy()
                out['e2_rows'] = e2.detach().numpy()[-8:].copy()
                # every one of the 2 x 4096 embedding rows, as two float64 checksums per row (sum, sum |.|),
                # and each tensor's sum / sum |.| / max |.|
                for name, e in (('e1', e1), ('e2', e2)):
                    ed = e.detach().double()
                    out[name + '_rowsum'] = ed.sum(dim=1).numpy().copy()
                    out[name + '_rowabs'] = ed.abs().sum(dim=1).numpy().copy()
                    out[name + '_chk'] = np.array([float(ed.sum()), float(ed.abs().sum()), float(ed.abs().max())])
                for k, p in net.named_parameters():
                    g = p.grad.detach()
                    out['gchk.' + k] = np.array(
                        [float(g.double().sum()), float(g.double().abs().sum()),
                         float(g.double().abs().max())])
                    out['grow.' + k] = g.numpy().reshape(g.shape[0], -1)[:4].copy()
            opt.step()
            losses.append(float(lv.detach()))
        out['losses'] = np.array(losses)
        for k, v in net.state_dict().items():
            out['after_chk.' + k] = np.array([float(v.double().sum()),
                                              float(v.double().abs().sum())])
        out['kw'] = np.array(repr(kw))
        np.savez_compressed(
            os.path.join(OUT, 'train_c2_bn%d.npz' % int(bn)), **out)


def g5_cosdist(abnet3):
    """G5: abnet3.utils.cosine_distance (utils.py:40-60)."""
    rng = np.random.default_rng(5)
    out = {}
    cases = {}
    a = rng.standard_normal((37, 40)).astype(np.float32)
    b = rng.standard_normal((29, 40)).astype(np.float32)
    cases['f32'] = (a, b)
    cases['f64'] = (a.astype(np.float64), b.astype(np.float64))
    cases['one'] = (a[:1], b[:1])
    az = a.copy()
    bz = b.copy()
    az[3] = 0
    az[10] = 0
    bz[7] = 0
    cases['zero'] = (az, bz)
    bd = a[:29] + 1e-3 * rng.standard_normal((29, 40)).astype(np.float32)
    cases['near'] = (a, bd.astype(np.float32))
    pos = np.abs(rng.standard_normal((50, 40))).astype(np.float32)
    cases['pos'] = (pos[:30], pos[20:])
    for name, (x, y) in cases.items():
        out[name + '.x'], out[name + '.y'] = x, y
        try:
            out[name + '.d'] = abnet3.utils.cosine_distance(x, y)
        except AssertionError:
            out[name + '.d'] = np.array('AssertionError')
    np.savez_compressed(os.path.join(OUT, 'cosdist.npz'), **out)


def g6_stack(abnet3):
    """G6: FeaturesGenerator.stack_fbanks (features.py:135-159)."""
    rng = np.random.default_rng(6)
    fg = abnet3.features.FeaturesGenerator.__new__(
        abnet3.features.FeaturesGenerator)
    out = {}
    for name, (T, D, n) in {'t100_n7': (100, 40, 7), 't100_n3': (100, 40, 3),
                            't5_n7': (5, 40, 7), 't2_n7': (2, 40, 7),
                            't17_n1': (17, 13, 1)}.items():
        f = rng.standard_normal((T, D)).astype(np.float32)
        out[name + '.in'] = f
        out[name + '.n'] = np.array(n)
        out[name + '.out'] = fg.stack_fbanks(f, nframes=n)
    np.savez_compressed(os.path.join(OUT, 'stack.npz'), **out)


def g7_frames(abnet3):
    """G7: OriginalDataLoader.load_frames_from_pairs (dataloader.py:166-261)
    with a fake accessor and the build's oracle DTW standing in for the absent
    third-party dtw.DTW (parity unpinned for the DTW itself)."""
    sys.path.insert(0, REPO)
    from oracle import dtw_oracle
    rng = np.random.default_rng(7)
    feats = {'u%d' % i: rng.standard_normal((n, 40)).astype(np.float32)
             for i, n in enumerate((90, 70, 120, 64))}
    times = {k: (np.arange(len(v)) * 0.01 + 0.0025) for k, v in feats.items()}
    acc = abnet3.utils.Features_Accessor(times, feats)

    def oracle_align(f1, f2):
        d = abnet3.utils.cosine_distance(f1, f2)
        p1, p2 = dtw_oracle.dtw_path(d)
        return list(p1), list(p2)

    abnet3.dataloader.get_dtw_alignment = oracle_align
    out = {}
    for k, v in feats.items():
        out['feat.' + k] = v
    pairs = [('u0', 0.10, 0.42, 'u1', 0.05, 0.31, 'same'),
             ('u2', 0.50, 0.93, 'u3', 0.11, 0.37, 'same'),
             ('u0', 0.33, 0.61, 'u2', 0.70, 1.05, 'diff'),
             ('u1', 0.20, 0.21, 'u3', 0.30, 0.46, 'diff'),   # 1-frame token
             ('u3', 0.40, 0.30, 'u1', 0.10, 0.20, 'same'),   # s>e: skipped
             ('u1', 0.02, 0.29, 'u1', 0.31, 0.64, 'same')]
    out['pairs'] = np.array([' '.join(map(str, p)) for p in pairs])
    # an empty token (no frame time inside [0.20, 0.20]) is legal only without
    # align_different_words (the reference indexes into it otherwise)
    empty = ('u1', 0.20, 0.20, 'u3', 0.30, 0.46, 'diff')
    out['pairs_empty'] = np.array(' '.join(map(str, empty)))
    for align in (False, True):
        dl = abnet3.dataloader.OriginalDataLoader(
            'unused', 'unused', align_different_words=align)
        dl.features = acc
        grouped = abnet3.utils.group_pairs(pairs + ([] if align else [empty]))
        X1, X2, Y = dl.load_frames_from_pairs(grouped)
        out['align%d.X1' % align] = X1
        out['align%d.X2' % align] = X2
        out['align%d.Y' % align] = Y
    np.savez_compressed(os.path.join(OUT, 'frames.npz'), **out)


def g8_multitask(abnet3):
    """G8: SiameseMultitaskNetwork (model.py:211-376) + weighted_loss_multi
    (loss.py:140-182), re-enacting TrainerSiameseMultitask.give_batch_to_network
    (trainer.py:259-279) and trainer.py:236-242."""
    import torch
    cases = {
        'sig': dict(activation_layer='sigmoid', batch_norm=False, num_hidden_layers_shared=1,
                    num_hidden_layers_spk=1, num_hidden_layers_phn=0),
        'relu_bn': dict(activation_layer='relu', batch_norm=True, num_hidden_layers_shared=2,
                        num_hidden_layers_spk=0, num_hidden_layers_phn=1),
        'tanh0': dict(activation_layer='tanh', batch_norm=False, num_hidden_layers_shared=0,
                      num_hidden_layers_spk=0, num_hidden_layers_phn=0),
    }
    for name, extra in cases.items():
        kw = dict(input_dim=40, hidden_dim=64, output_dim=24, p_dropout=0.0,
                  type_init='xavier_uni')
        kw.update(extra)
        x1, x2, y_spk = make_inputs(48, 40, 3)
        np.random.seed(11)
        y_phn = np.random.choice([1, -1], 48)
        out = {'x1': x1.numpy(), 'x2': x2.numpy(), 'y_spk': y_spk, 'y_phn': y_phn,
               'kw': np.array(repr(kw))}
        torch.manual_seed(5)
        net = abnet3.model.SiameseMultitaskNetwork(**kw)
        out.update(sd_to_np(net))
        net.eval()
        with torch.no_grad():
            s1, p1, s2, p2 = net(x1, x2)
        for k, v in (('spk1', s1), ('phn1', p1), ('spk2', s2), ('phn2', p2)):
            out['eval_' + k] = v.numpy()
        for oname, weight in (('sgd', 0.3), ('adadelta', 0.5), ('adam', 1.0)):
            torch.manual_seed(5)
            net = abnet3.model.SiameseMultitaskNetwork(**kw)
            loss_mod = abnet3.loss.weighted_loss_multi(
                loss_spk=abnet3.loss.coscos2(avg=False),
                loss_phn=abnet3.loss.cosmargin(avg=True, margin=0.4), weight=weight)
            opt = OPTIMS[oname](torch, net.parameters())
            net.train()
            tag = '%s.w%g' % (oname, weight)
            losses = []
            for s in range(3):
                emb = net(x1, x2)
                lv = loss_mod(emb[0], emb[1], emb[2], emb[3], torch.from_numpy(y_spk),
                              torch.from_numpy(y_phn))
                opt.zero_grad()
                lv.backward()
                if s == 0:
                    for k, p in net.named_parameters():
                        # dead branches (hidden_layers_spk / _phn) get no gradient at all
                        out['%s.grad0.%s' % (tag, k)] = (
                            p.grad.detach().numpy().copy() if p.grad is not None
                            else np.zeros(0, dtype=np.float32))
                    for k, v in zip(('spk1', 'phn1', 'spk2', 'phn2'), emb):
                        out['%s.%s_0' % (tag, k)] = v.detach().numpy().copy()
                opt.step()
                losses.append(float(lv.detach()))
            out['%s.losses' % tag] = np.array(losses, dtype=np.float64)
            for k, v in net.state_dict().items():
                out['%s.after.%s' % (tag, k)] = v.detach().numpy().copy()
        np.savez_compressed(os.path.join(OUT, 'multitask_%s.npz' % name), **out)

    # speaker labels of the multitask loader (dataloader.py:195-201,235-241): the
    # reference compares the speaker strings with `is`
    sys.path.insert(0, REPO)
    from oracle import dtw_oracle
    rng = np.random.default_rng(8)
    feats = {'u%d' % i: rng.standard_normal((n, 40)).astype(np.float32)
             for i, n in enumerate((80, 60, 75))}
    times = {k: (np.arange(len(v)) * 0.01 + 0.0025) for k, v in feats.items()}
    acc = abnet3.utils.Features_Accessor(times, feats)

    def oracle_align(f1, f2):
        d = abnet3.utils.cosine_distance(f1, f2)
        a, b = dtw_oracle.dtw_path(d)
        return list(a), list(b)

    abnet3.dataloader.get_dtw_alignment = oracle_align
    import tempfile
    with tempfile.NamedTemporaryFile('w', suffix='.spk', delete=False) as fh:
        fh.write('u0 alice\nu1 alice\nu2 b\n')
        spk_path = fh.name
    fid2spk = abnet3.utils.read_spkid_file(spk_path)
    os.unlink(spk_path)
    pairs = [('u0', 0.10, 0.40, 'u1', 0.05, 0.33, 'same'),    # same speaker name, two files
             ('u0', 0.12, 0.30, 'u0', 0.41, 0.66, 'same'),    # same file
             ('u1', 0.20, 0.45, 'u2', 0.10, 0.31, 'diff'),
             ('u2', 0.05, 0.22, 'u2', 0.40, 0.61, 'diff')]
    out = {'pairs': np.array([' '.join(map(str, q)) for q in pairs]),
           'spk_file': np.array('u0 alice\nu1 alice\nu2 b\n')}
    for k, v in feats.items():
        out['feat.' + k] = v
    dl = abnet3.dataloader.OriginalDataLoader('unused', 'unused', align_different_words=False)
    dl.features = acc
    X1, X2, y_spk, y_phn = dl.load_frames_from_pairs(abnet3.utils.group_pairs(pairs),
                                                     fid2spk=fid2spk)
    out['X1'], out['X2'], out['y_spk'], out['y_phn'] = X1, X2, y_spk, y_phn
    np.savez_compressed(os.path.join(OUT, 'multitask_frames.npz'), **out)


NO_AVX512 = 'AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL'


def near_duplicate_pair(p):
    """Token pair p of the drop-decision set: 176 x 40 frames (M*N*K > 10^6, the
    regular sgemm kernel), the second token = the first plus noise of a size that
    puts cos(x_i, y_i) within a few ulp of 1.  Regenerated from the seed by the tests
    (numpy's PCG64 stream); `in_chk` in the fixture guards against a drifted stream."""
    rng = np.random.default_rng(5000 + p)
    n = 176
    x = rng.standard_normal((n, 40)).astype(np.float32)
    if p % 3 == 2:
        x = np.abs(x)                            # filterbank-like: all cosines > 0.5
    eps = [0.0, 3e-4, 6e-4, 8e-4, 1e-3, 1.3e-3, 2e-3, 4e-3][p % 8]
    y = (x + np.float32(eps) * rng.standard_normal((n, 40)).astype(np.float32)).astype(np.float32)
    if p % 16 >= 8:
        y = (y * np.float32(1.0 + 0.37 * (p % 5))).astype(np.float32)   # same direction, other norm
    return x, y


def g5l_cosdist_libm(abnet3):
    """G5L: cosine_distance on numpy's libm path (see the module docstring)."""
    import hashlib
    if os.environ.get('NPY_DISABLE_CPU_FEATURES') != NO_AVX512:
        import subprocess
        env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=NO_AVX512)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--only', 'G5L'], env=env)
        return
    rng = np.random.default_rng(55)
    out = {}
    cases = {}
    cases['big'] = (rng.standard_normal((300, 40)).astype(np.float32),
                    rng.standard_normal((280, 40)).astype(np.float32))
    pos = np.abs(rng.standard_normal((530, 40))).astype(np.float32)
    cases['bigpos'] = (pos[:260], pos[260:])
    z = rng.standard_normal((290, 40)).astype(np.float32)
    w = rng.standard_normal((270, 40)).astype(np.float32)
    z[5] = 0; z[77] = 0; w[0] = 0; w[200] = 0
    cases['bigzero'] = (z, w)
    z2, w2 = z.copy(), w.copy()
    w2[13] = -2.0 * z2[13]                          # cos = -1 up to rounding
    w2[14] = 0.5 * z2[14]                           # cos = +1 up to rounding
    cases['bigdup'] = (z2, w2)
    wide = rng.standard_normal((190, 280)).astype(np.float32)   # stacked 7 x 40 features
    cases['wide'] = (wide[:100], wide[100:])
    for name, (x, y) in cases.items():
        out[name + '.x'], out[name + '.y'] = x, y
        try:
            d = abnet3.utils.cosine_distance(x, y)
            d32 = d.astype(np.float32)
            assert (d32.astype(np.float64) == d).all()      # float32 values in a float64 container
            out[name + '.d32'] = d32
        except AssertionError:
            out[name + '.d32'] = np.zeros((0, 0), dtype=np.float32)
            out[name + '.dropped'] = np.array(True)
    P = 48
    dropped, hashes, in_chk = [], [], []
    for p in range(P):
        x, y = near_duplicate_pair(p)
        in_chk.append([float(x.astype(np.float64).sum()), float(y.astype(np.float64).sum())])
        try:
            d = abnet3.utils.cosine_distance(x, y)
            dropped.append(False)
            hashes.append(hashlib.sha256(d.astype(np.float32).tobytes()).hexdigest())
        except AssertionError:
            dropped.append(True)
            hashes.append('')
    out['near.dropped'] = np.array(dropped)
    out['near.sha256'] = np.array(hashes)
    out['near.in_chk'] = np.array(in_chk)
    print('   near-duplicate pairs dropped by the reference: %d of %d' % (sum(dropped), P))
    np.savez_compressed(os.path.join(OUT, 'cosdist_libm.npz'), **out)


def g9_frames_loader(abnet3):
    """G9: FramesDataLoader (dataloader.py:580-739) and the temporal coherence pairs
    of OriginalDataLoader (:314-352), with a fake accessor and the build's oracle DTW
    standing in for the absent third-party dtw.DTW (as in G7)."""
    import random
    sys.path.insert(0, REPO)
    from oracle import dtw_oracle
    rng = np.random.default_rng(9)
    feats = {'u%d' % i: rng.standard_normal((n, 40)).astype(np.float32)
             for i, n in enumerate((90, 70, 120, 64, 100))}
    times = {k: (np.arange(len(v)) * 0.01 + 0.0025) for k, v in feats.items()}

    def oracle_align(f1, f2):
        d = abnet3.utils.cosine_distance(f1, f2)
        p1, p2 = dtw_oracle.dtw_path(d)
        return list(p1), list(p2)

    abnet3.dataloader.get_dtw_alignment = oracle_align
    train = [('u0', 0.10, 0.42, 'u1', 0.05, 0.31, 'same'),
             ('u2', 0.50, 0.93, 'u3', 0.11, 0.37, 'same'),
             ('u0', 0.33, 0.61, 'u2', 0.70, 1.05, 'diff'),
             ('u1', 0.20, 0.21, 'u3', 0.30, 0.46, 'diff'),   # 1-frame token
             ('u3', 0.40, 0.30, 'u1', 0.10, 0.20, 'same'),   # s > e: skipped
             ('u1', 0.02, 0.29, 'u4', 0.31, 0.64, 'same'),
             ('u4', 0.05, 0.44, 'u2', 0.15, 0.50, 'same'),
             ('u4', 0.60, 0.95, 'u0', 0.45, 0.85, 'diff'),
             ('u3', 0.02, 0.30, 'u4', 0.50, 0.80, 'diff')]
    dev = [('u0', 0.50, 0.80, 'u3', 0.20, 0.52, 'same'),
           ('u1', 0.30, 0.55, 'u2', 0.20, 0.41, 'diff'),
           ('u2', 0.02, 0.33, 'u4', 0.20, 0.49, 'same')]
    out = {'train_pairs': np.array([' '.join(map(str, p)) for p in train]),
           'dev_pairs': np.array([' '.join(map(str, p)) for p in dev])}
    for k, v in feats.items():
        out['feat.' + k] = v

    cases = {   # name: (ctor kwargs, numpy seed, sequence of epochs: T(rain) / D(ev))
        'full': (dict(batch_size=50, randomize_dataset=True), 9, 'TTDT'),
        'norand': (dict(batch_size=64, randomize_dataset=False), 10, 'TDT'),
        'sub': (dict(batch_size=40, randomize_dataset=True, max_batches_per_epoch=2), 11, 'TTTDTTT'),
        'tiny': (dict(batch_size=5000, randomize_dataset=True), 12, 'TD'),   # fewer pairs than one batch
    }
    for name, (kw, seed, epochs) in cases.items():
        acc = abnet3.utils.Features_Accessor(dict(times), {k: v.copy() for k, v in feats.items()})
        dl = abnet3.dataloader.FramesDataLoader('unused', 'unused', **kw)
        dl.features = acc
        dl.pairs = {'train': list(train), 'dev': list(dev)}
        np.random.seed(seed)
        X1s, X2s, Ys, sizes, nb = [], [], [], [], []
        for mode in epochs:
            n = 0
            for X1, X2, y in dl.batch_iterator(train_mode=(mode == 'T')):
                X1s.append(X1.numpy()); X2s.append(X2.numpy()); Ys.append(y.numpy())
                sizes.append(len(y))
                n += 1
            nb.append(n)
        out[name + '.kw'] = np.array(repr(kw))
        out[name + '.seed'] = np.array(seed)
        out[name + '.epochs'] = np.array(epochs)
        out[name + '.X1'] = np.vstack(X1s)
        out[name + '.X2'] = np.vstack(X2s)
        out[name + '.y'] = np.concatenate(Ys)
        out[name + '.sizes'] = np.array(sizes)
        out[name + '.batches_per_epoch'] = np.array(nb)
        out[name + '.n_frame_pairs'] = np.array([len(dl.frame_pairs['train']), len(dl.frame_pairs['dev'])])

    # temporal coherence pairs added to a word-pair batch (tcl = 0.3)
    acc = abnet3.utils.Features_Accessor(dict(times), {k: v.copy() for k, v in feats.items()})
    dl = abnet3.dataloader.OriginalDataLoader('unused', 'unused', tcl=0.3)
    dl.features = acc
    dl.train_files = ['u0', 'u2', 'u3', 'u4']       # explicit order (the reference builds it from a set)
    batch = dl.load_frames_from_pairs(abnet3.utils.group_pairs(train[:4]))
    random.seed(4)
    X1, X2, Y = dl.add_tcl_to_batch(batch)
    out['tcl.train_files'] = np.array(dl.train_files)
    out['tcl.n_before'] = np.array(len(batch[2]))
    out['tcl.X1'], out['tcl.X2'], out['tcl.Y'] = X1, X2, Y
    np.savez_compressed(os.path.join(OUT, 'frames_loader.npz'), **out)


def g10_mvn(abnet3):
    """G10: mean / variance normalisation as the reference's test states it (test/test_features.py:37-281).
    h5features / h5py are absent, so FeaturesGenerator.mean_variance_normalisation itself cannot run; what the
    reference's test pins is re-enacted: its literal inputs, the frames a VAD keeps (the reference's own
    read_vad_file + filter_vad_one_file / filter_vad_whole_dataset on its own Features_Accessor), the statistics it
    asserts (np.mean / np.std of the kept frames, axis 0 or None) and the output it asserts
    ((feature - mean) / (std + eps), abnet3/features.py:240,293)."""
    import tempfile
    from abnet3.features import FeaturesGenerator
    from abnet3.utils import read_vad_file, Features_Accessor
    out = {}
    t = lambda n: np.arange(n, dtype=float) * 0.01 + 0.0025
    vad_text = "file,start,stop\nfile1,0.0025,0.5000\nfile1,0.7525,1.000\n"
    with tempfile.NamedTemporaryFile('w', suffix='.vad', delete=False) as fh:
        fh.write(vad_text)
    vad = read_vad_file(fh.name)
    os.unlink(fh.name)
    cases = {
        # test_normalization (:37-85)
        'global': ([np.full((100, 40), 1.0), np.full((150, 40), 2.0)], False, None),
        # test_normalization_per_file (:87-140)
        'per_file': ([np.vstack([np.full((100, 40), 1.), np.full((100, 40), -1.)]),
                      np.vstack([np.full((100, 40), 1.), np.full((100, 40), 2.)])], True, None),
        # test_normalization_with_VAD (:142-204)
        'global_vad': ([np.vstack([np.full((50, 40), 1.0), np.full((50, 40), -1.0)]),
                        np.vstack([np.full((50, 40), 1.0), np.full((50, 40), -1.0)])], False, vad),
        # test_norm_per_file_with_VAD (:206-281)
        'per_file_vad': ([np.vstack([np.full((50, 40), 1.0), np.full((50, 40), -1.0)]),
                          np.vstack([np.full((50, 40), 1.0), np.full((50, 40), -1.0)])], True, vad),
    }
    items = ['file1', 'file2']
    fg = FeaturesGenerator()
    for name, (features, per_file, vad_data) in cases.items():
        times = [t(f.shape[0]) for f in features]
        for i, f in enumerate(features):
            out['%s.x%d' % (name, i)] = f.astype(np.float32)
            out['%s.t%d' % (name, i)] = times[i]
        out[name + '.per_file'] = np.array(int(per_file))
        out[name + '.vad'] = np.array(vad_text if vad_data is not None else '')
        eps = np.finfo(features[0].dtype).eps
        for per_channel in (1, 0):
            axis = 0 if per_channel else None
            tag = '%s.pc%d' % (name, per_channel)
            if per_file:
                for i, (f, tm) in enumerate(zip(features, times)):
                    kept = f
                    if vad_data is not None and items[i] in vad_data:
                        kept = fg.filter_vad_one_file(f, tm, vad_data[items[i]])
                    mean, std = np.mean(kept, axis=axis), np.std(kept, axis=axis)
                    out['%s.kept%d' % (tag, i)] = np.array(kept.shape[0])
                    out['%s.mean%d' % (tag, i)] = np.atleast_1d(mean)
                    out['%s.std%d' % (tag, i)] = np.atleast_1d(std)
                    out['%s.out%d' % (tag, i)] = (f - mean) / (std + eps)
            else:
                acc = Features_Accessor({k: tm for k, tm in zip(items, times)},
                                        {k: f.astype(np.float32) for k, f in zip(items, features)})
                if vad_data is not None:
                    fg.filter_vad_whole_dataset(acc, vad_data)
                kept = np.vstack(list(acc.features.values())).astype(np.float64)
                mean, std = np.mean(kept, axis=axis), np.std(kept, axis=axis)
                out[tag + '.kept'] = np.array(kept.shape[0])
                out[tag + '.mean'] = np.atleast_1d(mean)
                out[tag + '.std'] = np.atleast_1d(std)
                for i, f in enumerate(features):
                    out['%s.out%d' % (tag, i)] = (f - mean) / (std + eps)
    # the literals the reference's test spells out
    assert int(out['global_vad.pc1.kept']) == 75 + 100 and int(out['per_file_vad.pc1.kept0']) == 75
    assert np.allclose(out['per_file.pc0.mean1'], 1.5) and np.allclose(out['per_file.pc0.mean0'], 0.0)
    np.savez_compressed(os.path.join(OUT, 'mvn.npz'), **out)


def g11_gridsearch(abnet3):
    """G11: the caller's side of the boundary.  GridSearch.run_single_experiment (gridsearch.py:145-202) builds every
    object as getattr(abnet3.<module>, cfg['class'])(**cfg['arguments']) after injecting a few arguments; the
    fixture holds the reference's own test configuration (test/data/buckeye.yaml -> default_params, as data) and
    what the reference's classes are when built from it on this machine (sampler excluded: out of scope; the
    reference's trainer needs tensorboardX's SummaryWriter only inside train())."""
    import inspect
    import json
    import yaml
    import abnet3.trainer
    import abnet3.embedder
    with open(os.path.join(REF, 'test', 'data', 'buckeye.yaml')) as fh:
        params = yaml.safe_load(fh)['default_params']
    exp = '/tmp/abnet3_g11'
    info = {}

    def build(module, section, inject):
        cfg = params[section]
        cls = getattr(module, cfg['class'])
        args = dict(cfg['arguments'] or {})
        args.update(inject)
        accepted = set(inspect.signature(cls.__init__).parameters) - {'self'}
        has_var_kw = any(p.kind == p.VAR_KEYWORD for p in inspect.signature(cls.__init__).parameters.values())
        rejected = sorted(k for k in args if k not in accepted and not has_var_kw)
        info[section + '.rejected_kwargs'] = rejected
        return cls(**{k: v for k, v in args.items() if k not in rejected})

    features = build(abnet3.features, 'features', {})
    model = build(abnet3.model, 'model', {'output_path': os.path.join(exp, 'network')})
    loss = build(abnet3.loss, 'loss', {})
    dataloader = build(abnet3.dataloader, 'dataloader',
                       {'pairs_path': os.path.join(exp, 'pairs'), 'features_path': features.output_path})
    trainer = build(abnet3.trainer, 'trainer', {'network': model, 'loss': loss, 'dataloader': dataloader,
                                                'log_dir': os.path.join(exp, 'logs')})
    embedder = build(abnet3.embedder, 'embedder', {'network': model, 'output_path': os.path.join(exp, 'embeddings.h5f'),
                                                   'feature_path': features.output_path,
                                                   'network_path': model.output_path + '.pth'})
    info['model.n_parameters'] = int(sum(p.numel() for p in model.parameters()))
    info['model.state_dict_keys'] = list(model.state_dict().keys())
    info['model.whoami_keys'] = sorted(model.whoami().keys())
    info['loss.class'] = type(loss).__name__
    info['loss.whoami_keys'], info['loss.avg'] = sorted(loss.whoami().keys()), bool(loss.avg)
    info['trainer.optimizer'] = type(trainer.optimizer).__name__
    info['trainer.lr'] = trainer.optimizer.param_groups[0]['lr']
    info['trainer.num_epochs'], info['trainer.patience'] = trainer.num_epochs, trainer.patience
    info['dataloader.batch_size'] = dataloader.batch_size
    info['dataloader.num_max_minibatches'] = dataloader.num_max_minibatches
    info['embedder.batch_size'] = embedder.batch_size
    info['features.run'] = features.run
    with open(os.path.join(OUT, 'gridsearch_buckeye.json'), 'w') as fh:
        json.dump({'default_params': params, 'reference': info}, fh, indent=1, sort_keys=True)


def _kl_rows(torch, p, q):
    """KL(p||q), KL(q||p) per row as the reference's KLLoss.forward writes them (abnet3/loss.py:127-137)."""
    return torch.sum(p * torch.log(p / q), 1), torch.sum(q * torch.log(q / p), 1)


def _kl_draw(torch, B, D, scale, margin, softmax):
    """[B, D] logits scale * randn for both sides; rows whose KL (either direction, fp32) lies within 1e-4 of the
    margin are drawn again, so that no hinge subgradient is decided by rounding."""
    z1, z2 = scale * torch.randn(B, D), scale * torch.randn(B, D)
    for _ in range(100):
        k1, k2 = _kl_rows(torch, softmax(z1), softmax(z2))
        bad = ((k1 - margin).abs() < 1e-4) | ((k2 - margin).abs() < 1e-4)
        if not bool(bad.any()):
            return z1, z2
        n = int(bad.sum())
        z1[bad], z2[bad] = scale * torch.randn(n, D), scale * torch.randn(n, D)
    raise RuntimeError('could not draw rows away from the margin')


def g12_kl_loss(abnet3):
    """G12: KLLoss (abnet3/loss.py:108-137).  (a) on probability rows (softmax of 3 randn logits): loss and the
    gradients w.r.t. the rows; (b) behind nn.Softmax() from logits, gradients w.r.t. the logits, with the reference's
    own float64 evaluation (the same code on float64 tensors: its losses, and for the near-uniform cases -- 0.01 randn
    logits -- its gradients); (c) SiameseNetwork(last_non_linearity='softmax') trained 3 steps with KLLoss (C1 =
    40->100->50, B = 32), BatchNorm off / on, SGD / Adadelta: losses, first-step gradients (the same for both
    optimizers: stored once), parameters after 3 steps; the float64 run's losses.  The Linear layers' initial
    parameters are stored once (BatchNorm draws nothing: the BN network's Linear layers start from the same values)."""
    import torch
    import torch.nn as nn
    out = {}
    sm = nn.Softmax()
    # (name, B, D, logit scale, margin, avg, label dtype)
    cases_a = [('a0', 8, 100, 3.0, 1, True, 'i64'), ('a1', 21, 39, 3.0, 1, False, 'i64'),
               ('a2', 21, 39, 3.0, 0.5, True, 'i64'), ('a3', 29, 7, 3.0, 0.5, False, 'f32'),
               ('a4', 29, 7, 3.0, 3, True, 'i64'), ('a5', 8, 100, 3.0, 3, False, 'i64')]
    cases_b = [('b0', 8, 100, 3.0, 1, True, 'i64'), ('b1', 21, 39, 3.0, 0.5, False, 'i64'),
               ('b2', 29, 7, 3.0, 3, True, 'f32'), ('b3', 33, 7, 3.0, 1, False, 'i64'),
               ('u0', 8, 100, 0.01, 1, True, 'i64'), ('u1', 21, 39, 0.01, 0.5, False, 'i64')]
    names = []
    for i, (name, B, D, scale, margin, avg, ydt) in enumerate(cases_a + cases_b):
        torch.manual_seed(1200 + i)
        np.random.seed(1200 + i)
        logits = name[0] != 'a'
        z1, z2 = _kl_draw(torch, B, D, scale, margin, sm)
        y = np.random.choice([1, -1, 0, 2], B)
        y = y.astype(np.float32) if ydt == 'f32' else y.astype(np.int64)
        loss_mod = abnet3.loss.KLLoss(margin=margin, avg=avg)
        out[name + '.margin'], out[name + '.avg'] = np.float64(margin), np.int64(avg)
        out[name + '.y'] = y
        for dt, sfx in ((torch.float32, ''), (torch.float64, '.f64')):
            if not logits and dt == torch.float64:
                continue
            if logits:
                a = z1.to(dt).clone().requires_grad_(True)
                b = z2.to(dt).clone().requires_grad_(True)
                p, q = sm(a), sm(b)
            else:
                a = sm(z1).detach().clone().requires_grad_(True)
                b = sm(z2).detach().clone().requires_grad_(True)
                p, q = a, b
            lv = loss_mod(p, q, torch.from_numpy(y))
            lv.backward()
            if dt == torch.float32:         # (the float64 run's inputs are these, widened)
                out[name + '.in1'], out[name + '.in2'] = a.detach().numpy().copy(), b.detach().numpy().copy()
            out[name + '.loss' + sfx] = np.float64(float(lv.detach()))
            if dt == torch.float32 or name.startswith('u'):
                out[name + '.g1' + sfx], out[name + '.g2' + sfx] = a.grad.numpy().copy(), b.grad.numpy().copy()
        names.append(name)
    out['cases'] = np.array(names)
    # (c) three training steps of a softmax network with KLLoss
    x1, x2, y = make_inputs(32, 40, 0)
    out['c.x1'], out['c.x2'], out['c.y'] = x1.numpy(), x2.numpy(), y
    for bn in (False, True):
        kw = dict(input_dim=40, num_hidden_layers=0, hidden_dim=100, output_dim=50, p_dropout=0.0,
                  type_init='xavier_uni', activation_layer='sigmoid', batch_norm=bn, last_non_linearity='softmax')
        out['c.bn%d.kw' % bn] = np.array(repr(kw))
        linear = {k: v for k, v in sd_to_np(build_net(abnet3, 0, **kw), 'c.p.').items()
                  if k.endswith(('emb.0.weight', 'emb.0.bias', 'layer.0.weight', 'layer.0.bias'))}
        for k, v in linear.items():
            assert k not in out or np.array_equal(out[k], v), k
        out.update(linear)
        for oname in ('sgd', 'adadelta'):
            for dt, sfx in ((torch.float32, ''), (torch.float64, '.f64')):
                net = build_net(abnet3, 0, **kw).to(dt)
                batches = [(x1.to(dt), x2.to(dt), y)]
                run = {}
                tag = 'c.bn%d.%s%s' % (bn, oname, sfx)
                run_steps(abnet3, net, abnet3.loss.KLLoss(), oname, batches, 3, run, tag)
                out[tag + '.losses'] = run[tag + '.losses']
                if dt == torch.float64:
                    continue
                for k, v in run.items():
                    if k.startswith(tag + '.after.'):
                        out[k] = v
                    elif k.startswith(tag + '.grad0.'):
                        key = 'c.bn%d.grad0.' % bn + k[len(tag + '.grad0.'):]
                        assert key not in out or np.array_equal(out[key], v), key
                        out[key] = v
    np.savez_compressed(os.path.join(OUT, 'kl_loss.npz'), **out)


# G13 network configurations: name -> (unit class, unit kwargs, pre-net params, post-net params, network kwargs)
MM_D1, MM_D2, MM_B = 10, 6, 16
MM_CONFIGS = {
    'concat': ('ConcatenationIntegration', {}, [[10, 16, 12], [6, 16, 12]], [24, 8], dict(activation_layer='sigmoid')),
    'sum': ('SumIntegration', {}, [[10, 16, 12], [6, 16, 12]], [12, 8], dict(activation_layer='tanh')),
    'fixed_sum': ('BiWeightedFixed', dict(integration_mode='sum', weight_value=0.3), [[10, 16, 12], [6, 16, 12]],
                  [12, 8], dict(activation_layer='relu')),
    'fixed_concat': ('BiWeightedFixed', dict(integration_mode='concat'), [[10, 16, 12], [6, 16, 12]], [24, 8],
                     dict(activation_layer='sigmoid')),
    'scalar_sum': ('BiWeightedScalarLearnt', dict(integration_mode='sum'), [[10, 16, 12], [6, 16, 12]], [12, 8],
                   dict(activation_layer='sigmoid')),
    'scalar_concat_lr': ('BiWeightedScalarLearnt', dict(integration_mode='concat'), [[10, 16, 12], [6, 16, 12]],
                         [24, 8], dict(activation_layer='tanh', attention_lr=0.01)),
    'deep_k1_sum': ('BiWeightedDeepLearnt', dict(net_params=[[12, 1], [12, 1]], integration_mode='sum'),
                    [[10, 16, 12], [6, 16, 12]], [12, 8], dict(activation_layer='sigmoid')),
    'deep_kd_sum': ('BiWeightedDeepLearnt', dict(net_params=[[12, 12], [12, 12]], integration_mode='sum',
                                                  activation_type='tanh'),
                    [[10, 16, 12], [6, 16, 12]], [12, 8], dict(activation_layer='relu')),
    'deep_k1_concat_async0': ('BiWeightedDeepLearnt', dict(net_params=[[10, 4, 1], [6, 4, 1]], integration_mode='concat'),
                              [[10, 16, 12], [6, 16, 12]], [24, 8],
                              dict(activation_layer='sigmoid', asynchronous_integration_index=0)),
    'deep_kd_concat_async1_bn': ('BiWeightedDeepLearnt', dict(net_params=[[16, 12], [16, 12]], integration_mode='concat'),
                                 [[10, 16, 12], [6, 16, 12]], [24, 8],
                                 dict(activation_layer='tanh', asynchronous_integration_index=1, batch_norm=True,
                                      attention_lr=0.05)),
    'nopost_deep_k1': ('BiWeightedDeepLearnt', dict(net_params=[[12, 1], [12, 1]], integration_mode='sum'),
                       [[10, 16, 12], [6, 16, 12]], None, dict(activation_layer='sigmoid')),
}
MM_SEEDS = {name: 1300 + i for i, name in enumerate(MM_CONFIGS)}


def mm_build(abnet3, name, seed=None):
    """The reference network of configuration `name` under its seeds (torch and numpy)."""
    import torch
    cls, ukw, pre, post, nkw = MM_CONFIGS[name]
    seed = MM_SEEDS[name] if seed is None else seed
    torch.manual_seed(seed)
    np.random.seed(seed)
    unit = getattr(abnet3.integration, cls)(**ukw)
    net = abnet3.model.MultimodalSiameseNetwork(integration_unit=unit, pre_integration_net_params=pre,
                                                post_integration_net_params=post, **nkw)
    return net


def mm_state(net, prefix):
    """Every tensor of the reference network, the pre-nets under the port's key names (pre_nets.<i>.<j>.*)."""
    out = {prefix + k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    if net.pre:
        for i, pn in enumerate(net.pre_nets):
            for k, v in pn.state_dict().items():
                out['%spre_nets.%d.%s' % (prefix, i, k)] = v.detach().numpy().copy()
    return out


def mm_named_params(net):
    """(port key, parameter) of every parameter the reference trains."""
    out = [(k, p) for k, p in net.named_parameters()]
    if net.pre:
        for i, pn in enumerate(net.pre_nets):
            out += [('pre_nets.%d.%s' % (i, k), p) for k, p in pn.named_parameters()]
    return out


def mm_batch(torch, seed, B=MM_B):
    torch.manual_seed(seed)
    xa1, xa2 = torch.randn(B, MM_D1), torch.randn(B, MM_D1)
    xb1, xb2 = torch.randn(B, MM_D2), torch.randn(B, MM_D2)
    y = torch.from_numpy(np.random.RandomState(seed).choice([1, -1], B))
    return [xa1, xb1], [xa2, xb2], y


def g13_multimodal(abnet3):
    """G13: the multimodal family (see the module docstring)."""
    import torch
    out = {}
    loss_mod = abnet3.loss.coscos2(avg=False)
    for name in MM_CONFIGS:
        net = mm_build(abnet3, name)
        out.update(mm_state(net, name + '.init.'))
        out[name + '.arch'] = np.array(net.architecture_str())
        X1, X2, y = mm_batch(torch, MM_SEEDS[name] + 50)
        for m in range(2):
            out['%s.X1_%d' % (name, m)], out['%s.X2_%d' % (name, m)] = X1[m].numpy(), X2[m].numpy()
        out[name + '.y'] = y.numpy()
        init = {k: v.detach().clone() for k, v in net.state_dict().items()}
        init_pre = [{k: v.detach().clone() for k, v in pn.state_dict().items()} for pn in (net.pre_nets if net.pre else [])]
        for optim_name, make in (('sgd', lambda p: torch.optim.SGD(p, lr=0.001, momentum=0.9)),
                                 ('adadelta', lambda p: torch.optim.Adadelta(p, lr=0.1))):
            net.load_state_dict(init)
            for pn, sd in zip(net.pre_nets if net.pre else [], init_pre):
                pn.load_state_dict(sd)
            net.train()
            opt = make(net.parameters())
            losses = []
            for s in range(3):
                e1, e2 = net(X1, X2)
                lv = loss_mod(e1, e2, y)
                opt.zero_grad()
                lv.backward()
                if s == 0 and optim_name == 'sgd':
                    out[name + '.e1'], out[name + '.e2'] = e1.detach().numpy().copy(), e2.detach().numpy().copy()
                    out[name + '.loss'] = np.float64(float(lv))
                    for k, p in mm_named_params(net):
                        out['%s.grad.%s' % (name, k)] = p.grad.detach().numpy().copy()
                    w = net.integration_unit.get_weights() if hasattr(net.integration_unit, 'get_weights') else None
                    if isinstance(w, torch.Tensor) and w.numel() > 1:
                        out[name + '.w_last'] = w.detach().numpy().copy()
                opt.step()
                losses.append(float(lv))
            out['%s.%s.losses' % (name, optim_name)] = np.array(losses)
            out.update(mm_state(net, '%s.%s.after.' % (name, optim_name)))
        # the same network in float64 (the yardstick of the fp32 results: the reference's own fp32 gradients are up
        # to 1e-3 off in these tiny towers, where the post-net's bias gradient is a heavily cancelled sum)
        net.load_state_dict(init)
        for pn, sd in zip(net.pre_nets if net.pre else [], init_pre):
            pn.load_state_dict(sd)
        net.double()
        for pn in (net.pre_nets if net.pre else []):
            pn.double()
        if isinstance(getattr(net.integration_unit, 'weight', None), torch.Tensor) and \
                not isinstance(net.integration_unit.weight, torch.nn.Parameter):
            net.integration_unit.weight = net.integration_unit.weight.double()
        e1, e2 = net([x.double() for x in X1], [x.double() for x in X2])
        lv = loss_mod(e1, e2, y)
        lv.backward()
        out[name + '.f64.loss'] = np.float64(float(lv))
        for k, p in mm_named_params(net):
            out['%s.f64.grad.%s' % (name, k)] = p.grad.detach().numpy().copy()

    # the integration units alone: out = unit(x) and every gradient for a random upstream gradient g
    units = {
        'u_sum': ('SumIntegration', {}, 9, 9, None),
        'u_concat': ('ConcatenationIntegration', {}, 9, 5, None),
        'u_fixed_sum': ('BiWeightedFixed', dict(integration_mode='sum', weight_value=0.3), 9, 9, None),
        'u_fixed_concat': ('BiWeightedFixed', dict(integration_mode='concat', weight_value=0.7), 9, 5, None),
        'u_scalar_sum': ('BiWeightedScalarLearnt', dict(integration_mode='sum', weight_value=0.4), 9, 9, None),
        'u_scalar_concat': ('BiWeightedScalarLearnt', dict(integration_mode='concat', weight_value=0.6), 9, 5, None),
        'u_deep_k1_sum': ('BiWeightedDeepLearnt', dict(net_params=[[9, 1], [9, 1]], integration_mode='sum'), 9, 9, 1),
        'u_deep_kd_sum_tanh': ('BiWeightedDeepLearnt', dict(net_params=[[9, 9], [9, 9]], integration_mode='sum',
                                                          activation_type='tanh'), 9, 9, 9),
        'u_deep_k1_concat': ('BiWeightedDeepLearnt', dict(net_params=[[9, 1], [5, 1]], integration_mode='concat'), 9, 5, 1),
        'u_deep_kd_concat': ('BiWeightedDeepLearnt', dict(net_params=[[9, 9], [9, 9]], integration_mode='concat'), 9, 9, 9),
    }
    R = 13
    for i, (name, (cls, kw, d1, d2, K)) in enumerate(units.items()):
        torch.manual_seed(1400 + i)
        np.random.seed(1400 + i)
        unit = getattr(abnet3.integration, cls)(**kw)
        x1 = torch.randn(R, d1, requires_grad=True)
        x2 = torch.randn(R, d2, requires_grad=True)
        if K is not None:
            z = (2 * torch.randn(R, K)).requires_grad_()
            unit.compute_attention_weight = lambda i1, i2, z=z, u=unit: u.activation_layer(z)
            o = unit([x1, x2], diff_input=[x1, x2])
        else:
            o = unit([x1, x2])
        g = torch.randn(o.shape)
        o.backward(g)
        out[name + '.x1'], out[name + '.x2'], out[name + '.g'] = x1.detach().numpy(), x2.detach().numpy(), g.numpy()
        out[name + '.out'] = o.detach().numpy()
        out[name + '.dx1'], out[name + '.dx2'] = x1.grad.numpy(), x2.grad.numpy()
        out[name + '.mode'] = np.array(getattr(unit, 'integration_mode', 'concat' if 'concat' in name else 'sum'))
        if K is not None:
            out[name + '.z'], out[name + '.dz'] = z.detach().numpy(), z.grad.numpy()
            out[name + '.act'] = np.array(unit.activation_type)
        if cls == 'BiWeightedScalarLearnt':
            out[name + '.w'] = unit.weight.detach().numpy()
            out[name + '.dw'] = unit.weight.grad.numpy()
        elif cls == 'BiWeightedFixed':
            out[name + '.w'] = np.float64(unit.weight)

    # headstart schedules (trainer.py:281-365), optimize_model re-enacted by hand (its loss.data[0] fails on 0-dim
    # tensors): 4 epochs of 2 batches, Adadelta(0.1); the parameters after every epoch
    for tag, hs in (('hs_true', (2, True, 0.3)), ('hs_false', (2, False, 0.3))):
        net = mm_build(abnet3, 'deep_k1_sum', seed=1500)
        out.update(mm_state(net, tag + '.init.'))
        batches = [mm_batch(torch, 1510 + b) for b in range(2)]
        for b, (X1, X2, y) in enumerate(batches):
            for m in range(2):
                out['%s.b%d.X1_%d' % (tag, b, m)], out['%s.b%d.X2_%d' % (tag, b, m)] = X1[m].numpy(), X2[m].numpy()
            out['%s.b%d.y' % (tag, b)] = y.numpy()
        opt = torch.optim.Adadelta(net.parameters(), lr=0.1)
        epochs_left = hs[0]
        net.integration_unit.set_headstart_weight(hs[2])
        losses = []
        for epoch in range(4):
            if epochs_left == 0:
                if not hs[1]:
                    net.freeze_training()
                net.integration_unit.start_training()
            net.train()
            for X1, X2, y in batches:
                e1, e2 = net(X1, X2)
                lv = loss_mod(e1, e2, y)
                opt.zero_grad()
                lv.backward()
                opt.step()
                losses.append(float(lv))
            if epochs_left > -1:
                epochs_left -= 1
            out.update(mm_state(net, '%s.epoch%d.' % (tag, epoch)))
        out[tag + '.losses'] = np.array(losses)

    # MultimodalDataLoader: two modalities through the G9 fake accessor and oracle DTW, two epochs
    sys.path.insert(0, REPO)
    from oracle import dtw_oracle
    rng = np.random.default_rng(13)
    lens = (60, 48, 75, 52)
    feats0 = {'u%d' % i: rng.standard_normal((n, 12)).astype(np.float32) for i, n in enumerate(lens)}
    feats1 = {'u%d' % i: rng.standard_normal((n, 7)).astype(np.float32) for i, n in enumerate(lens)}
    times = {k: (np.arange(len(v)) * 0.01 + 0.0025) for k, v in feats0.items()}

    def oracle_align(f1, f2):
        d = abnet3.utils.cosine_distance(f1, f2)
        p1, p2 = dtw_oracle.dtw_path(d)
        return list(p1), list(p2)

    abnet3.dataloader.get_dtw_alignment = oracle_align
    train = [('u0', 0.10, 0.42, 'u1', 0.05, 0.31, 'same'),
             ('u2', 0.20, 0.63, 'u3', 0.11, 0.37, 'same'),
             ('u0', 0.33, 0.51, 'u2', 0.40, 0.65, 'diff'),
             ('u1', 0.02, 0.29, 'u3', 0.21, 0.44, 'same'),
             ('u3', 0.02, 0.30, 'u0', 0.20, 0.40, 'diff')]
    dev = [('u0', 0.30, 0.55, 'u3', 0.20, 0.45, 'same'),
           ('u1', 0.10, 0.35, 'u2', 0.20, 0.41, 'diff')]
    out['dl.train_pairs'] = np.array([' '.join(map(str, p)) for p in train])
    out['dl.dev_pairs'] = np.array([' '.join(map(str, p)) for p in dev])
    for k in feats0:
        out['dl.feat0.' + k], out['dl.feat1.' + k] = feats0[k], feats1[k]
    for name, kw, seed in (('dl_rand', dict(batch_size=20, randomize_dataset=True), 21),
                           ('dl_sub', dict(batch_size=16, randomize_dataset=True, max_batches_per_epoch=3), 22)):
        dl = abnet3.dataloader.MultimodalDataLoader('unused', ['m0', 'm1'], **kw)
        dl.features_dict = {'m0': abnet3.utils.Features_Accessor(dict(times), {k: v.copy() for k, v in feats0.items()}),
                            'm1': abnet3.utils.Features_Accessor(dict(times), {k: v.copy() for k, v in feats1.items()})}
        dl.pairs = {'train': list(train), 'dev': list(dev)}
        np.random.seed(seed)
        X1s, X2s, Ys, sizes = [[], []], [[], []], [], []
        for mode in 'TDT':
            for X1, X2, y in dl.batch_iterator(train_mode=(mode == 'T')):
                for m in range(2):
                    X1s[m].append(X1[m].numpy()); X2s[m].append(X2[m].numpy())
                Ys.append(y.numpy()); sizes.append(len(y))
        out[name + '.kw'] = np.array(repr(kw))
        out[name + '.seed'] = np.array(seed)
        for m in range(2):
            out['%s.X1_%d' % (name, m)], out['%s.X2_%d' % (name, m)] = np.vstack(X1s[m]), np.vstack(X2s[m])
        out[name + '.y'] = np.concatenate(Ys)
        out[name + '.sizes'] = np.array(sizes)
    np.savez_compressed(os.path.join(OUT, 'multimodal.npz'), **out)


def g14_pairs_loader(abnet3):
    """G14: the reference's PairsDataLoader.load_pairs on its own test data."""
    import contextlib
    import io
    import json
    import random
    import shutil
    src = os.path.join(REF, 'test', 'data', 'dataloader')
    dst = os.path.join(OUT, 'pairs_loader')
    os.makedirs(dst, exist_ok=True)
    for f in ('pairs_knn.txt', 'id_to_file.txt'):
        shutil.copyfile(os.path.join(src, f), os.path.join(dst, f))
    real_sample = random.sample

    def sample_sorted(population, k, **kw):
        return real_sample(sorted(population) if isinstance(population, (set, frozenset)) else population, k, **kw)

    seed, cases = 3, []
    for method in ('files', 'split_each_file'):
        for ratio in (0.5, 0.7):
            for mapped in (True, False):
                dl = abnet3.dataloader.PairsDataLoader(
                    pairs_path=os.path.join(dst, 'pairs_knn.txt'), features_path=None,
                    id_to_file=os.path.join(dst, 'id_to_file.txt') if mapped else None,
                    ratio_split_train_test=ratio, split_method=method)
                random.seed(seed)
                random.sample = sample_sorted
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        dl.load_pairs()
                finally:
                    random.sample = real_sample
                cases.append({'split_method': method, 'ratio': ratio, 'id_to_file': mapped, 'seed': seed,
                              'train': dl.pairs['train'], 'test': dl.pairs['test'],
                              'tokens_train': sorted(list(t) for t in dl.tokens['train']),
                              'tokens_test': sorted(list(t) for t in dl.tokens['test']),
                              'files': sorted(dl.files)})
    with open(os.path.join(dst, 'load_pairs.json'), 'w') as fh:
        json.dump({'cases': cases}, fh, indent=0)
        fh.write('\n')


# G15's hand-made clusters: (speakers of the type, tokens per cell).  Every two speakers share at most one type.
SMALL_SPEAKERS = ('A', 'B', 'C', 'D', 'E', 'F')
SMALL_TYPES = [('AB', (4, 3)), ('AC', (1, 5)), ('AD', (3, 1)), ('BC', (2, 2)), ('BD', (6, 1)), ('CD', (1, 2)),
               ('AEF', (2, 3, 1)), ('BE', (4, 2)), ('CF', (1, 3)), ('DE', (2, 1)), ('D', (4,)), ('F', (6,))]
SAMPLER_MODES = (('log', 'log'), ('f', 'f'), ('f2', '1'), ('1', '1'))
SAMPLER_COUNT_CASES = [(10, 0.75, 0.5), (10.0, 0.75, 0.5), (45.0, 0.75, 0.5), (5012, 0.75, 0.5), (1000, 0.5, 0.5),
                       (999, 0.3, 0.7), (7, 0.75, 0.5), (350000, 0.5, 0.5), (101, 0.66, 0.33), (3.0, 0.75, 0.5)]


# G15's second hand-made set: speakers A and B share types 0 and 1 (one colliding quadruple); the keys with C are free
COLLIDE_TYPES = [('AB', (2, 1)), ('AB', (1, 3)), ('CA', (2, 1)), ('C', (3,))]


def write_collide_clusters(dst):
    lines = []
    for t, (speakers, sizes) in enumerate(COLLIDE_TYPES):
        lines.append('%d word%02d' % (t, t))
        for spk, size in zip(speakers, sizes):
            lines += ['%s0 %.3f %.3f' % (spk.lower(), 1.0 + 2 * t + 0.5 * k, 1.25 + 2 * t + 0.5 * k) for k in range(size)]
        lines.append('')
    with open(os.path.join(dst, 'collide.classes'), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    with open(os.path.join(dst, 'collide.spkid'), 'w') as fh:
        fh.write(''.join('%s0 %s\n' % (spk.lower(), spk) for spk in 'ABC'))


def write_small_clusters(dst):
    """The hand-made cluster file and its speaker map: two files per speaker, tokens one after the other."""
    clock = {}
    lines, n_tok = [], 0
    for t, (speakers, sizes) in enumerate(SMALL_TYPES):
        lines.append('%d word%02d' % (t, t))
        for spk, size in zip(speakers, sizes):
            for k in range(size):
                fid = '%s%d' % (spk.lower(), (t + k) % 2)
                t0 = clock.get(fid, 0.5)
                dur = 0.25 + 0.05 * ((3 * t + k) % 7)
                lines.append('%s %.3f %.3f' % (fid, t0, t0 + dur))
                clock[fid] = t0 + dur + 0.125
                n_tok += 1
        lines.append('')
    assert n_tok == 60 and len(SMALL_TYPES) == 12
    with open(os.path.join(dst, 'small.classes'), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    with open(os.path.join(dst, 'small.spkid'), 'w') as fh:
        for spk in SMALL_SPEAKERS:
            for k in range(2):
                fh.write('%s%d %s\n' % (spk.lower(), k, spk))


def g15_sampler(abnet3):
    """G15: the reference's sampler on its own two cluster files and on a hand-made, collision-free one."""
    import contextlib
    import io
    import json
    import shutil
    import yaml
    import abnet3.sampler
    from abnet3.utils import cumulative_distribution, read_spkid_file
    dst = os.path.join(OUT, 'sampler')
    os.makedirs(dst, exist_ok=True)
    for f in ('english.test.classes', 'english.split.test.classes'):
        shutil.copyfile(os.path.join(REF, 'test', 'data', f), os.path.join(dst, f))
    # the speaker map of the reference's test/test_sampler.py:70-81, as the file read_spkid_file reads
    english = {'s0101a': 1, 's0102a': 1, 's2001a': 20, 's2401a': 24, 's2402b': 24, 's2403b': 24, 's2404b': 24,
               's2405b': 24, 's2403a': 24, 's2702a': 27}
    with open(os.path.join(dst, 'english.spkid'), 'w') as fh:
        for fid, spk in english.items():
            fh.write('%s %d\n' % (fid, spk))
    write_small_clusters(dst)
    write_collide_clusters(dst)
    plain = lambda v: v.item() if hasattr(v, 'item') else v
    record = {'modes': [list(m) for m in SAMPLER_MODES], 'fixtures': {}}
    arrays = {}
    for name, classes, spkid in (('english', 'english.test.classes', 'english.spkid'),
                                 ('english_split', 'english.split.test.classes', 'english.spkid'),
                                 ('small', 'small.classes', 'small.spkid'),
                                 ('collide', 'collide.classes', 'collide.spkid')):
        sam = abnet3.sampler.SamplerClusterSiamese()
        spk_of = read_spkid_file(os.path.join(dst, spkid))
        with contextlib.redirect_stdout(io.StringIO()):
            clusters = sam.parse_input_file(os.path.join(dst, classes))
            sam.spkid_from_file = spk_of
            train, dev = sam.split_each_file(clusters)
            descr = sam.analyze_clusters(clusters, spk_of)
            token_dict = sam.generate_token_dict(descr)
            for tm, sm in SAMPLER_MODES:
                p = sam.type_speaker_sampling_p(std_descr=descr, type_sampling_mode=tm, spk_sampling_mode=sm)
                if name == 'small':
                    assert all(p[cfg] for cfg in p), (tm, sm)
                for cfg, table in p.items():          # (the tables go to probabilities.npz: keys joined with '|')
                    tag = '%s/%s,%s/%s' % (name, tm, sm, cfg)
                    arrays[tag + '/keys'] = np.array(['|'.join(str(plain(k)) for k in key) for key in table], dtype=str)
                    arrays[tag + '/p'] = np.array(list(table.values()), dtype=np.float64)
        cells = set(zip(descr['tokens_speaker'], descr['tokens_type']))
        speakers, types = sorted(set(s for s, t in cells)), sorted(set(t for s, t in cells))
        quads = [(s, s2, i, j) for s in speakers for s2 in speakers if s < s2 for i in types for j in types if i < j
                 and {(s, i), (s, j), (s2, i), (s2, j)} <= cells]
        if name == 'collide':
            assert len(quads) == 1, quads
        if name == 'small':
            assert not quads, quads
            assert len(speakers) == 6 and len(descr['types']) == 12 and len(descr['tokens']) == 60
        fx = {'classes': classes, 'spkid': spkid, 'ratio_train_dev': sam.ratio_train_dev, 'clusters': clusters,
              'split_each_file': {'train': train, 'dev': dev},
              'descr': {k: ({str(a): int(b) for a, b in v.items()} if isinstance(v, dict) else
                            [plain(x) for x in v]) for k, v in descr.items()},
              'token_dict': [[int(t), str(s), [int(i) for i in ids]] for (t, s), ids in token_dict.items()],
              'n_colliding_quadruples': len(quads)}
        if name == 'small':
            counts = []
            p = sam.type_speaker_sampling_p(std_descr=descr, type_sampling_mode='1', spk_sampling_mode='1')
            cdf = {k: cumulative_distribution(v) for k, v in p.items()}
            for num, r_spk, r_type in SAMPLER_COUNT_CASES:
                sam.ratio_same_diff_spk, sam.ratio_same_diff_type = r_spk, r_type
                with contextlib.redirect_stdout(io.StringIO()):
                    drawn = sam.sample_batch(p, cdf, token_dict, num_samples=num)
                counts.append({'num_samples': num, 'ratio_same_diff_spk': r_spk, 'ratio_same_diff_type': r_type,
                               'counts': {cfg: len(v) for cfg, v in drawn.items()}})
            fx['sample_batch_counts'] = counts
        record['fixtures'][name] = fx
    with open(os.path.join(REF, 'test', 'data', 'buckeye.yaml')) as fh:
        record['buckeye_sampler'] = yaml.safe_load(fh)['default_params']['sampler']
    np.savez_compressed(os.path.join(dst, 'probabilities.npz'), **arrays)
    with open(os.path.join(dst, 'reference.json'), 'w') as fh:
        json.dump(record, fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')


ALL = {'G1': g1_tower, 'G2': g2_train_c1, 'G3': g3_loss_edge,
       'G4': g4_train_mid, 'G5': g5_cosdist, 'G6': g6_stack, 'G7': g7_frames,
       'G8': g8_multitask, 'G5L': g5l_cosdist_libm, 'G9': g9_frames_loader, 'G10': g10_mvn, 'G11': g11_gridsearch,
       'G12': g12_kl_loss, 'G13': g13_multimodal, 'G14': g14_pairs_loader, 'G15': g15_sampler}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    abnet3 = import_reference()
    import torch
    torch.set_num_threads(1)      # deterministic summation order in fixtures
    which = [s for s in args.only.split(',') if s] or list(ALL)
    for g in which:
        print('generating', g, flush=True)
        ALL[g](abnet3)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print('golden dir: %.1f KB' % (total / 1024))


if __name__ == '__main__':
    main()
