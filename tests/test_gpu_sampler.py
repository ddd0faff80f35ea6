"""abn_sample_pairs (abnet3_amd/csrc/sampler.hip) on the MI355X against tests/sampler_np.py, its restatement, bit
for bit; its memory on a cluster set whose K^2 table could not exist; and SamplerClusterSiamese.sample() end to
end into OriginalDataLoader and one epoch of training."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN

import sampler_np
from abnet3_amd import sampler as S

pytestmark = pytest.mark.gpu

DIR = os.path.join(GOLDEN, 'sampler')
FIXTURES = {'english': ('english.test.classes', 'english.spkid'),
            'english_split': ('english.split.test.classes', 'english.spkid'),
            'small': ('small.classes', 'small.spkid'),
            'collide': ('collide.classes', 'collide.spkid')}
ALL_MODES = ['1', 'f', 'f2', 'log', 'fcube']
# 0, 1 and one wavefront more or less per configuration, in every position; then 10^5 of each
COUNTS = [(0, 0, 0, 0), (1, 1, 1, 1), (63, 64, 65, 1), (65, 63, 0, 64), (64, 65, 63, 0), (10 ** 5,) * 4]


def describe(name):
    classes, spkid = FIXTURES[name]
    sam = S.SamplerClusterSiamese()
    clusters = sam.parse_input_file(os.path.join(DIR, classes))
    return sam.analyze_clusters(clusters, S.read_spkid_file(os.path.join(DIR, spkid)))


def device_draw(dev_tables, counts, seed, block=S.DEFAULT_BLOCK):
    import torch
    tok1, tok2, key = S.sample_pairs_device(dev_tables, counts, seed, block)
    torch.cuda.synchronize()
    return tok1.cpu().numpy(), tok2.cpu().numpy(), key.cpu().numpy()


def assert_same_bits(got, want, what):
    for name, g, w in zip(('tok1', 'tok2', 'key'), got, want[:3]):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.flatnonzero(g != w)[:5])


@pytest.mark.parametrize('mode', ALL_MODES)
@pytest.mark.parametrize('name', list(FIXTURES))
def test_kernel_equals_the_restatement_bit_for_bit(name, mode):
    """Tokens and shuffle keys; english.test.classes has a configuration with empty support (no type has two
    speakers: Stype_Dspk yields -1 tokens) and cells of one token."""
    descr = describe(name)
    tables = S.build_tables(descr, mode, mode)
    restated = sampler_np.build_tables(descr, mode, mode)
    for k, v in restated.items():
        assert np.array_equal(tables[k], v) if isinstance(v, np.ndarray) else tables[k] == v, k
    if name == 'english':
        assert int(tables['total'][1]) == 0 and (np.diff(tables['tok_beg']) == 1).any()
    dev = S.DeviceTables(tables)
    for counts in COUNTS:
        seed = 1000 * len(mode) + sum(counts)
        want = sampler_np.sample_pairs(restated, counts, seed)
        assert_same_bits(device_draw(dev, counts, seed), want, (name, mode, counts))
        if name == 'english' and counts[1]:
            lo = counts[0]
            assert (want[0][lo:lo + counts[1]] == -1).all()
    # a seed above 2^32 reaches the second key word
    assert_same_bits(device_draw(dev, (65, 65, 65, 65), (3 << 32) + 1), sampler_np.sample_pairs(restated, (65,) * 4, (3 << 32) + 1), 'seed')


def test_a_type_without_tokens_is_accepted():
    """A cluster that a split emptied still counts as a type (analyze_clusters numbers the clusters it is given):
    more types than cells is no argument error, and the draws equal the restatement."""
    sam = S.SamplerClusterSiamese()
    clusters = sam.parse_input_file(os.path.join(DIR, 'english.split.test.classes'))
    clusters = [[]] + clusters[:1] + [[], [], []] + clusters[1:] + [[]]
    descr = sam.analyze_clusters(clusters, S.read_spkid_file(os.path.join(DIR, 'english.spkid')))
    tables = S.build_tables(descr, 'log', 'log')
    assert tables['n_type'] == 7 > tables['n_cells'] == 4
    restated = sampler_np.build_tables(descr, 'log', 'log')
    for k, v in restated.items():
        assert np.array_equal(tables[k], v) if isinstance(v, np.ndarray) else tables[k] == v, k
    dev = S.DeviceTables(tables)
    assert_same_bits(device_draw(dev, (200, 200, 200, 200), 3), sampler_np.sample_pairs(restated, (200,) * 4, 3), 'empty types')


def test_launch_geometry_does_not_change_the_output():
    tables = S.build_tables(describe('small'), 'log', 'log')
    dev = S.DeviceTables(tables)
    counts = (1000, 777, 1025, 63)
    a, b, c = (device_draw(dev, counts, 5, block) for block in (64, 256, 1024))
    assert_same_bits(a, b, 'block 64 / 256')
    assert_same_bits(a, c, 'block 64 / 1024')


def test_bad_arguments_are_refused_before_launch():
    import torch
    from abnet3_amd import _lib
    lib = _lib.load()
    dev = S.DeviceTables(S.build_tables(describe('small'), 'log', 'log'))
    out = torch.full((3, 64), -7, dtype=torch.int64, device='cuda')
    n = lambda *c: (ctypes.c_int64 * 4)(*c)
    call = lambda tables, counts, block, o=out: lib.abn_sample_pairs(tables, counts, 0, _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]),
                                                                    block, _lib.stream())
    for block in (0, 32, 100, 2048):
        assert call(ctypes.byref(dev.struct), n(1, 1, 1, 1), block) == _lib.E_ARG
        assert b'block' in lib.abn_last_error()
    assert call(ctypes.byref(dev.struct), n(1, -1, 1, 1), 256) == _lib.E_ARG
    assert call(ctypes.byref(dev.struct), n(2 ** 30, 2 ** 30, 1, 1), 256) == _lib.E_ARG
    assert call(None, n(1, 1, 1, 1), 256) == _lib.E_ARG
    assert lib.abn_sample_pairs(ctypes.byref(dev.struct), n(1, 1, 1, 1), 0, None, None, None, 256, _lib.stream()) == _lib.E_ARG
    broken = type(dev.struct).from_buffer_copy(dev.struct)
    broken.cum_m = None
    assert call(ctypes.byref(broken), n(1, 1, 1, 1), 256) == _lib.E_ARG
    broken = type(dev.struct).from_buffer_copy(dev.struct)
    broken.n_cells = 0
    assert call(ctypes.byref(broken), n(1, 1, 1, 1), 256) == _lib.E_ARG
    torch.cuda.synchronize()
    assert (out == -7).all()                                    # nothing was launched
    with pytest.raises(_lib.HipLibraryError, match='block'):
        S.sample_pairs_device(dev, (1, 1, 1, 1), 0, block=96)


def synthetic_description(n_spk, n_type, n_tok, seed):
    """Random (speaker, type) per token, Zipf-like over types: ~n_tok cells when n_spk n_type >> n_tok."""
    rng = np.random.default_rng(seed)
    typ = np.minimum((n_type * rng.random(n_tok) ** 2).astype(np.int64), n_type - 1)
    typ = np.unique(typ, return_inverse=True)[1]                      # every type index is in use
    spk = rng.integers(0, n_spk, n_tok)
    order = np.argsort(typ, kind='stable')
    typ, spk = typ[order], spk[order]
    return {'tokens': None, 'tokens_type': typ.tolist(), 'tokens_speaker': ['s%04d' % s for s in spk],
            'types': np.bincount(typ).tolist()}


def test_a_cluster_set_whose_table_could_not_exist():
    """K >= 10^5 cells, 500 000 pairs: device memory stays O(K + tokens + N).  Around the upload of the tables and
    the launch there are three allocations -- the table blob, the two token arrays as one tensor, the keys: table bytes
    + 16 bytes per pair.  torch's caching allocator charges a whole block: it serves a request above 1 MiB from a
    segment rounded up to 2 MiB and hands a block out unsplit when what would remain is under 1 MiB, so each
    allocation may be charged up to 2 MiB more than it asked for (the cache is emptied first, so that blocks left by
    earlier tests play no part); where the allocator reports the REQUESTED bytes, those are held to the sizes alone.
    Around the whole draw -- sort by shuffle key and the gathers included -- at most sixteen allocations are alive at
    once and they hold at most eight output sets (sorted keys and indices, the sort's double buffers, the gathered
    tokens and configuration indices).  The K^2 table would hold 8 K^2 bytes."""
    import torch
    descr = synthetic_description(n_spk=400, n_type=20000, n_tok=160000, seed=2)
    tables = S.build_tables(descr, 'log', 'log')
    K = tables['n_cells']
    assert K >= 10 ** 5
    with pytest.raises(ValueError, match='max_keys'):
        S.explicit_table(descr, 'Dtype_Dspk')
    counts = S.pair_counts(500000, 0.5, 0.5)
    n = [counts[c] for c in S.CONFIGS]
    N = sum(n)
    assert N == 500000
    from abnet3_amd import _lib
    table_bytes = sum(tables[k].nbytes for k in _lib.SamplerTables.POINTERS)
    out_bytes = 16 * N
    block_slack = 2 << 20                                             # per allocation: see the docstring
    requested = 'requested_bytes.all.peak'

    def baseline():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        return torch.cuda.memory_allocated(), torch.cuda.memory_stats().get('requested_bytes.all.current')
    base, base_req = baseline()
    dev = S.DeviceTables(tables)
    tok1, tok2, key = S.sample_pairs_device(dev, n, 9)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert dev.nbytes <= table_bytes + 16 * 16                        # (the tables' 16-byte alignment)
    assert peak <= table_bytes + out_bytes + 3 * block_slack, (peak, table_bytes, out_bytes)
    if base_req is not None and requested in torch.cuda.memory_stats():
        asked = torch.cuda.memory_stats()[requested] - base_req
        assert asked <= dev.nbytes + out_bytes + 3 * 512, (asked, dev.nbytes, out_bytes)
    assert table_bytes < 200 * K and peak * 1000 < 8 * K * K
    got = (tok1.cpu().numpy(), tok2.cpu().numpy(), key.cpu().numpy())
    assert_same_bits(got, sampler_np.sample_pairs(tables, n, 9), 'K = %d' % K)
    # every pair is of its configuration
    spk, typ = np.asarray(descr['tokens_speaker']), np.asarray(descr['tokens_type'])
    off = np.concatenate([[0], np.cumsum(n)])
    for q in range(4):
        a, b = got[0][off[q]:off[q + 1]], got[1][off[q]:off[q + 1]]
        assert (a >= 0).all() and (b >= 0).all()
        assert ((spk[a] == spk[b]) == (q in (0, 2))).all() and ((typ[a] == typ[b]) == (q in (0, 1))).all()
        assert (a != b).all() and (q < 2 or (typ[a] < typ[b]).all())
    del tok1, tok2, key, dev
    base, _ = baseline()
    t1, t2, cfg = S.draw_pairs(descr, counts, 'log', 'log', 9)
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= table_bytes + 8 * out_bytes + 16 * block_slack, (peak, table_bytes, out_bytes)
    assert (table_bytes + 8 * out_bytes + 16 * block_slack) * 100 < 8 * K * K
    order = sampler_np.final_order(got[2])
    assert np.array_equal(t1, got[0][order]) and np.array_equal(t2, got[1][order])
    assert np.array_equal(cfg, np.searchsorted(off[1:4], order, side='right'))


def test_sample_then_load_then_train(tmp_path, monkeypatch):
    """sample() writes both pair directories, OriginalDataLoader loads them, one epoch of TrainerSiamese.train()
    runs; the same / diff line counts are the sums of the four counts."""
    import fake_h5features                     # (tests/ is on the path: conftest and sampler_np come from it too)
    monkeypatch.setitem(sys.modules, 'h5features', fake_h5features)
    import abnet3_amd.loss as L
    from abnet3_amd.dataloader import OriginalDataLoader
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    from abnet3_amd.utils import read_dataset
    rng = np.random.default_rng(3)
    spk_of = S.read_spkid_file(os.path.join(DIR, 'small.spkid'))
    feat_path = str(tmp_path / 'features.h5f')
    items = sorted(spk_of)
    feats = [rng.standard_normal((2400, 40)).astype(np.float32) for _ in items]
    fake_h5features.write(feat_path, 'features', items, [np.arange(2400) * 0.01 + 0.0025 for _ in items], feats)
    out = str(tmp_path / 'pairs')
    sam = S.SamplerClusterSiamese(std_file=os.path.join(DIR, 'small.classes'), spkid_file=os.path.join(DIR, 'small.spkid'),
                                  directory_output=out, num_total_sampled_pairs=200, ratio_same_diff_spk=0.5,
                                  split_method='split_each_file', seed=4)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        sam.sample()
    n_train = int(200 * 0.7)
    clusters = sam.parse_input_file(sam.std_file)
    descrs = [sam.analyze_clusters(c, spk_of) for c in sam.split_each_file(clusters)]
    for sub, num, descr in (('train_pairs', n_train, descrs[0]), ('dev_pairs', 200 - n_train, descrs[1])):
        lines = read_dataset(os.path.join(out, sub, 'dataset'))
        counts = S.pair_counts(num, 0.5, 0.5)
        empty = [c for q, c in enumerate(S.CONFIGS) if int(S.build_tables(descr, 'log', 'log')['total'][q]) == 0]
        same = sum(counts[c] for c in ('Stype_Sspk', 'Stype_Dspk') if c not in empty)
        diff = sum(counts[c] for c in ('Dtype_Sspk', 'Dtype_Dspk') if c not in empty)
        assert sum(1 for l in lines if l[6] == 'same') == same and sum(1 for l in lines if l[6] == 'diff') == diff
        assert same > 0 and diff > 0
        tokens = set((f, round(s, 2), round(e, 2)) for f, s, e in descr['tokens'])
        assert all((l[0], l[1], l[2]) in tokens and (l[3], l[4], l[5]) in tokens for l in lines)
    assert len([w for w in caught if 'no admissible pair' in str(w.message)]) == sum(
        1 for d in descrs for q in range(4) if int(S.build_tables(d, 'log', 'log')['total'][q]) == 0)
    # the same seed writes the same files
    again = str(tmp_path / 'pairs_again')
    sam.directory_output = again
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sam.sample()
    for sub in ('train_pairs', 'dev_pairs'):
        assert open(os.path.join(out, sub, 'dataset')).read() == open(os.path.join(again, sub, 'dataset')).read()
    net = SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=24, p_dropout=0.0,
                         activation_layer='sigmoid', output_path=str(tmp_path / 'network'))
    dl = OriginalDataLoader(pairs_path=out, features_path=feat_path, batch_size=8, num_max_minibatches=100)
    tr = TrainerSiamese(network=net, loss=L.coscos2(avg=False), optimizer_type='adadelta', lr=0.1, num_epochs=1, patience=5,
                        dataloader=dl, log_dir=str(tmp_path / 'logs'))
    tr.train()
    assert len(tr.train_losses) == 2 and np.isfinite(tr.train_losses).all() and np.isfinite(tr.dev_losses).all()


def test_sample_batches_writes_batch_files(tmp_path):
    descr = describe('small')
    sam = S.SamplerClusterSiamese(sample_batches=True, batch_size=8)
    n = sam.write_tokens(descr=descr, batch_size=8, num_samples=100, out_dir=str(tmp_path), seed=1)
    files = sorted(os.listdir(str(tmp_path)))
    assert files == sorted('pair_%d.batch' % i for i in range(1, 100 // 8)) and n == sum(S.pair_counts(100, 0.75, 0.5).values())
    for f in files:
        assert len(open(os.path.join(str(tmp_path), f)).read().splitlines()) == 8
