"""Pair sampling from word clusters (abnet3/sampler.py): SamplerBuilder, DummySampler, SamplerPairs,
SamplerCluster, SamplerClusterSiamese with the reference's constructor keywords, whoami() and sample().

    python -m abnet3_amd.sampler CLUSTERS.classes WAV2SPK.lst OUT_DIR [--num_total_sampled_pairs N] ...

sample() reads a .classes file of word clusters and a "<file> <speaker>" list, splits the clusters into train and
dev, and writes <directory_output>/train_pairs/dataset and dev_pairs/dataset (`f1 s1 e1 f2 s2 e2 same|diff`, times
%.2f) -- what OriginalDataLoader(pairs_path=directory_output) reads.  Parsing, the three splits, analyze_clusters,
generate_token_dict and the four per-configuration counts follow the reference line for line.  Two differences,
both on purpose:

 * split_clusters_ratio and split_clusters_on_file (and parse_input_file's max_num_clusters subset) draw from
   generators seeded with `self.seed` (numpy.random.RandomState(seed) and random.Random(seed)); the reference
   draws from the unseeded global generators, so its split changes from run to run.  split_each_file is
   deterministic and identical.
 * the pairs are drawn on the GPU (abn_sample_pairs, csrc/sampler.hip) from O(cells) tables, not from the
   reference's dictionary of all ordered pairs of cells (sampler.py:444-472: K^2 entries for K cells).

THE DISTRIBUTION.  A cell c = (s, t) is a speaker and a cluster index with n_c >= 1 tokens; T_t is the token count
of type t; g is the type_sampling_mode function and f the spk_sampling_mode function, each one of
1, x, sqrt x, cbrt x, log(1 + x) ('1', 'f2', 'f', 'fcube', 'log'; f('1') maps 0 to 0); u_c = g(T_t) f(n_c).
(The reference normalises p_types and p_spk_types separately before it multiplies them: constants per
configuration, they drop out.)

  configuration  support                                        weight                    tokens
  Stype_Sspk     cells                                          g(T_t) f(n_c) [n_c >= 2]  two distinct tokens of c, uniform
  Stype_Dspk     ordered (a, b), same type, different speaker   g(T_t) f(n_a) f(n_b)      one of each, uniform
  Dtype_Sspk     unordered {a, b}, same speaker, other type     u_a u_b                   one of each; lower type first
  Dtype_Dspk     ordered (a, b), other speaker, other type      u_a u_b                   one of each; lower type first

This equals the reference's table for the first three configurations always, and for Dtype_Dspk whenever
spk_sampling_mode = '1' or no four cells (s, i), (s, j), (s', i), (s', j) all exist.  Where they do, the
reference writes its key (s, s', min, max) twice (sampler.py:469-472), the later write wins, and the tokens are
then drawn from the other pair of cells (:681-686): a key collision, NOT reproduced here.  explicit_table()
materialises the definition above for small inputs (tests, inspection); sample() never calls it.

THE TABLES (build_tables; include/abnet3_hip.h, abn_sampler_tables).  Weights are scaled integers:
  u~_c = max(1, rint(S_u u_c)),  S_u = (2^32 - 2K - 2) / sum_c u_c          (so that sum u~ < 2^32)
  f~_c = max(1, rint(S_f f(n_c))),  S_f = (2^32 - 2K - 2) / max_t sum_{c in t} f(n_c)
(sums by math.fsum: one correctly rounded value whatever the order).  Every marginal is then a product of two
32-bit quantities and every total fits 64 bits; a 128-bit Philox draw r is mapped onto a range M as
floor(r M / 2^128).  DESIGN.md section 5 derives how far the realised distribution can lie from the definition.
"""
import argparse
import codecs
import ctypes
import math
import os
import random
import warnings
from collections import defaultdict

import numpy as np

CONFIGS = ('Stype_Sspk', 'Stype_Dspk', 'Dtype_Sspk', 'Dtype_Dspk')
SAMPLING_MODES = ('1', 'f', 'f2', 'log', 'fcube')
PAIR_TYPE = {'Stype_Sspk': 'same', 'Stype_Dspk': 'same', 'Dtype_Sspk': 'diff', 'Dtype_Dspk': 'diff'}
EXPLICIT_TABLE_MAX_KEYS = 2000000
WEIGHT_RANGE = 1 << 32
DEFAULT_BLOCK = 256


def sampling_function(mode):
    """The function a sampling mode applies to a token count (sampler.py:378-387, :425-438), on float64 arrays.
    Mode '1' maps 0 to 0 as the speaker function does; a type never has 0 tokens."""
    mode = str(mode)
    if mode not in SAMPLING_MODES:
        raise AssertionError('Transformation not implemented: %r' % (mode,))
    return {'1': lambda x: (np.asarray(x, dtype=np.float64) != 0).astype(np.float64),
            'f2': lambda x: np.asarray(x, dtype=np.float64),
            'f': lambda x: np.sqrt(np.asarray(x, dtype=np.float64)),
            'fcube': lambda x: np.cbrt(np.asarray(x, dtype=np.float64)),
            'log': lambda x: np.log(1 + np.asarray(x, dtype=np.float64))}[mode]


def print_token(tok):
    return '{0} {1:.2f} {2:.2f}'.format(tok[0], tok[1], tok[2])


def read_spkid_file(spkid_file):
    spk = {}
    with open(spkid_file, 'r') as fh:
        for line in fh:
            fid, spkid = line.strip().split(' ')
            assert fid not in spk
            spk[fid] = spkid
    return spk


def read_spk_list(spk_file):
    with open(spk_file, 'r') as fh:
        return [line.strip() for line in fh]


class SamplerBuilder(object):
    """Sampler interface (sampler.py:23-64): batch_size, run ('never' | 'once' | 'always'), directory_output (the
    folder that receives train_pairs / dev_pairs), ratio_train_dev, seed."""

    def __init__(self, batch_size=8, run='once', input_file=None,
                 directory_output=None, ratio_train_dev=0.7, seed=0):
        super(SamplerBuilder, self).__init__()
        self.batch_size = batch_size
        self.run = run
        self.directory_output = directory_output
        self.seed = seed
        self.ratio_train_dev = ratio_train_dev
        assert self.run in ['never', 'once', 'always']

    def whoami(self):
        raise NotImplementedError('Unimplemented whoami for class:', self.__class__.__name__)

    def parse_input_file(self, input_file=None):
        raise NotImplementedError('Unimplemented parse_input_file for class:', self.__class__.__name__)

    def sample_batch(self):
        raise NotImplementedError('Unimplemented sample_batch for class:', self.__class__.__name__)


class DummySampler(SamplerBuilder):
    """For a dataloader that samples by itself: the gridsearch YAML needs a sampler (sampler.py:67-82)."""

    def __init__(self, *args, **kwargs):
        print("Warning. You're using the dummy sampler, it won't do anything")
        super().__init__()

    def whoami(self):
        return {'params': self.__dict__, 'class_name': self.__class__.__name__}

    def sample(self):
        print("Dummy sampler : not sampling anything.")


class SamplerPairs(SamplerBuilder):
    """Sampler interface based on pairs of similar words (sampler.py:84-89)."""

    def __init__(self, *args, **kwargs):
        super(SamplerPairs, self).__init__(*args, **kwargs)


class SamplerCluster(SamplerBuilder):
    """Sampler based on clusters of words (sampler.py:92-575).  std_file: the clusters; spkid_file: "<file>
    <speaker>" lines; spk_list_file: accepted and stored (the reference reads it and never uses it);
    type_sampling_mode / spk_sampling_mode: the functions applied to the type and speaker frequencies;
    split_method: 'clusters', 'files' or 'split_each_file'."""
    SPLIT_CLUSTERS = "clusters"
    SPLIT_FILES = "files"
    SPLIT_EACH_FILE = "split_each_file"
    SPLIT_METHODS = [SPLIT_CLUSTERS, SPLIT_FILES, SPLIT_EACH_FILE]

    def __init__(self, max_size_cluster=10, ratio_same_diff_spk=0.75,
                 ratio_same_diff_type=0.5,
                 type_sampling_mode='log', spk_sampling_mode='log',
                 std_file=None, spk_list_file=None, spkid_file=None,
                 max_num_clusters=None,
                 sample_batches=False,
                 num_total_sampled_pairs=None,
                 split_method=SPLIT_CLUSTERS,
                 *args, **kwargs):
        super(SamplerCluster, self).__init__(*args, **kwargs)
        self.max_size_cluster = max_size_cluster
        self.ratio_same_diff_spk = ratio_same_diff_spk
        self.ratio_same_diff_type = ratio_same_diff_type
        self.type_sampling_mode = type_sampling_mode
        self.spk_sampling_mode = spk_sampling_mode
        self.std_file = std_file
        self.spk_list_file = spk_list_file
        self.spkid_file = spkid_file
        self.max_num_clusters = max_num_clusters
        self.sample_batches = sample_batches
        self.num_total_sampled_pairs = num_total_sampled_pairs
        self.split_method = split_method
        assert split_method in self.SPLIT_METHODS

    def parse_input_file(self, input_file=None, max_num_clusters=None):
        """The clusters of a .classes file: "Class <id>" header, one "<file> <onset> <offset>" line per token, a
        blank line after each cluster (sampler.py:143-186).  max_num_clusters keeps a random subset."""
        with codecs.open(input_file, "r", "utf-8") as fh:
            lines = fh.readlines()
        clusters = []
        i = 0
        while i < len(lines):
            cluster = []
            tokens = lines[i].strip().split(" ")
            assert len(tokens) == 2, 'problem line {} '.format(i) + str(tokens)
            i = i + 1
            tokens = lines[i].strip().split(" ")
            assert len(tokens) == 3, "Empty class!"
            fid, t0, t1 = tokens
            cluster.append([fid, float(t0), float(t1)])
            new_class = False
            while not new_class:
                i = i + 1
                tokens = lines[i].strip().split(" ")
                if len(tokens) == 3:
                    fid, t0, t1 = tokens
                    cluster.append([fid, float(t0), float(t1)])
                else:
                    assert tokens == ['']
                    new_class = True
                    clusters.append(cluster)
                    i = i + 1
        if max_num_clusters is not None and 0 < max_num_clusters < len(clusters):
            clusters = random.Random(self.seed).sample(clusters, max_num_clusters)
        return clusters

    def split_clusters_ratio(self, clusters):
        """Clusters larger than max_size_cluster are split by the ratio, token by token; the others go whole to
        train or dev (sampler.py:188-228).  The draws come from numpy.random.RandomState(self.seed) -- the
        reference's come from the unseeded global generator."""
        rng = np.random.RandomState(self.seed)
        train_clusters, dev_clusters = [], []
        num_clusters = len(clusters)
        num_train = int(self.ratio_train_dev * num_clusters)
        train_idx = set(rng.choice(num_clusters, num_train, replace=False).tolist())
        for idx, cluster in enumerate(clusters):
            size_cluster = len(cluster)
            if self.max_size_cluster > 1 and self.max_size_cluster < size_cluster:
                num_train = int(self.ratio_train_dev * size_cluster)
                rand_idx = rng.permutation(range(size_cluster))
                train_clusters.append([cluster[j] for j in rand_idx[:num_train]])
                dev_clusters.append([cluster[j] for j in rand_idx[num_train:]])
            elif idx in train_idx:
                train_clusters.append(cluster)
            else:
                dev_clusters.append(cluster)
        return train_clusters, dev_clusters

    def split_clusters_on_file(self, clusters):
        """Every wav file goes to train or to dev as a whole (sampler.py:230-258).  The dev files are drawn by
        random.Random(self.seed) -- the reference's by the unseeded global generator."""
        files = list(self.spkid_from_file)
        num_files_test = int(len(files) * (1 - self.ratio_train_dev))
        dev_files = set(random.Random(self.seed).sample(files, num_files_test))
        train_clusters, dev_clusters = [], []
        for c in clusters:
            train_c = [[f, s, e] for f, s, e in c if f not in dev_files]
            dev_c = [[f, s, e] for f, s, e in c if f in dev_files]
            if train_c:
                train_clusters.append(train_c)
            if dev_c:
                dev_clusters.append(dev_c)
        return train_clusters, dev_clusters

    def split_each_file(self, clusters):
        """The beginning of each file goes to train, its end to dev: a token is dev when its onset lies beyond
        ratio_train_dev x (the file's largest offset) (sampler.py:260-293).  Deterministic."""
        len_files = defaultdict(int)
        for c in clusters:
            for f, s, e in c:
                len_files[f] = max(len_files[f], e)
        train_threshold = {f: len_files[f] * self.ratio_train_dev for f in len_files}
        train_clusters, dev_clusters = [], []
        for c in clusters:
            train_c = [[f, s, e] for f, s, e in c if not s > train_threshold[f]]
            dev_c = [[f, s, e] for f, s, e in c if s > train_threshold[f]]
            if train_c:
                train_clusters.append(train_c)
            if dev_c:
                dev_clusters.append(dev_c)
        return train_clusters, dev_clusters

    def analyze_clusters(self, clusters, get_spkid_from_fid=None):
        """The description sampling works from (sampler.py:296-350): tokens, tokens_type, tokens_speaker, types
        (tokens per cluster), speakers {speaker: tokens}, speakers_types {speaker: clusters it appears in},
        types_speakers (speakers per cluster).  Without a map a file is its own speaker."""
        if get_spkid_from_fid is None:
            class MyDict(dict):
                def __missing__(self, key):
                    return key
            get_spkid_from_fid = MyDict()
        tokens = [f for c in clusters for f in c]
        nb_unique_tokens = len(set((a, b, c) for a, b, c in tokens))
        if len(tokens) != nb_unique_tokens:
            print("Warning : Your dataset has %s duplicates" % (len(tokens) - nb_unique_tokens))
        tokens_type = [i for i, c in enumerate(clusters) for f in c]
        tokens_speaker = [get_spkid_from_fid[f[0]] for f in tokens]
        types = [len(c) for c in clusters]
        speakers = {}
        names, counts = np.unique(tokens_speaker, return_counts=True) if tokens else ([], [])
        for spk, n in zip(names, counts):
            speakers[spk] = int(n)
        speakers_types = {spk: 0 for spk in speakers}
        types_speakers = []
        for c in clusters:
            cluster_speakers = np.unique([get_spkid_from_fid[f[0]] for f in c])
            for spk in cluster_speakers:
                speakers_types[spk] = speakers_types[spk] + 1
            types_speakers.append(len(cluster_speakers))
        return {'tokens': tokens, 'tokens_type': tokens_type, 'tokens_speaker': tokens_speaker, 'types': types,
                'speakers': speakers, 'speakers_types': speakers_types, 'types_speakers': types_speakers}

    def generate_token_dict(self, std_descr):
        """{(type, speaker): [token ids]} (sampler.py:475-484)."""
        tokens = defaultdict(list)
        for tok_id, (t, s) in enumerate(zip(std_descr['tokens_type'], std_descr['tokens_speaker'])):
            tokens[(t, s)].append(tok_id)
        return tokens

    def type_speaker_sampling_p(self, std_descr=None, type_sampling_mode='f', spk_sampling_mode='f'):
        """{configuration: {key: probability}} as the reference returns it (sampler.py:486-569), from
        explicit_table: small inputs only, and with this module's Dtype_Dspk (see the module docstring)."""
        out = {}
        for config in CONFIGS:
            keys, p = explicit_table(std_descr, config, type_sampling_mode, spk_sampling_mode)
            out[config] = dict(zip(keys, p.tolist()))
        return out


def pair_counts(num_samples, ratio_same_diff_spk, ratio_same_diff_type):
    """The four per-configuration counts of sample_batch, int() truncations included (sampler.py:634-639)."""
    num_same_spk = int((num_samples) * (1 - ratio_same_diff_spk))
    num_diff_spk = num_samples - num_same_spk
    return {'Stype_Sspk': int(num_same_spk * (1 - ratio_same_diff_type)),
            'Stype_Dspk': int(num_diff_spk * (1 - ratio_same_diff_type)),
            'Dtype_Sspk': int(num_same_spk * (ratio_same_diff_type)),
            'Dtype_Dspk': int(num_diff_spk * (ratio_same_diff_type))}


def cells_of(descr):
    """The cells of a description in T order (type, then speaker index): speaker names (sorted: the index is the
    rank), and per cell its speaker index, type, and token ids (ascending)."""
    names, spk_of_tok = np.unique(np.asarray(descr['tokens_speaker'], dtype=object).astype(str), return_inverse=True)
    typ_of_tok = np.asarray(descr['tokens_type'], dtype=np.int64)
    nspk = len(names)
    cell_key = typ_of_tok * nspk + spk_of_tok
    order = np.argsort(cell_key, kind='stable')
    keys, first, counts = np.unique(cell_key[order], return_index=True, return_counts=True)
    return {'speakers': [str(s) for s in names], 'spk': (keys % nspk).astype(np.int32), 'type': (keys // nspk).astype(np.int32),
            'count': counts.astype(np.int64), 'tok_beg': np.append(first, len(order)).astype(np.int32),
            'toks': order.astype(np.int32), 'n_type': len(descr['types'])}


def cell_weights(cells, type_sampling_mode, spk_sampling_mode):
    """(u_c, f_c) in float64, T order."""
    g, f = sampling_function(type_sampling_mode), sampling_function(spk_sampling_mode)
    type_tokens = np.bincount(cells['type'], weights=cells['count'], minlength=cells['n_type'])
    fw = f(cells['count'])
    return g(type_tokens)[cells['type']] * fw, fw


def quantise(w, denom, K):
    """max(1, rint(S w)) as uint64, S = (2^32 - 2K - 2) / denom."""
    scale = float(WEIGHT_RANGE - 2 * K - 2) / denom
    return np.maximum(np.rint(scale * w), 1.0).astype(np.uint64)


def build_tables(descr, type_sampling_mode='log', spk_sampling_mode='log'):
    """abn_sample_pairs' tables as host numpy arrays, keyed by the fields of abn_sampler_tables (plus 'speakers',
    'u_t' and the sizes).  O(cells + tokens) memory and time."""
    cells = cells_of(descr)
    K = len(cells['spk'])
    if K < 1 or K >= (1 << 24):
        raise ValueError('build_tables: %d cells, 1 .. 2^24 - 1 supported' % K)
    n_spk, n_type = len(cells['speakers']), cells['n_type']
    u_w, f_w = cell_weights(cells, type_sampling_mode, spk_sampling_mode)
    spk_t, type_t = cells['spk'], cells['type']
    type_beg = np.searchsorted(type_t, np.arange(n_type + 1)).astype(np.int32)
    f_type_w = [math.fsum(f_w[type_beg[t]:type_beg[t + 1]].tolist()) for t in range(n_type)]
    u_t = quantise(u_w, math.fsum(u_w.tolist()), K)
    f_t = quantise(f_w, max(f_type_w), K)
    assert int(u_t.sum()) < WEIGHT_RANGE
    cum_u_t, cum_f_t = np.cumsum(u_t, dtype=np.uint64), np.cumsum(f_t, dtype=np.uint64)

    def group_totals(cum, beg):                    # per-group sums from an inclusive running sum (groups may be empty)
        edge = np.concatenate([[np.uint64(0)], cum])[beg]
        return edge[1:] - edge[:-1]
    F_type, U_type = group_totals(cum_f_t, type_beg), group_totals(cum_u_t, type_beg)
    assert int(F_type.max()) < WEIGHT_RANGE
    s2t = np.lexsort((type_t, spk_t)).astype(np.int32)
    spk_s, type_s, u_s = spk_t[s2t], type_t[s2t], u_t[s2t]
    spk_beg = np.searchsorted(spk_s, np.arange(n_spk + 1)).astype(np.int32)
    cum_u_s = np.cumsum(u_s, dtype=np.uint64)
    U_spk = group_totals(cum_u_s, spk_beg)
    cum_spk = np.cumsum(U_spk, dtype=np.uint64)
    U = cum_spk[-1]
    m = np.empty((4, K), dtype=np.uint64)
    m[0] = u_t * (cells['count'] >= 2).astype(np.uint64)
    m[1] = u_t * (F_type[type_t] - f_t)
    m[2] = u_s * (U_spk[spk_s] - u_s)
    m[3] = u_s * (U - U_spk[spk_s] - U_type[type_s] + u_s)
    cum_m = np.cumsum(m, axis=1, dtype=np.uint64)
    return {'speakers': cells['speakers'], 'n_cells': K, 'n_spk': n_spk, 'n_type': n_type, 'n_tok': len(cells['toks']),
            'total': cum_m[:, -1].copy(), 'spk_t': spk_t, 'type_t': type_t, 'type_beg': type_beg,
            'u_t': u_t.astype(np.uint32), 'f_t': f_t.astype(np.uint32), 'cum_u_t': cum_u_t, 'cum_f_t': cum_f_t,
            'tok_beg': cells['tok_beg'], 'toks': cells['toks'], 'spk_s': spk_s, 'type_s': type_s, 's2t': s2t,
            'spk_beg': spk_beg, 'u_s': u_s.astype(np.uint32), 'cum_u_s': cum_u_s, 'cum_spk': cum_spk, 'cum_m': cum_m}


def explicit_table(descr, config, type_sampling_mode='log', spk_sampling_mode='log', max_keys=EXPLICIT_TABLE_MAX_KEYS,
                   return_cells=False):
    """(keys, probabilities) of one configuration exactly as the module docstring defines it, in float64, with
    the reference's key tuples: (spk, type), (spk, spk2, type), (spk, min type, max type),
    (spk, spk2, min type, max type).  Two ordered pairs of cells share a Dtype_Dspk key where four cells
    (s, i), (s, j), (s', i), (s', j) exist: their probabilities add up under that key.  return_cells=True gives
    the support itself instead of keys: ((spk_a, type_a), (spk_b, type_b)) per entry, a the first cell.
    For tests and inspection: the table holds up to (cells)^2 entries and is refused when that exceeds max_keys.
    sample() never builds it."""
    if config not in CONFIGS:
        raise ValueError('unknown configuration %r' % (config,))
    cells = cells_of(descr)
    K = len(cells['spk'])
    if K * K > max_keys and config != 'Stype_Sspk':
        raise ValueError('explicit_table: %d cells give up to %d keys, more than max_keys = %d; the table is for small '
                         'inputs (sample() draws from O(cells) tables instead)' % (K, K * K, max_keys))
    u, f = cell_weights(cells, type_sampling_mode, spk_sampling_mode)
    name, spk, typ, cnt = cells['speakers'], cells['spk'], cells['type'], cells['count']
    cell = [(name[spk[c]], int(typ[c])) for c in range(K)]
    pairs, w = [], []
    if config == 'Stype_Sspk':
        for c in range(K):
            pairs.append((cell[c], cell[c]))
            w.append(u[c] if cnt[c] >= 2 else 0.0)
    else:
        for a in range(K):
            for b in range(K):
                same_spk, same_type = spk[a] == spk[b], typ[a] == typ[b]
                if config == 'Stype_Dspk' and same_type and not same_spk:
                    pairs.append((cell[a], cell[b]))
                    w.append(u[a] * f[b])
                elif config == 'Dtype_Sspk' and same_spk and typ[a] < typ[b]:
                    pairs.append((cell[a], cell[b]))
                    w.append(u[a] * u[b])
                elif config == 'Dtype_Dspk' and not same_spk and not same_type:
                    pairs.append((cell[a], cell[b]))
                    w.append(u[a] * u[b])
    w = np.asarray(w, dtype=np.float64)
    total = math.fsum(w.tolist())
    p = w / total if total > 0 else w
    if return_cells:
        return pairs, p
    merged = {}
    for ((sa, ta), (sb, tb)), v in zip(pairs, p.tolist()):
        key = {'Stype_Sspk': (sa, ta), 'Stype_Dspk': (sa, sb, ta), 'Dtype_Sspk': (sa, min(ta, tb), max(ta, tb)),
               'Dtype_Dspk': (sa, sb, min(ta, tb), max(ta, tb))}[config]
        merged[key] = merged.get(key, 0.0) + v
    return list(merged), np.asarray(list(merged.values()), dtype=np.float64)


class DeviceTables(object):
    """build_tables' arrays in ONE device buffer, and the abn_sampler_tables that points into it."""

    def __init__(self, tables, device=None):
        import torch
        from . import _lib
        self.host = tables
        offsets, size = {}, 0
        for name in _lib.SamplerTables.POINTERS:
            offsets[name] = size
            size += (tables[name].nbytes + 15) // 16 * 16
        blob = np.zeros(size, dtype=np.uint8)
        for name in _lib.SamplerTables.POINTERS:
            raw = np.ascontiguousarray(tables[name]).view(np.uint8).reshape(-1)
            blob[offsets[name]:offsets[name] + raw.size] = raw
        self.buffer = torch.from_numpy(blob).to(device if device is not None else 'cuda')
        self.nbytes = size
        self.struct = _lib.SamplerTables()
        for name in ('n_cells', 'n_spk', 'n_type', 'n_tok'):
            setattr(self.struct, name, int(tables[name]))
        for q in range(4):
            self.struct.total[q] = int(tables['total'][q])
        for name in _lib.SamplerTables.POINTERS:
            setattr(self.struct, name, self.buffer.data_ptr() + offsets[name])


def sample_pairs_device(dev_tables, counts, seed, block=DEFAULT_BLOCK, out=None):
    """abn_sample_pairs: (tok1, tok2 int32, key int64) device tensors of sum(counts) elements, configuration after
    configuration, in draw order.  out: (toks int32 [2, n], key int64 [n]) to write into instead of new tensors."""
    import torch
    from . import _lib
    lib = _lib.load()
    n = (ctypes.c_int64 * 4)(*[int(c) for c in counts])
    total = sum(int(c) for c in counts)
    dev = dev_tables.buffer.device
    if out is None:
        toks = torch.empty(2, total, dtype=torch.int32, device=dev)
        key = torch.empty(total, dtype=torch.int64, device=dev)
    else:
        toks, key = out
        if (toks.dtype, key.dtype, tuple(toks.shape), tuple(key.shape)) != (torch.int32, torch.int64, (2, total), (total,)):
            raise ValueError('sample_pairs_device: out must be int32 [2, %d] and int64 [%d]' % (total, total))
        _lib.require_device(toks, key)
    with torch.cuda.device(dev):
        _lib.check(lib.abn_sample_pairs(ctypes.byref(dev_tables.struct), n, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                        _lib.ptr(toks[0]), _lib.ptr(toks[1]), _lib.ptr(key), int(block), _lib.stream()),
                   'abn_sample_pairs')
    return toks[0], toks[1], key


def draw_pairs(descr, counts, type_sampling_mode, spk_sampling_mode, seed, block=DEFAULT_BLOCK):
    """The pairs of one data set in their final (shuffled) order: (tok1, tok2, configuration index) host arrays.
    A configuration with empty support yields no pairs and one warning."""
    import torch
    counts = [int(counts[c]) for c in CONFIGS]
    if not len(descr['tokens_type']):
        if sum(counts):
            warnings.warn('this data set has no token: no pairs')
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    tables = build_tables(descr, type_sampling_mode, spk_sampling_mode)
    for q, config in enumerate(CONFIGS):
        if counts[q] > 0 and int(tables['total'][q]) == 0:
            warnings.warn('%s: no admissible pair of cells in this data set, its %d pairs are left out' % (config, counts[q]))
            counts[q] = 0
    dev_tables = DeviceTables(tables)
    tok1, tok2, key = sample_pairs_device(dev_tables, counts, seed, block)
    order = torch.sort(key, stable=True).indices                  # ascending key, ties by index
    config = torch.bucketize(order, torch.tensor(np.cumsum(counts)[:3], device=key.device), right=True)
    return tok1[order].cpu().numpy(), tok2[order].cpu().numpy(), config.cpu().numpy()


class SamplerClusterSiamese(SamplerCluster):
    """Sampler for a Siamese network based on clusters of words (sampler.py:578-878)."""

    def __init__(self, *args, **kwargs):
        super(SamplerClusterSiamese, self).__init__(*args, **kwargs)

    def whoami(self):
        return {'params': self.__dict__, 'class_name': self.__class__.__name__}

    def sample_batch(self, descr, num_samples=5012, seed=None):
        """{configuration: [(tok1, tok2), ...]} with the reference's counts per configuration
        (sampler.py:589-688), drawn on the GPU; within a configuration the pairs keep their shuffled order."""
        counts = pair_counts(num_samples, self.ratio_same_diff_spk, self.ratio_same_diff_type)
        tok1, tok2, config = draw_pairs(descr, counts, self.type_sampling_mode, self.spk_sampling_mode,
                                        self.seed if seed is None else seed)
        return {name: [(int(a), int(b)) for a, b in zip(tok1[config == q], tok2[config == q])]
                for q, name in enumerate(CONFIGS)}

    def write_tokens(self, descr=None, batch_size=8, num_samples=0, out_dir=None, seed=0,
                     type_sampling_mode=None, spk_sampling_mode=None):
        """Draws num_samples pairs and writes them: one `dataset` file, or pair_<i>.batch files of batch_size
        lines with sample_batches (sampler.py:690-742, its range(1, num_samples // batch_size) included).  The
        sampling modes default to the instance's."""
        counts = pair_counts(num_samples, self.ratio_same_diff_spk, self.ratio_same_diff_type)
        tok1, tok2, config = draw_pairs(descr, counts,
                                        self.type_sampling_mode if type_sampling_mode is None else type_sampling_mode,
                                        self.spk_sampling_mode if spk_sampling_mode is None else spk_sampling_mode, seed)
        printed = [print_token(tok) for tok in descr['tokens']]
        kind = [PAIR_TYPE[c] for c in CONFIGS]
        lines = ['%s %s %s\n' % (printed[a], printed[b], kind[q]) for a, b, q in zip(tok1, tok2, config)]
        if self.sample_batches:
            for idx in range(1, int(num_samples // batch_size)):
                with open(os.path.join(out_dir, 'pair_' + str(idx) + '.batch'), 'w') as fh:
                    fh.writelines(lines[(idx - 1) * batch_size:idx * batch_size])
        else:
            with open(os.path.join(out_dir, 'dataset'), 'w') as fh:
                fh.write(''.join(lines))
        return len(lines)

    def export_pairs(self, out_dir=None, descr=None, type_sampling_mode=None, spk_sampling_mode=None,
                     seed=0, batch_size=8, num_samples=None):
        """num_samples None: num (num - 1) / 2 for num = the fewest tokens any speaker has (sampler.py:766-768).
        The sampling modes given here are the ones drawn with (None: the instance's); the batch size is the
        instance's, as in the reference."""
        if num_samples is None:
            num = np.min(list(descr['speakers'].values()))
            num_samples = num * (num - 1) / 2
        return self.write_tokens(descr=descr, batch_size=self.batch_size, num_samples=num_samples,
                                 out_dir=out_dir, seed=seed, type_sampling_mode=type_sampling_mode,
                                 spk_sampling_mode=spk_sampling_mode)

    def split(self, clusters):
        if self.split_method == self.SPLIT_CLUSTERS:
            return self.split_clusters_ratio(clusters)
        if self.split_method == self.SPLIT_FILES:
            return self.split_clusters_on_file(clusters)
        if self.split_method == self.SPLIT_EACH_FILE:
            return self.split_each_file(clusters)
        raise ValueError("split method doesn't exist")

    def sample(self):
        """Cluster file + speaker map -> train_pairs / dev_pairs under directory_output (sampler.py:775-878).
        The dev set is drawn with seed + 1."""
        get_spkid_from_fid = read_spkid_file(self.spkid_file)
        self.spkid_from_file = get_spkid_from_fid
        clusters = self.parse_input_file(self.std_file, self.max_num_clusters)
        train_clusters, dev_clusters = self.split(clusters)
        train_descr = self.analyze_clusters(train_clusters, get_spkid_from_fid)
        dev_descr = self.analyze_clusters(dev_clusters, get_spkid_from_fid)
        train_pairs_dir = os.path.join(self.directory_output, 'train_pairs')
        dev_pairs_dir = os.path.join(self.directory_output, 'dev_pairs')
        os.makedirs(train_pairs_dir, exist_ok=True)
        os.makedirs(dev_pairs_dir, exist_ok=True)
        if self.num_total_sampled_pairs is not None:
            num_samples_train = int(self.num_total_sampled_pairs * self.ratio_train_dev)
            num_samples_dev = self.num_total_sampled_pairs - num_samples_train
        else:
            num_samples_train, num_samples_dev = None, None
        n_train = self.export_pairs(out_dir=train_pairs_dir, descr=train_descr, seed=self.seed,
                                    batch_size=self.batch_size, num_samples=num_samples_train)
        n_dev = self.export_pairs(out_dir=dev_pairs_dir, descr=dev_descr, seed=self.seed + 1,
                                  batch_size=self.batch_size, num_samples=num_samples_dev)
        print('SamplerClusterSiamese: %d clusters -> %d train pairs, %d dev pairs in %s'
              % (len(clusters), n_train, n_dev, self.directory_output))


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.sampler', description=__doc__.split('\n\n')[0])
    ap.add_argument('std_file', help='word clusters (.classes)')
    ap.add_argument('spkid_file', help='"<file id> <speaker id>" lines')
    ap.add_argument('directory_output', help='receives train_pairs/ and dev_pairs/')
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--ratio_train_dev', type=float, default=0.7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--max_size_cluster', type=int, default=10)
    ap.add_argument('--ratio_same_diff_spk', type=float, default=0.75)
    ap.add_argument('--ratio_same_diff_type', type=float, default=0.5)
    ap.add_argument('--type_sampling_mode', default='log', choices=SAMPLING_MODES)
    ap.add_argument('--spk_sampling_mode', default='log', choices=SAMPLING_MODES)
    ap.add_argument('--spk_list_file', default=None)
    ap.add_argument('--max_num_clusters', type=int, default=None)
    ap.add_argument('--sample_batches', action='store_true')
    ap.add_argument('--num_total_sampled_pairs', type=int, default=None)
    ap.add_argument('--split_method', default=SamplerCluster.SPLIT_CLUSTERS, choices=SamplerCluster.SPLIT_METHODS)
    SamplerClusterSiamese(**vars(ap.parse_args(argv))).sample()


if __name__ == '__main__':
    main()
