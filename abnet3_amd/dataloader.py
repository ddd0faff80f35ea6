"""Pair -> frame batch builders on MI355X: the surface of abnet3/dataloader.py.

Mirrors (file:line relative to the reference checkout)
  DataLoader            abnet3/dataloader.py:29-40
  OriginalDataLoader    abnet3/dataloader.py:43-352  (load_frames_from_pairs,
                        batch_iterator, temporal coherence pairs)
  FramesDataLoader      abnet3/dataloader.py:580-739 (align once, frame batches)
  PairsDataLoader       abnet3/dataloader.py:355-546 (a k-nearest-neighbour pairs file instead of the
                        sampler's clusters: discovery.py writes one)
What changes underneath: the whole feature corpus lives in HBM as ONE
[frames, D] tensor (DeviceCorpus); "same" word pairs are DTW-aligned on the GPU
in batched launches (utils.dtw_align_batch) and cached, since the alignment of a
pair never changes between epochs (the reference recomputes it every epoch,
dataloader.py:189); frames are gathered on the device (abn_gather_rows), so the
iterator yields device tensors and the trainer's .cuda() is a no-op.  Batch
composition, order, the seed-0 permutation and label dtypes follow the
reference statement by statement.
"""
import os
import random
from collections import defaultdict

import numpy as np
import torch

from . import _lib, parallel
from .utils import (Features_Accessor, dtw_align_batch, group_pairs, read_dataset,
                    read_spkid_file)


class DataLoader:

    def batch_iterator(self, train_mode=True):
        raise NotImplementedError("You must implement batch iterator" +
                                  " in DataLoader class.")

    def whoami(self):
        raise NotImplementedError("You must implement whoami in DataLoader class")


def gather_rows(table, idx):
    """table[idx] on the device (feat[path, :], dataloader.py:204-205)."""
    lib = _lib.load()
    _lib.require_tensor('gather_rows', 'table', table, torch.float32, 2)
    if not isinstance(idx, torch.Tensor) or idx.dim() != 1:
        raise ValueError('gather_rows: idx must be one row of table row numbers (a 1-d tensor)')
    idx = idx.to(torch.int64).contiguous()
    _lib.require_device(idx)
    out = torch.empty(idx.numel(), table.shape[1], dtype=torch.float32, device=table.device)
    _lib.check(lib.abn_gather_rows(_lib.ptr(table), _lib.ptr(idx), idx.numel(),
                                   table.shape[1], _lib.ptr(out), _lib.stream()),
               'abn_gather_rows')
    return out


class DeviceCorpus(object):
    """Every utterance's frames as one [total_frames, D] float32 tensor in HBM,
    plus host-side row offsets and frame times (Features_Accessor semantics:
    a token is the frames with on <= t <= off, utils.py:127-131)."""

    def __init__(self, features, times):
        self.names = list(features.keys())
        self.offset, self.length, self.times = {}, {}, {}
        chunks, o = [], 0
        for k in self.names:
            f = np.ascontiguousarray(features[k], dtype=np.float32)
            self.offset[k], self.length[k] = o, f.shape[0]
            self.times[k] = np.asarray(times[k])
            chunks.append(f)
            o += f.shape[0]
        self.dim = chunks[0].shape[1]
        self.table = torch.from_numpy(np.concatenate(chunks, axis=0)).cuda()
        self.total = o
        self._init_lookup()

    @classmethod
    def from_table(cls, table, names, lengths, times):
        """The same corpus from features that are already in HBM (FeaturesGenerator.features_from_waves):
        `table` [sum(lengths), D] float32 on the device, utterance k = its rows
        [sum(lengths[:k]), sum(lengths[:k + 1])); times {name: [T] frame times}."""
        _lib.require_device(table)
        self = cls.__new__(cls)
        self.names = list(names)
        self.offset, self.length, self.times = {}, {}, {}
        o = 0
        for k, n in zip(self.names, lengths):
            self.offset[k], self.length[k] = o, int(n)
            self.times[k] = np.asarray(times[k])
            o += int(n)
        assert o == table.shape[0], 'lengths do not add up to the table'
        self.dim = table.shape[1]
        self.table = table
        self.total = o
        self._init_lookup()
        return self

    def _init_lookup(self):
        self._tokens = {}                    # (name, on, off) -> (first global row, frames)
        self._sorted = {}                    # name -> are its frame times non-decreasing (then: binary search)

    def _name(self, f):
        b = f.encode('UTF-8') if isinstance(f, str) else f
        return b if b in self.offset else f

    def token(self, f, on, off):
        """(first global row, number of frames) of the token (f, on, off)."""
        key = (f, on, off)
        hit = self._tokens.get(key)
        if hit is not None:
            return hit
        k = self._name(f)
        t = self.times[k]
        srt = self._sorted.get(k)
        if srt is None:
            srt = self._sorted[k] = bool(len(t) < 2 or np.all(t[1:] >= t[:-1]))
        if srt:
            # np.where((t >= on) & (t <= off)) of sorted times is one run of frames: two binary searches
            lo, hi = int(np.searchsorted(t, on, 'left')), int(np.searchsorted(t, off, 'right'))
            out = (self.offset[k] + lo, hi - lo) if hi > lo else (self.offset[k], 0)
        else:
            ind = Features_Accessor.get_indices_between(t, on, off)
            if len(ind) == 0:
                out = (self.offset[k], 0)
            else:
                assert ind[-1] - ind[0] + 1 == len(ind), 'frame times must be sorted'
                out = (self.offset[k] + int(ind[0]), len(ind))
        self._tokens[key] = out
        return out

    def token_frames(self, f, frame_on, frame_off):
        k = self._name(f)
        lo, hi, _ = slice(frame_on, frame_off).indices(self.length[k])
        return self.offset[k] + lo, max(0, hi - lo)


class AlignCache(object):
    """The DTW alignments of a loader: key (f1, s1, e1, f2, s2, e2, frames) -> (idx1, idx2) global-row index tensors on
    the device, or None for a dropped pair (an empty token, a NaN distance: dataloader.py:188-191).  A batched DTW call
    returns its paths as two FLAT device tensors; the cache keeps those and, per key, where its path sits in them
    (`span`: chunk, first element, length) -- the per-key views are made when somebody asks for one (the iterator, the
    tests), not for all of a dataset's 10^4 pairs at once, and a batch plan gathers straight from the flat tensors."""

    def __init__(self):
        self.span = {}
        self.chunks = []                     # [(g1, g2)]: flat int64 device tensors of one share of one align_pairs call

    def add_chunk(self, g1, g2):
        self.chunks.append((g1, g2))
        return len(self.chunks) - 1

    def compact(self):
        """All chunks as ONE.  The iterator path calls align_pairs per batch -- a chunk per call, thousands of small tensors
        -- and every plan build walks and concatenates all of them: once compacted, a plan build finds one tensor to gather
        from (views handed out earlier keep their own storage alive)."""
        if len(self.chunks) <= 1:
            return
        base = np.concatenate(([0], np.cumsum([c[0].numel() for c in self.chunks]))).astype(np.int64)
        g1 = torch.cat([c[0] for c in self.chunks])
        g2 = torch.cat([c[1] for c in self.chunks])
        self.span = {k: (None if sp is None else (0, int(base[sp[0]]) + sp[1], sp[2])) for k, sp in self.span.items()}
        self.chunks = [(g1, g2)]

    def put(self, key, chunk, start, n):
        self.span[key] = (chunk, start, n) if n else None

    def _views(self, sp):
        if sp is None:
            return None
        c, st, n = sp
        g1, g2 = self.chunks[c]
        return g1[st:st + n], g2[st:st + n]

    def __contains__(self, key):
        return key in self.span

    def __len__(self):
        return len(self.span)

    def __getitem__(self, key):
        return self._views(self.span[key])

    def get(self, key, default=None):
        if key not in self.span:
            return default
        return self._views(self.span[key])

    def items(self):
        for key, sp in self.span.items():
            yield key, self._views(sp)

    def keys(self):
        return self.span.keys()


class BatchPlan(object):
    """Every batch of a dataset as index lists in HBM: batch b is the frame pairs
    [offsets[b], offsets[b + 1]) of (idx1, idx2, labels) -- global rows of `table` and the pair labels,
    already in the order the reference's iterator would yield them (vstack order, then the seed-0
    permutation, abnet3/dataloader.py:248-255) -- and `order` is the batch ids one pass visits (this
    rank's share).  A trainer that understands plans (TrainerSiamese) gathers batch b with ONE launch
    (abn_gather_pairs) into the buffers of a captured step; materialise(b) gives the tensors the plain
    iterator yields."""

    def __init__(self, table, idx1, idx2, labels, offsets, order, has_arrays=None):
        self.table, self.idx1, self.idx2, self.labels = table, idx1, idx2, labels
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.order = [int(b) for b in order]
        # batches none of whose word pairs survived (the reference's np.vstack([]) raises ValueError,
        # dataloader.py:247) as opposed to batches of zero frames (empty tokens: an empty batch comes out)
        self.has_arrays = has_arrays

    def __len__(self):
        return len(self.order)

    def span(self, b):
        """(first frame pair, number of frame pairs) of batch b"""
        return int(self.offsets[b]), int(self.offsets[b + 1] - self.offsets[b])

    def materialise(self, b):
        first, n = self.span(b)
        if n == 0 and (self.has_arrays is None or not self.has_arrays[b]):
            raise ValueError('need at least one array to concatenate')
        sl = slice(first, first + n)
        return (gather_rows(self.table, self.idx1[sl]), gather_rows(self.table, self.idx2[sl]), self.labels[sl])

    def __iter__(self):
        for b in self.order:
            yield self.materialise(b)


class OriginalDataLoader(DataLoader):
    """Loads the pairs file created by the sampler, creates the frame pairs and
    shuffles inside the batches (abnet3/dataloader.py:43-352)."""

    TCL_DISTANCE_SAME = [1]
    TCL_DISTANCES_DIFF = [15, 20, 25, 30]

    def __init__(self, pairs_path, features_path, num_max_minibatches=1000,
                 seed=None, batch_size=8, shuffle_between_epochs=False,
                 align_different_words=False,
                 tcl=0.0, tcl_seed=None):
        assert 0 <= tcl < 1
        self.pairs_path = pairs_path
        self.features_path = features_path
        self.statistics_training = defaultdict(int)
        self.seed = seed
        self.num_max_minibatches = num_max_minibatches
        self.batch_size = batch_size
        self.features = None          # DeviceCorpus
        self.shuffle_between_epochs = shuffle_between_epochs
        self.align_different_words = align_different_words
        self.tcl = tcl
        # None: the temporal-coherence pairs are drawn per batch from `random`, like the reference's; an integer: on the
        # device by abn_tcl_pairs with this seed, for the whole pass at once (plan(True) then has the mixed batches)
        self.tcl_seed = tcl_seed
        self.tcl_epoch = 0            # passes drawn so far: the generator's epoch word
        self.train_files = None
        self.pairs = {'train': None, 'dev': None}
        self._align = AlignCache()    # (f1,s1,e1,f2,s2,e2,frames) -> (idx1, idx2) | None

    def __getstate__(self):
        return (self.pairs_path, self.features_path, self.statistics_training,
                self.seed, self.num_max_minibatches, self.batch_size)

    def whoami(self):
        return {'params': self.__getstate__(),
                'class_name': self.__class__.__name__}

    # -- data ----------------------------------------------------------------
    def set_data(self, features, times, train_pairs=None, dev_pairs=None):
        """In-memory injection of what load_data() reads from disk: features
        {utt: [T, D]}, times {utt: [T]}, pairs [(f1,s1,e1,f2,s2,e2,type), ...]."""
        self.features = DeviceCorpus(features, times)
        if train_pairs is not None:
            self.pairs['train'] = list(train_pairs)
        if dev_pairs is not None:
            self.pairs['dev'] = list(dev_pairs)
        if self.pairs['train'] is not None:
            self.train_files = list({p[0] for p in self.pairs['train']} |
                                    {p[3] for p in self.pairs['train']})

    def load_data(self):
        """Load only once the features, and the pairs (dataloader.py:125-145)."""
        if self.features is None:
            try:
                import h5features
            except ImportError:
                raise ImportError('features_path is an h5features file and the '
                                  'h5features package is not installed; use '
                                  'set_data() with in-memory arrays')
            with h5features.Reader(self.features_path, 'features') as fh:
                feats = fh.read()
            self.features = DeviceCorpus(feats.dict_features(), feats.dict_labels())
        if self.pairs['train'] is None:
            self.pairs['train'] = read_dataset(
                os.path.join(self.pairs_path, 'train_pairs/dataset'))
        if self.pairs['dev'] is None:
            self.pairs['dev'] = read_dataset(
                os.path.join(self.pairs_path, 'dev_pairs/dataset'))
        self.train_files = list({p[0] for p in self.pairs['train']} |
                                {p[3] for p in self.pairs['train']})

    # -- alignment -------------------------------------------------------------
    def _token(self, f, s, e, frames):
        return self.features.token_frames(f, s, e) if frames else self.features.token(f, s, e)

    # cells (sum of n1*n2) one batched DTW call may cover: bounds the call's workspace whatever the
    # size of the dataset; its [pairs, stride] path arrays (2 x int32) and what _align_chunk makes of
    # them (int64 copies, a mask) are bounded separately: ALIGN_PATH_BYTES per entry, ALIGN_PATH_BUDGET in all
    ALIGN_CELL_BUDGET = 1 << 30
    ALIGN_PATH_BYTES = 28
    ALIGN_PATH_BUDGET = 4 << 30

    shards_itself = True          # see parallel.py: the trainer must not shard again

    def _align_chunk(self, todo):
        """One batched DTW call for the keys in `todo`: (path lengths on the host,
        flat global-row index tensors g1, g2 on the device, concatenated in order)."""
        o1, n1, o2, n2 = [], [], [], []
        for f1, s1, e1, f2, s2, e2, fr in todo:
            a, b = self._token(f1, s1, e1, fr), self._token(f2, s2, e2, fr)
            o1.append(a[0]); n1.append(a[1]); o2.append(b[0]); n2.append(b[1])
        table = self.features.table
        res = dtw_align_batch(table, o1, n1, table, o2, n2)
        lens = res.path_len.cpu().numpy()
        dev = table.device
        mask = res.mask()
        g1 = (res.path1.long() + torch.tensor(o1, device=dev)[:, None])[mask]
        g2 = (res.path2.long() + torch.tensor(o2, device=dev)[:, None])[mask]
        return lens, g1, g2

    def align_pairs(self, same_pairs, frames=False, exchange=False):
        """DTW-aligns every not-yet-cached 'same' pair in batched GPU calls
        (get_dtw_alignment, dataloader.py:189), at most ALIGN_CELL_BUDGET cells per
        call.  Dropped pairs (NaN distance, dataloader.py:188-191) are cached as None.
        exchange=True under torch.distributed: the pairs are split over the ranks
        (pair k goes to rank k % R), each rank aligns its share and the index lists
        are all-gathered, so that every rank ends up with every alignment."""
        rank, ws = parallel.world()
        exchange = exchange and parallel.active()
        keys, queued = [], set()
        for p in same_pairs:
            key = tuple(p) + (frames,)
            if key in queued:
                continue
            f1, s1, e1, f2, s2, e2 = p
            if (s1 > e1) or (s2 > e2):
                continue
            keys.append(key)
            queued.add(key)
        if exchange:
            # The ranks' caches differ (an epoch of sharded batches fills them with rank-specific entries),
            # the pair list does not: agree on the work first -- a key is skipped only when EVERY rank holds
            # it -- so that all ranks cut the same list and nobody leaves before the collectives.
            have = np.array([k in self._align for k in keys], dtype=np.int64)
            have = parallel.all_reduce_min(have)
            todo = [k for k, h in zip(keys, have) if not h]
        else:
            todo = [k for k in keys if k not in self._align]
        if not todo:             # (with exchange: the same list on every rank, see above)
            return
        mine = todo[rank::ws] if exchange else todo
        lens_all, g1_all, g2_all = [], [], []
        chunk, cells, stride = [], 0, 0
        for key in mine + [None]:
            if key is not None:
                f1, s1, e1, f2, s2, e2, fr = key
                a, b = self._token(f1, s1, e1, fr)[1], self._token(f2, s2, e2, fr)[1]
                c = a * b
                st = max(stride, a + b - 1)
                # the [pairs, stride] path arrays (and the gather's temporaries) grow with pairs x the LONGEST
                # path of the chunk, not with the cells: one long token among many short pairs must not blow them up
                if not chunk or (cells + c <= self.ALIGN_CELL_BUDGET and
                                 (len(chunk) + 1) * st * self.ALIGN_PATH_BYTES <= self.ALIGN_PATH_BUDGET):
                    chunk.append(key)
                    cells += c
                    stride = st
                    continue
            if chunk:
                lens, g1, g2 = self._align_chunk(chunk)
                lens_all.append(lens); g1_all.append(g1); g2_all.append(g2)
            chunk, cells, stride = ([key], c, a + b - 1) if key is not None else ([], 0, 0)
        dev = self.features.table.device
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        lens = np.concatenate(lens_all) if lens_all else np.zeros(0, dtype=np.int32)
        g1 = torch.cat(g1_all) if g1_all else empty
        g2 = torch.cat(g2_all) if g2_all else empty
        if exchange:
            lens_r = parallel.all_gather_varlen(torch.from_numpy(lens.astype(np.int64)))
            g1_r = parallel.all_gather_varlen(g1)
            g2_r = parallel.all_gather_varlen(g2)
            shares = [(todo[r::ws], lens_r[r].cpu().numpy(), g1_r[r], g2_r[r]) for r in range(ws)]
        else:
            shares = [(mine, lens, g1, g2)]
        for keys, lens, g1, g2 in shares:
            lens = np.asarray(lens, dtype=np.int64)
            chunk = self._align.add_chunk(g1, g2)
            starts = np.cumsum(lens) - lens
            for key, st, ln in zip(keys, starts.tolist(), lens.tolist()):
                # ln == 0: an empty token or a NaN distance: the reference's try/except
                # drops the pair (dataloader.py:188-191)
                self._align.put(key, chunk, st, ln)

    def prefetch_alignments(self):
        """Aligns every 'same' pair of the train and dev sets up front, in one
        large batched launch each (what FramesDataLoader.load_all_frames does
        serially, dataloader.py:617-671)."""
        self.load_data()
        for mode in ('train', 'dev'):
            if self.pairs[mode]:
                self.align_pairs(group_pairs(self.pairs[mode])['same'], exchange=True)

    # -- batches ---------------------------------------------------------------
    def same_speaker(self, fid2spk, f1, f2):
        """+1 / -1 speaker label of a word pair.  The reference compares the two
        speaker STRINGS with `is` (dataloader.py:197,237): under CPython that is
        true when both tokens come from the same file (the same dict value), or
        when the ids are equal one-character strings (interned) -- two files of
        one multi-character speaker count as DIFFERENT speakers.  speaker_match =
        'identity' (default) reproduces that; 'equal' compares the ids."""
        a, b = fid2spk[f1], fid2spk[f2]
        if getattr(self, 'speaker_match', 'identity') == 'equal':
            return a == b
        return f1 == f2 or (a == b and len(a) <= 1)

    def frames_from_pairs_device(self, pairs, seed=0, frames=False, fid2spk=None):
        """load_frames_from_pairs (dataloader.py:166-261) producing device
        tensors: X1, X2 float32 [n, D], y float64 [n]; with fid2spk (the
        multitask loader) X1, X2, y_spk, y_phn."""
        self.align_pairs(pairs['same'], frames)
        dev = self.features.table.device
        idx1, idx2, ys, ys_spk = [], [], [], []
        d1, d2 = [], []                       # diff pairs: host index arrays, ONE upload per batch
        for f1, s1, e1, f2, s2, e2 in pairs['same']:
            if (s1 > e1) or (s2 > e2):
                continue
            al = self._align.get((f1, s1, e1, f2, s2, e2, frames))
            if al is None:
                continue
            self.statistics_training['SameType'] += 1
            idx1.append(al[0]); idx2.append(al[1])
            ys.append(np.ones(len(al[0])))
            if fid2spk:
                same = self.same_speaker(fid2spk, f1, f2)
                ys_spk.append((1 if same else -1) * np.ones(len(al[0])))
                self.statistics_training['SameTypeSameSpk' if same else 'SameTypeDiffSpk'] += 1
        for f1, s1, e1, f2, s2, e2 in pairs['diff']:
            if (s1 > e1) or (s2 > e2):
                continue
            (a0, n1), (b0, n2) = self._token(f1, s1, e1, frames), self._token(f2, s2, e2, frames)
            if self.align_different_words:
                # the shorter word is stretched along the diagonal (:216-225);
                # key=len keeps the FIRST on ties, like min()/max()
                if n2 < n1:
                    mn0, mnl, mx0, mxl = b0, n2, a0, n1
                else:
                    mn0, mnl = a0, n1
                    mx0, mxl = (b0, n2) if n2 > n1 else (a0, n1)
                mapping = np.rint(np.linspace(0, mnl - 1, num=mxl)).astype(int)
                w1 = mx0 + np.arange(mxl)
                w2 = mn0 + mapping
            else:
                m = min(n1, n2)
                w1 = a0 + np.arange(m)
                w2 = b0 + np.arange(m)
            d1.append(w1.astype(np.int64))
            d2.append(w2.astype(np.int64))
            ys.append(-1 * np.ones(min(n1, n2)))
            self.statistics_training['DiffType'] += 1
            if fid2spk:
                same = self.same_speaker(fid2spk, f1, f2)
                ys_spk.append((1 if same else -1) * np.ones(min(n1, n2)))
                self.statistics_training['DiffTypeSameSpk' if same else 'DiffTypeDiffSpk'] += 1
        if d1:                                # after the same pairs, like the reference's vstack order
            both = torch.from_numpy(np.concatenate(d1 + d2)).to(dev)
            n_d = both.numel() // 2
            idx1.append(both[:n_d])
            idx2.append(both[n_d:])
        if not idx1:
            raise ValueError('need at least one array to concatenate')
        i1, i2 = torch.cat(idx1), torch.cat(idx2)
        y = np.concatenate(ys)
        np.random.seed(seed)
        ind = np.random.permutation(len(y))
        ind_d = torch.from_numpy(ind).to(dev)
        X1 = gather_rows(self.features.table, i1[ind_d])
        X2 = gather_rows(self.features.table, i2[ind_d])
        if fid2spk:
            y_spk = np.concatenate(ys_spk)
            assert len(y) == len(y_spk), 'not same number of labels...'
            return (X1, X2, torch.from_numpy(y_spk[ind]).to(dev),
                    torch.from_numpy(y[ind]).to(dev))
        return X1, X2, torch.from_numpy(y[ind]).to(dev)

    def load_frames_from_pairs(self, pairs, seed=0, fid2spk=None, frames=False):
        """numpy front end with the reference's return types: (X1, X2, y), or
        (X1, X2, y_spk, y_phn) when a speaker mapping is given."""
        out = self.frames_from_pairs_device(pairs, seed, frames, fid2spk)
        return tuple(t.cpu().numpy() for t in out)

    def batch_iterator(self, train_mode=True):
        """Iterator over (X1, X2, y) batches of `batch_size` WORD pairs
        (dataloader.py:263-312)."""
        if train_mode and self._tcl_on_device():
            plan = self.plan(True)           # the pass's temporal-coherence pairs are drawn at once: the plan's batches
            for b in plan.order:
                yield plan.materialise(b)
            return
        self.load_data()
        mode = 'train' if train_mode else 'dev'
        pairs = self.pairs[mode]
        num_pairs = len(pairs)
        if self.shuffle_between_epochs:
            self._shuffle_pairs(pairs)
        batches = [pairs[idx:idx + self.batch_size]
                   for idx in range(0, num_pairs, self.batch_size)]
        selected_batches = self._select_batches(len(batches), train_mode)
        # one batched DTW launch for everything this epoch will touch ON THIS RANK
        self.align_pairs([p[:6] for b in selected_batches for p in batches[b]
                          if p[6] == 'same'])
        for batch_id in selected_batches:
            batch = self.frames_from_pairs_device(group_pairs(batches[batch_id]))
            if self.tcl > 0:
                batch = self.add_tcl_to_batch(batch)
            yield batch

    # -- the same batches as index lists in HBM (BatchPlan) -------------------------------
    _PERMS = {}          # n -> np.random.seed(0); np.random.permutation(n)  (dataloader.py:248-249)

    @classmethod
    def _seed0_permutation(cls, n):
        p = cls._PERMS.get(n)
        if p is None:
            # RandomState(0) is the generator np.random.seed(0) re-creates: the same permutation, and the
            # global stream is left alone until the pass is over (plan(): see there)
            p = cls._PERMS[n] = np.random.RandomState(0).permutation(n)
        return p

    def _plan_store(self, mode):
        """(idx1, idx2, labels, offsets) of EVERY batch of self.pairs[mode] -- batch b = pairs
        [b * batch_size, (b + 1) * batch_size) -- built once per pairs list: the content of a batch never
        changes between epochs (alignments are cached, the permutation is seeded with 0 every time), only
        which batches an epoch visits and in which order does.
        One pass over the pairs collects, per ENTRY of a batch (frames_from_pairs_device's order: the batch's same
        pairs, then its diff pairs), where its rows sit in one flat source -- the DTW calls' flat path tensors for a
        same pair, a host-built index run for a diff pair -- and how many rows / labels it has; everything after that
        is array arithmetic: one gather index for the whole dataset, the per-batch seed-0 permutations applied to it,
        one upload, two device gathers."""
        pairs = self.pairs[mode]
        cached = getattr(self, '_plans', {}).get(mode)
        if cached is not None and cached[0] is pairs and cached[1] == len(pairs):
            return cached[2]
        self.align_pairs([p[:6] for p in pairs if p[6] == 'same'], exchange=True)
        dev = self.features.table.device
        bs = self.batch_size
        P = len(pairs)
        nb = (P + bs - 1) // bs
        self._align.compact()
        span, token = self._align.span, self.features.token
        chunk_base = np.concatenate(([0], np.cumsum([c[0].numel() for c in self._align.chunks]))).astype(np.int64)
        n_aligned = int(chunk_base[-1])
        # entries: (batch, 0 same | 1 diff, offset in the source, rows, labels); diff runs are appended behind the paths
        e_batch, e_kind, e_off, e_rows, e_lab = [], [], [], [], []
        d_a0, d_b0, d_m = [], [], []             # diff pairs cut to the shorter token: runs a0 .. a0 + m, b0 .. b0 + m
        d1, d2 = [], []                          # align_different_words: explicit index arrays
        d_total = 0
        adw = self.align_different_words
        for i, (f1, s1, e1, f2, s2, e2, kind) in enumerate(pairs):
            if (s1 > e1) or (s2 > e2):
                assert kind in ('same', 'diff'), 'Unsupported pair type'
                continue
            if kind == 'same':
                sp = span.get((f1, s1, e1, f2, s2, e2, False))
                if sp is None:
                    continue
                e_batch.append(i // bs); e_kind.append(0); e_off.append(chunk_base[sp[0]] + sp[1]); e_rows.append(sp[2]); e_lab.append(sp[2])
                continue
            assert kind == 'diff', 'Unsupported pair type'
            (a0, n1), (b0, n2) = token(f1, s1, e1), token(f2, s2, e2)
            if adw:
                # the shorter word is stretched along the diagonal (dataloader.py:216-225); ties keep the FIRST, like min() / max()
                if n2 < n1:
                    mn0, mnl, mx0, mxl = b0, n2, a0, n1
                else:
                    mn0, mnl = a0, n1
                    mx0, mxl = (b0, n2) if n2 > n1 else (a0, n1)
                mapping = np.rint(np.linspace(0, mnl - 1, num=mxl)).astype(int)
                d1.append((mx0 + np.arange(mxl)).astype(np.int64)); d2.append((mn0 + mapping).astype(np.int64))
                rows = mxl
            else:
                rows = min(n1, n2)
                d_a0.append(a0); d_b0.append(b0); d_m.append(rows)
            # (the labels count min(n1, n2) frames, dataloader.py:231, whatever the number of rows is)
            e_batch.append(i // bs); e_kind.append(1); e_off.append(n_aligned + d_total); e_rows.append(rows); e_lab.append(min(n1, n2))
            d_total += rows
        E = len(e_batch)
        e_batch = np.asarray(e_batch, dtype=np.int64)
        e_kind = np.asarray(e_kind, dtype=np.int64)
        e_off = np.asarray(e_off, dtype=np.int64)
        e_rows = np.asarray(e_rows, dtype=np.int64)
        e_lab = np.asarray(e_lab, dtype=np.int64)
        # a batch's same pairs come before its diff pairs, each kind in file order
        order = np.argsort(e_batch * 2 + e_kind, kind='stable')
        e_batch, e_kind, e_off, e_rows, e_lab = e_batch[order], e_kind[order], e_off[order], e_rows[order], e_lab[order]
        rows_b = np.bincount(e_batch, weights=e_rows, minlength=nb).astype(np.int64) if E else np.zeros(nb, dtype=np.int64)
        lab_b = np.bincount(e_batch, weights=e_lab, minlength=nb).astype(np.int64) if E else np.zeros(nb, dtype=np.int64)
        offsets = np.concatenate(([0], np.cumsum(lab_b))).astype(np.int64)
        row0 = np.cumsum(rows_b) - rows_b
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        if E:
            # the diff pairs' index runs (host arithmetic, one upload), behind the aligned paths in the flat source
            if adw:
                dd1 = np.concatenate(d1) if d1 else np.zeros(0, dtype=np.int64)
                dd2 = np.concatenate(d2) if d2 else np.zeros(0, dtype=np.int64)
            else:
                m = np.asarray(d_m, dtype=np.int64)
                ramp = np.arange(int(m.sum()), dtype=np.int64) - np.repeat(np.cumsum(m) - m, m)
                dd1 = np.repeat(np.asarray(d_a0, dtype=np.int64), m) + ramp
                dd2 = np.repeat(np.asarray(d_b0, dtype=np.int64), m) + ramp
            both = torch.from_numpy(np.concatenate((dd1, dd2))).to(dev)
            src1 = torch.cat([c[0] for c in self._align.chunks] + [both[:dd1.size]])
            src2 = torch.cat([c[1] for c in self._align.chunks] + [both[dd1.size:]])
            R = int(e_rows.sum())
            gidx = np.repeat(e_off - (np.cumsum(e_rows) - e_rows), e_rows) + np.arange(R, dtype=np.int64)
            # the reference permutes len(y) = n indices and applies them to the rows AND the labels
            # (dataloader.py:247-255): with align_different_words a batch can hold more rows than labels,
            # and the permutation then draws from its first n rows
            perm = self._seed0_permutation
            perms = [perm(int(n)) for n in lab_b]
            perm_rows = np.concatenate([r0 + q for r0, q in zip(row0.tolist(), perms)])
            perm_lab = np.concatenate([o + q for o, q in zip(offsets[:-1].tolist(), perms)])
            take = torch.from_numpy(gidx[perm_rows]).to(dev)
            i1, i2 = src1[take], src2[take]
            y = torch.from_numpy(np.repeat(np.where(e_kind == 0, 1.0, -1.0), e_lab)[perm_lab]).to(dev)
        else:
            i1, i2, y = empty, empty, torch.zeros(0, dtype=torch.float64, device=dev)
        # (statistics_training counts a pair every time an epoch visits it: plan() adds these per visited batch)
        counts = np.stack([np.bincount(e_batch[e_kind == 0], minlength=nb), np.bincount(e_batch[e_kind == 1], minlength=nb)], axis=1).astype(np.int64).reshape(nb, 2)
        store = (i1, i2, y, offsets, counts, counts.sum(axis=1) > 0)
        if not hasattr(self, '_plans'):
            self._plans = {}
        self._plans[mode] = (pairs, len(pairs), store)
        return store

    def plan(self, train_mode=True):
        """batch_iterator(train_mode) as a BatchPlan (same batches, same order, same draws from the global
        RNGs), or None where only the iterator applies (temporal-coherence pairs drawn per batch from `random`).
        With tcl > 0 and a tcl_seed the training pass has a plan: every batch is the tcl = 0 plan's batch followed by
        its temporal-coherence pairs, drawn for the whole pass by one abn_tcl_pairs launch (_tcl_mix)."""
        if self.tcl > 0 and not (train_mode and self._tcl_on_device()):
            return None
        self.load_data()
        mode = 'train' if train_mode else 'dev'
        pairs = self.pairs[mode]
        if self.shuffle_between_epochs:
            self._shuffle_pairs(pairs)
            getattr(self, '_plans', {}).pop(mode, None)      # the batches' composition changed
        i1, i2, y, offsets, counts, has_arrays = self._plan_store(mode)
        selected = self._select_batches(len(offsets) - 1, train_mode)
        order = [int(b) for b in selected]
        if order:
            self.statistics_training['SameType'] += int(counts[order, 0].sum())
            self.statistics_training['DiffType'] += int(counts[order, 1].sum())
            # the iterator would leave numpy's global generator where its last batch put it
            # (np.random.seed(0); np.random.permutation(n), dataloader.py:248-249): so does the plan
            np.random.seed(0)
            np.random.permutation(int(offsets[order[-1] + 1] - offsets[order[-1]]))
        if self.tcl > 0:
            i1, i2, y, offsets = self._tcl_mix((i1, i2, y, offsets))
        return BatchPlan(self.features.table, i1, i2, y, offsets, order, has_arrays)

    @staticmethod
    def _shuffle_pairs(pairs):
        """random.shuffle(pairs) (dataloader.py:276-277); under torch.distributed the
        permutation is rank 0's, whatever the other ranks' `random` state is."""
        if parallel.world()[1] == 1:
            random.shuffle(pairs)
            return
        perm = list(range(len(pairs)))
        random.shuffle(perm)                     # same draws as shuffling the list itself
        perm = parallel.broadcast_array(perm)
        pairs[:] = [pairs[i] for i in perm]

    def _select_batches(self, num_batches, train_mode):
        """The epoch's batch ids in visiting order (dataloader.py:291-299).  Under
        torch.distributed rank 0's draw is broadcast and rank r keeps ids r, r+R, ...
        of it: disjoint, together complete (train: up to R-1 batches at the end are
        left out so that every rank takes the same number of steps)."""
        if self.num_max_minibatches < num_batches:
            selected_batches = np.random.choice(range(num_batches),
                                                self.num_max_minibatches,
                                                replace=False)
        else:
            selected_batches = np.random.permutation(range(num_batches))
        rank, ws = parallel.world()
        if ws > 1:
            selected_batches = parallel.broadcast_array(selected_batches)
            selected_batches = parallel.shard_ids(selected_batches, rank, ws, equal=train_mode)
        return selected_batches

    def add_tcl_to_batch(self, batch):
        X1, X2, Y = batch
        num_pairs = len(Y)
        num_pairs_to_add = int((self.tcl * num_pairs) / (1 - self.tcl))
        X1_tcl, X2_tcl, Y_tcl = self.temporal_coherence_loss(num_pairs_to_add)
        return (torch.cat((X1, X1_tcl)), torch.cat((X2, X2_tcl)),
                torch.cat((Y, Y_tcl.to(Y.dtype))))

    def temporal_coherence_loss(self, num_pairs):
        """Dupoux & Synnaeve (2016) temporal coherence pairs (dataloader.py:324-352)."""
        c = self.features
        i1, i2, Y = [], [], []
        per_it = len(self.TCL_DISTANCES_DIFF) + len(self.TCL_DISTANCE_SAME)
        for _ in range(round(num_pairs / per_it)):
            files = self.train_files if self.train_files is not None else c.names
            f = c._name(random.choice(files))
            t = random.choice(range(c.length[f] - max(self.TCL_DISTANCES_DIFF)))
            for delta in self.TCL_DISTANCE_SAME:
                i1.append(c.offset[f] + t); i2.append(c.offset[f] + t + delta); Y.append(1)
            for delta in self.TCL_DISTANCES_DIFF:
                i1.append(c.offset[f] + t); i2.append(c.offset[f] + t + delta); Y.append(-1)
        dev = c.table.device
        return (gather_rows(c.table, torch.tensor(i1, dtype=torch.int64, device=dev)),
                gather_rows(c.table, torch.tensor(i2, dtype=torch.int64, device=dev)),
                torch.tensor(Y, device=dev))

    # -- temporal-coherence pairs drawn on the device (abn_tcl_pairs) ------------------------------------------
    def _tcl_on_device(self):
        return self.tcl > 0 and getattr(self, 'tcl_seed', None) is not None

    @classmethod
    def tcl_iterations(cls, num_pairs):
        """Draws that temporal_coherence_loss(num_pairs) makes (dataloader.py:332-333; Python's round): each gives
        len(TCL_DISTANCE_SAME) + len(TCL_DISTANCES_DIFF) frame pairs."""
        return round(num_pairs / (len(cls.TCL_DISTANCES_DIFF) + len(cls.TCL_DISTANCE_SAME)))

    def tcl_pairs_to_add(self, num_pairs):
        """Frame pairs add_tcl_to_batch asks for behind a batch of num_pairs (dataloader.py:317)."""
        return int((self.tcl * num_pairs) / (1 - self.tcl))

    def _tcl_tables(self):
        """The files the device draw picks from, as device tables (first table row, frames) and the host copy of the
        lengths: train_files when the pairs are loaded, else every file, sorted by name.  A file of at most
        max(TCL_DISTANCES_DIFF) frames has no frame t with t + max in it (the reference's random.choice(range(<= 0))
        raises when such a file is drawn): it is left out, with one warning."""
        c = self.features
        deltas = list(self.TCL_DISTANCE_SAME) + list(self.TCL_DISTANCES_DIFF)
        max_diff = max(self.TCL_DISTANCES_DIFF)
        if max(self.TCL_DISTANCE_SAME) > max_diff:
            raise ValueError('temporal coherence: max(TCL_DISTANCE_SAME) = %d exceeds max(TCL_DISTANCES_DIFF) = %d'
                             % (max(self.TCL_DISTANCE_SAME), max_diff))
        files = self.train_files if self.train_files is not None else c.names
        names = sorted({c._name(f) for f in files}, key=lambda k: k.decode('UTF-8') if isinstance(k, bytes) else str(k))
        key = (id(c), tuple(names), tuple(deltas))
        tab = getattr(self, '_tcl_tab', None)
        if tab is not None and tab['key'] == key:
            return tab
        keep = [k for k in names if c.length[k] > max_diff]
        if len(keep) < len(names) and not getattr(self, '_tcl_warned', False):
            import warnings
            self._tcl_warned = True
            warnings.warn('temporal coherence: %d of %d files have at most %d frames and are left out of the draw'
                          % (len(names) - len(keep), len(names), max_diff))
        if not keep:
            raise ValueError('temporal coherence: no file has more than %d frames' % max_diff)
        host = np.array([[c.offset[k] for k in keep], [c.length[k] for k in keep]], dtype=np.int64)
        dev = torch.from_numpy(host).to(c.table.device)
        tab = self._tcl_tab = dict(key=key, names=keep, host=host, dev=dev, deltas=np.array(deltas, dtype=np.int32),
                                   n_same=len(self.TCL_DISTANCE_SAME))
        return tab

    def _tcl_fill(self, n_iter, epoch, idx1, idx2, labels, dst=None, first_iter=0):
        """One abn_tcl_pairs launch: iterations first_iter .. first_iter + n_iter - 1 of pass `epoch`, written into
        idx1 / idx2 / labels at dst[i] (packed when dst is None)."""
        tab = self._tcl_tables()
        lib = _lib.load()
        _lib.require_device(idx1, idx2, labels, dst)
        assert idx1.dtype == torch.int64 and idx2.dtype == torch.int64 and labels.dtype in (torch.int64, torch.float64)
        assert idx1.numel() == idx2.numel() == labels.numel() and (dst is None or (dst.dtype == torch.int64 and dst.numel() >= n_iter))
        host, dev, deltas = tab['host'], tab['dev'], tab['deltas']
        _lib.check(lib.abn_tcl_pairs(_lib.ptr(dev[0]), _lib.ptr(dev[1]), host[1].ctypes.data, host.shape[1],
                                     deltas.ctypes.data, len(deltas), tab['n_same'], int(n_iter), int(first_iter),
                                     int(self.tcl_seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, _lib.ptr(dst),
                                     _lib.ptr(idx1), _lib.ptr(idx2), _lib.ptr(labels), int(labels.dtype == torch.float64),
                                     idx1.numel(), _lib.stream()), 'abn_tcl_pairs')

    def _tcl_mix(self, store):
        """The tcl = 0 plan's arrays with every batch's temporal-coherence pairs behind its word pairs: batch b of n
        frame pairs gets 5 * round(int(tcl n / (1 - tcl)) / 5) more (add_tcl_to_batch, dataloader.py:314-322; labels
        float64 as np.concatenate makes them).  The arrays persist -- the word-pair part is copied once per store, the
        drawn part is refilled in place by one launch per pass, so the addresses a trainer's captured steps hold stay
        valid from epoch to epoch."""
        i1, i2, y, offsets = store
        mix = getattr(self, '_tcl_mixed', None)
        if mix is None or mix['src'][0] is not i1 or mix['src'][1] is not offsets:
            dev = i1.device
            per_it = len(self.TCL_DISTANCE_SAME) + len(self.TCL_DISTANCES_DIFF)
            n_b = np.diff(offsets).astype(np.int64)
            its = np.array([self.tcl_iterations(self.tcl_pairs_to_add(int(n))) for n in n_b], dtype=np.int64)
            new_off = np.concatenate(([0], np.cumsum(n_b + per_it * its))).astype(np.int64)
            total, n_iter = int(new_off[-1]), int(its.sum())
            # where the word pairs go (one index for all batches), and where each iteration's pairs start
            head = np.repeat(new_off[:-1] - offsets[:-1], n_b) + np.arange(int(offsets[-1]), dtype=np.int64)
            k = np.arange(n_iter, dtype=np.int64) - np.repeat(np.cumsum(its) - its, its)
            dst = np.repeat(new_off[:-1] + n_b, its) + per_it * k
            up = torch.from_numpy(np.concatenate((head, dst))).to(dev)
            head_d, dst_d = up[:head.size], up[head.size:].contiguous()
            m1 = torch.zeros(total, dtype=torch.int64, device=dev)
            m2 = torch.zeros(total, dtype=torch.int64, device=dev)
            my = torch.zeros(total, dtype=torch.float64, device=dev)
            m1[head_d], m2[head_d], my[head_d] = i1, i2, y.to(torch.float64)
            mix = self._tcl_mixed = dict(src=(i1, offsets), idx1=m1, idx2=m2, labels=my, offsets=new_off, dst=dst_d, n_iter=n_iter)
        if mix['n_iter']:
            self._tcl_fill(mix['n_iter'], self.tcl_epoch, mix['idx1'], mix['idx2'], mix['labels'], dst=mix['dst'])
        self.tcl_epoch += 1
        return mix['idx1'], mix['idx2'], mix['labels'], mix['offsets']


class TemporalCoherenceDataLoader(OriginalDataLoader):
    """Temporal-coherence pairs only (abnet3/dataloader.py:549-577; Dupoux & Synnaeve 2016): a training pass is
    num_max_minibatches batches of round(batch_size / 5) draws -- a random file, a random frame t, the 'same' pair
    (t, t + 1) and the 'diff' pairs (t, t + 15 / 20 / 25 / 30) --, no word pairs, no DTW; the sampled dev pairs serve
    evaluation and early stopping as in OriginalDataLoader.

    The reference draws with Python's `random` in a host loop.  Here a whole pass is drawn by ONE abn_tcl_pairs launch
    (Philox4x32-10 keyed by `seed`, counter = (iteration, epoch): reproducible, independent of `random`) into
    persistent index arrays, which plan(True) hands out as a BatchPlan: the trainer's captured steps read their batch
    from them and survive from epoch to epoch, every epoch with fresh pairs.  The batches the iterator or
    materialise() yield are views of these arrays: the next training pass overwrites them.
    Files of at most max(TCL_DISTANCES_DIFF) frames are left out of the draw (the reference crashes when it draws one).
    As in the reference, self.batch_size ends up as `batch_size`, so the dev batches hold batch_size WORD pairs;
    test_words_batch_size is accepted and has no effect."""

    def __init__(self, pairs_path, features_path, batch_size=500,
                 test_words_batch_size=8,
                 num_max_minibatches=1000, seed=0):
        super().__init__(pairs_path, features_path,
                         num_max_minibatches=num_max_minibatches,
                         batch_size=test_words_batch_size)
        self.batch_size = batch_size
        self.seed = seed
        self.tcl_seed = seed
        self._tcl_arrays = None

    def _tcl_on_device(self):
        return False                       # (tcl = 0: the dev pass is OriginalDataLoader's)

    def _train_plan(self):
        self.load_data()
        per_it = len(self.TCL_DISTANCE_SAME) + len(self.TCL_DISTANCES_DIFF)
        its = self.tcl_iterations(self.batch_size)
        nb = int(self.num_max_minibatches)
        total = nb * its * per_it
        self._tcl_tables()                 # (raises before anything is allocated when no file is eligible)
        dev = self.features.table.device
        a = self._tcl_arrays
        if a is None or a[0].numel() != total or a[0].device != dev:
            a = self._tcl_arrays = tuple(torch.zeros(total, dtype=torch.int64, device=dev) for _ in range(3))
        # every rank draws the whole pass (one launch) and visits its share of the batches: r, r + R, ...
        self._tcl_fill(nb * its, self.tcl_epoch, a[0], a[1], a[2])
        self.tcl_epoch += 1
        rank, ws = parallel.world()
        order = parallel.shard_ids(list(range(nb)), rank, ws, equal=True)
        offsets = np.arange(nb + 1, dtype=np.int64) * (its * per_it)
        return BatchPlan(self.features.table, a[0], a[1], a[2], offsets, order)

    def plan(self, train_mode=True):
        if train_mode:
            return self._train_plan()
        return super().plan(False)

    def batch_iterator(self, train_mode=True):
        if train_mode:
            plan = self._train_plan()
            for b in plan.order:
                yield plan.materialise(b)
        else:
            yield from super().batch_iterator(False)


class FramesDataLoader(OriginalDataLoader):
    """Batches of exactly `batch_size` FRAME pairs, shuffled across the whole
    dataset; alignment happens once (abnet3/dataloader.py:580-739)."""

    def __init__(self, pairs_path, features_path,
                 batch_size=100, randomize_dataset=True, max_batches_per_epoch=None):
        super().__init__(pairs_path, features_path)
        self.randomize_dataset = randomize_dataset
        self.batch_size = batch_size
        self.frame_pairs = {'train': None, 'dev': None}   # (idx1, idx2, y) device
        self.max_batches_per_epoch = max_batches_per_epoch
        if self.max_batches_per_epoch is not None:
            self.batch_position = 0

    def load_data(self):
        super(FramesDataLoader, self).load_data()
        for mode in ('train', 'dev'):
            if self.frame_pairs[mode] is None and self.pairs[mode] is not None:
                self.frame_pairs[mode] = self.load_all_frames(self.pairs[mode])

    def load_all_frames(self, pairs):
        """The frame-pair dataset (global row of frame 1, of frame 2, +-1) for
        all word pairs (dataloader.py:617-671), shuffled once."""
        pairs = group_pairs(pairs)
        self.align_pairs(pairs['same'], exchange=True)     # DTW work split over the ranks
        dev = self.features.table.device
        # where every kept pair's rows sit in one flat source (the DTW calls' flat path tensors, then the diff pairs'
        # index runs): one gather index for the dataset instead of a view and a label array per pair
        self._align.compact()
        span, token = self._align.span, self.features.token
        chunk_base = np.concatenate(([0], np.cumsum([c[0].numel() for c in self._align.chunks]))).astype(np.int64)
        s_off, s_len = [], []
        for f1, s1, e1, f2, s2, e2 in pairs['same']:
            if (s1 > e1) or (s2 > e2):
                continue
            sp = span.get((f1, s1, e1, f2, s2, e2, False))
            if sp is None:
                continue
            s_off.append(chunk_base[sp[0]] + sp[1]); s_len.append(sp[2])
        self.statistics_training['SameType'] += len(s_len)
        d_a0, d_b0, d_m = [], [], []          # diff pairs: index runs cut to the shorter token
        for f1, s1, e1, f2, s2, e2 in pairs['diff']:
            if (s1 > e1) or (s2 > e2):
                continue
            (a0, n1), (b0, n2) = token(f1, s1, e1), token(f2, s2, e2)
            d_a0.append(a0); d_b0.append(b0); d_m.append(min(n1, n2))
        self.statistics_training['DiffType'] += len(d_m)
        if not s_len and not d_m:
            z = torch.zeros(0, dtype=torch.int64, device=dev)
            return z, z, z
        s_off, s_len = np.asarray(s_off, dtype=np.int64), np.asarray(s_len, dtype=np.int64)
        m = np.asarray(d_m, dtype=np.int64)
        n_same, n_diff = int(s_len.sum()), int(m.sum())
        gidx = np.repeat(s_off - (np.cumsum(s_len) - s_len), s_len) + np.arange(n_same, dtype=np.int64)
        ramp = np.arange(n_diff, dtype=np.int64) - np.repeat(np.cumsum(m) - m, m)
        dd1 = np.repeat(np.asarray(d_a0, dtype=np.int64), m) + ramp
        dd2 = np.repeat(np.asarray(d_b0, dtype=np.int64), m) + ramp
        up = torch.from_numpy(np.concatenate((gidx, dd1, dd2))).to(dev)
        take, r1, r2 = up[:n_same], up[n_same:n_same + n_diff], up[n_same + n_diff:]
        if n_same:
            src1 = torch.cat([c[0] for c in self._align.chunks]) if len(self._align.chunks) > 1 else self._align.chunks[0][0]
            src2 = torch.cat([c[1] for c in self._align.chunks]) if len(self._align.chunks) > 1 else self._align.chunks[0][1]
            i1, i2 = torch.cat((src1[take], r1)), torch.cat((src2[take], r2))
        else:
            i1, i2 = r1, r2
        y = torch.cat((torch.ones(n_same, dtype=torch.int64, device=dev), -torch.ones(n_diff, dtype=torch.int64, device=dev)))
        return self._shuffle((i1, i2, y))

    @staticmethod
    def _shuffle(fp):
        # np.random.shuffle(list) and np.random.permutation(n) draw the same
        # permutation from the same global state (dataloader.py:670)
        # (under torch.distributed every rank applies rank 0's permutation)
        perm = parallel.broadcast_array(np.random.permutation(len(fp[2])))
        perm = torch.from_numpy(perm).to(fp[2].device)
        return fp[0][perm], fp[1][perm], fp[2][perm]

    def load_batch(self, sl, mode):
        i1, i2, y = self.frame_pairs[mode]
        return (gather_rows(self.features.table, i1[sl]),
                gather_rows(self.features.table, i2[sl]), y[sl])

    def _batch_ids(self, train_mode):
        """The shuffles and the batch ids of one pass (dataloader.py:686-739), this rank's share."""
        self.load_data()
        mode = 'train' if train_mode else 'dev'
        num_pairs = len(self.frame_pairs[mode][2])
        num_batches = num_pairs // self.batch_size
        if num_batches == 0:
            num_batches = 1
        if mode == 'dev' or self.max_batches_per_epoch is None:
            batch_ids = range(num_batches)
            if self.randomize_dataset:
                self.frame_pairs[mode] = self._shuffle(self.frame_pairs[mode])
        else:
            if self.batch_position >= num_batches:
                if self.randomize_dataset:
                    self.frame_pairs[mode] = self._shuffle(self.frame_pairs[mode])
                self.batch_position = 0
            batch_ids = range(self.batch_position,
                              min(self.batch_position + self.max_batches_per_epoch,
                                  num_batches))
            self.batch_position += self.max_batches_per_epoch
        rank, ws = parallel.world()
        if ws > 1:       # rank r gathers batches r, r+R, ... of the epoch's (shared) order
            batch_ids = parallel.shard_ids(list(batch_ids), rank, ws, equal=train_mode)
        return list(batch_ids)

    def batch_iterator(self, train_mode=True):
        """(dataloader.py:686-739)"""
        mode = 'train' if train_mode else 'dev'
        for i in self._batch_ids(train_mode):
            yield self.load_batch(slice(i * self.batch_size,
                                        i * self.batch_size + self.batch_size), mode)

    def plan(self, train_mode=True):
        """batch_iterator(train_mode) as a BatchPlan: the same shuffles, batch b = frame pairs
        [b * batch_size, (b + 1) * batch_size) of the (re)shuffled dataset."""
        ids = self._batch_ids(train_mode)
        mode = 'train' if train_mode else 'dev'
        i1, i2, y = self.frame_pairs[mode]
        num_pairs = len(y)
        num_batches = max(1, num_pairs // self.batch_size)
        offsets = np.minimum(np.arange(num_batches + 1, dtype=np.int64) * self.batch_size, num_pairs)
        return BatchPlan(self.features.table, i1, i2, y, offsets, ids)


class PairsDataLoader(OriginalDataLoader):
    """Takes a pairs file instead of the sampler's cluster-derived dataset (abnet3/dataloader.py:355-546): one
    line `file1 file2 begin1 end1 begin2 end2 distance` per discovered pair, file ids as integers (mapped to names
    through `id_to_file`, lines `id name`, when given), begin / end as FRAME indices -- a token is
    features[file][begin:end] --, the distance ignored.  discovery.KnnPairMiner writes both files.

    The pairs are split into 'train' and 'test' by whole files (SPLIT_FILES) or by position inside every file
    (SPLIT_EACH_FILE); an epoch is drawn from Python's `random` call for call as the reference draws it, so that
    after random.seed(s) the epoch's pair list is the reference's.  Batches are built on the device path of
    OriginalDataLoader (all 'same' pairs of the epoch DTW-aligned in one batched call, frames gathered in HBM)
    and arrive as device tensors.  Under torch.distributed the trainer shards the iterator's batches (every rank
    must then have seeded `random` alike)."""
    SPLIT_FILES = "files"
    SPLIT_EACH_FILE = "split_each_file"
    SPLIT_METHODS = [SPLIT_FILES, SPLIT_EACH_FILE]

    shards_itself = False

    def __init__(self, pairs_path, features_path, id_to_file,
                 ratio_split_train_test=0.7,
                 batch_size=8, train_iterations=10000, test_iterations=500,
                 proportion_positive_pairs=0.5,
                 align_different_words=True,
                 split_method=SPLIT_EACH_FILE):
        self.pairs_path = pairs_path
        self.features_path = features_path
        self.features = None          # DeviceCorpus
        self.id_to_file = id_to_file
        self.pairs = {'train': None, 'test': None}
        self.ratio_split_train_test = ratio_split_train_test
        self.batch_size = batch_size
        self.align_different_words = align_different_words
        self.iterations = {'train': train_iterations, 'test': test_iterations}
        self.proportion_positive_pairs = proportion_positive_pairs
        self.split_method = split_method
        assert split_method in self.SPLIT_METHODS
        self.tokens = {'train': [], 'test': []}
        self.statistics_training = defaultdict(int)
        self.files = set()
        self.seed = 0
        self.tcl = 0.0
        self.train_files = None
        self._align = AlignCache()

    def __getstate__(self):
        """For pickle: the features (and the pairs read from the file) stay out of the state."""
        return (self.pairs_path, self.features_path, self.id_to_file, self.ratio_split_train_test,
                self.align_different_words, self.proportion_positive_pairs)

    def __setstate__(self, state):
        """Rebuilds the loader from __getstate__'s tuple and reloads its data (dataloader.py:407-423).  What the
        tuple does not carry (batch size, iterations, split method) takes the constructor's default, and the
        features are only read when there is a features_path to read them from."""
        pairs_path, features_path, id_to_file, ratio, align_different_words, proportion = state
        self.__init__(pairs_path, features_path, id_to_file, ratio_split_train_test=ratio,
                      proportion_positive_pairs=proportion, align_different_words=align_different_words)
        if features_path is not None:
            self.load_data()
        elif pairs_path is not None:
            self.load_pairs()

    def set_data(self, features, times, train_pairs=None, test_pairs=None):
        """In-memory injection of what load_data() reads from features_path: features {utt: [T, D]},
        times {utt: [T]}; optionally the split pair lists ([f1, b1, e1, f2, b2, e2], frame indices)."""
        self.features = DeviceCorpus(features, times)
        if train_pairs is not None or test_pairs is not None:
            self.pairs['train'] = [list(p) for p in (train_pairs or [])]
            self.pairs['test'] = [list(p) for p in (test_pairs or [])]
            self._set_tokens()

    def load_data(self):
        if self.pairs['train'] is None:
            self.load_pairs()
        if self.features is None:
            try:
                import h5features
            except ImportError:
                raise ImportError('features_path is an h5features file and the '
                                  'h5features package is not installed; use '
                                  'set_data() with in-memory arrays')
            with h5features.Reader(self.features_path, 'features') as fh:
                feats = fh.read()
            self.features = DeviceCorpus(feats.dict_features(), feats.dict_labels())

    def load_pairs(self):
        """Reads the pairs file and splits it (dataloader.py:439-474): 7 space-separated fields per line, the
        7th (the distance) ignored; ids mapped through id_to_file when given, kept as ints otherwise."""
        pairs = []
        file_mapping = {}
        if self.id_to_file is not None:
            with open(self.id_to_file, 'r') as f:
                for fid, name in (l.strip().split() for l in f):
                    file_mapping[int(fid)] = name
        with open(self.pairs_path, 'r') as f:
            for line in f:
                file1, file2, begin1, end1, begin2, end2, _distance = line.split(' ')
                file1, file2 = int(file1), int(file2)
                file1 = file_mapping.get(file1, file1)
                file2 = file_mapping.get(file2, file2)
                self.files.add(file1)
                self.files.add(file2)
                pairs.append([file1, int(begin1), int(end1), file2, int(begin2), int(end2)])
        if self.split_method == self.SPLIT_FILES:
            self.pairs['train'], self.pairs['test'] = self.split_train_test(pairs)
        elif self.split_method == self.SPLIT_EACH_FILE:
            self.pairs['train'], self.pairs['test'] = self.split_train_test_each_file(pairs)
        self._set_tokens()

    def _set_tokens(self):
        """tokens[mode]: every distinct (file, begin, end) of the mode's pairs, in the iteration order of a set
        (as dataloader.py:469-474 builds them)."""
        for mode in ('train', 'test'):
            tokens = set()
            for file1, begin1, end1, file2, begin2, end2 in self.pairs[mode]:
                tokens.add((file1, begin1, end1))
                tokens.add((file2, begin2, end2))
            self.tokens[mode] = list(tokens)

    def split_train_test(self, pairs):
        """Train and test by splitting the FILES in two subsets; pairs across the two are dropped
        (dataloader.py:476-494).  The test files are random.sample(sorted(self.files), n): the reference samples
        from the set itself, which is an error from Python 3.11 on and whose order is not reproducible."""
        num_files_test = int(len(self.files) * (1 - self.ratio_split_train_test))
        dev_files = set(random.sample(sorted(self.files), num_files_test))
        train_pairs, dev_pairs = [], []
        for pair in pairs:
            file1, file2 = pair[0], pair[3]
            if file1 in dev_files and file2 in dev_files:
                dev_pairs.append(pair)
            elif file1 not in dev_files and file2 not in dev_files:
                train_pairs.append(pair)
        return train_pairs, dev_pairs

    def split_train_test_each_file(self, pairs):
        """Every file is cut at ratio * (the largest end seen in it): a pair trains when its first token begins
        before its file's cut and its second at or before its own, tests when both begin after; the rest
        straddles and is dropped (dataloader.py:496-519, comparisons as there)."""
        len_files = defaultdict(int)
        for file1, _, e1, file2, _, e2 in pairs:
            len_files[file1] = max(len_files[file1], e1)
            len_files[file2] = max(len_files[file2], e2)
        threshold = {f: n * self.ratio_split_train_test for f, n in len_files.items()}
        train_pairs, dev_pairs = [], []
        for p in pairs:
            file1, s1, _, file2, s2, _ = p
            if s1 > threshold[file1] and s2 > threshold[file2]:
                dev_pairs.append(p)
            elif s1 < threshold[file1] and s2 <= threshold[file2]:
                train_pairs.append(p)
        return train_pairs, dev_pairs

    def epoch_pairs(self, train_mode=True):
        """One epoch's word pairs, [f1, b1, e1, f2, b2, e2, 'same' | 'diff'], drawn as dataloader.py:521-546
        draws them: iterations * batch_size pairs of which proportion_positive_pairs are positives sampled
        without replacement (all of them when there are not enough), the rest pairs of tokens drawn with
        replacement and paired consecutively; then shuffled."""
        mode = 'train' if train_mode else 'test'
        all_positive_pairs = self.pairs[mode]
        tokens = self.tokens[mode]
        num_pairs = self.iterations[mode] * self.batch_size
        num_positive_pairs = int(num_pairs * self.proportion_positive_pairs)
        if num_positive_pairs > len(all_positive_pairs):
            print("Not enough positive pairs to sample this number of iterations. "
                  "There is only {}, but {} requested".format(len(all_positive_pairs), num_positive_pairs))
            num_positive_pairs = len(all_positive_pairs)
        num_negative_pairs = num_pairs - num_positive_pairs
        positive_pairs = random.sample(all_positive_pairs, num_positive_pairs)
        positive_pairs = [list(pair) + ['same'] for pair in positive_pairs]
        tokens = random.choices(tokens, k=2 * num_negative_pairs)
        negative_pairs = [list(tokens[i]) + list(tokens[i + 1]) + ['diff'] for i in range(0, len(tokens), 2)]
        pairs = positive_pairs + negative_pairs
        random.shuffle(pairs)
        return pairs

    def batch_iterator(self, train_mode=True):
        """Iterator over the (X1, X2, y) device batches of one epoch: slices of batch_size word pairs of
        epoch_pairs(), until the iterations are done or a slice is empty."""
        self.load_data()
        iterations = self.iterations['train' if train_mode else 'test']
        pairs = self.epoch_pairs(train_mode)
        # one batched DTW launch for every positive pair the epoch's batches will touch
        self.align_pairs([p[:6] for p in pairs[:iterations * self.batch_size] if p[6] == 'same'], frames=True)
        for i in range(iterations):
            pairs_batch = pairs[i * self.batch_size: (i + 1) * self.batch_size]
            if len(pairs_batch) == 0:
                break
            yield self.frames_from_pairs_device(group_pairs(pairs_batch), frames=True)

    def plan(self, train_mode=True):
        return None                    # (the epoch is drawn per pass from `random`: the iterator)

    def prefetch_alignments(self):
        self.load_data()
        for mode in ('train', 'test'):
            if self.pairs[mode]:
                self.align_pairs(self.pairs[mode], frames=True)


class WordPairDataLoader(OriginalDataLoader):
    """Batches of WORD pairs for trainer.TrainerSequencePairs and loss.SoftDTWLoss (not in the reference): the same pairs
    files, `batch_size` word pairs per batch, and NO alignment pass -- the alignment is soft-DTW's, inside the loss, and
    moves with the weights.

    A batch is (X, off1, n1, off2, n2, y): X [rows, D] float32 on the device, the frames of all side-1 tokens followed by
    those of all side-2 tokens, gathered with one gather_rows call (one index upload per batch); off1, n1, off2, n2 host
    integer arrays into X (word pair p is X[off1[p] : off1[p] + n1[p]] against X[off2[p] : off2[p] + n2[p]]; no two ranges
    overlap); y [P] int64 on the device, +1 for a 'same' pair and -1 otherwise.  A pair with an empty token, or with a token
    of more than softdtw.max_len() frames, is dropped (statistics_training: 'DroppedEmpty', 'DroppedLong'; the kept ones
    count as 'SameType' / 'DiffType'); a batch whose pairs are all dropped is not yielded.  Tokens are not windowed.
    The loader hands out no BatchPlan: `plan` is not an attribute of it, so the trainer takes the iterator."""

    def __init__(self, pairs_path, features_path, **kwargs):
        super(WordPairDataLoader, self).__init__(pairs_path, features_path, **kwargs)
        assert self.tcl == 0, 'WordPairDataLoader: temporal-coherence pairs are frame pairs; tcl must be 0'

    @property
    def plan(self):
        raise AttributeError('WordPairDataLoader hands out no BatchPlan')           # hasattr(loader, 'plan') is False

    def prefetch_alignments(self):
        """Nothing to do: there is no alignment pass."""

    def word_pairs_device(self, pairs):
        """One batch from [(f1, s1, e1, f2, s2, e2, type), ...], or None when every pair is dropped."""
        from . import softdtw
        cap = softdtw.max_len()
        a0, n1, b0, n2, ys = [], [], [], [], []
        for f1, s1, e1, f2, s2, e2, kind in pairs:
            (a, na), (b, nb) = self._token(f1, s1, e1, False), self._token(f2, s2, e2, False)
            if s1 > e1 or s2 > e2 or na == 0 or nb == 0:
                self.statistics_training['DroppedEmpty'] += 1
                continue
            if na > cap or nb > cap:
                self.statistics_training['DroppedLong'] += 1
                continue
            same = kind == 'same'
            self.statistics_training['SameType' if same else 'DiffType'] += 1
            a0.append(a); n1.append(na); b0.append(b); n2.append(nb)
            ys.append(1 if same else -1)
        if not ys:
            return None
        n1, n2 = np.asarray(n1, dtype=np.int32), np.asarray(n2, dtype=np.int32)
        off1 = (np.cumsum(n1, dtype=np.int64) - n1).astype(np.int64)
        off2 = (int(n1.sum()) + np.cumsum(n2, dtype=np.int64) - n2).astype(np.int64)
        rows = np.concatenate([np.repeat(np.asarray(a0, dtype=np.int64) - off1, n1),
                               np.repeat(np.asarray(b0, dtype=np.int64) - off2, n2)]) + np.arange(int(n1.sum()) + int(n2.sum()))
        table = self.features.table
        both = torch.from_numpy(np.concatenate([rows, np.asarray(ys, dtype=np.int64)])).to(table.device)      # one upload
        X = gather_rows(table, both[:len(rows)])
        return X, off1, n1, off2, n2, both[len(rows):]

    def batch_iterator(self, train_mode=True):
        """Iterator over (X, off1, n1, off2, n2, y) batches of `batch_size` word pairs."""
        self.load_data()
        pairs = self.pairs['train' if train_mode else 'dev']
        if self.shuffle_between_epochs:
            self._shuffle_pairs(pairs)
        batches = [pairs[idx:idx + self.batch_size] for idx in range(0, len(pairs), self.batch_size)]
        for batch_id in self._select_batches(len(batches), train_mode):
            batch = self.word_pairs_device(batches[batch_id])
            if batch is not None:
                yield batch


class MultiTaskDataLoader(OriginalDataLoader):
    """Batches (X1, X2, y_spk, y_phn) for the multitask siamese network
    (abnet3/dataloader.py:742-792).  fid2spk_file: lines "<file id> <speaker id>".
    speaker_match: see OriginalDataLoader.same_speaker."""

    def __init__(self, pairs_path, features_path, fid2spk_file=None,
                 speaker_match='identity', **kwargs):
        super().__init__(pairs_path, features_path, **kwargs)
        assert speaker_match in ('identity', 'equal')
        self.fid2spk_file = fid2spk_file
        self.speaker_match = speaker_match

    def plan(self, train_mode=True):
        return None                    # (four tensors per batch: the iterator)

    def batch_iterator(self, train_mode=True):
        self.load_data()
        mode = 'train' if train_mode else 'dev'
        pairs = self.pairs[mode]
        num_pairs = len(pairs)
        batches = [pairs[idx:idx + self.batch_size]
                   for idx in range(0, num_pairs, self.batch_size)]
        fid2spk = read_spkid_file(self.fid2spk_file)
        selected_batches = self._select_batches(len(batches), train_mode)
        self.align_pairs([p[:6] for b in selected_batches for p in batches[b]
                          if p[6] == 'same'])
        for idx in selected_batches:
            yield self.frames_from_pairs_device(group_pairs(batches[idx]), fid2spk=fid2spk)



class MultimodalDataLoader(FramesDataLoader):
    """FramesDataLoader over several frame-synchronous feature sets (abnet3/dataloader.py:794-980): the DTW
    alignment runs on the first modality, and every modality's rows are gathered with the same frame-pair
    indices (one DeviceCorpus table per modality, laid out like the first one; abn_gather_pairs per modality).
    Batches are ([X1_m for m], [X2_m for m], y).  The reference's check_consistency is a TODO; here the
    modalities must hold the same items with the same frame counts (ValueError otherwise)."""

    def __init__(self, pairs_path, features_path,
                 batch_size=500, randomize_dataset=False,
                 max_batches_per_epoch=None):
        super().__init__(pairs_path, features_path, batch_size,
                         randomize_dataset, max_batches_per_epoch)
        self.corpora = None              # [DeviceCorpus] per modality

    def __getstate__(self):
        return (self.pairs_path, self.features_path, self.statistics_training, self.seed,
                self.num_max_minibatches, self.batch_size)

    def check_consistency(self, features):
        """features: one {item: [T, D_m]} per modality.  Raises ValueError unless every modality holds the items
        of the first with the same number of frames."""
        first = features[0]
        for m, feats in enumerate(features[1:], 1):
            if set(feats.keys()) != set(first.keys()):
                raise ValueError('MultimodalDataLoader: modality %d does not hold the items of modality 0 '
                                 '(%d against %d items)' % (m, len(feats), len(first)))
            for k, f in first.items():
                if len(feats[k]) != len(f):
                    raise ValueError('MultimodalDataLoader: item %r has %d frames in modality 0 and %d in '
                                     'modality %d' % (k, len(f), len(feats[k]), m))

    def set_data(self, features, times, train_pairs=None, dev_pairs=None):
        """In-memory injection: features = [{utt: [T, D_m]} per modality], times = {utt: [T]} (the first
        modality's frame times locate the tokens of all)."""
        features = list(features)
        self.check_consistency(features)
        names = list(features[0].keys())
        self.corpora = [DeviceCorpus({k: f[k] for k in names}, times) for f in features]
        super().set_data(features[0], times, train_pairs, dev_pairs)
        self.features = self.corpora[0]

    def load_data(self):
        if self.corpora is None:
            try:
                import h5features
            except ImportError:
                raise ImportError('features_path lists h5features files and the h5features package is not '
                                  'installed; use set_data() with in-memory arrays')
            feats, times = [], None
            for path in self.features_path:
                with h5features.Reader(path, 'features') as fh:
                    data = fh.read()
                feats.append(data.dict_features())
                if times is None:
                    times = data.dict_labels()
            self.check_consistency(feats)
            names = list(feats[0].keys())
            self.corpora = [DeviceCorpus({k: f[k] for k in names}, times) for f in feats]
        self.features = self.corpora[0]
        super().load_data()

    def load_batch(self, sl, mode):
        i1, i2, y = self.frame_pairs[mode]
        first, stop, _ = sl.indices(len(y))
        n = max(0, stop - first)
        lib = _lib.load()
        X1, X2 = [], []
        for c in self.corpora:
            x12 = torch.empty(2 * n, c.dim, dtype=torch.float32, device=c.table.device)
            if n:
                _lib.check(lib.abn_gather_pairs(_lib.ptr(c.table), c.total, c.dim, _lib.ptr(i1), _lib.ptr(i2), first, n, n,
                                                None, 0, _lib.ptr(x12), None, None, _lib.stream()), 'abn_gather_pairs')
            X1.append(x12[:n])
            X2.append(x12[n:])
        return X1, X2, y[sl]

    def plan(self, train_mode=True):
        return None                    # (a list of tensors per tower: the iterator)
