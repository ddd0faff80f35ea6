"""PairsDataLoader on the MI355X: its batches against OriginalDataLoader.frames_from_pairs_device on the same grouped
pairs (the alignment itself is pinned against the C oracle elsewhere), the batch counts of the reference's iterator
test, and training from mined pairs through TrainerSiamese.train()."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_np  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from test_gpu_knn import planted_corpus  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mined(tmp_path_factory):
    from abnet3_amd.discovery import KnnPairMiner
    feats, times, _ = planted_corpus(np.random.default_rng(3))
    out = tmp_path_factory.mktemp('mined')
    pairs_path, map_path = KnnPairMiner(feats, times, lengths=(40, 60), k=10, min_similarity=0.5).write(str(out))
    return feats, times, pairs_path, map_path


@pytest.mark.parametrize('train_mode', [True, False])
def test_batches_equal_frames_from_pairs_device(mined, train_mode):
    from abnet3_amd.dataloader import OriginalDataLoader, PairsDataLoader
    from abnet3_amd.utils import group_pairs
    feats, times, pairs_path, map_path = mined
    dl = PairsDataLoader(pairs_path, None, map_path, ratio_split_train_test=0.6, batch_size=8, train_iterations=6,
                         test_iterations=4, split_method='files')
    random.seed(1)
    dl.set_data(feats, times)
    dl.load_data()
    mode = 'train' if train_mode else 'test'
    assert len(dl.pairs[mode]) > 8
    random.seed(5)
    got = [tuple(t.clone() for t in b) for b in dl.batch_iterator(train_mode)]
    state = random.getstate()
    random.seed(5)
    pairs = pairs_np.epoch_pairs(dl.pairs[mode], pairs_np.tokens_of(dl.pairs[mode]), dl.iterations[mode], 8, 0.5)
    assert random.getstate() == state
    ref = OriginalDataLoader('unused', 'unused', align_different_words=True)
    ref.features = dl.features
    want = pairs_np.batches(pairs, dl.iterations[mode], 8)
    assert len(got) == len(want) == dl.iterations[mode]
    n_same = 0
    for (X1, X2, y), batch in zip(got, want):
        R1, R2, ry = ref.frames_from_pairs_device(group_pairs(batch), frames=True)
        assert X1.is_cuda and X1.dtype == torch.float32 and y.dtype == torch.float64
        assert torch.equal(X1, R1) and torch.equal(X2, R2) and torch.equal(y, ry)
        n_same += int((y == 1).sum())
        assert set(y.cpu().tolist()) <= {1.0, -1.0}
    assert n_same > 0
    assert dl.statistics_training['SameType'] > 0 and dl.statistics_training['DiffType'] > 0


def test_batch_counts_of_the_reference_iterator_test():
    """test/test_dataloader.py:49-79: ids without a map, batch_size 2, 2 train and 3 test iterations -> 2 and 3
    batches.  With the 'files' split (the default split leaves this file's test set empty, and random.choices of no
    tokens raises, in the reference as here)."""
    from abnet3_amd.dataloader import PairsDataLoader
    dl = PairsDataLoader(os.path.join(GOLDEN, 'pairs_loader', 'pairs_knn.txt'), None, None, ratio_split_train_test=0.7,
                         train_iterations=2, test_iterations=3, proportion_positive_pairs=0.5, batch_size=2,
                         split_method='files')
    rng = np.random.default_rng(0)
    feats = {f: rng.standard_normal((79300, 3)).astype(np.float32) for f in range(5)}
    dl.set_data(feats, {f: np.arange(79300) * 0.01 for f in range(5)})
    random.seed(0)
    assert sum(1 for _ in dl.batch_iterator(train_mode=True)) == 2
    assert sum(1 for _ in dl.batch_iterator(train_mode=False)) == 3
    X1, X2, y = next(dl.batch_iterator(train_mode=True))
    assert X1.shape[1] == 3 and X1.shape == X2.shape and len(y) == len(X1)


def test_training_from_mined_pairs_lowers_the_dev_loss(mined, tmp_path):
    from abnet3_amd.dataloader import PairsDataLoader
    from abnet3_amd.loss import coscos2
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSiamese
    feats, times, pairs_path, map_path = mined
    dl = PairsDataLoader(pairs_path, None, map_path, ratio_split_train_test=0.6, batch_size=8, train_iterations=40,
                         test_iterations=15, split_method='files')
    random.seed(2)
    np.random.seed(2)
    torch.manual_seed(2)
    dl.set_data(feats, times)
    net = SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=100, output_dim=50, p_dropout=0.0,
                         activation_layer='sigmoid', output_path=str(tmp_path / 'network'))
    tr = TrainerSiamese(network=net, loss=coscos2(avg=False), num_epochs=3, patience=10, optimizer_type='adadelta',
                        lr=0.5, dataloader=dl, log_dir=str(tmp_path / 'runs'))
    tr.train()
    print('dev losses', tr.dev_losses, 'train losses', tr.train_losses)
    assert len(tr.dev_losses) == 4                       # the untrained pass, then three epochs
    assert all(np.isfinite(tr.dev_losses))
    assert tr.dev_losses[-1] < tr.dev_losses[0]
