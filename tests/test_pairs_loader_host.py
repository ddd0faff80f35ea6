"""PairsDataLoader without a GPU: load_pairs against the lists the reference's own class produced for its own
test files (tests/golden/pairs_loader/, tools/make_golden.py G14), and the epoch's pair list against the plain
restatement (tests/pairs_np.py).

The reference's test (test/test_dataloader.py:26-27) asserts 12 train / 6 test pairs at ratio 0.5 with the
constructor's default split method.  That default is 'split_each_file', for which the reference's load_pairs itself
yields 1 / 5 on these files (recorded in load_pairs.json); 12 / 6 is what its 'files' split yields, for any draw
(two of five files test: 3 file pairs x 2 lines; three train: 6 x 2).  Both facts are asserted below."""
import json
import os
import pickle
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_np  # noqa: E402
from conftest import GOLDEN  # noqa: E402

DIR = os.path.join(GOLDEN, 'pairs_loader')
PAIRS, IDS = os.path.join(DIR, 'pairs_knn.txt'), os.path.join(DIR, 'id_to_file.txt')
CASES = json.load(open(os.path.join(DIR, 'load_pairs.json')))['cases']


def loader(**kw):
    from abnet3_amd.dataloader import PairsDataLoader
    kw.setdefault('id_to_file', None)
    return PairsDataLoader(pairs_path=PAIRS, features_path=None, **kw)


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-%s-%s' % (c['split_method'], c['ratio'], 'names' if c['id_to_file'] else 'ids'))
def test_load_pairs_equals_the_reference(case):
    dl = loader(id_to_file=IDS if case['id_to_file'] else None, ratio_split_train_test=case['ratio'],
                split_method=case['split_method'])
    random.seed(case['seed'])
    dl.load_pairs()
    assert dl.pairs['train'] == case['train']
    assert dl.pairs['test'] == case['test']
    assert sorted(list(t) for t in dl.tokens['train']) == case['tokens_train']
    assert sorted(list(t) for t in dl.tokens['test']) == case['tokens_test']
    assert sorted(dl.files) == case['files']
    assert all(len(p) == 6 for p in dl.pairs['train'] + dl.pairs['test'])
    if case['id_to_file']:
        names = ['file%d' % i for i in range(5)]
        assert all(p[0] in names and p[3] in names for p in dl.pairs['train'] + dl.pairs['test'])
    else:
        assert all(isinstance(p[0], int) and isinstance(p[3], int) for p in dl.pairs['train'] + dl.pairs['test'])
    # the restatement agrees too
    random.seed(case['seed'])
    split = pairs_np.split_files if case['split_method'] == 'files' else pairs_np.split_each_file
    train, test = split(pairs_np.read_pairs(PAIRS, IDS if case['id_to_file'] else None), case['ratio'])
    assert (train, test) == (case['train'], case['test'])


@pytest.mark.parametrize('seed', range(5))
def test_counts_at_half(seed):
    """12 / 6 for the 'files' split whatever the draw; 1 / 5 for 'split_each_file' (module docstring)."""
    dl = loader(id_to_file=IDS, ratio_split_train_test=0.5, split_method='files')
    random.seed(seed)
    dl.load_pairs()
    assert (len(dl.pairs['train']), len(dl.pairs['test'])) == (12, 6)
    dl = loader(id_to_file=IDS, ratio_split_train_test=0.5)
    assert dl.split_method == dl.SPLIT_EACH_FILE
    dl.load_pairs()
    assert (len(dl.pairs['train']), len(dl.pairs['test'])) == (1, 5)


def test_class_surface():
    from abnet3_amd import dataloader
    cls = dataloader.PairsDataLoader
    assert (cls.SPLIT_FILES, cls.SPLIT_EACH_FILE) == ('files', 'split_each_file')
    assert cls.SPLIT_METHODS == ['files', 'split_each_file']
    dl = loader()
    assert (dl.ratio_split_train_test, dl.batch_size, dl.iterations, dl.proportion_positive_pairs,
            dl.align_different_words, dl.split_method) == (0.7, 8, {'train': 10000, 'test': 500}, 0.5, True,
                                                           'split_each_file')
    assert dl.pairs == {'train': None, 'test': None} and dl.tokens == {'train': [], 'test': []}
    assert dl.plan(True) is None and dl.plan(False) is None
    assert dl.whoami() == {'params': (PAIRS, None, None, 0.7, True, 0.5), 'class_name': 'PairsDataLoader'}
    with pytest.raises(AssertionError):
        loader(split_method='halves')
    back = pickle.loads(pickle.dumps(loader(id_to_file=IDS, ratio_split_train_test=0.5, split_method='files')))
    assert back.__getstate__() == (PAIRS, None, IDS, 0.5, True, 0.5)
    assert back.pairs['train'] is not None            # __setstate__ reloads the pairs


@pytest.mark.parametrize('ratio,batch,it_train,it_test,prop', [
    (0.7, 2, 2, 3, 0.5),          # the reference's iterator test: 2 and 3 batches
    (0.5, 4, 3, 2, 0.5),
    (0.5, 8, 50, 40, 0.5),        # more positives asked than there are: the clamp, negatives fill the epoch
    (0.5, 3, 5, 5, 1.0),          # positives only ... as far as they go
    (0.5, 3, 4, 4, 0.0),          # negatives only
])
@pytest.mark.parametrize('method', ['files', 'split_each_file'])
def test_epoch_pairs_equal_the_restatement(method, ratio, batch, it_train, it_test, prop, capsys):
    dl = loader(ratio_split_train_test=ratio, batch_size=batch, train_iterations=it_train, test_iterations=it_test,
                proportion_positive_pairs=prop, split_method=method)
    random.seed(11)
    dl.load_pairs()
    for seed, train_mode in ((0, True), (1, False), (2, True)):
        mode = 'train' if train_mode else 'test'
        if not dl.tokens[mode]:
            continue                                  # (random.choices of nothing raises, here as in the reference)
        its = it_train if train_mode else it_test
        random.seed(seed)
        mine = dl.epoch_pairs(train_mode)
        state = random.getstate()
        random.seed(seed)
        ref = pairs_np.epoch_pairs(dl.pairs[mode], pairs_np.tokens_of(dl.pairs[mode]), its, batch, prop)
        assert mine == ref
        assert random.getstate() == state             # the same number of draws
        assert len(mine) == its * batch
        n_pos = sum(p[6] == 'same' for p in mine)
        assert n_pos == min(int(its * batch * prop), len(dl.pairs[mode]))
        assert len(pairs_np.batches(mine, its, batch)) == its
    if prop == 0.5 and batch == 8:
        assert 'Not enough positive pairs' in capsys.readouterr().out
