"""abnet3_amd.sampler without a GPU: the host parts against what the reference produced (tests/golden/sampler,
tools/make_golden.py G15), the written-down distribution (explicit_table) against the reference's table, and the
tables abn_sample_pairs reads -- through tests/sampler_np.py, the restatement of the device path -- against that
distribution, exactly (Python integers) and by drawing."""
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import sampler_np
from abnet3_amd import sampler as S

DIR = os.path.join(GOLDEN, 'sampler')
MODES = [('log', 'log'), ('f', 'f'), ('f2', '1'), ('1', '1')]
ALL_MODES = ['1', 'f', 'f2', 'log', 'fcube']
FIXTURES = ['english', 'english_split', 'small', 'collide']
# seeds of the 10^6-pair draws (one per configuration); the restatement passes with these
DRAW_SEEDS = {'Stype_Sspk': 11, 'Stype_Dspk': 12, 'Dtype_Sspk': 13, 'Dtype_Dspk': 14}
N_DRAWS = 10 ** 6


@pytest.fixture(scope='module')
def ref():
    with open(os.path.join(DIR, 'reference.json')) as fh:
        record = json.load(fh)
    record['p'] = dict(np.load(os.path.join(DIR, 'probabilities.npz'), allow_pickle=False))
    return record


def ref_table(ref, name, modes, config):
    """{key tuple: probability} as the reference returned it."""
    tag = '%s/%s,%s/%s' % (name, modes[0], modes[1], config)
    n_spk = {'Stype_Sspk': 1, 'Stype_Dspk': 2, 'Dtype_Sspk': 1, 'Dtype_Dspk': 2}[config]
    out = {}
    for key, p in zip(ref['p'][tag + '/keys'].tolist(), ref['p'][tag + '/p'].tolist()):
        parts = key.split('|')
        out[tuple(parts[:n_spk]) + tuple(int(v) for v in parts[n_spk:])] = p
    return out


_DESCR = {}


def described(ref, name):
    """(sampler, clusters, description) of a fixture, computed once."""
    if name not in _DESCR:
        fx = ref['fixtures'][name]
        sam = S.SamplerClusterSiamese()
        clusters = sam.parse_input_file(os.path.join(DIR, fx['classes']))
        spk_of = S.read_spkid_file(os.path.join(DIR, fx['spkid']))
        sam.spkid_from_file = spk_of
        _DESCR[name] = (sam, clusters, sam.analyze_clusters(clusters, spk_of))
    return _DESCR[name]


_TABLES = {}


def tables_of(ref, name, modes):
    if (name, modes) not in _TABLES:
        _TABLES[(name, modes)] = sampler_np.build_tables(described(ref, name)[2], *modes)
    return _TABLES[(name, modes)]


# -- host parts against the golden records ------------------------------------------------------------------------

@pytest.mark.parametrize('name', FIXTURES)
def test_parse_split_analysis_and_token_dict_equal_the_reference(ref, name):
    fx = ref['fixtures'][name]
    sam, clusters, descr = described(ref, name)
    assert clusters == fx['clusters']
    assert sam.ratio_train_dev == fx['ratio_train_dev']
    train, dev = sam.split_each_file(clusters)
    assert train == fx['split_each_file']['train'] and dev == fx['split_each_file']['dev']
    assert set(descr) == set(fx['descr'])
    for k, v in fx['descr'].items():
        mine = descr[k]
        if isinstance(v, dict):
            assert {str(a): int(b) for a, b in mine.items()} == v, k
        else:
            assert [x.item() if hasattr(x, 'item') else x for x in mine] == v, k
    token_dict = sam.generate_token_dict(descr)
    assert [[t, str(s), ids] for (t, s), ids in token_dict.items()] == fx['token_dict']


def test_counts_equal_the_reference(ref):
    for case in ref['fixtures']['small']['sample_batch_counts']:
        assert S.pair_counts(case['num_samples'], case['ratio_same_diff_spk'], case['ratio_same_diff_type']) == case['counts'], case


def test_default_num_samples_is_pairs_of_the_poorest_speaker(ref, tmp_path, monkeypatch):
    """num_total_sampled_pairs None: num (num - 1) / 2, num = the fewest tokens of any speaker (sampler.py:766-768)."""
    sam, clusters, descr = described(ref, 'small')
    seen = {}
    monkeypatch.setattr(S.SamplerClusterSiamese, 'write_tokens', lambda self, **kw: seen.update(kw) or 0)
    sam.export_pairs(out_dir=str(tmp_path), descr=descr, num_samples=None)
    num = min(descr['speakers'].values())
    assert seen['num_samples'] == num * (num - 1) / 2 and num >= 2


# -- the reference's own test/test_sampler.py ---------------------------------------------------------------------

ENGLISH = [[['s0102a', 149.359, 149.66]],
           [['s2401a', 70.782, 71.282], ['s2402b', 14.639, 15.234], ['s2403b', 96.311, 96.739],
            ['s2404b', 96.311, 96.739], ['s2405b', 96.311, 96.739]],
           [['s2403a', 258.748, 259.267]], [['s0102a', 152.623, 153.083]], [['s2702a', 31.902, 32.37]],
           [['s0101a', 295.416, 295.955], ['s0101a', 546.471, 546.681]],
           [['s2001a', 217.712, 218.591], ['s2001a', 546.471, 546.681]]]
SPK_OF = {'s0101a': 1, 's0102a': 1, 's2001a': 20, 's2401a': 24, 's2402b': 24, 's2403b': 24, 's2404b': 24, 's2405b': 24,
          's2403a': 24, 's2702a': 27}


def n_words(clusters):
    return sum(len(c) for c in clusters)


def test_reference_test_parse_input_file():
    sam = S.SamplerClusterSiamese()
    assert sam.parse_input_file(input_file=os.path.join(DIR, 'english.test.classes')) == ENGLISH
    assert len(sam.parse_input_file(os.path.join(DIR, 'english.test.classes'), max_num_clusters=3)) == 3


@pytest.mark.parametrize('method', ['split_clusters_ratio', 'split_clusters_on_file'])
def test_reference_test_random_splits(method):
    sam = S.SamplerClusterSiamese()
    clusters = sam.parse_input_file(os.path.join(DIR, 'english.test.classes'))
    sam.spkid_from_file = SPK_OF
    train, dev = getattr(sam, method)(clusters)
    assert n_words(train) + n_words(dev) == n_words(clusters)
    assert getattr(sam, method)(clusters) == (train, dev)                    # seeded: a run is repeatable
    other = S.SamplerClusterSiamese(seed=5)
    other.spkid_from_file = SPK_OF
    assert n_words(getattr(other, method)(clusters)[0]) + n_words(getattr(other, method)(clusters)[1]) == n_words(clusters)
    sam = S.SamplerClusterSiamese(max_size_cluster=3)
    train, dev = sam.split_clusters_ratio(clusters)
    assert n_words(train) + n_words(dev) == n_words(clusters)
    assert max(len(c) for c in train) <= 3


def test_reference_test_split_each_file():
    sam = S.SamplerClusterSiamese()
    clusters = sam.parse_input_file(os.path.join(DIR, 'english.split.test.classes'))
    sam.spkid_from_file = SPK_OF
    train, dev = sam.split_each_file(clusters)
    assert train == [[['s0102a', 10.0, 20.0], ['s0102a', 40.0, 50.0]], [['s2401a', 10.0, 20.0], ['s2402b', 40.0, 50.0]]]
    assert dev == [[['s2402b', 75.0, 100.0]], [['s0102a', 75.0, 100.0]]]


# -- the distribution as written down against the reference's table -----------------------------------------------

def assert_tables_match(mine, theirs, tol=1e-12):
    assert set(mine) == set(theirs), set(mine) ^ set(theirs)
    for k, p in theirs.items():
        assert abs(mine[k] - p) <= tol * p, (k, mine[k], p)


def colliding_keys(descr):
    """Dtype_Dspk keys that the reference writes twice: (s, s', i, j) for cells (s, i), (s, j), (s', i), (s', j)."""
    cells = set(zip((str(s) for s in descr['tokens_speaker']), descr['tokens_type']))
    speakers, types = sorted(set(s for s, t in cells)), sorted(set(t for s, t in cells))
    return set((s, s2, i, j) for s in speakers for s2 in speakers if s != s2 for i in types for j in types
               if i < j and {(s, i), (s, j), (s2, i), (s2, j)} <= cells)


@pytest.mark.parametrize('name,modes', [('small', m) for m in MODES] + [(n, m) for n in ('english', 'english_split') for m in MODES[2:]])
def test_explicit_table_equals_the_reference(ref, name, modes):
    """On the collision-free fixture in every recorded mode, on the reference's fixtures in speaker mode '1'."""
    descr = described(ref, name)[2]
    for config in S.CONFIGS:
        keys, p = S.explicit_table(descr, config, *modes)
        theirs = ref_table(ref, name, modes, config)
        if not theirs:
            assert not keys
            continue
        assert_tables_match(dict(zip(keys, p.tolist())), theirs)


@pytest.mark.parametrize('name', ['english', 'english_split', 'collide'])
@pytest.mark.parametrize('modes', MODES[:2])
def test_tables_differ_from_the_reference_exactly_in_colliding_keys(ref, name, modes):
    """The three collision-free configurations match.  Dtype_Dspk: the key sets are equal, and the keys whose
    probability differs are EXACTLY the keys of colliding quadruples, computed here from the cells: under such a key the
    reference holds its later write alone, the definition both ordered pairs of cells.  Every probability is divided
    by the sum over all keys, so a collision moves the others too: they are compared after renormalising both tables
    over the keys that do not collide (`collide`: one quadruple beside 14 free keys), and a colliding key by its ratio
    to that free mass (to the whole table where every key collides: `english_split`).  Without a quadruple
    (`english`) this is plain equality."""
    descr = described(ref, name)[2]
    for config in S.CONFIGS[:3]:
        keys, p = S.explicit_table(descr, config, *modes)
        theirs = ref_table(ref, name, modes, config)
        assert len(keys) == len(theirs)
        if theirs:
            assert_tables_match(dict(zip(keys, p.tolist())), theirs)
    keys, p = S.explicit_table(descr, 'Dtype_Dspk', *modes)
    mine, theirs = dict(zip(keys, p.tolist())), ref_table(ref, name, modes, 'Dtype_Dspk')
    collide = colliding_keys(descr)
    assert len(collide) == 2 * ref['fixtures'][name]['n_colliding_quadruples'] and collide <= set(mine)
    assert set(mine) == set(theirs)
    free = [k for k in mine if k not in collide]
    assert {'english': not collide, 'english_split': not free, 'collide': bool(collide) and bool(free)}[name]
    zm = math.fsum(mine[k] for k in free) if free else 1.0
    zt = math.fsum(theirs[k] for k in free) if free else 1.0
    differ = set(k for k in mine if abs(mine[k] / zm - theirs[k] / zt) > 1e-12 * theirs[k] / zt)
    assert differ == collide, (differ ^ collide)
    if collide:                       # the definition holds BOTH ordered pairs of cells under a colliding key
        pairs, pp = S.explicit_table(descr, 'Dtype_Dspk', *modes, return_cells=True)
        for k in collide:
            under = [v for ((sa, ta), (sb, tb)), v in zip(pairs, pp.tolist()) if (sa, sb, min(ta, tb), max(ta, tb)) == k]
            assert len(under) == 2 and abs(sum(under) - mine[k]) <= 1e-15


def test_explicit_table_refuses_large_inputs(ref):
    descr = described(ref, 'small')[2]
    with pytest.raises(ValueError, match='max_keys'):
        S.explicit_table(descr, 'Dtype_Dspk', max_keys=100)
    assert len(S.explicit_table(descr, 'Stype_Sspk', max_keys=100)[0]) == 23


# -- the device tables: layout, realised distribution, draws -------------------------------------------------------

@pytest.mark.parametrize('name', FIXTURES)
@pytest.mark.parametrize('mode', ALL_MODES)
def test_package_tables_equal_the_restatement(ref, name, mode):
    descr = described(ref, name)[2]
    mine, theirs = S.build_tables(descr, mode, mode), sampler_np.build_tables(descr, mode, mode)
    assert set(mine) == set(theirs)
    for k, v in theirs.items():
        if isinstance(v, np.ndarray):
            assert mine[k].dtype == v.dtype and mine[k].shape == v.shape and np.array_equal(mine[k], v), k
        else:
            assert mine[k] == v, k


@pytest.mark.parametrize('name,modes', [('small', m) for m in MODES] + [('english', MODES[0]), ('english_split', MODES[0]), ('collide', MODES[0])])
def test_realised_distribution_is_within_the_derived_bound(ref, name, modes):
    """Exactly (Fractions) from the tables and the restated searches: every key the definition gives is realised
    within distribution_bound (two quantised factors per weight, two mapped draws), no other
    key is realised at all, and the total is 1 to the mapping's bias."""
    descr, t = described(ref, name)[2], tables_of(ref, name, modes)
    bound = sampler_np.distribution_bound(t)
    assert bound < Fraction(1, 10 ** 6)
    for q, config in enumerate(S.CONFIGS):
        keys, p = S.explicit_table(descr, config, *modes)
        realised = sampler_np.realised_by_key(t, q)
        defined = {k: v for k, v in zip(keys, p.tolist()) if v > 0}
        assert set(realised) == set(defined), (config, set(realised) ^ set(defined))
        assert (int(t['total'][q]) == 0) == (not defined)
        for k, v in defined.items():
            # (explicit_table is float64: 1e-13 relative covers its own rounding)
            assert abs(realised[k] - Fraction(v)) <= (bound + Fraction(1, 10 ** 13)) * Fraction(v), (config, k)
        if defined:
            assert abs(sum(realised.values()) - 1) <= Fraction(1, 1 << 60)


@pytest.fixture(scope='module')
def million(ref):
    """10^6 pairs per configuration on the small fixture ('log', 'log'), drawn once by the restatement."""
    t = tables_of(ref, 'small', MODES[0])
    out = {}
    for q, config in enumerate(S.CONFIGS):
        counts = [0, 0, 0, 0]
        counts[q] = N_DRAWS
        out[config] = sampler_np.sample_pairs(t, counts, DRAW_SEEDS[config])
    return out


@pytest.mark.parametrize('q', range(4))
def test_a_million_draws_follow_the_definition(ref, million, q):
    """Every line key's count lies within 6 sqrt(N p (1 - p)) + 1 of N p, nothing of probability 0 is drawn, and a
    Stype_Sspk pair has two distinct tokens of its cell.  (Dtype_Dspk's keys (s, s', i, j) and (s', s, i, j) emit the
    same lines -- lower type first -- and are counted together.)"""
    config = S.CONFIGS[q]
    descr, t = described(ref, 'small')[2], tables_of(ref, 'small', MODES[0])
    tok1, tok2, key, ca, cb = million[config]
    assert len(tok1) == N_DRAWS and (tok1 >= 0).all() and (tok2 >= 0).all()
    spk, typ = np.asarray(descr['tokens_speaker']), np.asarray(descr['tokens_type'])
    # the tokens belong to the cells the pair was drawn for
    names = np.asarray(t['speakers'])
    assert (spk[tok1] == names[t['spk_t'][ca]]).all() and (typ[tok1] == t['type_t'][ca]).all()
    assert (spk[tok2] == names[t['spk_t'][cb]]).all() and (typ[tok2] == t['type_t'][cb]).all()
    if q == 0:
        assert (tok1 != tok2).all() and (ca == cb).all()
    if q >= 2:
        assert (typ[tok1] < typ[tok2]).all()
    assert ((spk[tok1] == spk[tok2]) == (q in (0, 2))).all() and ((typ[tok1] == typ[tok2]) == (q in (0, 1))).all()
    pairs, p = S.explicit_table(descr, config, *MODES[0], return_cells=True)
    expected = {}
    for (a, b), v in zip(pairs, p.tolist()):
        if q >= 2 and b[1] < a[1]:
            a, b = b, a
        expected[(a, b)] = expected.get((a, b), 0.0) + v
    cell_id = ca.astype(np.int64) * t['n_cells'] + cb
    ids, counts = np.unique(cell_id, return_counts=True)
    cell = [(t['speakers'][s], int(ty)) for s, ty in zip(t['spk_t'], t['type_t'])]
    seen = {(cell[i // t['n_cells']], cell[i % t['n_cells']]): int(n) for i, n in zip(ids.tolist(), counts.tolist())}
    assert set(seen) <= set(k for k, v in expected.items() if v > 0), 'a key of probability 0 was drawn'
    for k, v in expected.items():
        n = seen.get(k, 0)
        assert abs(n - N_DRAWS * v) <= 6 * math.sqrt(N_DRAWS * v * (1 - v)) + 1, (config, k, n, N_DRAWS * v)
    if q == 0:                                  # both orders of a cell's token pairs turn up, about equally
        assert abs(int((tok1 < tok2).sum()) - N_DRAWS / 2) <= 6 * math.sqrt(N_DRAWS / 4) + 1
    assert len(np.unique(key)) > N_DRAWS - 10 and (key >= 0).all()


def test_draws_do_not_depend_on_how_many_are_asked_for(ref):
    """Counter-based: pair i of configuration q is the same whatever the counts around it."""
    t = tables_of(ref, 'small', MODES[0])
    a = sampler_np.sample_pairs(t, [65, 64, 63, 1], 7)
    b = sampler_np.sample_pairs(t, [10, 64, 0, 1], 7)
    for x, y in zip(a, b):
        assert np.array_equal(x[:10], y[:10]) and np.array_equal(x[65:129], y[10:74]) and x[-1] == y[-1]


# -- the class surface --------------------------------------------------------------------------------------------

def test_buckeye_arguments_construct_the_sampler(ref):
    cfg = ref['buckeye_sampler']
    sam = getattr(S, cfg['class'])(**cfg['arguments'])
    assert sam.whoami()['class_name'] == 'SamplerClusterSiamese'
    params = sam.whoami()['params']
    for k, v in cfg['arguments'].items():
        assert params[k] == v
    assert params['type_sampling_mode'] == 'log' and params['split_method'] == 'clusters' and params['max_num_clusters'] is None
    with open(os.path.join(GOLDEN, 'gridsearch_buckeye.json')) as fh:
        assert json.load(fh)['default_params']['sampler'] == cfg
    assert S.DummySampler(batch_size=3).whoami()['class_name'] == 'DummySampler'
    assert issubclass(S.SamplerClusterSiamese, S.SamplerCluster) and issubclass(S.SamplerPairs, S.SamplerBuilder)
    with pytest.raises(AssertionError):
        S.SamplerClusterSiamese(run='sometimes')
    with pytest.raises(AssertionError):
        S.SamplerClusterSiamese(split_method='halves')
    with pytest.raises(NotImplementedError):
        S.SamplerCluster().whoami()


def test_the_entry_point_is_declared_bound_and_exported():
    import ctypes
    from abnet3_amd import _lib, build
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+abn_sample_pairs\s*\(', header)
    assert 'abn_sample_pairs' in _lib.SYMBOLS and 'sampler.hip' in build.SOURCES
    build.build()
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(lib._name), 'abn_sample_pairs')
    assert ctypes.sizeof(_lib.SamplerTables) == 16 + 32 + 16 * 8
    # argument errors come back before any launch (no GPU here)
    n = (ctypes.c_int64 * 4)(1, 0, 0, 0)
    assert lib.abn_sample_pairs(None, n, 0, None, None, None, 256, None) == _lib.E_ARG
    assert b'null' in lib.abn_last_error()
    t = _lib.SamplerTables()
    assert lib.abn_sample_pairs(ctypes.byref(t), n, 0, None, None, None, 256, None) == _lib.E_ARG
    assert b'n_cells' in lib.abn_last_error()
