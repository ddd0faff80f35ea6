"""abn_gmm_posteriors / abn_gmm_accumulate / abn_gmm_mstep and GmmPosteriorgram on the MI355X against tests/gmm_np.py.

The error bar.  Kernel and float32 numpy round the same products in different orders, so neither bounds the other.
Every error is scaled by the sum of the absolute values of the quantity's terms (float64 side); a case's yardstick
is the float32 numpy evaluation's own scaled maximum error against float64, and the kernel's scaled maximum must be
<= max(2^-22, 4 x yardstick).  The kernels have no score output: the scores are checked through lse, which is
1-Lipschitz in them (scale: the frame's largest score scale) and IS the score for K = 1 (three grid cases).
Posteriors: |dg| <= g expm1(2 bar) + 2^-22; statistics: the bar plus the posteriors' share sum_t |dg|_allowed |x~|.
The hard worst-case bound 2 (2D + 5) 2^-24 x scale on the scores must hold as well; through lse it is given the
fp32 log-sum-exp's own rounding on top: (K + 8) 2^-24 for the K-term sum, the exps and the log, and 2 x 2^-24 x scale
for the two roundings of max + log.  Each test prints the largest kernel / yardstick ratio it saw (-s shows it).

Largest kernel / yardstick ratio seen on the MI355X over all cases: 3.39 (lse; T = 129, K = 5, D = 100: kernel 3.46e-7
against 1.02e-7 of scale); posteriors reached 0.03 and statistics 0.025 of what they are allowed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLOOR = 2.0 ** -22
TS, KS, DS = (1, 127, 128, 129, 300, 1000), (1, 5, 127, 128, 130, 257), (1, 13, 39, 40, 100)
RATIOS = {'lse': 0.0, 'post': 0.0, 'stats': 0.0}


def shape_cases():
    cases, n = [], 0
    for T in TS:
        for K in KS:
            cases.append((T, K, DS[n % len(DS)], 0 if n % 2 == 0 else 2))       # n_ranges: by the grid / two ranges
            n += 1
    return cases


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_case(T, K, D, seed, spread=3.0, vlo=0.5, vhi=2.0, offset=0.0):
    """Frames around K centres, and a model near them: (x, shift, gv, w, m, v)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, D)) * spread
    x = (centres[rng.integers(0, K, size=T)] + rng.normal(size=(T, D)) + offset).astype(np.float32)
    shift = (x.astype(np.float64).mean(axis=0) if T > 1 else np.full(D, offset)).astype(np.float32)
    gv = np.maximum(x.astype(np.float64).var(axis=0), 1.0)
    m = centres + offset - shift.astype(np.float64) + 0.1 * rng.normal(size=(K, D))
    v = rng.uniform(vlo, vhi, size=(K, D))
    w = rng.dirichlet(np.full(K, 5.0))
    return x, shift, gv, w, m, v


def run_kernels(x, shift, gv, w, m, v, n_ranges=0, var_floor=0.01, min_count=1.0):
    """One E-step + M-step on the device: dict of host arrays."""
    from abnet3_amd import gmm
    table, dshift = dev(x, np.float32), dev(shift, np.float32)
    st = gmm.EMState(w, m, v, gv, table.device)
    A, B, c = (t.clone() for t in (st.A, st.B, st.c))
    lse, g = gmm.posteriors(table, dshift, A, B, c)
    lse2 = gmm.em_iteration(table, dshift, st, var_floor, min_count, n_ranges)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(lse, nan=7.0), torch.nan_to_num(lse2, nan=7.0))     # with and without the output
    return dict(lse=host(lse), g=host(g), sums=host(st.sums), stats=host(st.stats), w=host(st.w), mu=host(st.mu),
                var=host(st.var), A=host(st.A), B=host(st.B), c=host(st.c), A0=host(A), B0=host(B), c0=host(c))


def reference(x, shift, w, m, v):
    xc, bad = gmm_np.centre(x, shift)
    A, B, c = gmm_np.tables(w, m, v)
    out = dict(xc=xc, bad=bad, A=A, B=B, c=c, scale=gmm_np.score_scale(xc, bad, A, B, c))
    for name, dt in (('64', np.float64), ('32', np.float32)):
        s = gmm_np.scores(xc, bad, A, B, c, dt)
        lse, g = gmm_np.lse_post(s, bad)
        N, S1, S2 = gmm_np.statistics(g, xc, bad, dt)
        out.update({'s' + name: s, 'lse' + name: lse, 'g' + name: g, 'S' + name: np.concatenate([S1, S2, N[:, None]], axis=1)})
    return out


def check_case(got, ref, K, D, tag):
    """Both assertions of the module docstring on lse, posteriors and statistics; returns nothing, fills RATIOS."""
    bad, good = ref['bad'], ~ref['bad']
    assert np.array_equal(got['A0'], ref['A']) and np.array_equal(got['B0'], ref['B']) and np.array_equal(got['c0'], ref['c'])
    assert np.isnan(got['lse'][bad]).all() and not got['g'][bad].any()
    assert np.isfinite(got['lse'][good]).all() and np.isfinite(got['g']).all()
    if not good.any():
        return
    scale_t = ref['scale'].max(axis=1)[good]
    y_s = (np.abs(ref['s32'].astype(np.float64) - ref['s64'])[good] / ref['scale'][good]).max()
    y_l = (np.abs(ref['lse32'].astype(np.float64) - ref['lse64'])[good] / scale_t).max()
    yard = max(y_s, y_l)
    bar = max(FLOOR, 4.0 * yard)
    e_l = np.abs(got['lse'].astype(np.float64) - ref['lse64'])[good]
    k_l = (e_l / scale_t).max()
    print('%s: lse kernel %.3g yardstick %.3g (ratio %.2f, bar %.3g)' % (tag, k_l, yard, k_l / max(yard, FLOOR / 4), bar))
    RATIOS['lse'] = max(RATIOS['lse'], k_l / max(yard, FLOOR / 4))
    assert k_l <= bar, (tag, k_l, yard)
    hard = 2.0 * (2 * D + 5) * U * scale_t + (K + 8) * U + 2.0 * U * scale_t
    assert (e_l <= hard).all(), (tag, (e_l / hard).max())
    # posteriors
    bar_t = bar * scale_t
    g64 = ref['g64'][good]
    allowed = g64 * np.expm1(2.0 * bar_t)[:, None] + FLOOR
    e_g = np.abs(got['g'][good].astype(np.float64) - g64)
    RATIOS['post'] = max(RATIOS['post'], (e_g / allowed).max())
    assert (e_g <= allowed).all(), (tag, (e_g / allowed).max())
    assert np.abs(got['g'][good].astype(np.float64).sum(axis=1) - 1.0).max() < 1e-4
    # statistics [S1 | S2 | N]
    aug = np.abs(gmm_np.augment(ref['xc'], bad, np.float64))
    sscale = np.maximum(ref['g64'].T @ aug, 1e-300)
    y_st = (np.abs(ref['S32'].astype(np.float64) - ref['S64']) / sscale).max()
    share = np.zeros_like(sscale)
    share += (np.where(good[:, None], ref['g64'] * np.expm1(2.0 * bar * ref['scale'].max(axis=1))[:, None] + FLOOR, 0.0)).T @ aug
    e_st = np.abs(got['sums'] - ref['S64'])
    k_st = (e_st / sscale).max()
    print('%s: statistics kernel %.3g yardstick %.3g' % (tag, k_st, y_st))
    RATIOS['stats'] = max(RATIOS['stats'], (e_st / (max(FLOOR, 4.0 * y_st) * sscale + share)).max())
    assert (e_st <= max(FLOOR, 4.0 * y_st) * sscale + share).all(), (tag, k_st, y_st)
    assert got['stats'][1] == bad.sum() and got['stats'][3] == good.sum()
    assert abs(got['stats'][0] - ref['lse64'][good].sum()) <= (bar_t.sum() + 1e-9)


def check_mstep(got, gv, m_prev, v_prev, var_floor=0.01, min_count=1.0):
    """The M-step outputs against gmm_np's M-step applied to the kernel's own summed statistics (both float64)."""
    D = m_prev.shape[1]
    S = got['sums']
    w, m, v, starved = gmm_np.mstep(S[:, 2 * D], S[:, :D], S[:, D:2 * D], got['stats'][3], gv, m_prev, v_prev, var_floor, min_count)
    assert got['stats'][2] == starved
    for name, a, b in (('w', got['w'], w), ('mu', got['mu'], m), ('var', got['var'], v)):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), name
    A, B, c = gmm_np.tables(got['w'], got['mu'], got['var'])
    for name, a, b in (('A', got['A'], A), ('B', got['B'], B), ('c', got['c'], c)):
        fin = np.isfinite(b)
        assert np.array_equal(fin, np.isfinite(a)), name
        assert (np.abs(a[fin].astype(np.float64) - b[fin]) <= 2.0 ** -23 * np.abs(b[fin])).all(), name    # one rounding of a 1e-16 apart float64
    return starved


@pytest.mark.parametrize('T,K,D,n_ranges', shape_cases())
def test_e_step_and_m_step_on_the_shape_grid(T, K, D, n_ranges):
    x, shift, gv, w, m, v = make_case(T, K, D, seed=T * 1000 + K)
    got = run_kernels(x, shift, gv, w, m, v, n_ranges)
    check_case(got, reference(x, shift, w, m, v), K, D, 'T%d K%d D%d r%d' % (T, K, D, n_ranges))
    check_mstep(got, gv, m, v)
    print('largest kernel / bar ratios so far:', RATIOS)


def test_offset_table_centring_holds():
    x, shift, gv, w, m, v = make_case(300, 130, 39, seed=1, offset=50.0)
    assert abs(shift.mean() - 50.0) < 1.0
    got = run_kernels(x, shift, gv, w, m, v)
    ref = reference(x, shift, w, m, v)
    check_case(got, ref, 130, 39, 'offset +50')
    # ... and it is centring that holds it: the same frames without the offset give the same posteriors to the bar
    x0, shift0, _, _, _, _ = make_case(300, 130, 39, seed=1, offset=0.0)
    got0 = run_kernels(x0, shift0, gv, w, m + (shift.astype(np.float64) - 50.0 - shift0), v)
    assert np.abs(got0['g'] - got['g']).max() < 1e-2


def test_scores_spread_over_thousands_of_nats():
    x, shift, gv, w, m, v = make_case(300, 130, 40, seed=2, spread=30.0, vlo=0.05, vhi=0.2)
    ref = reference(x, shift, w, m, v)
    assert np.ptp(ref['s64'], axis=1).max() > 5000.0
    got = run_kernels(x, shift, gv, w, m, v)
    check_case(got, ref, 130, 40, 'spread')
    under = (ref['s64'] - ref['lse64'][:, None]) < -120.0
    assert under.any() and not got['g'][under].any()          # underflowed components are exactly 0


def test_far_component_is_starved_and_keeps_its_parameters():
    x, shift, gv, w, m, v = make_case(300, 5, 13, seed=3)
    m[2] = 1000.0
    got = run_kernels(x, shift, gv, w, m, v)
    check_case(got, reference(x, shift, w, m, v), 5, 13, 'far component')
    assert check_mstep(got, gv, m, v) == 1 and got['stats'][2] == 1
    assert np.array_equal(got['mu'][2], m[2]) and np.array_equal(got['var'][2], v[2])
    assert got['w'][2] < 1e-12 and abs(got['w'].sum() - 1.0) < 1e-12


def test_nan_and_inf_rows_are_counted_and_left_out():
    x, shift, gv, w, m, v = make_case(300, 130, 39, seed=4)
    rows = [0, 5, 127, 128, 299]
    xb = x.copy()
    xb[0, 3], xb[5, 0], xb[127, 38], xb[128, :], xb[299, 7] = np.nan, np.inf, -np.inf, np.nan, np.inf
    got = run_kernels(xb, shift, gv, w, m, v)
    ref = reference(xb, shift, w, m, v)
    assert list(np.flatnonzero(ref['bad'])) == rows
    check_case(got, ref, 130, 39, 'bad rows')
    assert got['stats'][1] == 5 and not got['g'][rows].any() and np.isnan(got['lse'][rows]).all()
    # the statistics are those of the table without the rows
    clean = np.delete(x, rows, axis=0)
    refc = reference(clean, shift, w, m, v)
    gotc = run_kernels(clean, shift, gv, w, m, v)
    sscale = np.maximum(refc['g64'].T @ np.abs(gmm_np.augment(refc['xc'], refc['bad'], np.float64)), 1e-300)
    assert np.abs(ref['S64'] - refc['S64']).max() < 1e-9
    assert (np.abs(got['sums'] - gotc['sums']) <= 2.0 ** -20 * sscale + 1e-5).all()


@pytest.mark.parametrize('T,n_ranges', [(300, 0), (300, 3), (1000, 3), (1000, 1)])
def test_frame_ranges(T, n_ranges):
    """300 frames: three ranges of one block, the last of 44 frames; 1000 frames in three ranges: 3, 3 and 2 blocks,
    the last block of 104 frames; one range: every block in one workgroup's registers.  Same statistics to the bar,
    and the same bits whenever the ranges are the same."""
    x, shift, gv, w, m, v = make_case(T, 130, 39, seed=5)
    got = run_kernels(x, shift, gv, w, m, v, n_ranges)
    check_case(got, reference(x, shift, w, m, v), 130, 39, 'T%d ranges %d' % (T, n_ranges))
    if T == 300:
        other = run_kernels(x, shift, gv, w, m, v, 3 - n_ranges)          # by the grid = 3 ranges here
        assert np.array_equal(other['sums'], got['sums'])


def test_two_calls_are_bit_identical():
    x, shift, gv, w, m, v = make_case(1000, 257, 40, seed=6)
    x[17, 2] = np.nan
    a = run_kernels(x, shift, gv, w, m, v)
    b = run_kernels(x, shift, gv, w, m, v)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.fixture(scope='module')
def separated():
    rng = np.random.default_rng(11)
    centres = np.array([[0.0, 0.0, 0.0], [12.0, 0.0, 3.0], [0.0, 12.0, -3.0], [-12.0, -12.0, 6.0]]) + 20.0
    lab = rng.integers(0, 4, size=2000)
    return (centres[lab] + rng.normal(size=(2000, 3))).astype(np.float32), lab


def test_fit_five_iterations(separated):
    from abnet3_amd.gmm import GmmPosteriorgram
    x, _ = separated
    g = GmmPosteriorgram(4, n_iter=5, tol=-np.inf).fit(dev(x, np.float32))
    assert len(g.log_likelihoods) == 5 and g.n_bad_ == 0
    kw = dict(n_iter=5, tol=-np.inf, shift=g.shift_, gv=g.gv_)
    r64, r32 = gmm_np.fit(x, 4, dtype=np.float64, **kw), gmm_np.fit(x, 4, dtype=np.float32, **kw)
    sm = np.abs(r64['m']).max() + np.sqrt(r64['v'].max())
    mine_m = g.means_ - g.shift_.astype(np.float64)
    for name, mine, a64, a32, sc in (('means', mine_m, r64['m'], r32['m'], sm), ('weights', g.weights_, r64['w'], r32['w'], 1.0),
                                      ('variances', g.variances_, r64['v'], r32['v'], sm * sm)):
        yard, k = np.abs(a32 - a64).max() / sc, np.abs(mine - a64).max() / sc
        print('fit %s: kernel %.3g yardstick %.3g' % (name, k, yard))
        assert k <= max(FLOOR, 4.0 * yard), (name, k, yard)
    ll64, ll32, ll = (np.asarray(a) for a in (r64['log_likelihoods'], r32['log_likelihoods'], g.log_likelihoods))
    wobble = max(FLOOR * np.abs(ll64).max(), 4.0 * np.abs(ll32 - ll64).max())
    assert (np.diff(ll) >= -wobble).all(), ll
    assert np.abs(ll - ll64).max() <= max(FLOOR * np.abs(ll64).max(), 4.0 * np.abs(ll32 - ll64).max()), (ll, ll64)
    assert abs(g.score(dev(x, np.float32)) - gmm_np.em_iteration(
        *gmm_np.centre(x, g.shift_), g.weights_, mine_m, g.variances_, g.gv_)[0]) < 1e-4


def test_fit_stops_on_tol_and_refuses_too_few_frames(separated):
    from abnet3_amd.gmm import GmmPosteriorgram
    x, _ = separated
    g = GmmPosteriorgram(4, n_iter=50, tol=1e-4).fit(dev(x, np.float32))
    ll = g.log_likelihoods
    assert 2 <= len(ll) < 50 and ll[-1] - ll[-2] < 1e-4
    xb = x[:6].copy()
    xb[:3] = np.nan
    with pytest.raises(ValueError, match='T < K'):
        GmmPosteriorgram(4).fit(dev(xb, np.float32))


def test_transform_of_a_corpus_and_downstream():
    from abnet3_amd import gmm
    from abnet3_amd.abx import ABXEvaluator, kl_tables
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=60, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    post = g.transform(corpus)
    assert isinstance(post, DeviceCorpus) and post.names == corpus.names and post.dim == 8 and post.total == corpus.total
    for k in corpus.names:
        assert post.length[k] == corpus.length[k] and post.offset[k] == corpus.offset[k]
        assert np.array_equal(post.times[k], corpus.times[k])
    shift, A, B, c = g.device_tables(corpus.table.device)
    _, direct = gmm.posteriors(corpus.table, shift, A, B, c)
    assert torch.equal(post.table, direct)                                        # row for row
    assert torch.equal(g.transform(corpus.table), direct) and torch.equal(g.transform(feats), direct)
    assert int(kl_tables(post.table).bad.sum().item()) == 0
    assert abs(float(post.table.sum(dim=1).mean().item()) - 1.0) < 1e-5
    r = ABXEvaluator(items, post, distance='kl').run('within')
    print('ABX (kl) on GMM posteriorgrams:', r)
    assert r.error < 50.0                 # the plumbing, not a quality claim
