"""Sparse transitions and far-apart emissions for the HMM chains (test infrastructure only): deterministic cases at the
feature level, the classification of an utterance as *in range* or *in the window*, and the invariants that need no
representation.

The chains of csrc/hmm_dense.hip and csrc/hmm.hip keep ahat, e = b bhat / c_t and bhat as linear-domain fp32.  The bars of
tests/test_gpu_hmm_dense.py and tests/test_gpu_hmm.py assume that every factor of every path is perturbed only
relatively; where a path's per-frame relative weight has to drop below about 2^-126 to be represented that is false (the
cause is range, not rounding).  This file builds the models that reach that region and says, from the float64 and float32
restatements alone, which utterances are still inside the unchanged bars (in range) and which are not (in the window).

The features.  Unit variances, D = 16, the mean of state k the code word a (B[k % 16] | B[k // 16]): B the 16 rows of the
biorthogonal code of length 8 (the Sylvester-Hadamard matrix H8 over its negative), a = sqrt(g / 8).  Two different words
differ in 4, 8, 12 or 16 coordinates, by 2 a each, so the score gap at a mean, |mu_j - mu_k|^2 / 2, is 8 a^2 hd / 4: g for
the nearest pairs (Hamming distance 4), 2 g, 3 g or 4 g for the others, and every mean has the norm sqrt(2 g).  K <= 256.
A frame is x_t = mean[s_t] + JITTER N(0, 1) along a planted state sequence s: the first state uniform, then the state is
kept with probability 1/2 and otherwise replaced by a uniform draw from the other states, so about half the transitions
of a sparse matrix are forced through its floor.

The matrices (floor eps = 2^-80 or 2^-100 on every other entry, each row renormalised once in float64 and rounded to
float32; 1 + K eps is 1 in float64, so a floor entry stays eps exactly):
    cyclic          stay 1/2, next (k + 1 mod K) 1/2; init uniform
    left_to_right   stay 1/2, next 1/2 without the wrap (the last state stays with 1); init: state 0, the floor elsewhere
    blocks          blocks of BLOCK states, uniform inside a block, the floor between the blocks; init: the first block
    counts          what the transition M-step makes (at alpha = 0) of the bigram and first-frame counts of the first two planted
                    sequences: count / row total, a row without a count uniform, then the floor; init likewise
The sticky model: weights with some components at 2^-79 .. 2^-60, some retired to 0 and the rest sharing the mass, and stay
in STAYS."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_dense_np as dn  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_np  # noqa: E402
from test_gpu_hmm import Case, FLOOR, U  # noqa: E402
from test_gpu_hmm_dense import DenseCase, stats_bar  # noqa: E402

D = 16
JITTER = 0.1
BLOCK = 4
N_UTT = 8
SHAPES = ((4, 24), (65, 300), (128, 140))                # (K, L) of the grid
EPS_EXP = (80, 100)                                      # the floors 2^-80 (TRANS_MIN) and 2^-100 (the constructor's promise)
GAPS = (20, 60, 90, 120, 160, 300)
MATRICES = ('cyclic', 'left_to_right', 'blocks', 'counts')
STAYS = (0.0, 0.9, 1.0 - 2.0 ** -20)


# ---- the features ------------------------------------------------------------------------------------------------------
def code_words(K):
    """[K, 16] of +-1: the module docstring's words."""
    assert 1 <= K <= 256
    h = np.array([[1.0]])
    for _ in range(3):
        h = np.block([[h, h], [h, -h]])
    b = np.concatenate([h, -h])
    k = np.arange(K)
    return np.concatenate([b[k % 16], b[k // 16]], axis=1)


def means(K, gap):
    return np.sqrt(gap / 8.0) * code_words(K)


def planted_states(rng, K, L):
    s = np.zeros(L, dtype=np.int64)
    for t in range(L):
        if t == 0 or (K > 1 and rng.random() >= 0.5):
            z = int(rng.integers(0, K if t == 0 else K - 1))
            s[t] = z if t == 0 or z < s[t - 1] else z + 1
        else:
            s[t] = s[t - 1]
    return s


def features(K, L, gap, seed, n_utt=N_UTT, bad_rows=()):
    """(x [n_utt L, 16] float32, shift float32, centred means m, variances v, lens, states [n_utt L]); bad_rows get a NaN."""
    rng = np.random.default_rng(seed)
    mu = means(K, gap)
    states = np.concatenate([planted_states(rng, K, L) for _ in range(n_utt)])
    x = (mu[states] + JITTER * rng.normal(size=(len(states), D))).astype(np.float32)
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    for r in bad_rows:
        x[r, r % D] = np.nan
    return x, shift, mu - shift.astype(np.float64), np.ones((K, D)), np.full(n_utt, L, dtype=np.int64), states


# ---- the matrices ------------------------------------------------------------------------------------------------------
def floored(p, eps):
    """float32: every entry below eps raised to it, each row renormalised once in float64 (a vector is one row)."""
    p = np.array(p, dtype=np.float64)
    p[p < eps] = eps
    return np.ascontiguousarray((p / p.sum(axis=-1, keepdims=True)).astype(np.float32))


def cyclic(K, eps):
    t = np.zeros((K, K))
    for k in range(K):
        t[k, k] += 0.5
        t[k, (k + 1) % K] += 0.5
    return floored(np.full(K, 1.0 / K), eps), floored(t, eps)


def left_to_right(K, eps):
    t = np.zeros((K, K))
    for k in range(K):
        t[k, k] += 0.5
        t[k, min(k + 1, K - 1)] += 0.5
    init = np.zeros(K)
    init[0] = 1.0
    return floored(init, eps), floored(t, eps)


def blocks(K, eps, size=BLOCK):
    size = min(size, max(1, K // 2))
    t, init = np.zeros((K, K)), np.zeros(K)
    for k in range(K):
        lo = (k // size) * size
        t[k, lo:min(lo + size, K)] = 1.0
    init[:size] = 1.0 / size
    return floored(init, eps), floored(t / t.sum(axis=1, keepdims=True), eps)


def from_counts(xi, first, eps):
    """dn.mstep at alpha = 0 from a uniform start, with the floor eps in TRANS_MIN's place."""
    xi, first = np.asarray(xi, dtype=np.float64), np.asarray(first, dtype=np.float64)
    K = len(first)
    den = xi.sum(axis=1, keepdims=True)
    t = np.where(den > 0, xi / np.where(den > 0, den, 1.0), 1.0 / K)
    i = first / first.sum() if first.sum() > 0 else np.full(K, 1.0 / K)
    return floored(i, eps), floored(t, eps)


def counts_of(states, lens, K, n_first=2):
    """(xi [K, K], first [K]) of the first n_first planted sequences."""
    off = np.cumsum(lens) - lens
    seqs = {u: states[off[u]:off[u] + lens[u]] for u in range(min(n_first, len(lens)))}
    first = np.zeros(K)
    for s in seqs.values():
        first[s[0]] += 1
    return dn.bigram_counts(seqs, K).astype(np.float64), first


def transitions(name, K, eps, states=None, lens=None):
    if name == 'counts':
        return from_counts(*counts_of(states, lens, K), eps=eps)
    return {'cyclic': cyclic, 'left_to_right': left_to_right, 'blocks': blocks}[name](K, eps)


# ---- the sticky model's weights ----------------------------------------------------------------------------------------
def tiny_weights(K, seed):
    """float64 weights summing to 1: of every four components one at 2^-79 .. 2^-60 (the exponents cycle), of every seven one
    retired to 0 (K >= 7), the others share the rest unequally."""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.full(K, 5.0))
    tiny = np.arange(K) % 4 == 1
    dead = (np.arange(K) % 7 == 3) & ~tiny
    if K < 3:
        tiny[:], dead[:] = False, False
    w[tiny] = 2.0 ** -(60.0 + np.arange(tiny.sum()) % 20)
    w[dead] = 0.0
    rest = ~(tiny | dead)
    w[rest] *= (1.0 - w[tiny].sum()) / w[rest].sum()
    return w


# ---- cases -----------------------------------------------------------------------------------------------------------------
class LazyTables(dict):
    """The device tables of a Case, made when first read: the host tests build cases without a device."""

    def __init__(self, host_tables):
        dict.__init__(self)
        self.host_tables = host_tables

    def __missing__(self, key):
        from test_gpu_hmm import dev
        self[key] = dev(self.host_tables[key], np.float32)
        return self[key]

    def __setitem__(self, key, value):
        if isinstance(value, np.ndarray):
            self.host_tables[key] = value
        else:
            dict.__setitem__(self, key, value)


def _host_side(case, x, shift, w, m, v, lens):
    """Case.__init__ without the uploads (the same gmm_np / hmm_np calls in the same order)."""
    case.x, case.lens = x, np.asarray(lens, dtype=np.int64)
    case.off = np.cumsum(case.lens) - case.lens
    case.K, case.D = m.shape
    case.xc, case.bad = gmm_np.centre(x, shift)
    case.A, case.B, case.c = gmm_np.tables(w, m, v)
    case.c0 = hmm_np.emission_offsets(m, v)
    case.w32 = np.asarray(w).astype(np.float32)
    case.d = LazyTables(dict(table=x, shift=shift, A=case.A, B=case.B, c0=case.c0, w=case.w32))
    case._ref = {}


class RangeCase(DenseCase):
    """DenseCase (its scores, references, bars and run) with the uploads deferred, and the filtered references taken from the
    smoothed run's ahat: forward_backward_fast's forward sweep is the same statements in both modes."""

    def __init__(self, x, shift, m, v, lens, init, trans, states=None, tag=''):
        _host_side(self, x, shift, np.full(len(m), 1.0 / len(m)), m, v, lens)
        self.init, self.trans, self.states, self.tag = init, trans, states, tag
        self.d.host_tables.update(init=init, trans=trans)

    def reference(self, smooth=True):
        if not smooth and ('dense', False) not in self._ref:
            zero = lambda r, k: np.zeros_like(r[k])
            self._ref[('dense', False)] = tuple(
                dict(r, post=r['ahat'], xi=zero(r, 'xi'), first=zero(r, 'first'), xi_utt=zero(r, 'xi_utt'), first_utt=zero(r, 'first_utt'))
                for r in DenseCase.reference(self, True))
        return DenseCase.reference(self, smooth)

    def log_tables(self):
        return dv.log_transitions(self.init, self.trans)


class StickyRangeCase(Case):
    """test_gpu_hmm.Case with the uploads deferred."""

    def __init__(self, x, shift, w, m, v, lens, tag=''):
        _host_side(self, x, shift, w, m, v, lens)
        self.tag = tag


def seed_of(name, K, eps_exp, gap):
    return 100000 * MATRICES.index(name) + 1000 * K + 10 * gap + eps_exp // 100


def dense_case(name, K, L, eps_exp, gap, n_utt=N_UTT, bad_rows=()):
    x, shift, m, v, lens, states = features(K, L, gap, seed_of(name, K, eps_exp, gap), n_utt, bad_rows)
    init, trans = transitions(name, K, 2.0 ** -eps_exp, states, lens)
    return RangeCase(x, shift, m, v, lens, init, trans, states, '%s K%d L%d eps2^-%d gap%d' % (name, K, L, eps_exp, gap))


def sticky_case(K, L, gap, n_utt=N_UTT, bad_rows=()):
    x, shift, m, v, lens, _ = features(K, L, gap, 7000 + 10 * K + gap, n_utt, bad_rows)
    return StickyRangeCase(x, shift, tiny_weights(K, K + gap), m, v, lens, 'sticky K%d L%d gap%d' % (K, L, gap))


def grid():
    return [(name, K, L, e, g) for name in MATRICES for K, L in SHAPES for e in EPS_EXP for g in GAPS]


# ---- the classification ------------------------------------------------------------------------------------------------------
def dense_errors(case, post, ahat, loglik, xi_utt=None, first_utt=None):
    """Per utterance, the largest error / bar of the five quantities against the float64 restatement under
    tests/test_gpu_hmm_dense.py's bars (a non-finite value counts as inf): dict of [n_utt] arrays.  Without the per-utterance
    statistics (the device adds them up over the corpus: corpus_stats_error) the dict holds the three others."""
    r = case.scores()
    ref64 = case.reference(True)[0]
    S = case.per_utterance(r['eps'] + r['delta'])
    bar_ll = S + 2.0 * U * case.per_utterance(np.abs(ref64['m']))
    out = {k: np.zeros(len(case.lens)) for k in ('gamma', 'ahat', 'loglik', 'xi', 'first')}
    with np.errstate(all='ignore'):
        for u, (o, n) in enumerate(zip(case.off, case.lens)):
            rel = np.expm1(2.0 * S[u])
            for name, mine, ref in (('gamma', post, ref64['post']), ('ahat', ahat, ref64['ahat'])):
                g = ref[o:o + n]
                e = np.abs(np.asarray(mine[o:o + n], dtype=np.float64) - g) / (g * rel + FLOOR)
                good = ~case.bad[o:o + n]
                sums = np.abs(np.asarray(mine[o:o + n], dtype=np.float64).sum(axis=1)[good] - 1.0) / (rel + FLOOR)
                out[name][u] = max(e.max(), sums.max() if good.any() else 0.0)
            out['loglik'][u] = abs(loglik[u] - ref64['loglik'][u]) / max(bar_ll[u], 1e-300)
            if xi_utt is None:
                continue
            st = np.concatenate([ref64['xi_utt'][u], ref64['first_utt'][u][None, :]])
            bar = stats_bar(st, ref64['n_good'][u:u + 1], S[u])
            e = np.abs(np.concatenate([xi_utt[u], first_utt[u][None, :]]) - st) / bar
            out['xi'][u], out['first'][u] = e[:case.K].max(), e[case.K:].max()
    if xi_utt is None:
        del out['xi'], out['first']
    for k in out:
        out[k] = np.where(np.isfinite(out[k]), out[k], np.inf)
    return out


def corpus_stats_error(case, stats):
    """(xi, first): the largest error / bar of a corpus' statistics [K + 1, K] under check_against_reference's bar."""
    r = case.scores()
    ref64 = case.reference(True)[0]
    S = case.per_utterance(r['eps'] + r['delta'])
    ref_st = np.concatenate([ref64['xi'], ref64['first'][None, :]])
    with np.errstate(all='ignore'):
        e = np.abs(np.asarray(stats, dtype=np.float64) - ref_st) / stats_bar(ref_st, ref64['n_good'], S.max())
    e = np.where(np.isfinite(e), e, np.inf)
    return float(e[:case.K].max()), float(e[case.K:].max())


def classify(case):
    """bool [n_utt]: True where the float32 restatement meets the bars on gamma, ahat, loglik, xi and first (in range), False
    where it does not (in the window).  Only the two restatements are read."""
    r32 = case.reference(True)[1]
    e = dense_errors(case, r32['post'], r32['ahat'], r32['loglik'], r32['xi_utt'], r32['first_utt'])
    return np.all([e[k] <= 1.0 for k in e], axis=0)


def sticky_errors(case, rho, post, ahat, loglik, stays):
    """dense_errors for the sticky chain under tests/test_gpu_hmm.py's bars: gamma, ahat, loglik, stays."""
    r = case.scores()
    ref64 = case.reference(rho, True)[0]
    S = case.per_utterance(r['eps'] + r['delta'])
    bar_ll = S + 2.0 * U * case.per_utterance(np.abs(ref64['m']))
    out = {k: np.zeros(len(case.lens)) for k in ('gamma', 'ahat', 'loglik', 'stays')}
    with np.errstate(all='ignore'):
        for u, (o, n) in enumerate(zip(case.off, case.lens)):
            rel = np.expm1(2.0 * S[u])
            for name, mine, ref in (('gamma', post, ref64['post']), ('ahat', ahat, ref64['ahat'])):
                g = ref[o:o + n]
                e = np.abs(np.asarray(mine[o:o + n], dtype=np.float64) - g) / (g * rel + FLOOR)
                good = ~case.bad[o:o + n]
                sums = np.abs(np.asarray(mine[o:o + n], dtype=np.float64).sum(axis=1)[good] - 1.0) / (rel + FLOOR)
                out[name][u] = max(e.max(), sums.max() if good.any() else 0.0)
            out['loglik'][u] = abs(loglik[u] - ref64['loglik'][u]) / max(bar_ll[u], 1e-300)
            bar_st = ref64['n_good'][u] * rel
            d = abs(stays[u] - ref64['stays'][u])
            out['stays'][u] = 0.0 if d == 0 else d / max(bar_st, 1e-300)
    for k in out:
        out[k] = np.where(np.isfinite(out[k]), out[k], np.inf)
    return out


def classify_sticky(case, rho):
    r32 = case.reference(rho, True)[1]
    e = sticky_errors(case, rho, r32['post'], r32['ahat'], r32['loglik'], r32['stays'])
    return np.all([e[k] <= 1.0 for k in e], axis=0)


# ---- the invariants ----------------------------------------------------------------------------------------------------
def row_sum_bar(case):
    """[T]: the existing bar on |sum_k post - 1| of a good row."""
    r = case.scores()
    return np.expm1(2.0 * case.rows(case.per_utterance(r['eps'] + r['delta']))) + FLOOR


def loglik_bar(case, m64):
    r = case.scores()
    return case.per_utterance(r['eps'] + r['delta']) + 2.0 * U * case.per_utterance(np.abs(m64))


def decoder_delta(case, li, lt):
    """[n_utt]: n_good delta of tests/hmm_dense_vit_np.py's docstring, per utterance."""
    s64 = case.scores()['s64']
    E = dv.score_bound(gmm_np.score_scale(case.xc, case.bad, case.A, case.B, case.c0), case.D).max(axis=1)
    lmax = dv.table_max(li, lt)
    out = np.zeros(len(case.lens))
    for u, (o, n) in enumerate(zip(case.off, case.lens)):
        good = ~case.bad[o:o + n]
        if good.any():
            out[u] = good.sum() * dv.delta(E[o:o + n][good], np.abs(s64[o:o + n][good]).max() + E[o:o + n][good].max(), lmax)
    return out


def violations(case, post, loglik, stats=None, log_prob=None, slack=None, n_good=None):
    """The names of the invariants a result breaks (an empty list: none).  They hold in exact arithmetic for any model:
    finite outputs; post >= 0; |sum_k post - 1| within the existing bar on good rows; xi >= 0; and, where the decoder's
    log_prob is given, log_prob - slack <= loglik <= log_prob + n_good ln K + slack."""
    bad = []
    post64 = np.asarray(post, dtype=np.float64)
    if not (np.isfinite(post64).all() and np.isfinite(loglik).all() and (stats is None or np.isfinite(stats).all())):
        bad.append('finite')
    with np.errstate(all='ignore'):
        if not (post64 >= 0).all():
            bad.append('post >= 0')
        good = ~case.bad
        if not (np.abs(post64.sum(axis=1) - 1.0)[good] <= row_sum_bar(case)[good]).all():
            bad.append('row sums')
        if stats is not None and not (np.asarray(stats) >= 0).all():
            bad.append('xi >= 0')
        if log_prob is not None:
            ng = np.asarray(n_good, dtype=np.float64)
            if not ((log_prob - slack <= loglik) & (loglik <= log_prob + ng * np.log(case.K) + slack)).all():
                bad.append('sandwich')
    return bad


# ---- the classification, pinned ------------------------------------------------------------------------------------------
# (matrix, K, floor exponent) -> the gaps of GAPS at which at least one of the N_UTT utterances is in the window; every other
# gap of GAPS is in range with all its utterances.  tests/test_hmm_range_host.py asserts this table against classify();
# tests/test_gpu_hmm_range.py takes its in-range and window lists from it.  The features' other states sit at 2, 3 and 4
# times the gap, so a gap of 20 already holds misses of 40 .. 80 nats and a gap of 90 or more mostly exact zeros: the window
# is not an interval of the gap.
WINDOW = {
    ('cyclic', 4, 80): (120,), ('cyclic', 4, 100): (120,),
    ('cyclic', 65, 80): (60, 120), ('cyclic', 65, 100): (20, 60, 90, 120),
    ('cyclic', 128, 80): (60,), ('cyclic', 128, 100): (20, 60, 120),
    ('left_to_right', 4, 80): (60, 120), ('left_to_right', 4, 100): (60, 120),
    ('left_to_right', 65, 80): (60, 120), ('left_to_right', 65, 100): (20, 60, 90, 120),
    ('left_to_right', 128, 80): (60, 120), ('left_to_right', 128, 100): (20, 60, 120),
    ('blocks', 4, 80): (120,), ('blocks', 4, 100): (120,),
    ('blocks', 65, 80): (60, 120), ('blocks', 65, 100): (20, 60, 90, 120),
    ('blocks', 128, 80): (60, 120), ('blocks', 128, 100): (20, 60, 90),
    ('counts', 4, 80): (), ('counts', 4, 100): (),
    ('counts', 65, 80): (60, 90, 120), ('counts', 65, 100): (60, 90, 120),
    ('counts', 128, 80): (60,), ('counts', 128, 100): (60, 120),
}
# Cases the grid was expected to hold in range (gaps 20 and 300 at every K, 60 at K = 4, 160 at the floor 2^-80) that are in
# the window once realised through features, and the nearest multiple of ten that is in range with every utterance, taken in
# their place: (matrix, K, L, floor exponent, listed gap, the gap taken).  The last one's window reaches from 30 to 85: above it
# the nearest is 90, a member of the grid already; below it 25, which is added.
MOVED = (
    ('cyclic', 65, 300, 100, 20, 10), ('cyclic', 128, 140, 100, 20, 10),
    ('left_to_right', 65, 300, 100, 20, 10), ('left_to_right', 128, 140, 100, 20, 10),
    ('blocks', 65, 300, 100, 20, 10), ('blocks', 128, 140, 100, 20, 10),
    ('left_to_right', 4, 24, 80, 60, 40), ('left_to_right', 4, 24, 100, 60, 25),
)
# The sticky chain on tiny_weights: (K, gap, index into STAYS) in the window; STICKY_EDGE sits at the bar itself (its worst
# utterance at 1.04 of the gamma bar) and is asserted on neither side.  Every other (K, gap, stay) of the grid is in range.
STICKY_WINDOW = ((65, 20, 2), (65, 60, 1), (65, 60, 2), (128, 60, 1), (128, 60, 2))
STICKY_EDGE = ((128, 20, 2),)


def bad_rows_for(L):
    """A first frame, a frame inside the second utterance and that utterance's last frame."""
    return (0, L + 3, 2 * L - 1)


# in-range cases run once more with bad_rows_for(L) (classified with those rows by the host test)
BAD_IN_RANGE = (('cyclic', 4, 24, 80, 20), ('counts', 65, 300, 100, 300), ('blocks', 128, 140, 80, 160), ('left_to_right', 128, 140, 100, 90))


def in_range_cases():
    out = [c for c in grid() if c[4] not in WINDOW[(c[0], c[1], c[3])]]
    return out + [(n, K, L, e, g) for n, K, L, e, _, g in MOVED]


def window_cases():
    return [c for c in grid() if c[4] in WINDOW[(c[0], c[1], c[3])]]


def sticky_grid():
    return [(K, L, g, i) for K, L in SHAPES for g in GAPS for i in range(len(STAYS))]
