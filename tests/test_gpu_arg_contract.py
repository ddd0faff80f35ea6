"""One argument contract for every Python entry, held before it launches.  SURFACE has a row per public function, method or
nn.Module.forward through which a caller's tensor or array reaches an abn_* entry: the smallest valid call, the entries
it claims, per array argument the dtype and rank the entry documents and whether it lives on the device or the host, and
the groups of arguments whose widths or lengths must agree.  Three tests are generated from the table
(tests/arg_contract.py holds the guard and the mutants):

  test_canonical_call              the valid call runs under the guard with nothing forbidden and reaches what it claims.
  test_value_preserving_mutations  one argument at a time becomes a strided / transposed view of a larger allocation, or
                                   the same values in a wider dtype (a python list, the other integer width, a strided
                                   slice for host arrays); the mutant's whole allocation is forbidden to every entry.
                                   Two outcomes pass: a refusal (ValueError, TypeError, AssertionError, HipLibraryError)
                                   before any launch, or completion with every output bit for bit the canonical call's.
                                   A caller's output tensor (out=, ids=) must be refused.  An argument documented to
                                   take several dtypes (the losses' labels) is held to completion in its wider dtype.
  test_shape_mutations_are_refused a table of the wrong rank, a member of a width group one column narrower or wider, a
                                   member of a length group one element shorter, a CPU tensor for a device one -- with
                                   every entry blocked: the wrapper has to refuse on its own, nothing is launched.

Every row has same_bits=True (the library promises equal bits for equal calls): no tolerance appears in this file.
tests/test_arg_contract_host.py holds every key of _lib.SYMBOLS to a row here, to QUERIES or to EXCLUDED; the entries of
include/abnet3_hip_next.h (the later HMM decoders, the in-batch contrastive loss) have rows all the same, and the guard
stands in front of them too.

What the table found in the wrappers as they stood before it (each is fixed in the change that added this file; L = LeakedPointer
at that argument of the entry, R = ReachedLibrary at the entry):
  model._SoftmaxRows                 z float64: L abn_softmax_rows 0; z of rank 3: R abn_softmax_rows; rank 1: IndexError
  integration units                  x1 / x2 float64: L abn_integrate_forward 0 / 2; unequal widths under 'sum': R; rank 1: IndexError
  features.deltas_of                 float64: L abn_deltas 0; rank 3, a CPU tensor: R abn_deltas; rank 1: IndexError
  features.stack_table               float64: L abn_stack_frames_batched 0; a CPU tensor, lengths that do not add up: R
  features.normalize_table           every view and float64: L abn_mvn_stats 0; a CPU tensor, lengths one short: R abn_mvn_stats
  features.fbank_batch / mfcc_batch  a python list for an utterance: AttributeError
  utils.cosine_distance              a rank-1 side: IndexError
  dataloader.gather_rows             table float64: L abn_gather_rows 0; rank 3: R
  utils.dtw_align_batch              feats float64: L abn_dtw_batched_overlap 0 / 2; rank 3, unequal widths, a short column: R
  abx.dtw_cost_batch (cosine, zero)  feats float64: L abn_dtw_cost_batched / _parallel_batched 0 / 2; unequal widths: R
  abx.abx_score                      a CPU dist, one distance short: R abn_abx_score
  discovery.knn_topk                 Q / C float64: L abn_knn_topk 0 / 2
  discovery.segment_vectors          table float64: L abn_segment_vectors 0
  eskmeans.candidate_scores / segment_dp   lm or lm_off one short: R abn_esk_score / abn_esk_segment
  gmm.posteriors, kmeans.assign      a CPU out= / ids=: R abn_gmm_posteriors / abn_kmeans_assign

A row's mutants run inside one test (55 rows x 3 tests, 1608 mutants): the listing of the suite stays short, and a failing
test names every mutant that failed and how.

Needs an MI355X: -m gpu.  Measured on an MI355X: the whole file takes 3 s (166 tests); the slowest case is
test_canonical_call[softmax-rows] at 0.7 - 0.9 s (the process's first autograd call), no other above 0.4 s."""
import numpy as np
import pytest

import arg_contract as AC
from test_gpu_dirty_memory import assert_same_bits, dev, host

pytestmark = pytest.mark.gpu

REFUSALS = None            # (ValueError, TypeError, AssertionError, HipLibraryError): filled at the first use (needs the package)
LABEL_DTYPES = ('int8', 'int32', 'int64', 'float32', 'float64')            # _lib.Y_DTYPE


def refusals():
    global REFUSALS
    if REFUSALS is None:
        from abnet3_amd._lib import HipLibraryError
        REFUSALS = (ValueError, TypeError, AssertionError, HipLibraryError)
    return REFUSALS


class A(object):
    """One array argument: the dtype and rank the entry documents; where = 'device', 'host' (a numpy array, uploaded by the
    wrapper) or 'any' (either is taken); takes = further dtypes the entry documents; out = the entry writes into it; row = a
    rank-1 argument that must not come as [1, n] either (mono samples: a second dimension would be channels)."""

    def __init__(self, dtype, rank, where='device', takes=(), out=False, row=False):
        self.dtype, self.rank, self.where, self.takes, self.out, self.row = dtype, rank, where, tuple(takes), out, row


class Row(object):
    """build() -> {name: value} (made once, never written to, but for out arguments); run(args) -> {name: numpy}; entries:
    what the row claims to reach; args: {name: A}; widths / lengths: groups of argument names whose column counts / first
    dimensions must agree (a group of one: the size is tied to something that is not an array argument); late: arguments
    the row's first launch does not take (a loss's labels behind a tower's forward) -- their shape mutations belong to the row
    of the entry that takes them, here they would only show that the forward was launched."""

    def __init__(self, name, entries, build, run, args, widths=(), lengths=(), same_bits=True, late=()):
        self.name, self.entries, self.build, self.run, self.args = name, tuple(entries), build, run, dict(args)
        self.widths, self.lengths, self.same_bits, self.late = tuple(widths), tuple(lengths), same_bits, tuple(late)

    def inputs(self):
        if self.name not in _BUILT:
            built = self.build()
            for k, a in self.args.items():
                v = built[k]
                assert str(v.dtype).replace('torch.', '') == a.dtype and v.ndim == a.rank, (self.name, k, v.dtype, v.ndim)
                assert isinstance(v, np.ndarray) == (a.where == 'host'), (self.name, k)
            _BUILT[self.name] = built
        return _BUILT[self.name]


_BUILT, _CANON = {}, {}


def rng_of(name):
    return np.random.default_rng(sum(ord(c) for c in name))


def f32(a):
    return np.asarray(a, dtype=np.float32)


# ======================================================================================================================
# shared inputs
# ======================================================================================================================
N1, N2 = np.array([5, 9, 12, 7, 3], dtype=np.int32), np.array([6, 4, 11, 8, 5], dtype=np.int32)


def starts(n):
    return (np.cumsum(n) - n).astype(np.int64)


PAIR_COLS = dict(o1=A('int64', 1, 'host'), n1=A('int32', 1, 'host'), o2=A('int64', 1, 'host'), n2=A('int32', 1, 'host'))


def pair_table(rng, D=8, prob=False):
    """Five pairs over two tables of 40 rows (the tokens end to end, then four rows nobody reads)."""
    draw = (lambda n: f32(rng.dirichlet(np.full(D, 0.5), n))) if prob else (lambda n: f32(rng.standard_normal((n, D))))
    return dict(f1=dev(draw(40)), f2=dev(draw(40)), o1=starts(N1), n1=N1.copy(), o2=starts(N2), n2=N2.copy())


UTT_OFF, UTT_LEN, UTT_T = np.array([0, 12, 30], dtype=np.int64), np.array([10, 15, 8], dtype=np.int64), 40
MIX_K, MIX_D = 4, 3


def mixture(rng):
    """A diagonal mixture of 4 components over 3 dimensions and 40 frames, the score tables on the device."""
    from abnet3_amd import gmm, hmm
    w = np.array([0.1, 0.2, 0.3, 0.4])
    m, v = rng.standard_normal((MIX_K, MIX_D)), rng.uniform(0.5, 1.5, (MIX_K, MIX_D))
    A_, B_, c = gmm.score_tables(w, m, v)
    return dict(table=dev(f32(rng.standard_normal((UTT_T, MIX_D)))), shift=dev(np.zeros(MIX_D, dtype=np.float32)), A=dev(A_), B=dev(B_),
                c=dev(c), c0=dev(hmm.emission_offsets(m, v)), w=dev(f32(w)), w64=w, m=m, v=v)


UTT_COLS = dict(off=A('int64', 1, 'host'), lens=A('int64', 1, 'host'))


# ======================================================================================================================
# the rows
# ======================================================================================================================
def tower_row():
    kw = dict(input_dim=8, num_hidden_layers=1, hidden_dim=16, output_dim=8, activation_layer='sigmoid', batch_norm=False, p_dropout=0.0)
    B = 9

    def build():
        rng = rng_of('tower')
        return dict(x1=dev(f32(rng.standard_normal((B, 8)))), x2=dev(f32(rng.standard_normal((B, 8)))), y=dev(rng.choice([1, -1], B).astype(np.int64)))

    def run(a):
        import torch
        import abnet3_amd.loss as L
        from abnet3_amd.model import SiameseNetwork
        torch.manual_seed(5)
        net = SiameseNetwork(**kw).cuda()
        net.train()
        e1, e2 = net(a['x1'], a['x2'])
        lv = L.coscos2(avg=False)(e1, e2, a['y'])
        lv.backward()
        out = dict(e1=host(e1), e2=host(e2), loss=host(lv))
        out.update({'g.' + k: host(q.grad) for k, q in net.named_parameters()})
        net.eval()
        with torch.no_grad():
            out['eval'] = host(net.forward_once(a['x1']))
        return out

    return Row('tower', ('abn_tower_forward', 'abn_tower_backward', 'abn_pair_loss'), build, run,
               dict(x1=A('float32', 2), x2=A('float32', 2), y=A('int64', 1, takes=LABEL_DTYPES)),
               widths=[('x1', 'x2')], lengths=[('x1', 'x2')], late=('y',))


def pair_loss_row():
    B, D = 9, 8

    def build():
        rng = rng_of('pair-loss')
        sig = lambda z: f32(1.0 / (1.0 + np.exp(-z)))
        return dict(e1=dev(sig(rng.standard_normal((B, D)))), e2=dev(sig(rng.standard_normal((B, D)))),
                    y=dev(rng.choice([1, -1], B).astype(np.int64)))

    def run(a):
        import abnet3_amd.loss as L
        lv, de = L.cosmargin(avg=True, margin=0.5).value_and_grad(a['e1'], a['e2'], a['y'])
        lz, dz = L.coscos2(avg=False).value_and_dz(a['e1'], a['e2'], a['y'], 'sigmoid', None)
        return dict(loss=host(lv), de=host(de), loss_dz=host(lz), dz=host(dz))

    return Row('pair-loss', ('abn_pair_loss', 'abn_pair_loss_dz', 'abn_pair_loss_ws_bytes'), build, run,
               dict(e1=A('float32', 2), e2=A('float32', 2), y=A('int64', 1, takes=LABEL_DTYPES)),
               widths=[('e1', 'e2')], lengths=[('e1', 'e2', 'y')])


def nce_row():
    B, D = 9, 8

    def build():
        rng = rng_of('nce')
        y = np.ones(B, dtype=np.int64)
        y[[2, 5]] = -1
        return dict(e1=dev(f32(rng.standard_normal((B, D)))), e2=dev(f32(rng.standard_normal((B, D)))), y=dev(y),
                    groups=dev(np.array([0, 0, 1, 2, 2, 3, 4, 5, 5], dtype=np.int32)))

    def run(a):
        import abnet3_amd.loss as L
        lv, de = L.InfoNCELoss(temperature=0.1, avg=True).value_and_grad(a['e1'], a['e2'], a['y'], a['groups'])
        return dict(loss=host(lv), de=host(de))

    return Row('nce-loss', ('abnt_nce_loss', 'abnt_nce_ws_bytes', 'abnt_nce_max_d'), build, run,
               dict(e1=A('float32', 2), e2=A('float32', 2), y=A('int64', 1, takes=LABEL_DTYPES), groups=A('int32', 1)),
               widths=[('e1', 'e2')], lengths=[('e1', 'e2', 'y', 'groups')])


def softmax_row():
    def build():
        rng = rng_of('softmax')
        return dict(z=dev(f32(3 * rng.standard_normal((9, 8)))), g=dev(f32(rng.standard_normal((9, 8)))))

    def run(a):
        from abnet3_amd.model import _SoftmaxRows
        z = a['z'].detach().requires_grad_(True)
        p = _SoftmaxRows.apply(z)
        p.backward(a['g'])
        return dict(p=host(p), dz=host(z.grad))

    # (g reaches the backward through torch's autograd engine, which holds its shape and dtype to the output's)
    return Row('softmax-rows', ('abn_softmax_rows', 'abn_softmax_rows_backward'), build, run, dict(z=A('float32', 2)))


def integrate_row():
    def build():
        rng = rng_of('integrate')
        return dict(x1=dev(f32(rng.standard_normal((9, 8)))), x2=dev(f32(rng.standard_normal((9, 8)))), g=dev(f32(rng.standard_normal((9, 8)))))

    def run(a):
        from abnet3_amd.integration import BiWeightedFixed
        x1, x2 = a['x1'].detach().requires_grad_(True), a['x2'].detach().requires_grad_(True)
        y = BiWeightedFixed('sum', 0.3)([x1, x2])
        y.backward(a['g'])
        return dict(out=host(y), dx1=host(x1.grad), dx2=host(x2.grad))

    return Row('integrate', ('abn_integrate_forward', 'abn_integrate_backward'), build, run, dict(x1=A('float32', 2), x2=A('float32', 2)),
               widths=[('x1', 'x2')], lengths=[('x1', 'x2')])


FS = 16000


def frontend_row(method, batched):
    """fbank / mfcc with deltas and deltasdeltas on 1000 and 450 float32 samples (7 and 3 frames)."""
    def build():
        rng = rng_of('frontend')
        return dict(w0=f32(1000 * rng.standard_normal(1000)), w1=f32(1000 * rng.standard_normal(450)))

    def run(a):
        from abnet3_amd.features import FeaturesGenerator
        fg = FeaturesGenerator(method='mfcc' if method == 'mfcc' else 'fbanks', deltas=True, deltasdeltas=True)
        if batched:
            table, nfr = (fg.mfcc_batch if method == 'mfcc' else fg.fbank_batch)([a['w0'], a['w1']], FS)
            return dict(table=host(table), nfr=np.asarray(nfr))
        one = fg.mfcc_from_samples if method == 'mfcc' else fg.fbank_from_samples
        return dict(t0=host(one(a['w0'], FS)), t1=host(one(a['w1'], FS)))

    if method == 'mfcc':
        entries = ('abn_mfcc_batched', 'abn_deltas_batched') if batched else ('abn_mfcc', 'abn_deltas_batched')
    else:
        entries = ('abn_fbank_batched', 'abn_deltas_batched') if batched else ('abn_fbank', 'abn_deltas')
    # the sound is documented as int16 or float: anything but int16 is converted to float32 on the way in
    return Row('%s-%s' % (method, 'batched' if batched else 'single'), entries, build, run,
               dict(w0=A('float32', 1, 'host', row=True), w1=A('float32', 1, 'host', row=True)),
               late=() if batched else ('w1',))                        # (one call per utterance: w0's has run when w1 is looked at)


def table_rows():
    """The front end's table-level entries on a [40, 8] table of two utterances (30 and 10 frames)."""
    def build():
        return dict(table=dev(f32(rng_of('table').standard_normal((40, 8)) * 3 + 12)), lengths=np.array([30, 10], dtype=np.int64))

    def fg(**kw):
        from abnet3_amd.features import FeaturesGenerator
        return FeaturesGenerator(**kw)

    def deltas(a):
        return dict(d=host(fg().deltas_of(a['table'])))

    def stack_one(a):
        # (numpy in -> numpy out, device tensor in -> device tensor out, in the dtype that came in: the values are copies)
        out = fg().stack_fbanks(a['table'], nframes=3)
        return dict(s=np.asarray(out if isinstance(out, np.ndarray) else host(out), dtype=np.float32))

    def stack_all(a):
        return dict(s=host(fg(nframes=3).stack_table(a['table'], a['lengths'])))

    def mvn(per_file):
        def run(a):
            out, stats = fg(norm_per_channel=True, norm_per_file=per_file).normalize_table(a['table'], a['lengths'])
            stats = stats if per_file else [stats]
            res = dict(out=host(out))
            for i, (mean, std) in enumerate(stats):
                res['mean%d' % i], res['std%d' % i] = host(mean), host(std)
            return res
        return run

    T, L = A('float32', 2), A('int64', 1, 'host')
    return [Row('deltas-of', ('abn_deltas',), build, deltas, dict(table=T)),
            Row('stack-fbanks', ('abn_stack_frames',), build, stack_one, dict(table=A('float32', 2, 'any'))),
            Row('stack-table', ('abn_stack_frames_batched',), build, stack_all, dict(table=T, lengths=L), lengths=[('lengths',)]),
            Row('normalize-table', ('abn_mvn_stats', 'abn_mvn_apply', 'abn_mvn_ws_bytes'), build, mvn(False), dict(table=T)),
            Row('normalize-table-per-file', ('abn_mvn_stats', 'abn_mvn_apply'), build, mvn(True), dict(table=T, lengths=L), lengths=[('lengths',)])]


def cosine_row(f64):
    dt = 'float64' if f64 else 'float32'

    def build():
        rng = rng_of('cosine')
        return dict(x=rng.standard_normal((9, 8)).astype(dt), y=rng.standard_normal((7, 8)).astype(dt))

    def run(a):
        from abnet3_amd.utils import cosine_distance
        return dict(d=cosine_distance(a['x'], a['y']))

    # (both sides in one precision: float32 against float64 is refused, as the reference refuses it)
    return Row('cosine-distance-' + dt, ('abn_cosine_distance_f64' if f64 else 'abn_cosine_distance',), build, run,
               dict(x=A(dt, 2, 'host'), y=A(dt, 2, 'host')), widths=[('x', 'y')])


def gather_row():
    def build():
        rng = rng_of('gather')
        return dict(table=dev(f32(rng.standard_normal((40, 8)))), idx=dev(rng.integers(0, 40, 9).astype(np.int64)))

    def run(a):
        from abnet3_amd.dataloader import gather_rows
        return dict(rows=host(gather_rows(a['table'], a['idx'])))

    return Row('gather-rows', ('abn_gather_rows',), build, run, dict(table=A('float32', 2), idx=A('int64', 1)))


PAIR_GROUPS = dict(widths=[('f1', 'f2')], lengths=[('o1', 'n1', 'o2', 'n2')])
PAIR_ARGS = dict(PAIR_COLS, f1=A('float32', 2), f2=A('float32', 2))


def dtw_align_row():
    def run(a):
        from abnet3_amd.utils import dtw_align_batch
        res = dtw_align_batch(a['f1'], a['o1'], a['n1'], a['f2'], a['o2'], a['n2'])
        out = dict(plen=host(res.path_len), cost=host(res.total_cost))
        for p, g in enumerate(res.to_lists()):
            out['p1.%d' % p], out['p2.%d' % p] = g if g is not None else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        return out

    return Row('dtw-align', ('abn_dtw_batched_overlap', 'abn_dtw_host_stage_bytes'), lambda: pair_table(rng_of('dtw-align')), run, PAIR_ARGS,
               **PAIR_GROUPS)


def dtw_one_pair_row():
    def build():
        rng = rng_of('dtw-one-pair')
        return dict(feat1=f32(rng.standard_normal((9, 8))), feat2=f32(rng.standard_normal((7, 8))))

    def run(a):
        from abnet3_amd.utils import get_dtw_alignment
        p1, p2 = get_dtw_alignment(a['feat1'], a['feat2'])
        return dict(p1=np.asarray(p1), p2=np.asarray(p2))

    return Row('get-dtw-alignment', ('abn_dtw_batched_overlap',), build, run, dict(feat1=A('float32', 2, 'host'), feat2=A('float32', 2, 'host')),
               widths=[('feat1', 'feat2')])


def dtw_cost_row(how):
    def run(a):
        from abnet3_amd.abx import dtw_cost_batch
        c, l = dtw_cost_batch(a['f1'], a['o1'], a['n1'], a['f2'], a['o2'], a['n2'], parallel='zero' if how == 'zero' else 'drop')
        return dict(cost=host(c), plen=host(l))

    entry = 'abn_dtw_cost_parallel_batched' if how == 'zero' else 'abn_dtw_cost_batched'
    return Row('dtw-cost-' + how, (entry, 'abn_dtw_cost_max_n2'), lambda: pair_table(rng_of('dtw-cost')), run, PAIR_ARGS, **PAIR_GROUPS)


def search_row():
    def run(a):
        from abnet3_amd.qbe import subsequence_dtw_batch
        res = subsequence_dtw_batch(a['f2'], a['o2'], a['n2'], a['f1'], a['o1'], a['n1'], profile=True)
        return dict(cost=host(res[0]), plen=host(res[1]), start=host(res[2]), end=host(res[3]), prof_cost=host(res[4].cost),
                    prof_len=host(res[4].len), prof_start=host(res[4].start))

    return Row('search-cosine', ('abn_dtw_search_batched', 'abn_dtw_search_max_query'), lambda: pair_table(rng_of('search')), run, PAIR_ARGS,
               **PAIR_GROUPS)


LOCAL_NAMES = ('score', 'path_len', 'start1', 'start2', 'end1', 'end2')


def local_row():
    def run(a):
        from abnet3_amd.terms import local_dtw_batch
        res = local_dtw_batch(a['f1'], a['o1'], a['n1'], a['f2'], a['o2'], a['n2'], 0.5)
        return {k: host(t) for k, t in zip(LOCAL_NAMES, res)}

    return Row('local-cosine', ('abn_dtw_local_batched', 'abn_dtw_local_max_n2'), lambda: pair_table(rng_of('local')), run, PAIR_ARGS, **PAIR_GROUPS)


def kl_tables_row():
    def build():
        return dict(table=dev(f32(rng_of('kl-tables').dirichlet(np.full(8, 0.5), 40))))

    def run(a):
        from abnet3_amd.abx import kl_tables
        return {k: host(t) for k, t in zip('PLb', kl_tables(a['table']))}

    return Row('kl-tables', ('abn_kl_tables',), build, run, dict(table=A('float32', 2)))


KL_ARGS = dict(PAIR_COLS, P1=A('float32', 2), L1=A('float32', 2), bad1=A('uint8', 1), P2=A('float32', 2), L2=A('float32', 2), bad2=A('uint8', 1))
KL_GROUPS = dict(widths=[('P1', 'L1', 'P2', 'L2')], lengths=[('o1', 'n1', 'o2', 'n2'), ('P1', 'L1', 'bad1'), ('P2', 'L2', 'bad2')])


def kl_pairs(name):
    from abnet3_amd.abx import kl_tables
    t = pair_table(rng_of(name), prob=True)
    (P1, L1, b1), (P2, L2, b2) = kl_tables(t.pop('f1')), kl_tables(t.pop('f2'))
    t.update(P1=P1, L1=L1, bad1=b1, P2=P2, L2=L2, bad2=b2)
    return t


def kl_row(what):
    """The three entries that take (P, L, bad) triples as abx.kl_tables returns them."""
    def run(a):
        t1, t2 = (a['P1'], a['L1'], a['bad1']), (a['P2'], a['L2'], a['bad2'])
        if what == 'cost':
            from abnet3_amd.abx import dtw_cost_batch
            c, l = dtw_cost_batch(t1, a['o1'], a['n1'], t2, a['o2'], a['n2'], distance='kl')
            return dict(cost=host(c), plen=host(l))
        if what == 'search':
            from abnet3_amd.qbe import subsequence_dtw_batch
            res = subsequence_dtw_batch(t2, a['o2'], a['n2'], t1, a['o1'], a['n1'], distance='kl')
            return dict(cost=host(res[0]), plen=host(res[1]), start=host(res[2]), end=host(res[3]))
        from abnet3_amd.terms import local_dtw_batch
        return {k: host(t) for k, t in zip(LOCAL_NAMES, local_dtw_batch(t1, a['o1'], a['n1'], t2, a['o2'], a['n2'], 0.3, distance='kl'))}

    entry = {'cost': 'abn_dtw_cost_kl_batched', 'search': 'abn_dtw_search_kl_batched', 'local': 'abn_dtw_local_kl_batched'}[what]
    return Row(what + '-kl', (entry,), lambda: kl_pairs(what + '-kl'), run, KL_ARGS, **KL_GROUPS)


def abx_score_row():
    def build():
        from abnet3_amd.abx import enumerate_cells
        from test_abx_host import random_items
        rng = rng_of('abx-score')
        plan = enumerate_cells(*random_items(rng, 30, n_phones=2, n_ctx=1, n_spk=2), mode='within')
        assert len(plan.cells) and len(plan.P) > 1
        return dict(plan=plan, dist=dev(rng.integers(0, 5, len(plan.P)).astype(np.float64)))

    def run(a):
        from abnet3_amd.abx import abx_score
        s2, cnt = abx_score(a['dist'], a['plan'])
        return dict(s2=np.asarray(s2), cnt=np.asarray(cnt))

    return Row('abx-score', ('abn_abx_score',), build, run, dict(dist=A('float64', 1)), lengths=[('dist',)])


def lsh_rows():
    def build_sig():
        from abnet3_amd.prefilter import lsh_planes
        return dict(table=dev(f32(rng_of('lsh').standard_normal((40, 8)))), planes=lsh_planes(8, 64, seed=8))

    def run_sig(a):
        from abnet3_amd.prefilter import lsh_signatures
        sig, live = lsh_signatures(a['table'], a['planes'])
        return dict(sig=host(sig), live=host(live))

    def build_hits():
        from abnet3_amd.prefilter import lsh_planes, lsh_signatures
        t = pair_table(rng_of('lsh-hits'))
        planes = lsh_planes(8, 64, seed=8)
        # (side 2 repeats rows of side 1: hits exist)
        f1 = t.pop('f1')
        t.pop('f2')
        (s1, l1), (s2, l2) = lsh_signatures(f1, planes), lsh_signatures(f1.flip(0).contiguous(), planes)
        t.update(sig1=s1, live1=l1, sig2=s2, live2=l2)
        return t

    def run_hits(a):
        from abnet3_amd.prefilter import diag_hits_batch
        best, diag, end1 = diag_hits_batch(a['sig1'], a['live1'], a['o1'], a['n1'], a['sig2'], a['live2'], a['o2'], a['n2'], 16, 8, 1)
        return dict(best=host(best), diag=host(diag), end1=host(end1))

    hit_args = dict(PAIR_COLS, sig1=A('int32', 2), live1=A('uint8', 1), sig2=A('int32', 2), live2=A('uint8', 1))
    return [Row('lsh-signatures', ('abn_lsh_signatures',), build_sig, run_sig, dict(table=A('float32', 2), planes=A('float32', 2, 'host')),
                widths=[('table', 'planes')]),
            Row('lsh-diag-hits', ('abn_lsh_diag_hits_batched',), build_hits, run_hits, hit_args, widths=[('sig1', 'sig2')],
                lengths=[('o1', 'n1', 'o2', 'n2'), ('sig1', 'live1'), ('sig2', 'live2')])]


def edit_row():
    def build():
        rng = rng_of('edit')
        return dict(sym1=dev(rng.integers(0, 4, 40).astype(np.int32)), sym2=dev(rng.integers(0, 4, 40).astype(np.int32)), o1=starts(N1),
                    n1=N1.copy(), o2=starts(N2), n2=N2.copy())

    def run(a):
        from abnet3_amd.tde import edit_distance_batch
        return dict(dist=host(edit_distance_batch(a['sym1'], a['o1'], a['n1'], a['sym2'], a['o2'], a['n2'])))

    return Row('edit-distance', ('abn_edit_distance_batched', 'abn_edit_max_short'), build, run,
               dict(PAIR_COLS, sym1=A('int32', 1), sym2=A('int32', 1)), lengths=[('o1', 'n1', 'o2', 'n2')])


def knn_row():
    nq, nc, d, k = 9, 40, 8, 3

    def build():
        rng = rng_of('knn')
        unit = lambda x: f32(x / np.sqrt((x * x).sum(1))[:, None])
        meta = lambda n: np.stack([rng.integers(0, 3, n), rng.integers(0, 20, n), rng.integers(20, 40, n)], axis=1).astype(np.int32)
        return dict(Q=dev(unit(rng.standard_normal((nq, d)))), C=dev(unit(rng.standard_normal((nc, d)))), qm=dev(meta(nq)), cm=dev(meta(nc)))

    def run(a):
        from abnet3_amd.discovery import knn_topk
        idx, sim = knn_topk(a['Q'], a['C'], k, a['qm'], a['cm'])
        return dict(idx=host(idx), sim=host(sim))

    return Row('knn-topk', ('abn_knn_topk', 'abn_knn_ws_bytes'), build, run,
               dict(Q=A('float32', 2), C=A('float32', 2), qm=A('int32', 2), cm=A('int32', 2)),
               widths=[('Q', 'C'), ('qm', 'cm')], lengths=[('Q', 'qm'), ('C', 'cm')])


def segment_vectors_row():
    def build():
        rng = rng_of('segment-vectors')
        return dict(table=dev(f32(rng.standard_normal((40, 8)))), row0=np.array([0, 3, 10, 22, 31], dtype=np.int64),
                    L=np.array([5, 7, 12, 8, 9], dtype=np.int32))

    def run(a):
        from abnet3_amd.discovery import segment_vectors
        vec, keep = segment_vectors(a['table'], a['row0'], a['L'], 2)
        return dict(vec=host(vec), keep=host(keep))

    return Row('segment-vectors', ('abn_segment_vectors',), build, run,
               dict(table=A('float32', 2), row0=A('int64', 1, 'host'), L=A('int32', 1, 'host')), lengths=[('row0', 'L')])


def sample_pairs_row():
    counts, seed = (5, 4, 3, 1), (3 << 32) + 1

    def build():
        import torch
        from abnet3_amd import sampler as S
        from test_gpu_sampler import describe
        n = sum(counts)
        return dict(tables=S.build_tables(describe('small'), 'log', 'log'), toks=torch.zeros(2, n, dtype=torch.int32, device='cuda'),
                    key=torch.zeros(n, dtype=torch.int64, device='cuda'))

    def run(a):
        from abnet3_amd import sampler as S
        tok1, tok2, key = S.sample_pairs_device(S.DeviceTables(a['tables']), counts, seed, out=(a['toks'], a['key']))
        return dict(tok1=host(tok1), tok2=host(tok2), key=host(key))

    return Row('sample-pairs', ('abn_sample_pairs',), build, run, dict(toks=A('int32', 2, out=True), key=A('int64', 1, out=True)),
               widths=[('toks',)], lengths=[('key',)])


def samediff_rows():
    n, d = 12, 4

    def build():
        from abnet3_amd import samediff
        rng = rng_of('samediff')
        _, cbeg, cend = samediff.sort_by_type(['a'] * 4 + ['b'] * 5 + ['c'] * 3)
        return dict(X=dev(f32(rng.integers(-3, 4, (n, d)))), cbeg=cbeg, cend=cend, spk=rng.integers(0, 2, n).astype(np.int32),
                    thr=dev(f32([9.0, 4.0, 1.0, -2.0, -7.0])))

    def collect(a):
        from abnet3_amd import samediff
        pos_sim, pos_off = samediff.collect(a['X'], a['cbeg'], a['cend'])
        return dict(pos_sim=host(pos_sim), pos_off=np.asarray(pos_off))

    def count(a):
        from abnet3_amd import samediff
        hist, n_bad = samediff.pair_histogram(a['X'], a['cbeg'], a['cend'], a['thr'], a['spk'], 'swdp')
        return dict(hist=host(hist), n_bad=np.array([n_bad]))

    cols = dict(X=A('float32', 2), cbeg=A('int32', 1, 'host'), cend=A('int32', 1, 'host'))
    return [Row('sd-collect', ('abn_sd_collect',), build, collect, cols, lengths=[('X', 'cbeg', 'cend')]),
            Row('sd-count', ('abn_sd_count',), build, count, dict(cols, thr=A('float32', 1, 'any'), spk=A('int32', 1, 'host')),
                lengths=[('X', 'cbeg', 'cend', 'spk')])]


def esk_rows():
    frames, S, K, D = 2, 3, 5, 4
    lm = np.array([0, 3, 7, 12, 15, 20, 22, 26, 31, 40], dtype=np.int64)
    lm_off = np.array([0, 4, 6, 10], dtype=np.int64)

    def build_score():
        rng = rng_of('esk')
        return dict(table=dev(f32(rng.standard_normal((40, D)))), lm=lm.copy(), lm_off=lm_off.copy(), m=dev(f32(rng.standard_normal((K, frames * D)))),
                    b=dev(f32(rng.standard_normal(K))))

    def score(a):
        from abnet3_amd import eskmeans
        best, ids = eskmeans.candidate_scores(a['table'], a['lm'], a['lm_off'], a['m'], a['b'], frames, S, None)
        return dict(best=host(best), ids=host(ids))

    def build_dp():
        from abnet3_amd import eskmeans
        a = build_score()
        best, ids = eskmeans.candidate_scores(a['table'], a['lm'], a['lm_off'], a['m'], a['b'], frames, S, None)
        return dict(best=best, ids=ids, lm=lm.copy(), lm_off=lm_off.copy())

    def dp(a):
        from abnet3_amd import eskmeans
        out = eskmeans.segment_dp(a['best'], a['ids'], a['lm'], a['lm_off'], S)
        return dict(zip(('cut', 'word', 'span', 'objective', 'n_seg'), (host(t) for t in out)))

    marks = dict(lm=A('int64', 1, 'host'), lm_off=A('int64', 1, 'host'))
    return [Row('esk-score', ('abn_esk_score',), build_score, score, dict(marks, table=A('float32', 2), m=A('float32', 2), b=A('float32', 1)),
                widths=[('table',), ('m',)], lengths=[('m', 'b'), ('lm',), ('lm_off',)]),
            Row('esk-segment', ('abn_esk_segment',), build_dp, dp, dict(marks, best=A('float32', 1), ids=A('int32', 1)),
                lengths=[('best', 'ids'), ('lm',), ('lm_off',)])]


def gmm_rows():
    def build():
        import torch
        mix = mixture(rng_of('gmm'))
        mix['out'] = torch.zeros(UTT_T, MIX_K, dtype=torch.float32, device='cuda')
        return mix

    def post(a):
        from abnet3_amd import gmm
        lse, g = gmm.posteriors(a['table'], a['shift'], a['A'], a['B'], a['c'], out=a['out'])
        return dict(lse=host(lse), g=host(g))

    def em(a):
        from abnet3_amd import gmm
        st = gmm.EMState(a['w64'], a['m'], a['v'], np.ones(MIX_D), 'cuda')
        lse = gmm.em_iteration(a['table'], a['shift'], st, n_ranges=2)
        return dict(lse=host(lse), sums=host(st.sums), stats=host(st.stats), w=host(st.w), mu=host(st.mu), var=host(st.var), A=host(st.A),
                    B=host(st.B), c=host(st.c))

    T, V, M = A('float32', 2), A('float32', 1), A('float32', 2)
    return [Row('gmm-posteriors', ('abn_gmm_posteriors',), build, post, dict(table=T, shift=V, A=M, B=M, c=V, out=A('float32', 2, out=True)),
                widths=[('table', 'A', 'B'), ('out',)], lengths=[('A', 'B', 'c'), ('shift',), ('table', 'out')]),
            Row('gmm-em', ('abn_gmm_posteriors', 'abn_gmm_accumulate', 'abn_gmm_mstep', 'abn_gmm_ws_bytes'), build, em, dict(table=T, shift=V),
                widths=[('table',)], lengths=[('shift',)])]


def kmeans_rows():
    K, D = MIX_K, MIX_D

    def build():
        import torch
        from abnet3_amd import kmeans
        rng = rng_of('kmeans')
        mu = rng.standard_normal((K, D))
        m, b = kmeans.score_tables(mu)
        return dict(table=dev(f32(rng.standard_normal((UTT_T, D)))), shift=dev(np.zeros(D, dtype=np.float32)), m=dev(m), b=dev(b), mu=mu,
                    ids=torch.full((UTT_T,), -1, dtype=torch.int32, device='cuda'), off=UTT_OFF.copy(), lens=UTT_LEN.copy())

    def assign(a):
        from abnet3_amd import kmeans
        ids, best = kmeans.assign(a['table'], a['shift'], a['m'], a['b'], ids=a['ids'], want_best=True)
        return dict(ids=host(ids), best=host(best))

    def lloyd(a):
        from abnet3_amd import kmeans
        st = kmeans.LloydState(a['mu'], UTT_T, 'cuda')
        kmeans.lloyd_iteration(a['table'], a['shift'], st, n_ranges=2)
        return dict(ids=host(st.ids), sums=host(st.sums), stats=host(st.stats), mu=host(st.mu), m=host(st.m), b=host(st.b))

    def viterbi(min_duration):
        def run(a):
            from abnet3_amd import kmeans
            ids, obj, nsw = kmeans.viterbi(a['table'], a['off'], a['lens'], a['shift'], a['m'], a['b'], 3.0, ids=a['ids'], want_objective=True,
                                           min_duration=min_duration)
            return dict(ids=host(ids), objective=host(obj), n_switch=host(nsw))
        return run

    T, V, M, I = A('float32', 2), A('float32', 1), A('float32', 2), A('int32', 1, out=True)
    tabs = dict(table=T, shift=V, m=M, b=V, ids=I)
    groups = dict(widths=[('table', 'm')], lengths=[('m', 'b'), ('shift',), ('table', 'ids')])
    return [Row('kmeans-assign', ('abn_kmeans_assign',), build, assign, tabs, **groups),
            Row('kmeans-lloyd', ('abn_kmeans_assign', 'abn_kmeans_accumulate', 'abn_kmeans_update', 'abn_kmeans_ws_bytes'), build, lloyd,
                dict(table=T, shift=V), widths=[('table',)], lengths=[('shift',), ('table',)]),
            Row('kmeans-viterbi', ('abn_kmeans_viterbi', 'abn_kmeans_viterbi_ws_bytes'), build, viterbi(1), dict(tabs, **UTT_COLS),
                widths=groups['widths'], lengths=groups['lengths'] + [('off', 'lens')]),
            Row('kmeans-viterbi-dur', ('abnx_kmeans_viterbi_dur', 'abn_kmeans_viterbi_ws_bytes'), build, viterbi(2), dict(tabs, **UTT_COLS),
                widths=groups['widths'], lengths=groups['lengths'] + [('off', 'lens')])]


def hmm_rows():
    STAY, HSMM_L = 0.9, 4

    def build():
        import torch
        from abnet3_amd import hmm
        mix = mixture(rng_of('hmm'))
        lw, ls, lr = hmm.viterbi_tables(mix['w64'], STAY)
        init, trans = hmm.sticky_transitions(mix['w64'], STAY)
        li, lt = hmm.log_transitions(init, trans)
        _, lx = hmm.switch_log_transitions(init, trans)
        ld, lsd = hmm.duration_tables(*hmm.geometric_durations(trans, HSMM_L))
        mix.update(init=dev(init), trans=dev(trans), li=dev(li), lt=dev(lt), lx=dev(lx), ld=dev(ld), lsd=dev(lsd),
                   units=dev(rng_of('hmm-units').integers(0, MIX_K, UTT_T).astype(np.int32)))
        mix.update(lw=dev(lw), ls=dev(ls), lr=dev(lr), off=UTT_OFF.copy(), lens=UTT_LEN.copy(),
                   out=torch.zeros(UTT_T, MIX_K, dtype=torch.float32, device='cuda'), ids=torch.full((UTT_T,), -1, dtype=torch.int32, device='cuda'),
                   post=dev(f32(rng_of('hmm-post').dirichlet(np.ones(MIX_K), UTT_T))))
        return mix

    def fb(stats):
        def run(a):
            from abnet3_amd import hmm
            got = hmm.forward_backward(a['table'], a['off'], a['lens'], a['shift'], a['A'], a['B'], a['c0'], a['w'], STAY, 'smooth', out=a['out'],
                                       want_stay_k=stats)
            return dict(zip(('post', 'loglik', 'stays', 'n_good', 'stay_k'), (host(t) for t in got)))
        return run

    PATH = ('ids', 'log_prob', 'n_switch', 'n_good')

    def viterbi(min_duration):
        def run(a):
            from abnet3_amd import hmm
            got = hmm.viterbi(a['table'], a['off'], a['lens'], a['shift'], a['A'], a['B'], a['c0'], a['lw'], a['ls'], a['lr'], ids=a['ids'],
                              min_duration=min_duration)
            return dict(zip(PATH, (host(t) for t in got)))
        return run

    def dense_fb(a):
        from abnet3_amd import hmm
        got = hmm.dense_forward_backward(a['table'], a['off'], a['lens'], a['shift'], a['A'], a['B'], a['c0'], a['init'], a['trans'], 'smooth',
                                         out=a['out'], want_stats=True)
        return dict(zip(('post', 'loglik', 'n_good', 'stats'), (host(t) for t in got)))

    def dense_viterbi(min_duration):
        def run(a):
            from abnet3_amd import hmm
            got = hmm.dense_viterbi(a['table'], a['off'], a['lens'], a['shift'], a['A'], a['B'], a['c0'], a['li'], a['lt'], ids=a['ids'],
                                    min_duration=min_duration)
            return dict(zip(PATH, (host(t) for t in got)))
        return run

    def hsmm_viterbi(a):
        from abnet3_amd import hmm
        got = hmm.hsmm_viterbi(a['table'], a['off'], a['lens'], a['shift'], a['A'], a['B'], a['c0'], a['li'], a['lx'], a['ld'], a['lsd'], ids=a['ids'])
        return dict(zip(PATH, (host(t) for t in got)))

    def hard_stats(a):
        from abnet3_amd import hmm
        got = hmm.hard_stats(a['table'], a['off'], a['lens'], a['shift'], a['units'], MIX_K, n_ranges=2)
        return dict(zip(('counts', 'sums', 'n_good'), (host(t) for t in got)))

    def run_stats(a):
        from abnet3_amd import hmm
        dur, tail = hmm.run_stats(a['units'], a['off'], a['lens'], MIX_K, HSMM_L)
        return dict(dur=host(dur), tail=host(tail))

    def accumulate(a):
        from abnet3_amd import hmm
        return dict(sums=host(hmm.accumulate(a['table'], a['post'], a['shift'], 2)))

    T, V, M = A('float32', 2), A('float32', 1), A('float32', 2)
    emis = dict(UTT_COLS, table=T, shift=V, A=M, B=M, c0=V)
    fb_args = dict(emis, w=V, out=A('float32', 2, out=True))
    vit_args = dict(emis, lw=V, ls=V, lr=V, ids=A('int32', 1, out=True))
    vit_groups = dict(widths=[('table', 'A', 'B')], lengths=[('A', 'B', 'c0', 'lw', 'ls', 'lr'), ('shift',), ('table', 'ids'), ('off', 'lens')])
    dense_args = dict(emis, li=V, lt=M, ids=A('int32', 1, out=True))
    dense_groups = dict(widths=[('table', 'A', 'B'), ('lt',)], lengths=[('A', 'B', 'c0', 'li', 'lt'), ('shift',), ('table', 'ids'), ('off', 'lens')])
    fb_groups = dict(widths=[('table', 'A', 'B'), ('out',)], lengths=[('A', 'B', 'c0', 'w'), ('shift',), ('table', 'out'), ('off', 'lens')])
    return [Row('hmm-forward-backward', ('abn_hmm_forward_backward', 'abn_hmm_ws_bytes'), build, fb(False), fb_args, **fb_groups),
            Row('hmm-forward-backward-stats', ('abn_hmm_forward_backward_stats', 'abn_hmm_ws_bytes'), build, fb(True), fb_args, **fb_groups),
            Row('hmm-viterbi', ('abn_hmm_viterbi', 'abn_hmm_viterbi_ws_bytes'), build, viterbi(1), vit_args, **vit_groups),
            Row('hmm-viterbi-dur', ('abnx_hmm_viterbi_dur', 'abn_hmm_viterbi_ws_bytes'), build, viterbi(2), vit_args, **vit_groups),
            Row('hmm-dense-forward-backward', ('abny_hmm_dense_forward_backward', 'abny_hmm_dense_ws_bytes'), build, dense_fb,
                dict(emis, init=V, trans=M, out=A('float32', 2, out=True)), widths=[('table', 'A', 'B'), ('out',), ('trans',)],
                lengths=[('A', 'B', 'c0', 'init', 'trans'), ('shift',), ('table', 'out'), ('off', 'lens')]),
            Row('hmm-dense-viterbi', ('abnz_hmm_dense_viterbi', 'abnz_hmm_dense_viterbi_ws_bytes'), build, dense_viterbi(1), dense_args, **dense_groups),
            Row('hmm-dense-viterbi-dur', ('abnw_hmm_dense_viterbi_dur', 'abnw_hmm_dense_viterbi_dur_ws_bytes'), build, dense_viterbi(2), dense_args,
                **dense_groups),
            Row('hmm-hsmm-viterbi', ('abnu_hmm_hsmm_viterbi', 'abnu_hmm_hsmm_viterbi_ws_bytes'), build, hsmm_viterbi,
                dict(emis, li=V, lx=M, ld=M, lsd=V, ids=A('int32', 1, out=True)), widths=[('table', 'A', 'B'), ('lx',)],
                lengths=[('A', 'B', 'c0', 'li', 'lx', 'ld', 'lsd'), ('shift',), ('table', 'ids'), ('off', 'lens')]),
            Row('hmm-hard-stats', ('abnv_hmm_hard_stats', 'abnv_hmm_hard_stats_ws_bytes'), build, hard_stats,
                dict(UTT_COLS, table=T, shift=V, units=A('int32', 1)), widths=[('table',)], lengths=[('table', 'units'), ('shift',), ('off', 'lens')]),
            Row('hmm-run-stats', ('abnu_hmm_run_stats',), build, run_stats, dict(UTT_COLS, units=A('int32', 1)), lengths=[('off', 'lens')]),
            Row('hmm-accumulate', ('abn_hmm_accumulate', 'abn_hmm_accumulate_ws_bytes'), build, accumulate, dict(table=T, post=M, shift=V),
                widths=[('table',)], lengths=[('table', 'post'), ('shift',)])]


SURFACE = ([tower_row(), pair_loss_row(), nce_row(), softmax_row(), integrate_row()]
           + [frontend_row(m, b) for m in ('fbank', 'mfcc') for b in (False, True)] + table_rows()
           + [cosine_row(False), cosine_row(True), gather_row(), dtw_align_row(), dtw_one_pair_row(), dtw_cost_row('cosine'), dtw_cost_row('zero'), search_row(),
              local_row(), kl_tables_row(), kl_row('cost'), kl_row('search'), kl_row('local'), abx_score_row()]
           + lsh_rows() + [edit_row(), knn_row(), segment_vectors_row(), sample_pairs_row()] + samediff_rows() + esk_rows() + gmm_rows()
           + kmeans_rows() + hmm_rows())
assert len({r.name for r in SURFACE}) == len(SURFACE)


# ======================================================================================================================
# mutants
# ======================================================================================================================
INT_PARTNER = {'int32': np.int64, 'int64': np.int32}


def value_mutations(row):
    """(argument, kind) of every value-preserving mutant of the row: the view builders and wider() for tensors, a python
    list, the other integer width (floats: the wider dtype) and a strided slice for host arrays."""
    out = []
    for name, a in row.args.items():
        if a.where == 'host':
            kinds = ['list', 'other_int' if a.dtype in INT_PARTNER else 'wider', 'strided_rows'] + (['strided_cols', 'transposed'] if a.rank == 2 else [])
        else:
            kinds = (['strided_cols', 'transposed'] if a.rank == 2 else []) + ['strided_rows', 'wider']
        out += [(name, k) for k in kinds if not (k == 'wider' and a.dtype == 'float64')]
    return out


def value_mutant(t, kind):
    if kind == 'list':
        return t.tolist()
    if kind == 'other_int':
        return t.astype(INT_PARTNER[str(t.dtype)])
    if kind == 'wider':
        return AC.wider(t)
    return getattr(AC, kind)(t)


def shape_mutations(row):
    out = []
    for name, a in row.args.items():
        if a.rank == 2:
            out += [(name, 'rank_up'), (name, 'rank_down')]
        if a.row and name not in row.late:
            out.append((name, 'rank_up'))
        if a.where == 'device' and name not in row.late:
            out.append((name, 'cpu'))
    for group in row.widths:
        out += [(name, k) for name in group for k in ('narrower', 'broader')]
    for group in row.lengths:
        out += [(name, 'shorter') for name in group]
    return out


def shape_mutant(t, kind):
    is_np = isinstance(t, np.ndarray)
    if kind == 'rank_up':
        return t[None]
    if kind == 'rank_down':
        return t[:, 0]
    if kind == 'cpu':
        return t.cpu()
    if kind == 'narrower':
        return np.ascontiguousarray(t[:, :-1]) if is_np else t[:, :-1].contiguous()
    if kind == 'broader':
        import torch
        return np.concatenate([t, t[:, :1]], axis=1) if is_np else torch.cat([t, t[:, :1]], dim=1)
    assert kind == 'shorter'
    return t[:-1].copy() if is_np else t[:-1].clone()


def run_guarded(row, call, **guard):
    """(outputs or None for a refusal, the guard's log).  A refusal counts only when nothing was launched before it."""
    import torch
    from abnet3_amd import _lib
    out = None
    with AC.guarded(_lib.load(), **guard) as log:
        try:
            out = row.run(call)
            torch.cuda.synchronize()
        except refusals() as e:
            assert not log.launched, '%s refused (%r) after it had launched %s' % (row.name, e, log.launched)
            assert not log.blocked, '%s: the guard stopped %s and the wrapper turned that into %r' % (row.name, log.blocked, e)
            return None, log
    return {k: np.asarray(v, order='C') for k, v in out.items()}, log


def canonical(row):
    if row.name not in _CANON:
        out, log = run_guarded(row, dict(row.inputs()))
        assert out is not None, '%s: the valid call was refused' % row.name
        _CANON[row.name] = (out, log)
    return _CANON[row.name]


VALUE_CASES = [(r, n, k) for r in SURFACE for n, k in value_mutations(r)]
SHAPE_CASES = [(r, n, k) for r in SURFACE for n, k in shape_mutations(r)]


# ======================================================================================================================
# the tests
# ======================================================================================================================
@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_canonical_call(row):
    assert not set(row.entries) - set(AC.all_symbols()), sorted(set(row.entries) - set(AC.all_symbols()))
    out, log = canonical(row)
    missing = set(row.entries) - set(log.calls)
    assert not missing, 'the row claims entries it did not reach: %s (called: %s)' % (sorted(missing), sorted(set(log.calls)))
    assert not log.blocked and out
    if row.same_bits:                                                   # (what the mutation test compares against must be reproducible)
        again, _ = run_guarded(row, dict(row.inputs()))
        assert_same_bits(out, again, '%s: two valid calls' % row.name)


def check_value_mutant(row, name, kind):
    want, _ = canonical(row)
    a, call = row.args[name], dict(row.inputs())
    # (a caller's output holds what the last call wrote: the mutant is cut from zeros of its shape and dtype)
    mutant = value_mutant(call[name].clone().zero_() if a.out else call[name], kind)
    assert mutant is not None, 'no wider dtype for %s' % a.dtype
    call[name] = mutant
    legal = kind == 'wider' and str(mutant.dtype).replace('torch.', '') in a.takes
    forbidden = [] if legal or kind == 'list' else [AC.span(mutant)]
    got, log = run_guarded(row, call, forbidden=forbidden)             # (LeakedPointer is no refusal: it fails the mutant)
    if a.out:
        assert got is None, '%s took a caller\'s %s output %s and wrote through it' % (row.name, kind, name)
    if legal:
        assert got is not None, '%s refused %s in %s, a dtype it documents' % (row.name, name, mutant.dtype)
    if got is not None:
        assert row.same_bits
        assert_same_bits(want, got, '%s: %s as %s against the valid call' % (row.name, name, kind))


def check_shape_mutant(row, name, kind):
    call = dict(row.inputs())
    call[name] = shape_mutant(call[name], kind)
    got, log = run_guarded(row, call, block_all=True)                  # (ReachedLibrary is no refusal: it fails the mutant)
    assert got is None, '%s completed with %s %s without a library call?' % (row.name, name, kind)
    assert not log.blocked and not log.launched


def every_mutant(row, mutations, check):
    """Runs every mutant of the row -- one test per row, so that the suite's listing stays short -- and reports all that
    failed, each with its argument, its kind and what happened."""
    assert mutations, '%s has nothing to mutate' % row.name
    failed = []
    for name, kind in mutations:
        try:
            check(row, name, kind)
        except Exception as e:                                          # (AssertionError, LeakedPointer, ReachedLibrary, anything a wrapper lets out)
            failed.append('%s-%s: %s: %s' % (name, kind, type(e).__name__, str(e).splitlines()[0] if str(e) else ''))
    assert not failed, '%s: %d of %d mutants failed\n  %s' % (row.name, len(failed), len(mutations), '\n  '.join(failed))


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_value_preserving_mutations(row):
    every_mutant(row, value_mutations(row), check_value_mutant)


@pytest.mark.parametrize('row', SURFACE, ids=lambda r: r.name)
def test_shape_mutations_are_refused(row):
    every_mutant(row, shape_mutations(row), check_shape_mutant)


def test_counts_and_stereo_sound_are_refused():
    """What is no array and so has no row: the frame count of segment_vectors, the neighbour count of knn_topk (k > nc is
    legal: the places beyond the candidates hold -1 / -inf, include/abnet3_hip.h) and samples that are not mono."""
    from abnet3_amd import _lib
    from abnet3_amd.discovery import knn_topk, segment_vectors
    from abnet3_amd.features import FeaturesGenerator
    rows = {r.name: r for r in SURFACE}
    sv, kn = rows['segment-vectors'].inputs(), rows['knn-topk'].inputs()
    stereo = np.zeros((400, 2), dtype=np.float32)
    with AC.guarded(_lib.load(), block_all=True) as log:
        for K in (0, -1, 2.5, True, None):
            with pytest.raises(ValueError, match='segment_vectors'):
                segment_vectors(sv['table'], sv['row0'], sv['L'], K)
        for k in (0, -3, 1.5, True, None):
            with pytest.raises(ValueError, match='knn_topk'):
                knn_topk(kn['Q'], kn['C'], k, kn['qm'], kn['cm'])
        fg = FeaturesGenerator()
        for call in (lambda: fg.fbank_from_samples(stereo, FS), lambda: fg.mfcc_from_samples(stereo, FS),
                     lambda: fg.fbank_batch([stereo[:, 0], stereo], FS), lambda: fg.mfcc_batch([stereo], FS)):
            with pytest.raises(ValueError, match='mono'):
                call()
    assert not log.blocked and not log.launched
