"""Every library entry on a lagging side stream.  The other GPU tests run on the null stream, where a misplaced operation is
harmless: everything is ordered behind everything else.  Here each case runs once on the null stream and once inside
side_stream.lagging (tests/side_stream.py): the current stream is a fresh non-blocking stream, a calibrated delay sits in
front of every library entry and of every torch.empty / empty_like / zeros / zeros_like / full / ones, and torch.empty memory
is filled with 0xFF bytes behind such a delay.  A kernel, a memset, a helper launch, a read-back or a fill that goes to another
stream than the caller's runs ahead of its producers and of the poison fill, and the result is NaN / -1 or stale.

THE SWEEP (test_entry_on_a_lagging_side_stream), for every case of test_gpu_dirty_memory.CASES (imported, not copied) and for
the SECTION_CASES below: the lagging run called the entries the case claims, poisoned at least one allocation and put at
least one delay in front of an entry; it passes the case's own oracle at that family's existing bar; where the case promises
the same bits it equals the null-stream run bit for bit; a tower case took the kernel family it names (its run() asserts
the pair of paths).  No new tolerance is introduced.  Timing can only hide a mistake here, never fail correct code.

SECTION_CASES: the sections of abnet3_amd/_lib.py the dirty-memory ledger does not reach (abnx_ .. abnq_) and the five
abn_linear_* entries, one call each at the family's smallest shapes with more than one workgroup and a ragged tile, against
the family's float64 restatement at its existing bar.  No case captures a graph (CAPTURING is empty and asserted so): the
window is never open during a capture.

THE DETECTOR DETECTS (test_entries_sent_to_the_null_stream_fail_the_sweep): with _lib.stream() answering the null stream
while torch's fills stay on the lagging stream, the sweep must raise AssertionError -- on MUTANT_CASES only, whose inputs
reach the device through blocking uploads and whose kernels read no device-made index, take no ticket and never spin.

CACHES A CALLER CANNOT SEE (test_*_cache_*): an object that lazily builds device memory of its own must make it safe for
whichever stream calls next; the caller orders only its own tensors.  Stream A is stalled by one delay, the object's first
call runs on A, the same object is called at once on a stream B that does not wait for A, and both results equal the
null-stream result bit for bit.  Under this contract: FeaturesGenerator._tables, the _tables of KMeansQuantizer,
GmmPosteriorgram, StickyHmmPosteriorgram and TransitionHmmPosteriorgram, loss._UNIT and loss._WS.  NOT under it: objects with
user-visible state -- a network's parameters and weight image, kmeans.LloydState, gmm.EMState, a trainer: their callers
order their own streams.

Measured on an MI355X (side_stream.calibration() prints the three figures once per run): 2.38e6 _sleep cycles per
millisecond; an empty launch on an idle stream, launch to the end of its synchronize, 0.013 ms (so 20 of them are 0.26 ms);
the delay used is the floor, 0.500 ms = 1.19e6 cycles.  The whole file, 108 tests, takes 8.8 s (no case above 0.8 s; the
dirty-memory file takes 6 s).  With GPU_MAX_HW_QUEUES = 4 every fourth stream of torch's pool shares the null stream's
hardware queue and runs in submission order with it (side_stream.runs_ahead saw exactly that pattern): on such a stream the
null-stream mutant of cosine-distance-f32 passed the sweep, which is why side_stream.lagging picks its stream.
Needs an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

import side_stream
import test_gpu_dirty_memory as D
from dirty_memory import bits
from test_gpu_dirty_memory import Case, assert_same_bits, dev, host

pytestmark = pytest.mark.gpu

CAPTURING = {}          # case name -> reason: cases that capture a graph are kept out of the window by name.  None does.


# ======================================================================================================================
# the sections the dirty-memory ledger does not reach
# ======================================================================================================================
GAP_LENS = np.array([1, 2, 127, 128, 129, 290], dtype=np.int64)              # a gap of two rows behind every utterance but the last
GAP_OFF = np.array([0, 3, 7, 136, 266, 397], dtype=np.int64)
GAP_T = int(GAP_OFF[-1] + GAP_LENS[-1])
GAP_BAD = [8, 140, 263, 266, 400, 524, 525]


def gap_inside():
    return D.inside_rows(GAP_OFF, GAP_LENS, GAP_T)


def four(got):
    return dict(ids=host(got[0]), log_prob=host(got[1]), n_switch=host(got[2]), n_good=host(got[3]))


def check_four(out, ref, inside):
    assert np.array_equal(out['ids'][inside], ref[0][inside]) and (out['ids'][~inside] == -1).all()
    assert np.array_equal(out['log_prob'], ref[1]) and np.array_equal(out['n_switch'], ref[2]) and np.array_equal(out['n_good'], ref[3])


def min_duration_case():
    """abnx_kmeans_viterbi_dur / abnx_hmm_viterbi_dur through kmeans.viterbi / hmm.viterbi(min_duration=3) on the dirty-memory
    ledger's K = 130 chain inputs (utterances of 1, 127, 129 and 300 frames, a BAD frame): EQUAL to tests/vit_dur_np.py
    (tests/test_gpu_vit_dur.py:check_hmm / check_km)."""
    S, K = 3, 130

    def build():
        return dict(km=D.kmeans_viterbi_inputs(K), hmm=D.hmm_viterbi_inputs(K))

    def run(inp):
        from abnet3_amd import hmm, kmeans
        k, c = inp['km'], inp['hmm']
        shift = dev(np.zeros(D.CHAIN_D, dtype=np.float32))
        a = kmeans.viterbi(dev(k['x']), k['off'], D.CHAIN_LENS, shift, dev(k['m']), dev(k['b']), 3.0, want_objective=True, min_duration=S)
        b = hmm.viterbi(dev(c['x']), c['off'], D.CHAIN_LENS, shift, dev(c['A']), dev(c['B']), dev(c['c0']), dev(c['lw']), dev(c['ls']),
                        dev(c['lr']), min_duration=S)
        out = {'km.' + n: host(t) for n, t in zip(('ids', 'objective', 'n_switch'), a)}
        out.update({'hmm.' + n: v for n, v in four(b).items()})
        return out

    def oracle(inp, out):
        import units_np
        import vit_dur_np
        k, c = inp['km'], inp['hmm']
        inside = D.inside_rows(k['off'], D.CHAIN_LENS, k['T'])
        ref = vit_dur_np.viterbi(k['s'], k['good'], k['off'], D.CHAIN_LENS, *vit_dur_np.kmeans_tables(K, units_np.score_penalty(3.0)), S)
        assert np.array_equal(out['km.ids'][inside], ref[0][inside]) and (out['km.ids'][~inside] == -1).all()
        assert np.array_equal(out['km.objective'], ref[1]) and np.array_equal(out['km.n_switch'], ref[2])
        ref = vit_dur_np.viterbi(c['s'], c['good'], c['off'], D.CHAIN_LENS, c['lw'], c['ls'], c['lr'], S)
        check_four({n[4:]: v for n, v in out.items() if n.startswith('hmm.')}, ref, inside)
        for ids in (out['km.ids'], out['hmm.ids']):
            assert ids[D.CHAIN_BAD] == -1 and all(vit_dur_np.run_lengths_ok(ids[o:o + n], S) for o, n in zip(k['off'], D.CHAIN_LENS))

    return Case('section-min-duration-K130', ('abnx_kmeans_viterbi_dur', 'abnx_hmm_viterbi_dur'), build, run, oracle)


def dense_fb_case():
    """abny_hmm_dense_forward_backward through hmm.dense_forward_backward at K = 65, D = 13 on tests/test_gpu_hmm.py's
    utterances (1, 2, 127, 128, 129, 300 frames), both modes, with the statistics: tests/test_gpu_hmm_dense.py's
    check_against_reference."""
    K, Dm = 65, 13

    def build():
        import test_gpu_hmm_dense as H
        x, shift, w, m, v = H.make_model(int(sum(H.LENS)), K, Dm, seed=1000 * K + Dm)
        init, trans = H.random_transitions(K, 7 * K + Dm, 0.5)
        return dict(case=H.DenseCase(x, shift, w, m, v, H.LENS, init, trans))

    def run(inp):
        out = {}
        for mode in ('smooth', 'filter'):
            out.update({mode + '.' + k: v for k, v in inp['case'].run(mode).items()})
        return out

    def oracle(inp, out):
        import test_gpu_hmm_dense as H
        for mode in ('smooth', 'filter'):
            H.check_against_reference(inp['case'], {k[len(mode) + 1:]: v for k, v in out.items() if k.startswith(mode + '.')}, mode == 'smooth',
                                      'side stream K%d %s' % (K, mode))

    return Case('section-dense-fb-K65', ('abny_hmm_dense_forward_backward',), build, run, oracle)


def dense_exact_inputs(K, seed):
    from test_gpu_hmm_dense_vit import exact_case
    c = exact_case(GAP_T, K, 40, seed=seed)
    c['x'][GAP_BAD] = np.nan
    good = np.ones(GAP_T, dtype=bool)
    good[GAP_BAD] = False
    c['good'] = good
    return c


def dense_tables(c):
    shift = dev(np.zeros(40, dtype=np.float32))
    return [dev(c['x']), GAP_OFF, GAP_LENS, shift] + [dev(c[k]) for k in ('A', 'B', 'c0')]


def dense_viterbi_case(S):
    """abnz_hmm_dense_viterbi (S = 1) / abnw_hmm_dense_viterbi_dur (S = 3) through hmm.dense_viterbi at K = 65, D = 40 on the
    utterances and BAD frames of those files' dirty-memory tests: EQUAL to tests/hmm_dense_vit_np.py / hmm_dense_dur_np.py."""
    K = 65

    def run(c):
        from abnet3_amd import hmm
        return four(hmm.dense_viterbi(*dense_tables(c), dev(c['li']), dev(c['lt']), min_duration=S))

    def oracle(c, out):
        import hmm_dense_dur_np as dd
        import hmm_dense_vit_np as dv
        ref = dv.viterbi(c['s'], c['good'], GAP_OFF, GAP_LENS, c['li'], c['lt']) if S == 1 else \
            dd.viterbi(c['s'], c['good'], GAP_OFF, GAP_LENS, c['li'], c['lt'], S)
        check_four(out, ref, gap_inside())
        assert (out['ids'][GAP_BAD] == -1).all()

    name, entry = ('section-dense-viterbi-K65', 'abnz_hmm_dense_viterbi') if S == 1 else ('section-dense-viterbi-dur-K65', 'abnw_hmm_dense_viterbi_dur')
    return Case(name, (entry,), lambda: dense_exact_inputs(K, K), run, oracle)


def hard_stats_case():
    """abnv_hmm_hard_stats through hmm.hard_stats on tests/test_gpu_hmm_hard.py:exact_set at K = 127, D = 40, S = 3, two
    frame ranges: counts, sums and n_good EQUAL tests/hmm_hard_np.py (test_exact_inputs_equal_the_restatement)."""
    K, Dm, S = 127, 40, 3

    def build():
        import test_gpu_hmm_hard as H
        return dict(zip(('x', 'shift', 'ids', 'off', 'lens'), H.exact_set(K, Dm, S, seed=1000 * K + 10 * Dm + S)))

    def run(inp):
        from abnet3_amd import hmm
        got = hmm.hard_stats(dev(inp['x']), inp['off'], inp['lens'], dev(inp['shift']), dev(inp['ids'], np.int32), K, min_duration=S, n_ranges=3)
        return dict(counts=host(got[0]), sums=host(got[1]), n_good=host(got[2]))

    def oracle(inp, out):
        import hmm_hard_np as hh
        ref = hh.hard_stats(inp['x'], inp['off'], inp['lens'], inp['shift'], inp['ids'], K, S)
        assert np.array_equal(out['counts'], ref[0]) and np.array_equal(out['sums'], ref[1]) and np.array_equal(out['n_good'], ref[2])
        assert np.isfinite(out['sums']).all()

    return Case('section-hard-stats-K127', ('abnv_hmm_hard_stats',), build, run, oracle)


def hsmm_case():
    """abnu_hmm_hsmm_viterbi and abnu_hmm_run_stats through hmm.hsmm_viterbi / hmm.run_stats at K = 65, L = 20 on the utterances
    and BAD frames of tests/test_gpu_hmm_hsmm.py's dirty-memory test: EQUAL to tests/hmm_hsmm_np.py; the run statistics are
    taken of the device ids as they are, on the same stream."""
    K, L = 65, 20

    def build():
        from test_gpu_hmm_hsmm import with_durations
        c = dense_exact_inputs(K, K)
        good = c.pop('good')
        c = with_durations(c, L, seed=K)
        c['good'] = good
        return c

    def run(c):
        from abnet3_amd import hmm
        got = hmm.hsmm_viterbi(*dense_tables(c), dev(c['li']), dev(c['lx']), dev(c['ld']), dev(c['ls']))
        dur, tail = hmm.run_stats(got[0], GAP_OFF, GAP_LENS, K, L)
        return dict(four(got), dur=host(dur), tail=host(tail))

    def oracle(c, out):
        import hmm_hsmm_np as hs
        ref = hs.viterbi(c['s'], c['good'], GAP_OFF, GAP_LENS, c['li'], c['lx'], c['ld'], c['ls'])
        check_four(out, ref, gap_inside())
        want = hs.run_stats(ref[0], GAP_OFF, GAP_LENS, K, L)
        assert np.array_equal(out['dur'], want[0]) and np.array_equal(out['tail'], want[1]) and want[0].sum() > 0

    return Case('section-hsmm-K65-L20', ('abnu_hmm_hsmm_viterbi', 'abnu_hmm_run_stats'), build, run, oracle)


def nce_case():
    """abnt_nce_loss through InfoNCELoss.value_and_grad at B = 257, D = 100, temperature 0.07 (tests/nce_np.py's named case):
    tests/nce_np.py:check at its derived bars."""
    B, Dm, tau = 257, 100, 0.07

    def build():
        import nce_np
        e1, e2 = nce_np.make_case(B, Dm)
        return dict(e1=e1, e2=e2, y=nce_np.labels(B, 'all'))

    def run(inp):
        from abnet3_amd.loss import InfoNCELoss
        loss, de = InfoNCELoss(temperature=tau).value_and_grad(dev(inp['e1'], np.float32), dev(inp['e2'], np.float32), dev(inp['y']))
        return dict(loss=host(loss), de=host(de))

    def oracle(inp, out):
        import nce_np
        ref = nce_np.reference(inp['e1'], inp['e2'], inp['y'], tau)
        nce_np.check(out['loss'], out['de'][0], out['de'][1], ref, B, Dm, tau, True, 'side stream')

    return Case('section-nce-B257', ('abnt_nce_loss',), build, run, oracle)


def edit_hist_case():
    """abns_edit_cluster_hist through tde.cluster_histogram on tests/test_gpu_tde_full.py's table 'short-2' (150 clusters,
    sizes around the wavefront): hist, n_pairs and n_skipped EQUAL tests/tde_full_np.py."""
    def build():
        import test_gpu_tde_full as F
        return dict(t=F.table_of('short-2'))

    def run(inp):
        import test_gpu_tde_full as F
        hist, n_pairs, n_skipped = F.run(inp['t'])
        return dict(hist=np.asarray(hist), counts=np.array([n_pairs, n_skipped], dtype=np.int64))

    def oracle(inp, out):
        import test_gpu_tde_full as F
        F.assert_equal((out['hist'], int(out['counts'][0]), int(out['counts'][1])), F.reference('short-2'), 'side stream')

    return Case('section-edit-hist', ('abns_edit_cluster_hist',), build, run, oracle)


def recon_case():
    """abnr_recon_loss through CorrespondenceLoss.value_and_grad at B = 257, D = 39, both modes: tests/test_gpu_cae.py's bars
    (loss 4 x 2^-24 relative, gradients 3 x 2^-24 relative per element, exact zeros on the rows that do not count)."""
    B, Dm = 257, 39

    def build():
        import cae_np
        h = cae_np.draw(np.random.default_rng(1000 * B + Dm), B, Dm)
        h[4][0], h[4][1] = 1, -1
        return dict(h=h)

    def run(inp):
        from abnet3_amd.loss import CorrespondenceLoss
        d = [dev(a) for a in inp['h']]
        out = {}
        for mode in ('correspondence', 'autoencoder'):
            loss, dr = CorrespondenceLoss(mode=mode).value_and_grad(*d)
            out.update({mode + '.loss': host(loss), mode + '.dr': host(dr)})
        return out

    def oracle(inp, out):
        import cae_np
        from test_gpu_cae import GRAD_BAR, VALUE_BAR
        h = inp['h']
        for mode in ('correspondence', 'autoencoder'):
            lv, _, g1, g2 = cae_np.recon_loss(*h, mode, True, True)
            counted = cae_np.counted_rows(h[4], mode, B)
            assert abs(float(out[mode + '.loss']) - lv) <= VALUE_BAR * abs(lv), (mode, float(out[mode + '.loss']), lv)
            for g, w in zip(out[mode + '.dr'], (g1, g2)):
                assert (np.abs(g.astype(np.float64) - w) <= GRAD_BAR * np.abs(w)).all(), mode
                assert not bits(g[~counted]).any(), mode

    return Case('section-recon-B257', ('abnr_recon_loss',), build, run, oracle)


def softdtw_case():
    """abnq_softdtw_forward and abnq_softdtw_backward through softdtw.soft_dtw_batch(keep=True) / soft_dtw_backward on
    tests/test_gpu_sdtw.py:mixed_table (300 problems of lengths 1 .. 40): the backward runs on the same lagging stream as its
    forward, from the saved workspace; values and gradients of that test's ten problems at its bars against tests/sdtw_np.py."""
    gamma, Dm = 0.1, 8

    def build():
        import test_gpu_sdtw as T
        return dict(zip(('e', 'off1', 'n1', 'off2', 'n2', 'w'), T.mixed_table()))

    def run(inp):
        from abnet3_amd import softdtw
        value, handle = softdtw.soft_dtw_batch(dev(inp['e']), inp['off1'], inp['n1'], inp['off2'], inp['n2'], gamma, keep=True)
        g1, g2 = softdtw.soft_dtw_backward(handle, dev(inp['w']))
        return dict(value=host(value), g1=host(g1), g2=host(g2))

    def oracle(inp, out):
        import sdtw_np as S
        from test_gpu_sdtw import EPS, value_bar
        e, off1, n1, off2, n2, w = (inp[k] for k in ('e', 'off1', 'n1', 'off2', 'n2', 'w'))
        s1, s2 = np.cumsum(n1) - n1, np.cumsum(n2) - n2
        assert all(np.isfinite(out[k]).all() for k in out)
        for p in (2, 3, 5, 7, 11, 12, 39, 79, 150, 299):
            x, y = e[off1[p]:off1[p] + n1[p]], e[off2[p]:off2[p] + n2[p]]
            ref, yard = S.problem(x, y, gamma, float(w[p])), S.problem(x, y, gamma, float(w[p]), cell_dtype=np.float32)
            assert abs(float(out['value'][p]) - ref['value']) <= value_bar(n1[p], n2[p], Dm, ref['value']), p
            yerr = max(np.abs(yard['g1'] - ref['g1']).max(), np.abs(yard['g2'] - ref['g2']).max())
            gerr = max(np.abs(out['g1'][s1[p]:s1[p] + n1[p]] - ref['g1']).max(), np.abs(out['g2'][s2[p]:s2[p] + n2[p]] - ref['g2']).max())
            gmax = max(np.abs(ref['g1']).max(), np.abs(ref['g2']).max())
            assert gerr <= 16 * yerr + 4 * EPS * gmax, p

    return Case('section-softdtw-P300', ('abnq_softdtw_forward', 'abnq_softdtw_backward'), build, run, oracle)


def linear_case():
    """The five abn_linear_* entries at tests/test_gpu_linear_entries.py's (130, 72, 136) -- a ragged last row block, column
    block and k step on every tile --, sigmoid, fp32, every output and the split-K scratch from torch.empty: conftest.rel_err
    < 1e-5 against that file's float64 products.  (The dirty-memory ledger leaves these entries to that file's NaN-filled
    outputs; on a lagging stream the question is another one: which stream the launches and the split-K reduction take.)"""
    shape, act = (130, 72, 136), 1

    def build():
        import test_gpu_linear_entries as LE
        return dict(c=LE.case(*shape))

    def run(inp):
        import torch
        from abnet3_amd import _lib
        lib, p, c = _lib.load(), _lib.ptr, inp['c']
        rows, k, n = shape
        x, W, b, dz = dev(c['x']), dev(c['W']), dev(c['b']), dev(c['dz'])
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device='cuda')
        sc_n = lib.abn_linear_wgrad_scratch_floats(rows, k, n)
        y, dx = new(rows, n), new(rows, k)
        _lib.check(lib.abn_linear_forward(p(x), p(W), p(b), rows, k, n, act, p(y), _lib.stream()), 'abn_linear_forward')
        _lib.check(lib.abn_linear_dgrad(p(dz), p(W), rows, k, n, p(x), act, p(dx), _lib.stream()), 'abn_linear_dgrad')
        out = dict(y=host(y), dx=host(dx))
        dW, db, sc = new(n, k), new(n), new(sc_n)
        _lib.check(lib.abn_linear_wgrad(p(dz), p(x), rows, k, n, p(dW), p(db), p(sc), sc_n, _lib.stream()), 'abn_linear_wgrad')
        out.update(dW=host(dW), db=host(db))
        for name in ('abn_linear_backward', 'abn_linear_backward_prec'):
            dW, db, dx, sc = new(n, k), new(n), new(rows, k), new(sc_n)
            head = [p(dz), p(W), p(x), rows, k, n, act] + ([0] if name.endswith('prec') else [])
            _lib.check(getattr(lib, name)(*(head + [p(dW), p(db), p(dx), p(sc), sc_n, _lib.stream()])), name)
            out.update({name + '.dW': host(dW), name + '.db': host(db), name + '.dx': host(dx)})
        return out

    def oracle(inp, out):
        import test_gpu_linear_entries as LE
        from conftest import rel_err
        c = inp['c']
        dx = c['exact']['dx'] * LE.act_grad_f64(c['x64'], act)
        want = dict(y=LE.act_f64(c['z'] + c['b'].astype(np.float64), act), dx=dx, dW=c['exact']['dW'], db=c['exact']['db'])
        for name in ('abn_linear_backward', 'abn_linear_backward_prec'):
            want.update({name + '.dW': c['exact']['dW'], name + '.db': c['exact']['db'], name + '.dx': dx})
        assert want.keys() == out.keys()
        for k in want:
            assert rel_err(out[k], want[k]) < LE.TOL, (k, rel_err(out[k], want[k]))

    return Case('section-linear-entries', ('abn_linear_forward', 'abn_linear_dgrad', 'abn_linear_wgrad', 'abn_linear_backward',
                                           'abn_linear_backward_prec'), build, run, oracle)


SECTION_CASES = [min_duration_case(), dense_fb_case(), dense_viterbi_case(1), dense_viterbi_case(3), hard_stats_case(), hsmm_case(),
                 nce_case(), edit_hist_case(), recon_case(), softdtw_case(), linear_case()]
CASES = [c for c in D.CASES + SECTION_CASES if c.name not in CAPTURING]
assert len({c.name for c in CASES}) == len(CASES) and not CAPTURING

# the cases of the null-stream mutant: the issue's list, not to be widened (blocking uploads, no device-made index table, no
# ticket, no spin: a call that runs early writes a result that is then poisoned, and nothing reads out of bounds)
MUTANT_CASES = ('softmax-rows', 'mvn-per-channel', 'mvn-whole', 'stack-T5-n7', 'stack-T100-n3', 'arccos', 'cosine-distance-f32')
assert set(MUTANT_CASES) <= {c.name for c in D.CASES}


# ======================================================================================================================
# the sweep
# ======================================================================================================================
def run_null(case):
    import torch
    D.clear_caches()
    out = case.run(case.inputs())
    torch.cuda.synchronize()
    return {k: np.asarray(v, order='C') for k, v in out.items()}


def run_lagging(case):
    """One run of the case inside the window, ending with side.synchronize(): (outputs, side_stream.Lag)."""
    import torch
    from abnet3_amd import _lib
    D.clear_caches()
    assert not torch.cuda.is_current_stream_capturing()
    with side_stream.lagging(_lib.load(), side_stream.gpu_delay()) as lag:
        out = case.run(case.inputs())
        lag.side.synchronize()
    return {k: np.asarray(v, order='C') for k, v in out.items()}, lag


def sweep(case):
    import torch
    from abnet3_amd import _lib
    null = run_null(case)
    out, lag = run_lagging(case)
    assert lag.side.cuda_stream != torch.cuda.default_stream().cuda_stream
    missing = set(case.entries) - set(lag.calls)
    assert not missing, 'the case claims entries it did not reach: %s (called: %s)' % (sorted(missing), sorted(set(lag.calls)))
    assert int(lag.poisoned) > 0, 'no allocation of this case went through torch.empty: nothing was poisoned'
    assert lag.entry_delays > 0 and lag.alloc_delays > 0, lag
    case.oracle(case.inputs(), out)
    if case.same_bits:
        assert_same_bits(null, out, '%s: the null stream against the lagging side stream' % case.name)
    else:
        case.oracle(case.inputs(), null)
    if case.paths is not None:                                   # (a tower case's run() asserts the pair of paths it took)
        assert _lib.trace_paths and _lib.last_path['forward'] >= 0 and _lib.last_path['backward'] >= 0


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_entry_on_a_lagging_side_stream(case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sweep(case)


@pytest.mark.parametrize('case', [c for c in D.CASES if c.name in MUTANT_CASES], ids=lambda c: c.name)
def test_entries_sent_to_the_null_stream_fail_the_sweep(case, monkeypatch):
    """The only deliberate misuse of this file: the entries go to the null stream, torch's fills stay on the lagging stream."""
    import torch
    from abnet3_amd import _lib
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(_lib, 'stream', lambda: ctypes.c_void_p(0))
    try:
        with pytest.raises(AssertionError):
            sweep(case)
    finally:
        torch.cuda.synchronize()


def test_the_mutant_list_is_the_one_the_file_states():
    assert len([c for c in D.CASES if c.name in MUTANT_CASES]) == len(MUTANT_CASES) == 7


# ======================================================================================================================
# caches a caller cannot see
# ======================================================================================================================
def two_independent_streams(delay):
    """Streams A and B such that a launch on B was seen to finish while A was stalled (side_stream.runs_ahead)."""
    import torch
    a = torch.cuda.Stream()
    b, independent = side_stream.pick_stream(lambda s: s.cuda_stream != a.cuda_stream and side_stream.runs_ahead(s, a, delay))
    assert a.cuda_stream != b.cuda_stream
    return a, b


def on_two_streams(make, call):
    """make() -> a fresh object (its inputs uploaded and complete); call(obj) -> {name: device tensor}, no read-back of its
    own.  Returns (null-stream result, result of the first call on the stalled stream A, result of the call made at once
    on stream B, which does not wait for A) as host arrays."""
    import torch
    null = {k: host(v) for k, v in call(make()).items()}
    torch.cuda.synchronize()
    obj = make()
    torch.cuda.synchronize()
    delay = side_stream.gpu_delay()
    a, b = two_independent_streams(delay)
    with torch.cuda.stream(a):
        delay()
        on_a = call(obj)
    with torch.cuda.stream(b):
        on_b = call(obj)
        got_b = {k: host(v) for k, v in on_b.items()}
    with torch.cuda.stream(a):
        got_a = {k: host(v) for k, v in on_a.items()}
    torch.cuda.synchronize()
    return null, got_a, got_b


def assert_both_equal_null(null, got_a, got_b, what):
    assert_same_bits(null, got_a, what + ': the first call, on the stalled stream')
    assert_same_bits(null, got_b, what + ': the call at once on a second stream')


@pytest.mark.parametrize('method', ['fbanks', 'mfcc'])
def test_features_generator_cache_serves_a_second_stream(method):
    """FeaturesGenerator._tables (window, mel bank, bands, DCT table): passes as the code stands because every table is
    uploaded from pageable host memory with a blocking copy -- the host does not return from the first call's _table()
    before the tables are complete on the device, so any stream that calls next reads finished memory."""
    from abnet3_amd.features import FeaturesGenerator
    from test_gpu_mfcc import speech_like
    wave = speech_like(4000, D.FS, 4000)

    def call(fg):
        return dict(feats=(fg.mfcc_from_samples if method == 'mfcc' else fg.fbank_from_samples)(wave, D.FS))

    assert_both_equal_null(*on_two_streams(lambda: FeaturesGenerator(method=method, deltas=True, deltasdeltas=True), call), method)


def mixture(K=5, Dm=13, T=300):
    from abnet3_amd.gmm import GmmPosteriorgram
    from test_gpu_gmm import make_case
    x, shift, gv, w, m, v = make_case(T, K, Dm, seed=T * 1000 + K)
    g = GmmPosteriorgram(K)
    g.weights_, g.means_, g.variances_ = np.asarray(w, dtype=np.float64), m + shift.astype(np.float64), np.asarray(v, dtype=np.float64)
    g.shift_, g.gv_ = shift, np.asarray(gv, dtype=np.float64)
    return g, x


@pytest.mark.parametrize('model', ['kmeans', 'gmm', 'sticky-hmm', 'transition-hmm'])
def test_model_table_cache_serves_a_second_stream(model):
    """The _tables of KMeansQuantizer, GmmPosteriorgram, StickyHmmPosteriorgram and TransitionHmmPosteriorgram (the last two
    through the mixture's): pass as the code stands because device_tables() uploads every table from pageable host memory
    with a blocking copy -- the tables are complete before the first call's first launch is even enqueued."""
    from abnet3_amd import hmm
    from abnet3_amd.kmeans import KMeansQuantizer
    g, x = mixture()
    table = dev(x)

    def make():
        g._tables = None
        if model == 'kmeans':
            q = KMeansQuantizer(g.n_components)
            q.centroids_, q.shift_ = g.means_.copy(), g.shift_.copy()
            return q
        return {'gmm': lambda: g, 'sticky-hmm': lambda: hmm.StickyHmmPosteriorgram(g, 0.8),
                'transition-hmm': lambda: hmm.TransitionHmmPosteriorgram(g, stay=0.8)}[model]()

    def call(obj):
        if model == 'kmeans':
            return dict(ids=obj.predict(table), rows=obj.quantize(table))
        return dict(post=obj.transform(table))

    assert_both_equal_null(*on_two_streams(make, call), model)


def test_loss_scratch_cache_serves_a_second_stream():
    """loss._WS (the pair loss's zeroed scratch with its ticket word): passes as the code stands because the cache is keyed by
    (device, stream) -- stream B builds a buffer of its own, zeroed in B's order, and never sees A's."""
    import abnet3_amd.loss as L
    rng = np.random.default_rng(3)
    e1, e2 = dev(rng.standard_normal((300, 33)).astype(np.float32)), dev(rng.standard_normal((300, 33)).astype(np.float32))
    y = dev(rng.choice([1, -1], 300))

    def make():
        L._WS.clear()
        return L.coscos2(avg=True)

    def call(f):
        loss, de = f.value_and_grad(e1, e2, y)
        return dict(loss=loss, de=de)

    assert_both_equal_null(*on_two_streams(make, call), 'coscos2')
    assert len(L._WS) >= 2


def test_unit_gradient_cache_serves_a_second_stream():
    """loss._UNIT (the cached gradient seed 1.0): the 1.0 must be there for whichever stream reads it next.  The memory the
    allocator is likely to hand out on stream A is filled with NaN first, so a seed whose fill is still queued behind A's
    delay reads as NaN on B."""
    import torch
    import abnet3_amd.loss as L

    def make():
        L._UNIT.clear()
        s = torch.cuda.current_stream()
        junk = [torch.full((n,), float('nan'), device='cuda') for n in (1, 128, 1 << 18)]
        s.synchronize()
        del junk
        return torch.device('cuda', torch.cuda.current_device())

    def call(device):
        return dict(unit=L.unit_grad(device) * 1.0)

    null = host(call(make())['unit'])
    torch.cuda.synchronize()
    delay = side_stream.gpu_delay()
    a, b = two_independent_streams(delay)
    with torch.cuda.stream(a):
        device = make()                                          # (the NaN blocks go back to stream A's pool)
        delay()
        on_a = call(device)
    with torch.cuda.stream(b):
        got_b = host(call(device)['unit'])
    with torch.cuda.stream(a):
        got_a = host(on_a['unit'])
    torch.cuda.synchronize()
    assert null.tobytes() == got_a.tobytes() == got_b.tobytes() == np.float32(1.0).tobytes(), (null, got_a, got_b)
