#!/usr/bin/env python3
"""The zero-resource loop, no labels at any point: a synthetic corpus -> log-mel filterbanks (HIP) -> pair discovery
(KnnPairMiner: segment vectors + k-nearest neighbours on the matrix cores) -> PairsDataLoader -> a few epochs of
Siamese training -> embedding -> ABX.  The corpus' word labels are used twice only, to report: the precision of the
mined pairs, and the ABX item file ("phones" = word types).

    python examples/zero_resource.py [--utts 40] [--epochs 3] [--out /tmp/abnet3_zr] [--softmax] [--tcl] [--qbe]
                                     [--infonce] [--temperature T] [--cae] [--cae-pretrain N] [--cae-init-abnet]
                                     [--gmm] [--gmm-components 64] [--hmm-stay P|fit] [--hmm-fit N] [--hmm-trans N] [--hmm-decode] [--no-network] [--terms] [--terms-theta T]
                                     [--prefilter] [--alignment FILE] [--word-alignment FILE]
                                     [--kmeans] [--kmeans-clusters 50] [--kmeans-penalty P] [--kmeans-min-duration S]
                                     [--hmm-min-duration S] [--hmm-trans-viterbi] [--hmm-max-duration L]
                                     [--eskmeans] [--eskmeans-clusters 24] [--samediff]

--softmax runs the same loop with a softmax output layer and KLLoss: the embeddings are posteriorgrams, and their ABX
error is printed under both frame distances, the angular cosine and the symmetrised Kullback-Leibler divergence.
--infonce trains with the in-batch contrastive loss (InfoNCELoss, temperature T, default 0.1, untuned) instead of
coscos2: the 'same' pairs of a batch are the anchors and every other row of the batch is a negative.  It composes with
--tcl and with the mined-pairs route; it is not combined with --softmax.
--cae trains a correspondence autoencoder (CorrespondenceAutoencoder + CorrespondenceLoss through TrainerCorrespondence)
on the same pairs instead of the Siamese network -- each frame reconstructs its aligned partner -- and embeds its bottleneck;
--cae-pretrain N first runs N passes in which every frame reconstructs itself; --cae-init-abnet then trains the usual
Siamese network starting from the cAE's encoder (save_encoder's file) and embeds that one.  Untuned.  Under --cae the ABX of
the embeddings reads exactly parallel frames as distance 0 (ABXEvaluator(parallel='zero')): a network started from the cAE's
encoder gave some frames exactly parallel embeddings on this corpus, and the default rule drops every pair that holds two such frames.
--tcl skips the discovery step altogether: TemporalCoherenceDataLoader trains on temporal-coherence pairs (a frame and
its neighbour against frames 15-30 steps away, drawn on the GPU), and the dev pairs that early stopping needs are made
the same way from the last fifth of the files -- a stretch of frames against itself one frame later ("same") and
against a stretch of another file ("diff").
--qbe adds query-by-example search after the embedding (abnet3_amd/qbe.py): the first token of a few word types is
searched in every utterance by subsequence DTW, and the mean average precision of the rankings is printed.
--gmm adds the untrained baseline (abnet3_amd/gmm.py): a Gaussian mixture fitted on the filterbanks, its posteriorgrams
under the KL frame distance -- ABX, and with --qbe the search.  No network is trained on this route; --no-network stops
after it, otherwise its figures are printed again beside the embeddings'.  --hmm-stay P (or "fit": EM on the stay
probability) smooths the posteriorgrams with the sticky HMM of abnet3_amd/hmm.py and prints ABX (kl) of both.
--hmm-fit N trains that HMM by N iterations of Baum-Welch from the mixture (means, variances, weights and the stay)
and prints ABX (kl) of raw, smoothed and Baum-Welch-trained posteriorgrams side by side.  --hmm-trans N trains the
full-transition HMM (TransitionHmmPosteriorgram: a K x K transition matrix, K <= 128) by N iterations from the sticky
matrix and prints ABX (kl) of raw, sticky-smoothed and transition-smoothed posteriorgrams side by side.  --hmm-decode adds the
discrete units of that HMM's best path (StickyHmmPosteriorgram.decode, Viterbi): their bitrate and switch count beside
those of the frame-wise mixture argmax (stay = 0 through the same call), and ABX over the quantised frames (each frame
replaced by its unit's mean); with --hmm-trans N also the units of the full-transition HMM's best path
(TransitionHmmPosteriorgram.decode), and with --hmm-min-duration S those whose units last at least S frames under either
model.  Nothing in it is tuned on real speech.
--hmm-trans-viterbi (with --hmm-trans N) also trains the full-transition HMM by N iterations of Viterbi training
(TransitionHmmPosteriorgram.fit_viterbi: hard EM on the decoded path, with the minimum duration of --hmm-min-duration)
from the same start and prints its best-path log probability, changed ids and switches on a line of its own.
--terms replaces the pair miner by term discovery (abnet3_amd/terms.py): local-alignment DTW of every utterance against
every other -- over the filterbanks, or with --gmm over the mixture's posteriorgrams under the KL distance -- clustered
into a .classes file, from which SamplerClusterSiamese draws the train and dev pairs: the reference's canonical route,
with discovered clusters in place of labelled ones.  The purity of the clusters against the planted words is printed.
With --prefilter only the kernel pairs whose dot plot of LSH signatures holds a diagonal run are aligned
(abnet3_amd/prefilter.py, its untuned defaults); the share of kernel pairs aligned is printed.
With --alignment FILE (`file onset offset symbol` lines, a phone alignment of the corpus' files) the clusters are also
scored against it: NED and coverage (abnet3_amd/tde.py), the line `python -m abnet3_amd.tde` prints.  With
--word-alignment FILE as well (the same format, the symbols are words) the clusters of --terms or --eskmeans also get the
full line of `python -m abnet3_amd.tde --full`: token, type, boundary and grouping scores, NED within / across speaker.
--kmeans adds discrete units (abnet3_amd/kmeans.py): k-means over the embeddings -- with --no-network over the
filterbanks -- and prints the units' bitrate and the ABX error of the quantised frames (each frame replaced by its
centroid, the ZeroSpeech way of scoring units) next to the continuous ones.  --kmeans-penalty P prints a second line
for the penalised segmentation (KMeansQuantizer.segment: a cost of P, in units of the distortion, per new segment; no
tuned default): bitrate and ABX with the penalty beside those without.
--eskmeans (with --kmeans --kmeans-penalty P) adds full-coverage word segmentation (abnet3_amd/eskmeans.py): landmarks
at the boundaries of the penalised units, ES-KMeans over them, the number of segments and clusters, and how many edges
of the planted words lie within 30 ms of a chosen cut.  n_clusters, max_span and the landmark density are untuned.
--samediff adds same-different word discrimination (abnet3_amd/samediff.py) over the planted words' tokens: the average
precision of "same word" among all token pairs, under DTW over the filterbanks, under DTW over the embeddings, and under
the cosine of the embeddings' segment vectors (the objects KnnPairMiner searches and ESKMeans clusters).
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from abnet3_amd.abx import ABXEvaluator, Items                    # noqa: E402
from abnet3_amd.dataloader import DeviceCorpus, OriginalDataLoader, PairsDataLoader, TemporalCoherenceDataLoader   # noqa: E402
from abnet3_amd.discovery import KnnPairMiner                     # noqa: E402
from abnet3_amd.embedder import EmbedderSiamese                   # noqa: E402
from abnet3_amd.features import FeaturesGenerator                 # noqa: E402
from abnet3_amd.gmm import GmmPosteriorgram                       # noqa: E402
from abnet3_amd.hmm import StickyHmmPosteriorgram, TransitionHmmPosteriorgram, sticky_transitions      # noqa: E402
from abnet3_amd.kmeans import KMeansQuantizer, bitrate, unit_sequences   # noqa: E402
from abnet3_amd.loss import CorrespondenceLoss, InfoNCELoss, KLLoss, coscos2    # noqa: E402
from abnet3_amd.model import CorrespondenceAutoencoder, SiameseNetwork   # noqa: E402
from abnet3_amd.prefilter import TermPrefilter                   # noqa: E402
from abnet3_amd.samediff import SameDifferentEvaluator            # noqa: E402
from abnet3_amd.sampler import SamplerClusterSiamese              # noqa: E402
from abnet3_amd.tde import TermEvaluator, full_summary, summary                 # noqa: E402
from abnet3_amd.terms import TermDiscoverer                       # noqa: E402
from abnet3_amd.trainer import TrainerCorrespondence, TrainerSiamese   # noqa: E402
from end_to_end import synth_corpus                               # noqa: E402


def tcl_loader(fb, times, rng, stretch=12):
    """TemporalCoherenceDataLoader over the first four fifths of the files; label-free dev pairs from the rest."""
    names = sorted(fb)
    cut = max(1, len(names) * 4 // 5)
    held = [k for k in names[cut:] if len(fb[k]) > 2 * stretch] or names[:1]

    def stretch_of(k, shift=0):
        a = int(rng.integers(0, len(fb[k]) - stretch - 1)) if shift == 0 else shift
        return a, (k, float(times[k][a]), float(times[k][a + stretch - 1]))
    dev = []
    for i in range(64):
        k = held[i % len(held)]
        a, tok = stretch_of(k)
        if i % 2 == 0:
            dev.append(tok + stretch_of(k, a + 1)[1] + ('same',))
        else:
            dev.append(tok + stretch_of(held[(i + 1 + int(rng.integers(len(held)))) % len(held)])[1] + ('diff',))
    # (the train "pairs" only name the files that train: this loader never reads their tokens)
    train = [(k, 0.0, 0.1, k, 0.0, 0.1, 'diff') for k in names[:cut]]
    dl = TemporalCoherenceDataLoader(None, None, batch_size=500, num_max_minibatches=200, seed=0)
    dl.set_data(fb, times, train, dev)
    print('temporal coherence: %d files train, %d dev pairs from %d held-out files' % (cut, len(dev), len(held)))
    return dl


def qbe_search(corpus, tokens, names, label, distance, n_queries=8):
    """Query by example: the first token of each of a few word types is searched in every utterance; an utterance is
    relevant when it holds a token of the query's word (the query's own utterance included: it has to find itself)."""
    from abnet3_amd.qbe import QbeSearcher, max_query, mean_average_precision, precision_at_n
    first = {}
    for t in tokens:
        if t[3] not in first and corpus.token(t[0], t[1], t[2])[1] <= max_query():
            first[t[3]] = t
    queries = [first[w] for w in sorted(first)][:n_queries]
    res = QbeSearcher(corpus, distance=distance).search([(t[0], t[1], t[2]) for t in queries])
    holds = {(t[3], t[0]) for t in tokens}
    relevant = np.array([[(q[3], k) in holds for k in names] for q in queries])
    own = [res.ranking(i)[0] == names.index(q[0]) for i, q in enumerate(queries)]
    print('query by example on %s (%s): %d queries x %d utterances, MAP %.3f, P@N %.3f, %d of %d queries rank their own '
          'utterance first' % (label, distance, len(queries), len(names), mean_average_precision(res.score, relevant),
                               precision_at_n(res.score, relevant), sum(own), len(own)))


def word_items(tokens):
    keep = [t for t in tokens if t[2] - t[1] >= 0.1]
    return keep, Items([t[0] for t in keep], [t[1] for t in keep], [t[2] for t in keep], ['w%d' % t[3] for t in keep],
                       ['-'] * len(keep), ['-'] * len(keep), ['spk'] * len(keep))


def samediff_lines(corpus, tokens, label, vectors):
    """Same-different AP of the planted words' tokens (a word type per planted word) over `corpus`."""
    words = sorted({t[3] for t in tokens})
    ev = SameDifferentEvaluator([[(t[0], t[1], t[2]) for t in tokens if t[3] == w] for w in words], corpus)
    for distance in ('dtw', 'vectors') if vectors else ('dtw',):
        r = ev.evaluate(distance)
        print('same-different on %s (%s): AP %.3f, PRB %.3f (%d tokens of %d words, %d positives in %d pairs, %d dropped)'
              % (label, 'segment vectors' if distance == 'vectors' else 'DTW', r.ap, r.prb, r.n_tokens, r.n_types,
                 r.n_positives, r.n_pairs, r.n_bad + r.n_dropped_tokens))


def guess_theta(table, distance, rng, quantile=0.04, n=20000):
    """A crude, untuned stand-in for a tuned theta: the 4 % quantile of the frame distance between random frame pairs of
    the corpus, so that only the closest frame pairs add to a path."""
    x = table.cpu().numpy().astype(np.float64)
    a, b = x[rng.integers(0, len(x), n)], x[rng.integers(0, len(x), n)]
    if distance == 'kl':
        a, b = np.maximum(a, 1e-6), np.maximum(b, 1e-6)
        d = 0.5 * ((a - b) * (np.log(a) - np.log(b))).sum(axis=1)
    else:
        cos = (a * b).sum(axis=1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-30)
        d = np.arccos(np.clip(cos, -1.0, 1.0)) / np.pi
    return float(np.quantile(d, quantile))


def terms_loader(corpus, fb, times, tokens, out, distance, theta, rng, min_frames=15, alignment=None, prefilter=False, word_alignment=None):
    """features or posteriorgrams -> TermDiscoverer -> terms.classes -> SamplerClusterSiamese -> the loader of its pairs."""
    if theta is None:
        theta = guess_theta(corpus.table, distance, rng)
    td = TermDiscoverer(corpus, distance=distance, theta=theta, min_frames=min_frames,
                        prefilter=TermPrefilter(span=min_frames, min_hits=3 * min_frames // 4) if prefilter else None)
    matches, clusters = td.discover()
    classes = td.write(out + '_terms')[0]

    def word_at(f, lo, hi):
        t = times[td.names[f]]
        best = max((min(t[hi], tok[2]) - max(t[lo], tok[1]), tok[3]) for tok in tokens if tok[0] == td.names[f])
        return best[1] if best[0] >= 0.5 * (t[hi] - t[lo]) else -1
    pure = []
    for c in clusters:
        words = [word_at(*tok) for tok in c]
        pure.append(max(words.count(w) for w in set(words) if w != -1) / len(words) if set(words) != {-1} else 0.0)
    print('term discovery (%s, theta %.3g): %d matches, %d clusters, %d tokens; mean share of a cluster\'s tokens on its '
          'commonest planted word %.2f; %d of %d kernel pairs aligned'
          % (distance, theta, len(matches), len(clusters), sum(len(c) for c in clusters), float(np.mean(pure)) if pure else 0.0,
             td.n_aligned_pairs, td.n_kernel_pairs))
    if alignment is not None:
        print(summary(TermEvaluator(alignment).evaluate(clusters, td.names, td.corpus.times)))
        if word_alignment is not None:
            print(full_summary(td.term_scores(TermEvaluator(alignment), words=word_alignment)))
    if len(clusters) < 2:
        sys.exit('term discovery found %d cluster(s): nothing to sample pairs from (try another --terms-theta)' % len(clusters))
    spkid = out + '_terms/wav2spk.lst'
    with open(spkid, 'w') as fh:
        fh.write(''.join('%s spk\n' % k for k in td.names))
    pairs_dir = out + '_terms_pairs'
    SamplerClusterSiamese(std_file=classes, spkid_file=spkid, directory_output=pairs_dir, num_total_sampled_pairs=400,
                          ratio_same_diff_spk=1.0, max_size_cluster=20).sample()
    dl = OriginalDataLoader(pairs_path=pairs_dir, features_path=None, batch_size=8, num_max_minibatches=200)
    dl.set_data(fb, times)
    return dl


def gmm_route(fb, times, tokens, n_components, qbe, want_post=False, hmm_stay=None, hmm_fit=0, hmm_decode=False, hmm_min_duration=1, hmm_trans=0,
              hmm_trans_viterbi=False, hmm_max_duration=None):
    """features -> GmmPosteriorgram.fit -> transform -> ABX (kl), and the search: the line main() prints.  hmm_stay (a
    number, or 'fit'): the sticky-HMM smoothed posteriorgrams beside the raw ones; they are the ones returned.  hmm_fit
    (iterations): the posteriorgrams of the Baum-Welch-trained HMM beside both; then those are returned.  hmm_decode: the
    discrete units of the (trained, else smoothed) HMM's best path beside the frame-wise mixture argmax; hmm_min_duration > 1:
    and those of the best path whose units last at least that many frames.  hmm_trans (iterations): the posteriorgrams of
    the full-transition HMM, trained from the sticky matrix, beside the raw and the sticky-smoothed ones (the returned
    posteriorgrams stay the sticky route's).  hmm_trans_viterbi: as many iterations of Viterbi training
    (TransitionHmmPosteriorgram.fit_viterbi, with hmm_min_duration) from the same start, beside the Baum-Welch line;
    hmm_max_duration = L: that training with explicit unit durations (params 'mvtid', a free law up to L frames and a
    geometric tail) instead of the minimum duration, and hmm_decode then adds the best path under the learned durations."""
    names = list(fb)
    keep, items = word_items(tokens)
    corpus = DeviceCorpus({k: np.asarray(fb[k], dtype=np.float32) for k in names}, times)
    g = GmmPosteriorgram(n_components).fit(corpus)
    post = g.transform(corpus)
    r = ABXEvaluator(items, post, distance='kl').run('within')
    line = ('ABX error on GMM posteriorgrams (K = %d, %d EM iterations, log-likelihood %.3f, %d starved): kl %.2f %% '
            '(%d triplets)' % (n_components, len(g.log_likelihoods), g.log_likelihoods[-1], g.n_starved_, r.error, r.n_triplets))
    print(line)
    if (hmm_fit or hmm_trans) and hmm_stay is None:
        hmm_stay = 0.9
    if hmm_stay is not None:
        h = StickyHmmPosteriorgram(g, 0.9 if hmm_stay == 'fit' else float(hmm_stay))
        if hmm_stay == 'fit':
            h.fit_stay(corpus)
        raw_ll, post = g.score(corpus), h.transform(corpus)
        rs = ABXEvaluator(items, post, distance='kl').run('within')
        more = ('ABX error on sticky-HMM smoothed posteriorgrams (stay %.4f%s, log-likelihood per frame %.3f against %.3f): '
                'kl %.2f %% smoothed, %.2f %% raw (%d triplets)' % (h.stay_, ', fitted' if hmm_stay == 'fit' else '', h.score(corpus),
                                                                   raw_ll, rs.error, r.error, rs.n_triplets))
        print(more)
        line += '\n' + more
        dense = timed = None
        if hmm_trans:
            w = np.maximum(g.weights_, 1e-8)                         # (a starved component: the dense model has no retired units)
            init, trans = sticky_transitions(w / w.sum(), h.stay_)
            d = TransitionHmmPosteriorgram(g, trans, init).fit(corpus, n_iter=int(hmm_trans), tol=-np.inf)
            rd = ABXEvaluator(items, d.transform(corpus), distance='kl').run('within')
            more = ('ABX error on full-transition HMM posteriorgrams (%d iterations, alpha %g untuned, log-likelihood per frame %.3f -> '
                    '%.3f, mean self-transition %.4f, %d starved): kl %.2f %% transition-smoothed, %.2f %% sticky-smoothed, %.2f %% raw '
                    '(%d triplets)' % (len(d.log_likelihoods), d.alpha, d.log_likelihoods[0], d.score(corpus),
                                       float(np.diag(d.trans_).mean()), d.n_starved_, rd.error, rs.error, r.error, rd.n_triplets))
            print(more)
            line += '\n' + more
            dense = d
            if hmm_trans_viterbi and hmm_max_duration:
                timed = TransitionHmmPosteriorgram(g, trans, init).fit_viterbi(corpus, n_iter=int(hmm_trans), tol=-np.inf, params='mvtid',
                                                                               max_duration=int(hmm_max_duration))
                timed.decode(corpus, durations=True)
                more = ('full-transition HMM Viterbi training with explicit durations (%d iterations, L = %d and alpha %g untuned): '
                        'best-path score per frame %.3f -> %.3f, %d ids changed in the last iteration, %d switches, modes of the '
                        'units\' duration laws %s' % (len(timed.viterbi_log_probs), timed.dur_.shape[1], timed.alpha, timed.viterbi_log_probs[0],
                                                      float(timed.last_log_prob_.sum()) / max(int(timed.last_n_good_.sum()), 1),
                                                      timed.last_n_changed_, int(timed.last_n_switch_.sum()),
                                                      (np.argmax(timed.dur_, axis=1) + 1).tolist()))
                print(more)
                line += '\n' + more
            elif hmm_trans_viterbi:
                hv = TransitionHmmPosteriorgram(g, trans, init).fit_viterbi(corpus, n_iter=int(hmm_trans), tol=-np.inf,
                                                                            min_duration=hmm_min_duration)
                hv.decode(corpus, min_duration=hmm_min_duration)
                more = ('full-transition HMM Viterbi training (%d iterations, at least %d frames per unit, alpha %g untuned): best-path '
                        'log-probability per frame %.3f -> %.3f, %d ids changed in the last iteration, %d switches, mean self-transition '
                        '%.4f, %d starved' % (len(hv.viterbi_log_probs), hmm_min_duration, hv.alpha, hv.viterbi_log_probs[0],
                                              float(hv.last_log_prob_.sum()) / max(int(hv.last_n_good_.sum()), 1), hv.last_n_changed_,
                                              int(hv.last_n_switch_.sum()), float(np.diag(hv.trans_).mean()), hv.n_starved_))
                print(more)
                line += '\n' + more
        if hmm_fit:
            t = StickyHmmPosteriorgram(g, h.stay_).fit(corpus, n_iter=int(hmm_fit), tol=-np.inf)
            post = t.transform(corpus)
            rt = ABXEvaluator(items, post, distance='kl').run('within')
            more = ('ABX error on Baum-Welch-trained posteriorgrams (%d iterations, stay %.4f, log-likelihood per frame %.3f -> %.3f, '
                    '%d starved, %d retired): kl %.2f %% trained, %.2f %% smoothed, %.2f %% raw (%d triplets)'
                    % (len(t.log_likelihoods), t.stay_, t.log_likelihoods[0], t.score(corpus), t.n_starved_, t.n_retired_, rt.error,
                       rs.error, r.error, rt.n_triplets))
            print(more)
            line += '\n' + more
            h = t
        if hmm_decode:
            more = hmm_decode_lines(h, corpus, items, hmm_min_duration, dense, timed)
            print(more)
            line += '\n' + more
    if qbe:
        qbe_search(post, keep, names, 'GMM posteriorgrams' + (' (Baum-Welch-trained)' if hmm_fit else ' (smoothed)' if hmm_stay is not None else ''), 'kl')
    return (line, post) if want_post else line


def hmm_decode_lines(h, corpus, items, min_duration=1, dense=None, timed=None):
    """The units of the HMM's best path (StickyHmmPosteriorgram.decode) beside the frame-wise mixture argmax (stay = 0
    through the same call): bitrate with runs merged, switches, and ABX over the quantised frames.  min_duration > 1 adds
    the best path whose units last at least that many frames; dense (a trained TransitionHmmPosteriorgram) the best path
    under the full transition matrix (TransitionHmmPosteriorgram.decode), and with min_duration > 1 that model's best path
    whose units last at least that many frames as well; timed (a TransitionHmmPosteriorgram that has durations) the best
    path under its explicit unit durations (decode(durations=True))."""
    seconds = 0.01 * corpus.total
    out = []
    routes = [('sticky-HMM Viterbi units (stay %.4f)' % h.stay_, h, 1),
              ('frame-wise mixture argmax (stay 0)', StickyHmmPosteriorgram(h.gmm, 0.0), 1)]
    if min_duration > 1:
        routes.insert(1, ('sticky-HMM Viterbi units (stay %.4f, at least %d frames per unit)' % (h.stay_, min_duration), h, min_duration))
    if dense is not None:
        if min_duration > 1:
            routes.insert(1, ('full-transition HMM Viterbi units, at least %d frames per unit' % min_duration, dense, min_duration))
        routes.insert(1, ('full-transition HMM Viterbi units (mean self-transition %.4f)' % float(np.diag(dense.trans_).mean()), dense, None))
    if timed is not None and timed.dur_ is not None:
        routes.insert(1, ('full-transition HMM Viterbi units under explicit durations (L = %d)' % timed.dur_.shape[1], timed, 'durations'))
    for label, model, S in routes:
        kw = {} if S is None else {'durations': True} if S == 'durations' else {'min_duration': S}
        ids = model.decode(corpus, **kw)
        r = ABXEvaluator(items, model.quantize(corpus, **kw), parallel='zero').run('within')
        out.append('%s: %.0f bit/s with runs merged, %d switches, log-probability per frame %.3f; ABX error quantised %.2f %% '
                   '(%d triplets)' % (label, bitrate(unit_sequences(ids), seconds), int(model.last_n_switch_.sum()),
                                      float(model.last_log_prob_.sum()) / max(1, int(model.last_n_good_.sum())), r.error, r.n_triplets))
    out.append('(nothing here is tuned on real speech: neither the stay probability nor the number of components)')
    return '\n'.join(out)


def eskmeans_route(corpus, unit_ids, n_clusters, tokens=None, tolerance=0.03, alignment=None, word_alignment=None):
    """penalised unit ids -> landmarks -> ESKMeans.fit: segments, clusters, and how many edges of the planted words
    (`tokens`: (file, onset, offset, word) in seconds) lie within `tolerance` seconds of a chosen cut."""
    from abnet3_amd import eskmeans
    from abnet3_amd.kmeans import segments
    lms = eskmeans.landmarks_from_units(segments(unit_ids), {k: corpus.length[k] for k in corpus.names})
    esk = eskmeans.ESKMeans(n_clusters, frames=10, max_span=6, max_frames=100).fit(corpus, lms)
    line = ('ES-KMeans over %d landmarks (K = %d, %d iterations): %d segments in %d clusters, objective %.2f'
            % (sum(len(v) for v in lms.values()), n_clusters, len(esk.objective_), esk.n_segments_[-1], len(esk.clusters), esk.objective_[-1]))
    if tokens:
        cuts = esk.boundaries()
        edges = [(t[0].decode('UTF-8') if isinstance(t[0], bytes) else str(t[0]), e) for t in tokens for e in (t[1], t[2])]
        hit = sum(bool(len(cuts.get(f, ())) and np.abs(cuts[f] - e).min() <= tolerance) for f, e in edges)
        line += '; %d of %d planted word edges within %.0f ms of a cut' % (hit, len(edges), 1000 * tolerance)
    print(line)
    if alignment is not None and word_alignment is not None:
        print(full_summary(esk.term_scores(TermEvaluator(alignment), words=word_alignment)))
    return esk


def kmeans_route(corpus, items, label, n_clusters, penalty=None, esk_clusters=None, tokens=None, min_duration=1, alignment=None,
                 word_alignment=None, parallel='drop'):
    """frames -> KMeansQuantizer.fit -> unit ids (bitrate) and quantised frames (ABX) beside the continuous ones; with a
    penalty the same for the penalised segmentation (min_duration: its units last at least that many frames), and with
    esk_clusters ES-KMeans over its landmarks."""
    q = KMeansQuantizer(n_clusters).fit(corpus)
    seconds = 0.01 * corpus.total
    rate = bitrate(unit_sequences(q.predict(corpus), collapse=False), seconds)
    merged = bitrate(unit_sequences(q.predict(corpus)), seconds)
    cont = ABXEvaluator(items, corpus, parallel=parallel).run('within')
    # (quantised frames are identical by construction: parallel='zero' reads a cosine that rounds above 1 as distance 0
    # where the reference's rule drops the pair)
    quant = 'quantised %.2f %%' % ABXEvaluator(items, q.quantize(corpus), parallel='zero').run('within').error
    print('k-means units of the %s (K = %d, %d iterations, inertia %.4f, %d empty): %.0f bit/s (%.0f with runs merged); '
          'ABX error continuous %.2f %%, %s (%d triplets)'
          % (label, n_clusters, len(q.inertias), q.inertias[-1], q.n_empty_, rate, merged, cont.error, quant, cont.n_triplets))
    if penalty is not None:
        ids = q.segment(corpus, penalty, min_duration=min_duration)
        pen_abx = ABXEvaluator(items, q.quantize(corpus, penalty=penalty, min_duration=min_duration), parallel='zero').run('within').error
        print('  with penalty %g%s: %.0f bit/s with runs merged (%.0f without the penalty), %d switches (%d without); '
              'ABX error quantised %.2f %% (%s without)'
              % (penalty, ' and at least %d frames per unit' % min_duration if min_duration > 1 else '',
                 bitrate(unit_sequences(ids), seconds), merged, int(q.last_n_switch_.sum()),
                 sum(len(v) - 1 for v in unit_sequences(q.predict(corpus)).values() if len(v)), pen_abx, quant[len('quantised '):]))
        if esk_clusters:
            eskmeans_route(corpus, ids, esk_clusters, tokens, alignment=alignment, word_alignment=word_alignment)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=40)
    ap.add_argument('--words', type=int, default=12)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--min-similarity', type=float, default=0.8)
    ap.add_argument('--out', default='/tmp/abnet3_zr')
    ap.add_argument('--softmax', action='store_true', help='softmax output + KLLoss; ABX under cosine and KL')
    ap.add_argument('--tcl', action='store_true', help='no mined pairs: train on temporal-coherence pairs')
    ap.add_argument('--infonce', action='store_true', help='train with InfoNCELoss (in-batch negatives) instead of coscos2')
    ap.add_argument('--temperature', type=float, default=0.1, help='with --infonce: the temperature (untuned)')
    ap.add_argument('--cae', action='store_true', help='train a correspondence autoencoder on the pairs instead of the Siamese network; embed its bottleneck')
    ap.add_argument('--cae-pretrain', type=int, default=0, metavar='N', help='with --cae: N autoencoder passes first (every frame reconstructs itself)')
    ap.add_argument('--cae-init-abnet', action='store_true', help='with --cae: then train the Siamese network from the cAE\'s encoder and embed that')
    ap.add_argument('--qbe', action='store_true', help='after embedding: search a few planted words by example, print MAP')
    ap.add_argument('--gmm', action='store_true', help='the untrained baseline: GMM posteriorgrams of the filterbanks, ABX (kl)')
    ap.add_argument('--gmm-components', type=int, default=64)
    ap.add_argument('--hmm-stay', default=None, metavar='P|fit',
                    help='with --gmm: sticky-HMM smoothing of the posteriorgrams (abnet3_amd/hmm.py) with stay probability P, or '
                         'fitted by EM; ABX (kl) of raw and smoothed side by side')
    ap.add_argument('--hmm-fit', type=int, default=0, metavar='N',
                    help='with --gmm: N iterations of Baum-Welch on the sticky HMM (from --hmm-stay, default 0.9); ABX (kl) of raw, '
                         'smoothed and trained posteriorgrams')
    ap.add_argument('--hmm-trans', type=int, default=0, metavar='N',
                    help='with --gmm: N iterations of Baum-Welch on the full-transition HMM (K x K matrix, K <= 128) from the sticky '
                         'matrix of --hmm-stay (default 0.9); ABX (kl) of raw, sticky-smoothed and transition-smoothed posteriorgrams')
    ap.add_argument('--hmm-trans-viterbi', action='store_true',
                    help='with --hmm-trans N: also N iterations of Viterbi training (hard EM on the decoded path) from the same start, '
                         'with the minimum duration of --hmm-min-duration; nothing is tuned on real speech')
    ap.add_argument('--hmm-max-duration', type=int, default=None, metavar='L',
                    help='with --hmm-trans-viterbi: train explicit unit durations (a free law up to L frames, 2 .. 32, and a geometric '
                         'tail) instead of the minimum duration; --hmm-decode then decodes under them; L is untuned')
    ap.add_argument('--hmm-decode', action='store_true',
                    help='with --hmm-stay / --hmm-fit: the discrete units of the HMM\'s best path (Viterbi): bitrate, switches and ABX '
                         'of the quantised frames, beside the frame-wise mixture argmax; nothing is tuned on real speech')
    ap.add_argument('--no-network', action='store_true', help='with --gmm: stop after the mixture, train nothing')
    ap.add_argument('--terms', action='store_true', help='pairs from term discovery: clusters -> SamplerClusterSiamese')
    ap.add_argument('--terms-theta', type=float, default=None, help='default: a low quantile of random frame distances (untuned)')
    ap.add_argument('--prefilter', action='store_true', help='with --terms: align only the kernel pairs the LSH dot-plot prefilter keeps (untuned)')
    ap.add_argument('--alignment', default=None, metavar='FILE', help='with --terms: a phone alignment; NED and coverage of the clusters')
    ap.add_argument('--word-alignment', default=None, metavar='FILE',
                    help='with --alignment and --terms or --eskmeans: a word alignment in the same format; the full term scores of the clusters '
                         '(token, type, boundary, grouping, NED: abnet3_amd/tde.py)')
    ap.add_argument('--kmeans', action='store_true', help='discrete units: k-means of the embeddings (--no-network: of the filterbanks), bitrate and ABX')
    ap.add_argument('--kmeans-clusters', type=int, default=50)
    ap.add_argument('--kmeans-penalty', type=float, default=None, metavar='P',
                    help='with --kmeans: also the penalised segmentation, P per new segment in units of the distortion (untuned)')
    ap.add_argument('--kmeans-min-duration', type=int, default=1, metavar='S',
                    help='with --kmeans-penalty: every unit lasts at least S frames (1 .. 8, untuned)')
    ap.add_argument('--hmm-min-duration', type=int, default=1, metavar='S',
                    help='with --hmm-decode: also the best path whose units last at least S frames (1 .. 8, untuned)')
    ap.add_argument('--eskmeans', action='store_true', help='with --kmeans --kmeans-penalty P: ES-KMeans word segmentation over the units\' boundaries (untuned)')
    ap.add_argument('--eskmeans-clusters', type=int, default=24)
    ap.add_argument('--samediff', action='store_true', help='same-different AP of the planted words: DTW over filterbanks and embeddings, the embeddings\' segment vectors')
    args = ap.parse_args()
    if args.word_alignment is not None and (args.alignment is None or not (args.terms or args.eskmeans)):
        ap.error('--word-alignment scores the clusters of --terms or --eskmeans against --alignment')
    if args.eskmeans and not (args.kmeans and args.kmeans_penalty is not None):
        ap.error('--eskmeans takes its landmarks from --kmeans --kmeans-penalty P')
    if args.hmm_stay is not None and not args.gmm:
        ap.error('--hmm-stay smooths the posteriorgrams of --gmm')
    if args.hmm_fit and not args.gmm:
        ap.error('--hmm-fit trains the HMM over the mixture of --gmm')
    if args.hmm_trans and (not args.gmm or args.gmm_components > 128):
        ap.error('--hmm-trans trains the full-transition HMM over the mixture of --gmm, with --gmm-components <= 128')
    if args.hmm_trans_viterbi and not args.hmm_trans:
        ap.error('--hmm-trans-viterbi trains the model of --hmm-trans N')
    if args.hmm_max_duration is not None and not args.hmm_trans_viterbi:
        ap.error('--hmm-max-duration belongs to --hmm-trans-viterbi')
    if args.hmm_decode and args.hmm_stay is None and not args.hmm_fit:
        ap.error('--hmm-decode decodes the HMM of --hmm-stay or --hmm-fit')
    if args.infonce and args.softmax:
        ap.error('--infonce is a loss over cosine similarities; --softmax trains posteriorgrams with KLLoss')
    if (args.cae_pretrain or args.cae_init_abnet) and not args.cae:
        ap.error('--cae-pretrain and --cae-init-abnet belong to --cae')
    if args.cae and args.softmax:
        ap.error('--cae reconstructs filterbanks; --softmax trains posteriorgrams with KLLoss')
    if args.cae and args.infonce and not args.cae_init_abnet:
        ap.error('--infonce is the Siamese network\'s loss: with --cae it needs --cae-init-abnet')
    esk_k = args.eskmeans_clusters if args.eskmeans else None
    rng = np.random.default_rng(0)
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)

    wavs, tokens = synth_corpus(args.utts, args.words, rng)
    fg = FeaturesGenerator(norm_per_channel=True)
    fb, _ = fg.normalize_features({k: fg.fbank_from_samples(v, 16000).cpu().numpy() for k, v in wavs.items()})
    times = {k: np.arange(len(v)) * 0.01 + 0.0125 for k, v in fb.items()}

    gmm_line = post = None
    if args.gmm:
        gmm_line, post = gmm_route(fb, times, tokens, args.gmm_components, args.qbe, want_post=True, hmm_stay=args.hmm_stay, hmm_fit=args.hmm_fit, hmm_decode=args.hmm_decode,
                                   hmm_min_duration=args.hmm_min_duration, hmm_trans=args.hmm_trans,
                                   hmm_trans_viterbi=args.hmm_trans_viterbi, hmm_max_duration=args.hmm_max_duration)
    if args.no_network:
        if not (args.gmm or args.kmeans):
            ap.error('--no-network leaves nothing to do without --gmm or --kmeans')
        if args.kmeans:
            corpus = DeviceCorpus({k: np.asarray(v, dtype=np.float32) for k, v in fb.items()}, times)
            kmeans_route(corpus, word_items(tokens)[1], 'filterbanks', args.kmeans_clusters, args.kmeans_penalty, esk_k, tokens,
                         args.kmeans_min_duration, args.alignment, args.word_alignment)
        return

    if args.tcl:
        dl = tcl_loader(fb, times, rng)
    elif args.terms:
        if post is not None:
            dl = terms_loader(post, fb, times, tokens, args.out, 'kl', args.terms_theta, rng, alignment=args.alignment, prefilter=args.prefilter,
                              word_alignment=args.word_alignment)
        else:
            corpus = DeviceCorpus({k: np.asarray(v, dtype=np.float32) for k, v in fb.items()}, times)
            dl = terms_loader(corpus, fb, times, tokens, args.out, 'cosine', args.terms_theta, rng, alignment=args.alignment, prefilter=args.prefilter,
                              word_alignment=args.word_alignment)
    else:
        miner = KnnPairMiner(fb, times, min_similarity=args.min_similarity)
        pairs_path, map_path = miner.write(args.out + '_mined')
        a, b, sim = miner.pairs

        def word_at(seg):
            name = miner.names[miner.seg_file[seg]]
            lo, hi = miner.seg_begin[seg] * 0.01, (miner.seg_begin[seg] + miner.seg_len[seg]) * 0.01
            best = max((min(hi, t[2]) - max(lo, t[1]), t[3]) for t in tokens if t[0] == name)
            return best[1] if best[0] >= 0.5 * (hi - lo) else -1
        hits = [word_at(x) == word_at(y) != -1 for x, y in zip(a[:500], b[:500])]
        print('%d segments, %d mined pairs; %.1f %% of the top %d join two tokens of one word'
              % (miner.table.shape[0], len(a), 100 * np.mean(hits) if hits else 0.0, len(hits)))

        dl = PairsDataLoader(pairs_path, None, map_path, batch_size=8, train_iterations=200, test_iterations=50,
                             split_method='files')
        dl.set_data(fb, times)
    shape = dict(input_dim=40, num_hidden_layers=1, hidden_dim=200, output_dim=40, p_dropout=0.0, activation_layer='sigmoid')
    cae = None
    if args.cae:
        cae = CorrespondenceAutoencoder(output_path=args.out + '_cae', **shape)
        cae_trainer = TrainerCorrespondence(network=cae, loss=CorrespondenceLoss(avg=True), num_epochs=args.epochs, patience=30,
                                            optimizer_type='adadelta', lr=0.5, dataloader=dl, log_dir=args.out + '_runs')
        if args.cae_pretrain:
            print('cAE pretraining losses per pass:', ['%.4f' % v for v in cae_trainer.pretrain(args.cae_pretrain)])
        cae_trainer.train()
        print('cAE dev losses per epoch:', ['%.4f' % v for v in cae_trainer.dev_losses])
    net = SiameseNetwork(output_path=args.out + '_network', last_non_linearity='softmax' if args.softmax else 'default', **shape)
    if args.cae_init_abnet:
        cae.save_encoder(args.out + '_cae_encoder.pth')
        net.load_network(args.out + '_cae_encoder.pth')
    if cae is not None and not args.cae_init_abnet:
        net = cae                                        # (EmbedderSiamese reads output_dim and forward_once: the bottleneck)
    trainer = None if net is cae else TrainerSiamese(network=net, loss=KLLoss(avg=False) if args.softmax else InfoNCELoss(args.temperature, avg=False) if args.infonce else coscos2(avg=False),
                             num_epochs=args.epochs, patience=30,
                             optimizer_type='adadelta', lr=0.5, dataloader=dl, log_dir=args.out + '_runs')
    if trainer is not None:
        trainer.train()
        print('dev losses per epoch:', ['%.2f' % v for v in trainer.dev_losses])

    names = list(fb)
    emb = EmbedderSiamese(network=net, network_path=net.output_path + '.pth', feature_path=None,
                          output_path=None).embed_features([fb[k] for k in names])
    keep, items = word_items(tokens)
    for label, feats in (('filterbanks', fb), ('embeddings', dict(zip(names, emb)))):
        corpus = DeviceCorpus({k: np.asarray(feats[k], dtype=np.float32) for k in names}, times)
        if args.samediff:
            samediff_lines(corpus, keep, label, vectors=label == 'embeddings')
        # (--cae: exactly parallel frames are at distance 0 instead of dropping the pair: the docstring says why)
        parallel = 'zero' if args.cae and label == 'embeddings' else 'drop'
        r = ABXEvaluator(items, corpus, parallel=parallel).run('within')
        if args.softmax and label == 'embeddings':
            kl = ABXEvaluator(items, corpus, distance='kl').run('within')
            print('ABX error on %s: cosine %.2f %%, kl %.2f %% (%d triplets)' % (label, r.error, kl.error, r.n_triplets))
        else:
            print('ABX error on %s: %.2f %% (%d triplets)' % (label, r.error, r.n_triplets))
        if args.qbe:
            qbe_search(corpus, keep, names, label, 'kl' if args.softmax and label == 'embeddings' else 'cosine')
        if args.kmeans and label == 'embeddings':
            kmeans_route(corpus, items, label, args.kmeans_clusters, args.kmeans_penalty, esk_k, tokens, args.kmeans_min_duration,
                         args.alignment, args.word_alignment, parallel=parallel)
    if gmm_line:
        print(gmm_line)


if __name__ == '__main__':
    main()
