"""Times the ES-KMeans kernels (abn_esk_score, abn_esk_segment, abnet3_amd/csrc/eskmeans.hip).

Workload: tools/units_time.py's corpus (1.14 M frames as a synthetic clustered table, D = 40, seeded utterances of
200 .. 1000 frames), landmarks at the boundaries of penalised k-means units (256 units, --penalty), frames = 10, S = 6,
max_frames = --max-frames, K in {256, 1024} centroids taken from random segments.  Timed, per K, in the same process:

  abn_esk_score        one launch over every candidate slot (device events)
  unfused route (a)    what existed before: abn_segment_vectors over all allowed candidates into a [candidates, 400]
                       table (in chunks of --chunk rows), then abn_kmeans_assign on it; ids and scores are compared with
                       the fused kernel's, bit for bit
  floor (b)            abn_kmeans_assign alone on the prebuilt table of the same rows x 400
  abn_esk_segment      one launch
  one fit iteration    ESKMeans.iteration end to end: score, DP, read-back, the chosen segments' vectors, accumulate,
                       update (host clock around a synchronised call)

Every route settles the clock before its 15 timed calls; medians, minima and maxima are reported, with the peak device
bytes of each scoring route on top of the inputs: torch's peak-allocation counter around the route's buffers AND one
call of it (none of the entries takes a workspace, so the peak is the buffers).

python tools/esk_time.py [--frames 1140000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, FRAMES, SPAN, UNITS = 40, 10, 6, 256


def corpus(T, a):
    """(table, lm host, lm_off host): the table, and landmarks from penalised units."""
    import torch
    from abnet3_amd import eskmeans, kmeans
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + UNITS)
    centres = 3.0 * torch.randn(UNITS, D, device='cuda', generator=g)
    lab = torch.randint(0, UNITS, (T // 8 + 1,), device='cuda', generator=g).repeat_interleave(8)[:T]      # 80 ms "phones"
    table = (centres[lab] + 1.5 * torch.randn(T, D, device='cuda', generator=g) + 5.0).contiguous()
    table, shift, good = kmeans.prepare(table, 'euclidean')
    st = kmeans.LloydState(kmeans.initial_centroids(table, shift, good, UNITS, 0), T, table.device)
    for _ in range(3):
        kmeans.lloyd_iteration(table, shift, st)
    off, lens = cut(T, D + UNITS)
    ids = kmeans.viterbi(table, off, lens, shift, st.m, st.b, a.penalty)[0].cpu().numpy()
    by = {u: ids[o:o + n] for u, (o, n) in enumerate(zip(off, lens))}
    lms = eskmeans.landmarks_from_units(kmeans.segments(by), {u: int(n) for u, n in enumerate(lens)})
    _, lm, lm_off = eskmeans.pack_landmarks(lms, {u: int(o) for u, o in enumerate(off)}, {u: int(n) for u, n in enumerate(lens)})
    return table, lm, lm_off


def allowed(lm, lm_off, S, max_frames):
    """(slot, row0, n) of the allowed candidates, vectorised."""
    n_lm = len(lm)
    utt_end = np.repeat(lm_off[1:], np.diff(lm_off))
    slots, row0, n = [], [], []
    for s in range(1, S + 1):
        g = np.flatnonzero(np.arange(n_lm) + s < utt_end)
        length = lm[g + s] - lm[g]
        ok = (length <= max_frames) if s > 1 else np.ones(len(g), dtype=bool)
        slots.append(g[ok] * S + s - 1), row0.append(lm[g][ok]), n.append(length[ok])
    slots, row0, n = (np.concatenate(x) for x in (slots, row0, n))
    order = np.argsort(slots)
    return slots[order], row0[order], n[order]


def workload(table, lm, lm_off, K, a):
    import torch
    from abnet3_amd import _lib, eskmeans, kmeans
    lib = _lib.load()
    T, depth = table.shape[0], FRAMES * D
    n_lm, n_utt = len(lm), len(lm_off) - 1
    slots, row0, n = allowed(lm, lm_off, SPAN, a.max_frames)
    C = len(slots)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    lm_d, off_d, row0_d, n_d = dev(lm, np.int64), dev(lm_off, np.int64), dev(row0, np.int64), dev(n, np.int32)
    rng = np.random.default_rng(K)
    pick = np.sort(rng.choice(C, K, replace=False))
    vec, _ = eskmeans.segment_vectors(table, row0[pick], n[pick].astype(np.int32), FRAMES)
    mu = vec.to(torch.float64).cpu().numpy()
    m, b = (dev(x, np.float32) for x in kmeans.score_tables(mu))
    shift = torch.zeros(depth, dtype=torch.float32, device='cuda')
    res = {'T': T, 'D': D, 'frames': FRAMES, 'K': K, 'S': SPAN, 'max_frames': a.max_frames, 'utterances': n_utt, 'landmarks': n_lm,
           'frames_per_landmark': round(T / float(n_lm), 2), 'candidate_slots': n_lm * SPAN, 'allowed_candidates': C,
           'candidate_table_bytes_never_formed': 4 * C * depth, 'candidate_array_bytes': 8 * n_lm * SPAN}
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, int(torch.cuda.max_memory_allocated() - base)

    buf = {}

    def fused():
        best, ids = buf['best'], buf['ids']
        _lib.check(lib.abn_esk_score(_lib.ptr(table), T, D, _lib.ptr(lm_d), _lib.ptr(off_d), n_utt, n_lm, FRAMES, SPAN, a.max_frames,
                                     _lib.ptr(m), _lib.ptr(b), K, _lib.ptr(best), _lib.ptr(ids), _lib.stream()), 'abn_esk_score')

    def fused_route():
        buf['best'] = torch.empty(n_lm * SPAN, dtype=torch.float32, device='cuda')
        buf['ids'] = torch.empty(n_lm * SPAN, dtype=torch.int32, device='cuda')
        fused()
    _, res['fused_peak_bytes'] = peak_of(fused_route)
    best, ids = buf['best'], buf['ids']

    chunk = min(C, a.chunk)
    res['unfused_chunks'] = (C + chunk - 1) // chunk

    def assign(c0, c1):
        tab, u_ids, u_best = buf['tab'], buf['u_ids'], buf['u_best']
        _lib.check(lib.abn_kmeans_assign(_lib.ptr(tab), c1 - c0, depth, _lib.ptr(shift), _lib.ptr(m), _lib.ptr(b), K, None,
                                         _lib.ptr(u_ids[c0:c1]), _lib.ptr(u_best[c0:c1]), None, _lib.stream()), 'abn_kmeans_assign')

    def unfused():
        tab, keep = buf['tab'], buf['keep']
        for c0 in range(0, C, chunk):
            c1 = min(C, c0 + chunk)
            _lib.check(lib.abn_segment_vectors(_lib.ptr(table), D, _lib.ptr(row0_d[c0:c1]), _lib.ptr(n_d[c0:c1]), c1 - c0, FRAMES,
                                               _lib.ptr(tab), _lib.ptr(keep), _lib.stream()), 'abn_segment_vectors')
            assign(c0, c1)

    def floor():                                  # (the table holds the last chunk's rows: the same shape of work)
        for c0 in range(0, C, chunk):
            assign(c0, min(C, c0 + chunk))

    def unfused_route():
        buf['tab'] = torch.empty(chunk, depth, dtype=torch.float32, device='cuda')
        buf['keep'] = torch.empty(chunk, dtype=torch.uint8, device='cuda')
        buf['u_ids'] = torch.empty(C, dtype=torch.int32, device='cuda')
        buf['u_best'] = torch.empty(C, dtype=torch.float32, device='cuda')
        unfused()
    _, res['unfused_peak_bytes'] = peak_of(unfused_route)
    u_ids, u_best = buf['u_ids'], buf['u_best']
    fused()
    slots_d = dev(slots, np.int64)
    res['agreement'] = {'ids_that_differ': int((ids[slots_d] != u_ids).sum()),
                        'scores_whose_bits_differ': int((best[slots_d].view(torch.int32) != u_best.view(torch.int32)).sum()),
                        'slots_outside_the_allowed_set_with_an_id': int((ids >= 0).sum() - (ids[slots_d] >= 0).sum())}
    res['abn_esk_score'] = median_ms(fused)
    res['unfused_route'] = median_ms(unfused)
    res['abn_kmeans_assign_floor'] = median_ms(floor)
    res['abn_esk_score_again'] = median_ms(fused)
    ms = res['abn_esk_score']['median_ms']
    res['speedup_over_unfused_route'] = round(res['unfused_route']['median_ms'] / ms, 3)
    res['time_over_assign_floor'] = round(ms / res['abn_kmeans_assign_floor']['median_ms'], 3)
    res['candidates_per_s'] = round(C / (ms * 1e-3), 1)

    cutv = torch.empty(n_lm, dtype=torch.uint8, device='cuda')
    word = torch.empty(n_lm, dtype=torch.int32, device='cuda')
    span = torch.empty(n_lm, dtype=torch.int32, device='cuda')
    obj = torch.empty(n_utt, dtype=torch.float64, device='cuda')
    nseg = torch.empty(n_utt, dtype=torch.int32, device='cuda')

    def seg():
        _lib.check(lib.abn_esk_segment(_lib.ptr(best), _lib.ptr(ids), _lib.ptr(lm_d), _lib.ptr(off_d), n_utt, n_lm, SPAN, _lib.ptr(cutv),
                                       _lib.ptr(word), _lib.ptr(span), _lib.ptr(obj), _lib.ptr(nseg), _lib.stream()), 'abn_esk_segment')
    fused()
    res['abn_esk_segment'] = median_ms(seg)
    res['segments_chosen'] = int(nseg.clamp(min=0).sum())
    res['unreachable_utterances'] = int((nseg < 0).sum())
    del u_ids, u_best
    for k in ('tab', 'keep', 'u_ids', 'u_best'):
        del buf[k]
    torch.cuda.empty_cache()

    q = eskmeans.ESKMeans(K, FRAMES, SPAN, a.max_frames)
    st = kmeans.LloydState(mu, 0, table.device)
    ts = []
    for i in range(3 + a.fit_calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q.iteration(table, lm, lm_d, off_d, st, shift)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[3:]
    res['fit_iteration_end_to_end'] = {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(min(ts), 3), 'max_ms': round(max(ts), 3),
                                       'calls': a.fit_calls, 'clock': 'host, synchronised'}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--penalty', type=float, default=20.0, help='the unit segmentation\'s penalty (units of the distortion)')
    ap.add_argument('--max-frames', type=int, default=100)
    ap.add_argument('--chunk', type=int, default=1 << 21, help='rows of the unfused route\'s candidate table')
    ap.add_argument('--fit-calls', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'esk_time.json'))
    a = ap.parse_args()
    import torch
    table, lm, lm_off = corpus(a.frames, a)
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15,
           'workloads': [workload(table, lm, lm_off, 256, a), workload(table, lm, lm_off, 1024, a)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
