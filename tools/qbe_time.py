"""Times query-by-example search (abnet3_amd/qbe.py) on a synthetic corpus of the C5 pipeline's shape with no audio:
utterances of 2-10 s (200-1000 frames of 10 ms), D = 100, and about 100 queries of 0.3-1.0 s (30-100 frames) cut out
of them, every query against every utterance.

  abn_dtw_search_batched   the subsequence-DTW kernel alone on the whole pair table (device events), with and without
                           the per-frame profile
  abn_dtw_cost_batched     the cost-only kernel of the ABX evaluation on a pair table of the SAME (N, M) shapes and the
                           same rows (token 1 = the utterance, token 2 = the query), in the same process; the ratio of
                           the two cells/s figures is the figure of record
  QbeSearcher.search       end to end (host pair enumeration, upload, kernel, download, times), wall time

--distance kl: the same over a row softmax of the features (abn_dtw_search_kl_batched against abn_dtw_cost_kl_batched).

--parent-lib FILE: the same three routes (search, search with profile, cost on the same shapes) of another build of the
library (the parent commit's), timed alternately with this build's, outputs compared bit for bit (tools/abx_time.py:
versus_parent).

Every GPU route settles the clock (untimed calls for 0.3 s) before its timed calls; medians are reported.
python tools/qbe_time.py [--utts N] [--queries N] [--distance cosine|kl] [--parent-lib FILE] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from abnet3_amd import _lib
from abnet3_amd.qbe import QbeSearcher
from tools.abx_time import median_ms, parent_library, settle, versus_parent, wall  # noqa: F401


def synthetic(n_utts, n_queries, D=100, seed=0):
    """(feats, times, queries): smooth random trajectories (a random walk, renormalised) so that neighbouring frames
    resemble each other as speech frames do; query k is a stretch of utterance k % n_utts."""
    rng = np.random.default_rng(seed)
    feats, times = {}, {}
    for u in range(n_utts):
        n = int(rng.integers(200, 1001))
        f = np.cumsum(0.35 * rng.standard_normal((n, D)), axis=0) + rng.standard_normal((n, D))
        f -= f.mean(axis=0, keepdims=True)
        feats['utt%04d' % u] = (f / f.std()).astype(np.float32)
        times['utt%04d' % u] = (np.arange(n) + 0.5) * 0.01
    queries = []
    for k in range(n_queries):
        name = 'utt%04d' % (k % n_utts)
        m = int(rng.integers(30, 101))
        lo = int(rng.integers(0, len(feats[name]) - m))
        queries.append((name, lo * 0.01, (lo + m) * 0.01))            # frames lo .. lo + m - 1
    return feats, times, queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=200)
    ap.add_argument('--queries', type=int, default=100)
    ap.add_argument('--distance', choices=('cosine', 'kl'), default='cosine')
    ap.add_argument('--calls', type=int, default=9)
    ap.add_argument('--parent-lib', default=None, help="another build of the library (the parent commit's) to time beside this one")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    kl = a.distance == 'kl'
    feats, times, queries = synthetic(a.utts, a.queries)
    if kl:
        feats = {k: torch.softmax(torch.from_numpy(v), dim=1).numpy() for k, v in feats.items()}
    s = QbeSearcher(feats, times, distance=a.distance)
    c = s.corpus
    tok = np.array([c.token(*q) for q in queries], dtype=np.int64)
    U, Q = len(c.names), len(queries)
    qi, ui = np.divmod(np.arange(Q * U), U)
    u_off = np.array([c.offset[k] for k in c.names], dtype=np.int64)[ui]
    u_n = np.array([c.length[k] for k in c.names], dtype=np.int32)[ui]
    q_off, q_n = tok[qi, 0], tok[qi, 1].astype(np.int32)
    npairs, rows, D = Q * U, c.table.shape[0], c.table.shape[1]
    cells = int(np.dot(u_n.astype(np.int64), q_n.astype(np.int64)))
    lib = _lib.load()
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    tab = [dev(u_off, np.int64), dev(u_n, np.int32), dev(q_off, np.int64), dev(q_n, np.int32)]
    poff = np.concatenate(([0], np.cumsum(u_n.astype(np.int64))))
    d_poff, prows = dev(poff[:-1], np.int64), int(poff[-1])
    cost = torch.empty(npairs, dtype=torch.float64, device='cuda')
    plen, start, end = (torch.empty(npairs, dtype=torch.int32, device='cuda') for _ in range(3))
    pc = torch.empty(prows, dtype=torch.float64, device='cuda')
    pl, ps = (torch.empty(prows, dtype=torch.int32, device='cuda') for _ in range(2))
    ccost, cplen = torch.empty_like(cost), torch.empty_like(plen)
    table, t = c.table, s.tables
    ptr = _lib.ptr

    mine = (cost, plen, start, end, pc, pl, ps, ccost, cplen)

    def search(profile, l=lib, o=mine):
        out = [ptr(x) for x in o[:4]]
        out += [ptr(d_poff), prows] + [ptr(x) for x in o[4:7]] if profile else [None, 0, None, None, None]
        if kl:
            _lib.check(l.abn_dtw_search_kl_batched(ptr(t.P), ptr(t.L), rows, ptr(t.P), ptr(t.L), rows, *[ptr(x) for x in tab],
                                                   npairs, D, ptr(t.bad), ptr(t.bad), *out, _lib.stream()),
                       'abn_dtw_search_kl_batched')
        else:
            _lib.check(l.abn_dtw_search_batched(ptr(table), rows, ptr(table), rows, *[ptr(x) for x in tab], npairs, D, *out,
                                                _lib.stream()), 'abn_dtw_search_batched')

    def cost_only(l=lib, o=mine):
        if kl:
            _lib.check(l.abn_dtw_cost_kl_batched(ptr(t.P), ptr(t.L), rows, ptr(t.P), ptr(t.L), rows, *[ptr(x) for x in tab],
                                                 npairs, D, ptr(t.bad), ptr(t.bad), ptr(o[7]), ptr(o[8]), _lib.stream()),
                       'abn_dtw_cost_kl_batched')
        else:
            _lib.check(l.abn_dtw_cost_batched(ptr(table), rows, ptr(table), rows, *[ptr(x) for x in tab], npairs, D,
                                              ptr(o[7]), ptr(o[8]), _lib.stream()), 'abn_dtw_cost_batched')

    s_ms = median_ms(lambda: search(False), a.calls)
    c_ms = median_ms(cost_only, a.calls)
    p_ms = median_ms(lambda: search(True), a.calls)
    s_ms2 = median_ms(lambda: search(False), a.calls)
    c_ms2 = median_ms(cost_only, a.calls)
    torch.cuda.synchronize()
    own = np.flatnonzero(ui == qi % U)                                 # every query against the utterance it was cut from
    found = bool((start.cpu().numpy()[own] == (q_off - u_off)[own]).all() and (cost.cpu().numpy()[own] < 1e-2 * q_n[own]).all())
    res0 = s.search(queries)                                           # warm
    walls = []
    for _ in range(5):
        w, r = wall(lambda: s.search(queries))
        walls.append(w)
        assert r.score.tobytes() == res0.score.tobytes()
    name = 'abn_dtw_search_kl_batched' if kl else 'abn_dtw_search_batched'
    cname = 'abn_dtw_cost_kl_batched' if kl else 'abn_dtw_cost_batched'
    rate = lambda ms: round(cells / (ms * 1e-3), 1)
    res = {
        'device': torch.cuda.get_device_name(0), 'distance': a.distance,
        'set': '%d utterances of 200-1000 frames (%d rows), D = %d; %d queries of 30-100 frames cut from them; every query '
               'against every utterance' % (U, rows, D, Q),
        'pairs': npairs, 'cells': cells, 'mean_cells_per_pair': round(cells / npairs, 1),
        name + '_ms': round(s_ms, 4), name + '_ms_again': round(s_ms2, 4), name + '_cells_per_s': rate(s_ms),
        name + '_with_profile_ms': round(p_ms, 4), 'profile_entries': prows,
        cname + '_ms_same_shapes': round(c_ms, 4), cname + '_ms_same_shapes_again': round(c_ms2, 4),
        cname + '_cells_per_s': rate(c_ms),
        'search_over_cost_only_cells_per_s': round(c_ms / s_ms, 3),
        'every_query_finds_its_own_stretch': found,
        'searcher_end_to_end_s_median': round(float(np.median(walls)), 4),
        'protocol': 'settle 0.3 s of untimed calls, then the median of %d device-event timings per route; the routes '
                    'alternate in one process' % a.calls,
    }
    if a.parent_lib:
        parent = parent_library(a.parent_lib, lib, [name, cname])
        theirs = tuple(torch.empty_like(x) for x in mine)
        res['search_vs_parent_build'] = versus_parent(lambda: search(False), lambda: search(False, parent, theirs),
                                                      lambda: list(zip(mine[:4], theirs[:4])), a.calls)
        res['search_with_profile_vs_parent_build'] = versus_parent(lambda: search(True), lambda: search(True, parent, theirs),
                                                                   lambda: list(zip(mine[:7], theirs[:7])), a.calls)
        res['cost_same_shapes_vs_parent_build'] = versus_parent(cost_only, lambda: cost_only(parent, theirs),
                                                                lambda: list(zip(mine[7:], theirs[7:])), a.calls)
    line = json.dumps(res)
    print(line)
    if a.out:
        path = a.out
        merged = {}
        if os.path.exists(path):
            with open(path) as f:
                merged = json.load(f)
        merged[a.distance] = res
        with open(path, 'w') as f:
            json.dump(merged, f, indent=1)
            f.write('\n')
    for key, block in res.items():
        if key.endswith('_vs_parent_build'):
            assert block['outputs_bit_identical'], key


if __name__ == '__main__':
    main()
