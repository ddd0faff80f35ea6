"""Float64 numpy restatement of the ABX definition (abnet3_amd/abx.py's module docstring) by brute force: every item
triple (A, B, X) is tested against the conditions of the mode, nothing is grouped first.  Test infrastructure only."""
from collections import defaultdict

import numpy as np


def triplets(phones, contexts, speakers, mode):
    """[(cell key, A, B, X)] of every triplet of `mode`, by brute force over all item triples."""
    n = len(phones)
    out = []
    for a in range(n):
        for b in range(n):
            for x in range(n):
                if not (contexts[a] == contexts[b] == contexts[x]):
                    continue
                if phones[a] != phones[x] or phones[b] == phones[a]:
                    continue
                if mode == 'within':
                    if a == x or not (speakers[a] == speakers[b] == speakers[x]):
                        continue
                    sk = speakers[a]
                else:
                    if speakers[a] != speakers[b] or speakers[x] == speakers[a]:
                        continue
                    sk = (speakers[a], speakers[x])
                out.append(((phones[a], phones[b], contexts[a], sk), a, b, x))
    return out


def needed_pairs(trips):
    """The ordered pairs (P, Q) whose distance the triplets read: (A, X) and (B, X)."""
    return {(a, x) for _, a, _, x in trips} | {(b, x) for _, _, b, x in trips}


def cell_scores(trips, d):
    """{cell key: (2 x score sum, count)} with d a {(P, Q): float64 distance} mapping."""
    out = defaultdict(lambda: [0, 0])
    for key, a, b, x in trips:
        dax, dbx = d[(a, x)], d[(b, x)]
        out[key][0] += 2 if dax < dbx else (1 if dax == dbx else 0)
        out[key][1] += 1
    return {k: tuple(v) for k, v in out.items()}


def error(cells):
    """100 (1 - S): cell means, then unweighted means over contexts, speaker keys, phone pairs (float64)."""
    by_spk = defaultdict(list)
    for (p, q, _c, sk), (s2, n) in cells.items():
        by_spk[(p, q, sk)].append(np.float64(s2) / (2.0 * n))
    by_pair = defaultdict(list)
    for (p, q, _sk), v in by_spk.items():
        by_pair[(p, q)].append(np.mean(v))
    return 100.0 * (1.0 - np.mean([np.mean(v) for v in by_pair.values()]))


def dtw_distance(a, b):
    """d(P, Q) = total cost / path length of the C oracle's DTW (float64)."""
    from oracle import dtw_oracle as O
    dm = O.cosine_distance(a, b)
    return O.dtw_cost(dm) / len(O.dtw_path(dm)[0])
