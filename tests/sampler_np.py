"""numpy / Python-integer restatement of abn_sample_pairs (abnet3_amd/csrc/sampler.hip) and of the tables it reads
(abnet3_amd/sampler.py, build_tables): the generator, the table layout, the searches and the token picks, written
a second time so that the kernel can be compared bit for bit -- and the distribution the tables realise, computed
exactly in Python integers.  Not a test module.
"""
import math
from fractions import Fraction

import numpy as np

CONFIGS = ('Stype_Sspk', 'Stype_Dspk', 'Dtype_Sspk', 'Dtype_Dspk')
U64 = np.uint64
MASK32 = U64(0xFFFFFFFF)
S32 = U64(32)


def mode_function(mode):
    mode = str(mode)
    return {'1': lambda x: 1.0 if x else 0.0, 'f2': lambda x: float(x), 'f': lambda x: float(np.sqrt(np.float64(x))),
            'fcube': lambda x: float(np.cbrt(np.float64(x))), 'log': lambda x: float(np.log(1 + np.float64(x)))}[mode]


def build_tables(descr, type_mode, spk_mode):
    """The tables from a description, cell by cell in plain Python (abn_sampler_tables' layout)."""
    g, f = mode_function(type_mode), mode_function(spk_mode)
    speakers = sorted(set(str(s) for s in descr['tokens_speaker']))
    rank = {s: i for i, s in enumerate(speakers)}
    by_cell = {}
    for tok, (t, s) in enumerate(zip(descr['tokens_type'], descr['tokens_speaker'])):
        by_cell.setdefault((int(t), rank[str(s)]), []).append(tok)
    t_order = sorted(by_cell)                                   # (type, speaker)
    K, n_type, n_spk = len(t_order), len(descr['types']), len(speakers)
    type_tokens = [0] * n_type
    for (t, s), toks in by_cell.items():
        type_tokens[t] += len(toks)
    u_w = [g(type_tokens[t]) * f(len(by_cell[(t, s)])) for t, s in t_order]
    f_w = [f(len(by_cell[(t, s)])) for t, s in t_order]
    f_type = [math.fsum(w for w, (t, s) in zip(f_w, t_order) if t == ty) for ty in range(n_type)]
    su = float(2 ** 32 - 2 * K - 2) / math.fsum(u_w)
    sf = float(2 ** 32 - 2 * K - 2) / max(f_type)
    u_t = [max(1, int(np.rint(su * w))) for w in u_w]
    f_t = [max(1, int(np.rint(sf * w))) for w in f_w]
    s_order = sorted(range(K), key=lambda c: (t_order[c][1], t_order[c][0]))       # T indices by (speaker, type)

    def running(v):
        out, acc = [], 0
        for x in v:
            acc += x
            out.append(acc)
        return out
    u_s = [u_t[c] for c in s_order]
    U_spk = [sum(u_t[c] for c in range(K) if t_order[c][1] == s) for s in range(n_spk)]
    U_type = [sum(u_t[c] for c in range(K) if t_order[c][0] == t) for t in range(n_type)]
    F_type = [sum(f_t[c] for c in range(K) if t_order[c][0] == t) for t in range(n_type)]
    U = sum(u_t)
    assert U < 2 ** 32 and max(F_type) < 2 ** 32
    m = [[u_t[c] * (len(by_cell[t_order[c]]) >= 2) for c in range(K)],
         [u_t[c] * (F_type[t_order[c][0]] - f_t[c]) for c in range(K)],
         [u_t[c] * (U_spk[t_order[c][1]] - u_t[c]) for c in s_order],
         [u_t[c] * (U - U_spk[t_order[c][1]] - U_type[t_order[c][0]] + u_t[c]) for c in s_order]]
    assert all(sum(row) < 2 ** 64 for row in m)
    tok_beg, toks = [0], []
    for cell in t_order:
        toks += by_cell[cell]
        tok_beg.append(len(toks))
    first = lambda keys, n: [sum(1 for k in keys if k < i) for i in range(n + 1)]
    i32, u32, u64 = (lambda v: np.array(v, dtype=np.int32)), (lambda v: np.array(v, dtype=np.uint32)), \
        (lambda v: np.array(v, dtype=np.uint64))
    return {'speakers': speakers, 'n_cells': K, 'n_spk': n_spk, 'n_type': n_type, 'n_tok': len(toks),
            'total': u64([sum(row) for row in m]),
            'spk_t': i32([s for t, s in t_order]), 'type_t': i32([t for t, s in t_order]),
            'type_beg': i32(first([t for t, s in t_order], n_type)), 'u_t': u32(u_t), 'f_t': u32(f_t),
            'cum_u_t': u64(running(u_t)), 'cum_f_t': u64(running(f_t)), 'tok_beg': i32(tok_beg), 'toks': i32(toks),
            'spk_s': i32([t_order[c][1] for c in s_order]), 'type_s': i32([t_order[c][0] for c in s_order]),
            's2t': i32(s_order), 'spk_beg': i32(first([t_order[c][1] for c in s_order], n_spk)), 'u_s': u32(u_s),
            'cum_u_s': u64(running(u_s)), 'cum_spk': u64(running(U_spk)), 'cum_m': u64([running(row) for row in m])}


# -- the generator -----------------------------------------------------------------------------------------------

def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=U64) & MASK32 for c in (c0, c1, c2, c3))
    k0, k1 = U64(k0 & 0xFFFFFFFF), U64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + U64(0x9E3779B9)) & MASK32, (k1 + U64(0xBB67AE85)) & MASK32
    return c0, c1, c2, c3


def draw(i, q, slot, seed):
    i = np.asarray(i, dtype=U64)
    q = np.broadcast_to(np.asarray(q, dtype=U64), i.shape)
    return philox4x32_10(i & MASK32, i >> S32, q, np.full(i.shape, slot, dtype=U64), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def mulhi64(a, b):
    a, b = np.asarray(a, dtype=U64), np.asarray(b, dtype=U64)
    a0, a1, b0, b1 = a & MASK32, a >> S32, b & MASK32, b >> S32
    mid = a1 * b0 + ((a0 * b0) >> S32)
    mid2 = a0 * b1 + (mid & MASK32)
    return a1 * b1 + (mid >> S32) + (mid2 >> S32)


def map128(r, M):
    """floor(r M / 2^128), r = (x + 2^32 y) 2^64 + (z + 2^32 w)."""
    M = np.asarray(M, dtype=U64)
    rh, rl = (r[1] << S32) | r[0], (r[3] << S32) | r[2]
    with np.errstate(over='ignore'):
        lo = rh * M
        s = lo + mulhi64(rl, M)
    return mulhi64(rh, M) + (s < lo).astype(U64)


# -- the searches ------------------------------------------------------------------------------------------------

def upper(cum, lo, hi, x):
    """Per element: the first index in [lo, hi) with cum[index] > x, hi if none (cum ascending there)."""
    lo, hi = np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)
    while True:
        live = lo < hi
        if not live.any():
            return lo
        mid = (lo + hi) >> 1
        gt = cum[np.minimum(mid, len(cum) - 1)] > x
        hi = np.where(live & gt, mid, hi)
        lo = np.where(live & ~gt, mid + 1, lo)


def lower(v, lo, hi, x):
    lo, hi = np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)
    while True:
        live = lo < hi
        if not live.any():
            return lo
        mid = (lo + hi) >> 1
        ge = v[np.minimum(mid, len(v) - 1)] >= x
        hi = np.where(live & ge, mid, hi)
        lo = np.where(live & ~ge, mid + 1, lo)


def before(cum, i):
    return np.where(i > 0, cum[np.maximum(i - 1, 0)], U64(0))


def second_range(t, q, a):
    """The range the second draw is mapped onto, per first cell a (an index in q's order)."""
    if q == 1:
        ty = t['type_t'][a]
        tb, te = t['type_beg'][ty], t['type_beg'][ty + 1]
        return t['cum_f_t'][te - 1] - before(t['cum_f_t'], tb) - t['f_t'][a].astype(U64)
    sp = t['spk_s'][a]
    sb, se = t['spk_beg'][sp], t['spk_beg'][sp + 1]
    u_spk = t['cum_u_s'][se - 1] - before(t['cum_u_s'], sb)
    ua = t['u_s'][a].astype(U64)
    if q == 2:
        return u_spk - ua
    ty = t['type_s'][a]
    tb, te = t['type_beg'][ty], t['type_beg'][ty + 1]
    return t['cum_spk'][-1] - u_spk - (t['cum_u_t'][te - 1] - before(t['cum_u_t'], tb)) + ua


def dd_H(t, x, tb, te, base_t):
    c = upper(t['spk_t'], tb, te, x)
    h = t['cum_spk'][np.maximum(x, 0)] - (before(t['cum_u_t'], c) - base_t)
    return np.where(x < 0, U64(0), h)


def second_cell(t, q, a, y):
    """The second cell (index in q's order: T for q = 1, S for q = 2, 3) for first cell a and mapped draw y."""
    a, y = np.asarray(a, dtype=np.int64), np.asarray(y, dtype=U64).copy()
    if q == 1:
        ty = t['type_t'][a]
        tb, te = t['type_beg'][ty].astype(np.int64), t['type_beg'][ty + 1].astype(np.int64)
        base, fa = before(t['cum_f_t'], tb), t['f_t'][a].astype(U64)
        y = np.where(y >= before(t['cum_f_t'], a) - base, y + fa, y)
        return np.clip(upper(t['cum_f_t'], tb, te, base + y), tb, te - 1)
    sp = t['spk_s'][a].astype(np.int64)
    sb, se = t['spk_beg'][sp].astype(np.int64), t['spk_beg'][sp + 1].astype(np.int64)
    ua = t['u_s'][a].astype(U64)
    if q == 2:
        base = before(t['cum_u_s'], sb)
        y = np.where(y >= before(t['cum_u_s'], a) - base, y + ua, y)
        return np.clip(upper(t['cum_u_s'], sb, se, base + y), sb, se - 1)
    ty = t['type_s'][a]
    tb, te = t['type_beg'][ty].astype(np.int64), t['type_beg'][ty + 1].astype(np.int64)
    base_t = before(t['cum_u_t'], tb)
    u_spk = t['cum_u_s'][se - 1] - before(t['cum_u_s'], sb)
    y = np.where(y >= dd_H(t, sp - 1, tb, te, base_t), y + (u_spk - ua), y)
    lo, hi = np.zeros(a.shape, dtype=np.int64), np.full(a.shape, t['n_spk'], dtype=np.int64)
    while (lo < hi).any():
        live = lo < hi
        mid = (lo + hi) >> 1
        gt = dd_H(t, np.minimum(mid, t['n_spk'] - 1), tb, te, base_t) > y
        hi = np.where(live & gt, mid, hi)
        lo = np.where(live & ~gt, mid + 1, lo)
    x = np.clip(lo, 0, t['n_spk'] - 1)
    z = y - dd_H(t, x - 1, tb, te, base_t)
    xb, xe = t['spk_beg'][x].astype(np.int64), t['spk_beg'][x + 1].astype(np.int64)
    base_x = before(t['cum_u_s'], xb)
    e = lower(t['type_s'], xb, xe, ty)
    ec = np.minimum(e, t['n_cells'] - 1)
    cut = (e < xe) & (t['type_s'][ec] == ty) & (z >= before(t['cum_u_s'], e) - base_x)
    z = np.where(cut, z + t['u_s'][ec].astype(U64), z)
    return np.clip(upper(t['cum_u_s'], xb, xe, base_x + z), xb, xe - 1)


def sample_pairs(t, counts, seed):
    """abn_sample_pairs: (tok1, tok2 int32, key int64, cells a, b in T order), configuration after configuration."""
    K = t['n_cells']
    tok1, tok2, key, cell_a, cell_b = [], [], [], [], []
    with np.errstate(over='ignore'):
        for q in range(4):
            n = int(counts[q])
            i = np.arange(n, dtype=U64)
            rk = draw(i, q, 3, seed)
            key.append((((rk[1] << S32) | rk[0]) >> U64(1)).astype(np.int64))
            M = t['total'][q]
            if int(M) == 0 or n == 0:
                for out in (tok1, tok2, cell_a, cell_b):
                    out.append(np.full(n, -1, dtype=np.int32))
                continue
            r0, r1, r2 = draw(i, q, 0, seed), draw(i, q, 1, seed), draw(i, q, 2, seed)
            ra, rb = (r2[1] << S32) | r2[0], (r2[3] << S32) | r2[2]
            a = np.clip(upper(t['cum_m'][q], np.zeros(n, np.int64), np.full(n, K, np.int64), map128(r0, M)), 0, K - 1)
            if q == 0:
                ca = cb = a
            else:
                b = second_cell(t, q, a, map128(r1, second_range(t, q, a)))
                if q == 1:
                    ca, cb = a, b
                else:
                    swap = t['type_s'][b] < t['type_s'][a]
                    ca, cb = t['s2t'][np.where(swap, b, a)], t['s2t'][np.where(swap, a, b)]
            oa, ob = t['tok_beg'][ca].astype(np.int64), t['tok_beg'][cb].astype(np.int64)
            na, nb = t['tok_beg'][ca + 1] - oa, t['tok_beg'][cb + 1] - ob
            ia = mulhi64(ra, na.astype(U64)).astype(np.int64)
            if q == 0:
                ib = np.where(nb > 1, mulhi64(rb, np.maximum(nb - 1, 0).astype(U64)).astype(np.int64), 0)
                ib = np.where((ib >= ia) & (nb > 1), ib + 1, ib)
            else:
                ib = mulhi64(rb, nb.astype(U64)).astype(np.int64)
            tok1.append(t['toks'][oa + ia])
            tok2.append(t['toks'][ob + ib])
            cell_a.append(np.asarray(ca, dtype=np.int32))
            cell_b.append(np.asarray(cb, dtype=np.int32))
    cat = np.concatenate
    return cat(tok1).astype(np.int32), cat(tok2).astype(np.int32), cat(key), cat(cell_a), cat(cell_b)


def final_order(key):
    return np.argsort(key, kind='stable')


# -- what the tables realise, exactly ----------------------------------------------------------------------------

def _hits(lo, hi, M):
    """How many of the 2^128 values of r have lo <= floor(r M / 2^128) < hi."""
    ceil_div = lambda n, d: -((-n) // d)
    return ceil_div(hi << 128, M) - ceil_div(lo << 128, M)


def realised_distribution(t, q):
    """{(first cell, second cell) in T order, as the kernel ORDERS the draw: Fraction probability} of configuration
    q, from the tables and the restated search functions alone: the first cell's share of the 2^128 draws, times, for
    each second cell, the share of the draws whose mapped value the search sends to it (the breakpoints of the
    monotone search function are found by bisection on the restated function itself)."""
    K, M = t['n_cells'], int(t['total'][q])
    out = {}
    if M == 0:
        return out
    cum = [0] + [int(v) for v in t['cum_m'][q]]
    firsts = [a for a in range(K) if cum[a + 1] > cum[a]]
    p_first = {a: Fraction(_hits(cum[a], cum[a + 1], M), 1 << 128) for a in firsts}
    if q == 0:
        return {(a, a): p for a, p in p_first.items()}
    a_arr = np.array(firsts, dtype=np.int64)
    R = [int(v) for v in second_range(t, q, a_arr)]
    # the smallest y with second_cell(a, y) >= j, for every first cell and every j in 0 .. K (R where there is none)
    A = np.repeat(a_arr, K + 1)
    J = np.tile(np.arange(K + 1, dtype=np.int64), len(firsts))
    lo, hi = np.zeros(len(A), dtype=object), np.repeat(np.array(R, dtype=object), K + 1)
    for _ in range(34):
        live = lo < hi
        mid = (lo + hi) // 2
        probe = np.where(live, mid, 0).astype(U64)
        ge = second_cell(t, q, A, probe) >= J
        hi = np.where(live & ge, mid, hi)
        lo = np.where(live & ~ge, mid + 1, lo)
    assert (lo >= hi).all()
    brk = lo.reshape(len(firsts), K + 1)
    to_t = (lambda c: c) if q == 1 else (lambda c: int(t['s2t'][c]))
    for n, a in enumerate(firsts):
        for b in range(K):
            y0, y1 = int(brk[n, b]), int(brk[n, b + 1])
            if y1 > y0:
                out[(to_t(a), to_t(b))] = p_first[a] * Fraction(_hits(y0, y1, R[n]), 1 << 128)
    return out


def draw_key(t, q, ca, cb):
    """The reference's key tuple for cells ca, cb (T order) DRAWN in this order: (spk, type), (spk, spk2, type),
    (spk, min type, max type), (spk, spk2, min type, max type)."""
    name = t['speakers']
    sa, sb, ta, tb = name[t['spk_t'][ca]], name[t['spk_t'][cb]], int(t['type_t'][ca]), int(t['type_t'][cb])
    return [(sa, ta), (sa, sb, ta), (sa, min(ta, tb), max(ta, tb)), (sa, sb, min(ta, tb), max(ta, tb))][q]


def realised_by_key(t, q):
    """realised_distribution folded onto the reference's keys: {key tuple: Fraction} (Dtype_Sspk's key is unordered:
    both draw orders add up)."""
    out = {}
    for (ca, cb), p in realised_distribution(t, q).items():
        key = draw_key(t, q, ca, cb)
        out[key] = out.get(key, 0) + p
    return out


def quantisation_epsilon(t):
    """The largest relative error of one quantised factor: rint moves S w by at most 1/2, so
    |u~ / (S w) - 1| <= (1/2) / (u~ - 1/2) <= 1 / (2 u~_min - 1); 2^-50 covers S w's own float64 rounding."""
    smallest = min(int(t['u_t'].min()), int(t['f_t'].min()))
    assert smallest >= 2, 'a weight was clamped to 1: the bound does not cover it'
    return Fraction(1, 2 * smallest - 1) + Fraction(1, 1 << 50)


def distribution_bound(t):
    """Relative bound on |realised - defined| per key: a key's weight is a product of two
    quantised factors, the normaliser a sum of such products, and each of the two draws is mapped with a relative
    bias of at most M / 2^128 <= 2^-64."""
    e = quantisation_epsilon(t)
    return ((1 + e) / (1 - e)) ** 2 * (1 + Fraction(1, 1 << 64)) ** 2 - 1
