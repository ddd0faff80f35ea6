"""The float64 restatement of soft-DTW over cosine cells (include/abnet3_hip_next.h, section abnq_; abnet3_amd/softdtw.py,
abnet3_amd/loss.py: SoftDTWLoss): explicit loops over the cells and the paths (only a row's
dot product is numpy's).

    cells(x, y)                  (c, d, unit rows, 1 / max(norm, eps), norms) of one problem
    value_r(d, gamma)            the forward recurrence: (value, r with its +inf border)
    expected(d, r, gamma)        E, the expected alignment
    problem(x, y, gamma, w)      dict(value, r, E, g1, g2): value, both gradients of w * value
    brute_value(d, gamma)        -gamma log(sum over all monotone paths of exp(-cost / gamma)), n, m <= 5
    hard_cost(d)                 the DTW cost over the same cells
    divergence(x, y, gamma)      value(x, y) - (value(x, x) + value(y, y)) / 2 and its gradients
    loss(...)                    SoftDTWLoss and its gradient with respect to the rows of the table

`cell_dtype=np.float32` is the float32-cell YARDSTICK: the unit rows, c and d are computed and rounded in float32 (what a
kernel with float32 cells does), every recurrence and sum after them stays float64.  Its distance from the float64
restatement is the scale the kernel's gradients are measured on.  A plain helper module: no fixture, not a conftest."""
import numpy as np

EPS = 1e-6


def cells(x, y, cell_dtype=np.float64):
    """x [n, D], y [m, D].  Norms in float64 whatever the cell type; the unit rows, c and d in `cell_dtype`."""
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = x64.shape[0], y64.shape[0]
    nx, ny = np.zeros(n), np.zeros(m)
    for i in range(n):
        nx[i] = np.sqrt(np.dot(x64[i], x64[i]))
    for j in range(m):
        ny[j] = np.sqrt(np.dot(y64[j], y64[j]))
    ix, iy = 1.0 / np.maximum(nx, EPS), 1.0 / np.maximum(ny, EPS)
    xh = (x64 * ix[:, None]).astype(cell_dtype)
    yh = (y64 * iy[:, None]).astype(cell_dtype)
    c = np.zeros((n, m), dtype=cell_dtype)
    for i in range(n):
        for j in range(m):
            c[i, j] = np.dot(xh[i], yh[j])          # in cell_dtype (float32: numpy's blockwise sum, rounded per operation)
    d = (cell_dtype(1) - c).astype(cell_dtype)
    return dict(c=c, d=d, xh=xh, yh=yh, ix=ix, iy=iy, nx=nx, ny=ny)


def softmin(a, b, c, gamma):
    mn = min(a, b, c)
    s = 0.0
    for v in (a, b, c):
        if v != np.inf:
            s += np.exp(-(v - mn) / gamma)
    return mn - gamma * np.log(s)


def value_r(d, gamma):
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    r = np.full((n + 1, m + 1), np.inf)
    r[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            r[i, j] = d[i - 1, j - 1] + softmin(r[i - 1, j - 1], r[i - 1, j], r[i, j - 1], gamma)
    return r[n, m], r


def expected(d, r, gamma):
    """E[i][j] over the cells (0-based), from r with its border (1-based)."""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    E = np.zeros((n + 2, m + 2))
    E[n, m] = 1.0
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            if i == n and j == m:
                continue
            acc = 0.0
            for a, b in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
                if a <= n and b <= m:
                    acc += E[a, b] * np.exp((r[a, b] - r[i, j] - d[a - 1, b - 1]) / gamma)
            E[i, j] = acc
    return E[1:n + 1, 1:m + 1].copy()


def problem(x, y, gamma, w=1.0, cell_dtype=np.float64):
    cl = cells(x, y, cell_dtype)
    c, d = cl['c'].astype(np.float64), cl['d'].astype(np.float64)
    xh, yh = cl['xh'].astype(np.float64), cl['yh'].astype(np.float64)
    value, r = value_r(d, gamma)
    E = expected(d, r, gamma)
    n, m = d.shape
    D = xh.shape[1]
    g1, g2 = np.zeros((n, D)), np.zeros((m, D))
    for i in range(n):
        s, sc = np.zeros(D), 0.0
        for j in range(m):
            s += E[i, j] * yh[j]
            sc += E[i, j] * c[i, j]
        if cl['nx'][i] >= EPS:
            s = s - sc * xh[i]
        g1[i] = -(w * cl['ix'][i]) * s
    for j in range(m):
        s, sc = np.zeros(D), 0.0
        for i in range(n):
            s += E[i, j] * xh[i]
            sc += E[i, j] * c[i, j]
        if cl['ny'][j] >= EPS:
            s = s - sc * yh[j]
        g2[j] = -(w * cl['iy'][j]) * s
    return dict(value=value, r=r, E=E, g1=g1, g2=g2, d=d, c=c)


def monotone_paths(n, m):
    """Every path from (0, 0) to (n - 1, m - 1) by steps (1, 0), (0, 1), (1, 1)."""
    def go(i, j):
        if i == n - 1 and j == m - 1:
            yield [(i, j)]
            return
        for a, b in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
            if a < n and b < m:
                for rest in go(a, b):
                    yield [(i, j)] + rest
    return go(0, 0)


def brute_value(d, gamma):
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    assert n <= 5 and m <= 5
    costs = np.array([sum(d[i, j] for i, j in path) for path in monotone_paths(n, m)])
    mn = costs.min()
    return mn - gamma * np.log(np.exp(-(costs - mn) / gamma).sum())


def hard_cost(d):
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    r = np.full((n + 1, m + 1), np.inf)
    r[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            r[i, j] = d[i - 1, j - 1] + min(r[i - 1, j - 1], r[i - 1, j], r[i, j - 1])
    return r[n, m]


def divergence(x, y, gamma, w=1.0, cell_dtype=np.float64):
    """(value, gradient w.r.t. x, gradient w.r.t. y) of w (value(x, y) - (value(x, x) + value(y, y)) / 2)."""
    xy, xx, yy = problem(x, y, gamma, w, cell_dtype), problem(x, x, gamma, -0.5 * w, cell_dtype), problem(y, y, gamma, -0.5 * w, cell_dtype)
    v = xy['value'] - 0.5 * (xx['value'] + yy['value'])
    return v, xy['g1'] + xx['g1'] + xx['g2'], xy['g2'] + yy['g1'] + yy['g2']


def loss(e, off1, n1, off2, n2, y, gamma=0.1, margin=0.5, normalize=True, divergence_=False, avg=True, cell_dtype=np.float64):
    """SoftDTWLoss: (loss, terms [P], de [R, D]).  Within a side the problems' row ranges must not overlap."""
    e = np.asarray(e)
    P = len(n1)
    de = np.zeros(e.shape, dtype=np.float64)
    terms = np.zeros(P)
    total = 0.0
    scale = 1.0 / P if (avg and P > 0) else 1.0
    for p in range(P):
        a, b = int(off1[p]), int(off2[p])
        n, m = int(n1[p]), int(n2[p])
        x, yv = e[a:a + n], e[b:b + m]
        v = (divergence(x, yv, gamma, 1.0, cell_dtype) if divergence_ else problem(x, yv, gamma, 1.0, cell_dtype)['value'])
        v = v[0] if divergence_ else v
        norm = 1.0 / (n + m) if normalize else 1.0
        s = v * norm
        if y[p] == 1:
            t, dt = s, 1.0
        else:
            t, dt = max(0.0, margin - s), (-1.0 if margin - s > 0 else 0.0)
        terms[p] = t
        total += t
        wgt = scale * dt * norm
        if divergence_:
            _, gx, gy = divergence(x, yv, gamma, wgt, cell_dtype)
        else:
            q = problem(x, yv, gamma, wgt, cell_dtype)
            gx, gy = q['g1'], q['g2']
        de[a:a + n] += gx
        de[b:b + m] += gy
    return total * scale if P > 0 else 0.0, terms, de


def draw(rng, n, m, D, scale=1.0):
    """Two float32 sequences that are related (y = a warped, noisy x), so that the alignment is not flat."""
    x = rng.standard_normal((n, D)).astype(np.float32) * np.float32(scale)
    idx = np.rint(np.linspace(0, n - 1, m)).astype(int)
    y = (x[idx] + 0.5 * rng.standard_normal((m, D))).astype(np.float32)
    return x, y
