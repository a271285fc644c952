"""computeQuadricCostMatrix against exact arithmetic: a generator of symmetric 3 x 3 matrices S = cov1 + cov2
of a chosen condition number, positive definite and indefinite, and d^T S^-1 d in rational arithmetic.  d = m1 - m2 and
S = cov1 + cov2 are formed in float64 first, as the reference and the kernel both specify (assignment.cpp:716-717); everything
after that is exact."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53


def exact_quadric(d, S):
    """d^T S^-1 d for float64 d[3], S[3][3] by adjugate and determinant in rational arithmetic; None where det S == 0."""
    a = [[Fraction(float(S[i][j])) for j in range(3)] for i in range(3)]
    v = [Fraction(float(x)) for x in d]
    det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
           + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    if det == 0:
        return None
    adj = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            r = [x for x in range(3) if x != j]
            c = [x for x in range(3) if x != i]
            adj[i][j] = (-1) ** (i + j) * (a[r[0]][c[0]] * a[r[1]][c[1]] - a[r[0]][c[1]] * a[r[1]][c[0]])
    return sum(v[i] * adj[i][j] * v[j] for i in range(3) for j in range(3)) / det


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _split(rng, S):
    """S as a sum of two symmetric float64 matrices (what the caller holds: a landmark's and a measurement's covariance)."""
    t = rng.uniform(0.2, 0.8)
    c1 = S * t
    return c1, S - c1


def pairs(rng, n):
    """n (kind, m1, cov1, m2, cov2) with S = cov1 + cov2 symmetric: eigenvalues spread so that cond_2(S) covers 1 .. 1e12,
    every third indefinite; then the structured cases -- equal diagonal entries (the pivot search ties), diagonal S, d = 0."""
    out = []
    for i in range(n):
        logc = rng.uniform(0.0, 12.0)
        lam = 10.0 ** np.array([0.0, -logc * rng.random(), -logc]) * 10.0 ** rng.uniform(-2.0, 2.0)
        kind = "spd"
        if i % 3 == 2:
            lam = lam * rng.choice([-1.0, 1.0], size=3)
            if (lam > 0).all():
                lam[int(rng.integers(3))] *= -1.0
            kind = "indef"
        q = _rotation(rng)
        S = (q * lam) @ q.T
        S = (S + S.T) / 2
        m2 = rng.normal(size=3) * 5.0
        m1 = m2 + rng.normal(size=3) * 10.0 ** rng.uniform(-3.0, 1.0)
        out.append((kind,) + (m1,) + _split(rng, S)[:1] + (m2,) + _split(rng, S)[1:])
    for i in range(max(4, n // 20)):
        a, b, c = rng.uniform(1.0, 3.0), rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9)
        S = np.array([[a, b, c], [b, a, b], [c, b, a]])                       # equal diagonal: the pivot search ties
        out.append(("equal_diag", rng.normal(size=3), S / 2, rng.normal(size=3), S / 2))
        S = np.diag(10.0 ** rng.uniform(-6.0, 6.0, size=3))                   # diagonal S
        out.append(("diagonal", rng.normal(size=3), S * 0.25, rng.normal(size=3), S * 0.75))
        S = np.eye(3) * rng.uniform(0.5, 2.0)                                 # a multiple of the identity: every pivot ties
        out.append(("identity", rng.normal(size=3), S * 0.5, rng.normal(size=3), S * 0.5))
        m = rng.normal(size=3)
        q = _rotation(rng)
        S = (q * np.array([1.0, 0.1, 1e-5])) @ q.T
        S = (S + S.T) / 2
        out.append(("d_zero", m, S * 0.5, m.copy(), S * 0.5))                 # d = 0: the cost is exactly 0
    return out


def formed(p):
    """(d, S) as float64 forms them."""
    _, m1, c1, m2, c2 = p
    return np.asarray(m1, np.float64) - np.asarray(m2, np.float64), np.asarray(c1, np.float64) + np.asarray(c2, np.float64)


def scale_and_cond(d, S):
    """(d^T |S|^-1 d, cond_2(S)): the sum d^T S^-1 d = sum_i (q_i . d)^2 / lambda_i without its cancellation -- for a positive
    definite S the value itself -- and the 2-norm condition number of S."""
    lam, q = np.linalg.eigh(S)
    w = q.T @ d
    return float(np.sum(w * w / np.abs(lam))), float(np.abs(lam).max() / np.abs(lam).min())


def ratio(got, d, S):
    """|got - exact| / (eps cond_2(S) d^T|S|^-1 d); 0.0 where both are exactly 0."""
    ex = exact_quadric(d, S)
    sc, cond = scale_and_cond(d, S)
    err = abs(Fraction(float(got)) - ex)
    if err == 0:
        return 0.0
    return float(err / (Fraction(EPS) * Fraction(cond) * Fraction(sc))) if sc > 0 else float("inf")
