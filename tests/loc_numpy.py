"""Plain NumPy twins of the localisation kernels (csrc/loc_ops.hip): joint diagonalisation of a stack of symmetric matrices by Jacobi sweeps in the same pair order
(circle-method tournament) with the same angle rule, and the localisation functional.  Nothing here is shared with the code under test."""
import numpy as np

NOISE_FLOOR = 1.0e-28      # csrc/loc_core.h kNoiseFloor: a pair whose sums are below this fraction of sum_k ||Q^k||_F^2 is rounding noise and is not turned


def rr_pair(np_, r, j):
    """slot j of round r of the circle method for np_ (even) players; (p, q) with p < q"""
    n1 = np_ - 1
    p, q = (n1, r) if j == 0 else ((r + j) % n1, (r - j + n1) % n1)
    return (p, q) if p < q else (q, p)


def functional(Q):
    return float(sum((np.diag(q) ** 2).sum() for q in Q))


def pair_angle(Q, p, q, norm2):
    a = Q[:, p, q]
    d = 0.5 * (Q[:, p, p] - Q[:, q, q])
    y, x = 2.0 * float(a @ d), float(d @ d) - float(a @ a)
    if np.hypot(y, x) <= NOISE_FLOOR * norm2:
        return 0.0
    return 0.25 * np.arctan2(y, x)


def joint_diag(Q0, stop_angle=1e-10, max_sweeps=200):
    """-> (Q, U, sweeps, f, converged): U orthogonal from the identity, Q^k = U^T Q0^k U, f = sum_k sum_i (Q^k_ii)^2 maximal over plane rotations"""
    Q = np.array(Q0, dtype=np.float64, copy=True)
    K, m = Q.shape[0], Q.shape[1]
    U = np.eye(m)
    if m <= 1 or K == 0:
        return Q, U, 0, functional(Q), True
    norm2 = float((Q ** 2).sum())
    np_ = m + (m & 1)
    sweeps, converged = 0, False
    while sweeps < max_sweeps:
        thmax = 0.0
        for r in range(np_ - 1):
            pairs = [rr_pair(np_, r, j) for j in range(np_ // 2)]
            pairs = [(p, q) for p, q in pairs if q < m]      # the bye of an odd tournament
            th = np.array([pair_angle(Q, p, q, norm2) for p, q in pairs])
            thmax = max(thmax, float(np.abs(th).max()))
            ps, qs = np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])
            c, s = np.cos(th), np.sin(th)
            # the round's disjoint rotations p' = c p + s q, q' = -s p + c q: rows, then columns, and the columns of U
            Rp, Rq = Q[:, ps, :].copy(), Q[:, qs, :].copy()
            Q[:, ps, :], Q[:, qs, :] = c[None, :, None] * Rp + s[None, :, None] * Rq, c[None, :, None] * Rq - s[None, :, None] * Rp
            Cp, Cq = Q[:, :, ps].copy(), Q[:, :, qs].copy()
            Q[:, :, ps], Q[:, :, qs] = c * Cp + s * Cq, c * Cq - s * Cp
            Up, Uq = U[:, ps].copy(), U[:, qs].copy()
            U[:, ps], U[:, qs] = c * Up + s * Uq, c * Uq - s * Up
        sweeps += 1
        if thmax < stop_angle:
            converged = True
            break
    return Q, U, sweeps, functional(Q), converged


def stationarity(Q):
    """max over pairs of |sum_k a_k (Q^k_pp - Q^k_qq)| and min over pairs of sum d^2 - sum a^2"""
    K, m = Q.shape[0], Q.shape[1]
    g, h = 0.0, np.inf
    for p in range(m):
        for q in range(p + 1, m):
            a = Q[:, p, q]
            d = 0.5 * (Q[:, p, p] - Q[:, q, q])
            g = max(g, abs(float(a @ (2.0 * d))))
            h = min(h, float(d @ d) - float(a @ a))
    return g, h


def dipole_quadrature(mol, origin=(0.0, 0.0, 0.0), npts=12):
    """<a|r - origin|b> of a quemb_amd.integrals.Mole by Gauss-Hermite quadrature: the product of two Cartesian primitives is exp(-mu |A - B|^2) times a polynomial
    times exp(-p |r - P|^2), and each Cartesian factor of degree <= 2 npts - 1 is integrated exactly on the nodes x = P + t / sqrt(p).  No Hermite recursion.
    -> (3, nao, nao)"""
    t, w = np.polynomial.hermite.hermgauss(npts)
    n = mol.ncart
    out = np.zeros((3, n, n))
    o = np.asarray(origin, dtype=float)
    for i, fa in enumerate(mol.bfs):
        for j, fb in enumerate(mol.bfs):
            A, B = np.array(fa.ctr[:]), np.array(fb.ctr[:])
            for ia in range(fa.nprim):
                for ib in range(fb.nprim):
                    a, b = fa.ex[ia], fb.ex[ib]
                    p = a + b
                    P = (a * A + b * B) / p
                    pre = fa.co[ia] * fb.co[ib] * np.exp(-a * b / p * ((A - B) ** 2).sum())
                    s0, s1 = np.empty(3), np.empty(3)      # the overlap factor and the first-moment factor of each direction
                    for d in range(3):
                        x = P[d] + t / np.sqrt(p)
                        g = (x - A[d]) ** fa.lmn[d] * (x - B[d]) ** fb.lmn[d] * w / np.sqrt(p)
                        s0[d], s1[d] = g.sum(), (g * (x - o[d])).sum()
                    out[0, i, j] += pre * s1[0] * s0[1] * s0[2]
                    out[1, i, j] += pre * s0[0] * s1[1] * s0[2]
                    out[2, i, j] += pre * s0[0] * s0[1] * s1[2]
    return np.array([mol._sph2(x) for x in out])
