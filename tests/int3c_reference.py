"""An independent reference for the DF integrals (mu nu|P) and (P|Q): plain quadrature, no Boys function, no Hermite expansion coefficients, no
R_{tuv} table -- nothing of the McMurchie-Davidson scheme that csrc/int3c_core.h and csrc_host/gto_ints.c share.

    1/r12 = 2/sqrt(pi) int_0^inf exp(-u^2 r12^2) du

At fixed u the integral of three primitive Cartesian Gaussians (exponents a, b on A, B for electron 1; q on C for electron 2) is a product of three
2-D Gaussian moments, one per direction,

    int int (x1-A)^i (x1-B)^j (x2-C)^k exp(-a (x1-A)^2 - b (x1-B)^2 - q (x2-C)^2 - u^2 (x1-x2)^2) dx1 dx2.

With the origin at P = (aA + bB)/p, p = a + b, the exponent is -(ab/p)(A-B)^2 - y^T M y + 2 q C' y2 - q C'^2, M = [[p+u^2, -u^2], [-u^2, q+u^2]], C' = C - P.
Completing the square and substituting u^2 = rho t^2/(1-t^2), rho = pq/(p+q), everything becomes a polynomial in t^2:

    minimum of the form       rho C'^2 t^2                               (so the three directions give exp(-T t^2), T = rho |P-C|^2)
    position of the minimum   y0 = C' t^2 (q, -p)/(p+q) + (0, C')
    M^-1                      [[(1-t^2)/p + t^2/(p+q), t^2/(p+q)], [t^2/(p+q), (1-t^2)/q + t^2/(p+q)]],   det M^-1 = (1-t^2)/(pq)

and y = y0 + S z with S the (lower) Cholesky factor of M^-1 turns the moment into int int poly(z) exp(-z^2) dz1 dz2 / sqrt(det M): Gauss-Hermite, exact
for the degree <= 8 that occurs.  (S22 is formed from det M^-1 / S11^2, not from the difference that cancels as t -> 1.)  The Jacobians of the three
directions cancel the (1-t^2)^-3/2 of du, so that

    [ab|c] = 2/sqrt(pi) K_ab sqrt(rho) (pq)^-3/2 int_0^1 exp(-T t^2) G_x(t) G_y(t) G_z(t) dt,      K_ab = exp(-(ab/p) |A-B|^2)

with G_d the Gauss-Hermite sums: Gauss-Legendre in t, split at min(1, 8/sqrt(T)) so that a large T is resolved.  Contraction with the `co` / `ex` / `lmn`
records of `Mole.bfs` and the matrices of `Mole.c2s` gives blocks in the AO order and normalisation of integrals.aux_e2; (P|Q) is b = 0, l_b = 0.
The matrices of `Mole.c2s` are first made harmonic beyond float64 (`harmonic`): the integrals meant are those of the solid harmonics.
`ORDERS` holds two quadrature orders; `converged_block` evaluates at both and refuses a block on which they differ by more than 1e-13 of its largest
element.  `primitive_mp` is the same integral in mpmath at 30 digits for single primitives (a third opinion on the hardest blocks) and `block_mp` a whole
single-primitive block in mpmath, for the far f / g blocks that extended precision cannot certify to 1e-13;
`boys_mp` is the Boys function from mpmath's incomplete gamma function at 40 digits (used by the Boys checks only, never by the integrals here)."""
import functools

import numpy as np

ORDERS = ((12, 120), (9, 96))          # (Gauss-Hermite nodes per variable, Gauss-Legendre nodes per segment of t)
SELF_CHECK = 1e-13


LD = np.longdouble                      # the quadrature runs in extended precision where the platform has it: the Cartesian -> spherical step of an
                                        # f or g shell cancels two digits, which in float64 would leave the self-check no room


@functools.lru_cache(None)
def _gh(n):
    """Gauss-Hermite nodes and weights (weight exp(-z^2)): numpy's, polished by Newton steps on H_n in extended precision."""
    x = np.polynomial.hermite.hermgauss(n)[0].astype(LD)
    for _ in range(3):
        h0, h1 = np.ones_like(x), 2 * x                      # H_0, H_1; H_{k+1} = 2 x H_k - 2 k H_{k-1}; H_n' = 2 n H_{n-1}
        for k in range(1, n):
            h0, h1 = h1, 2 * x * h1 - 2 * k * h0
        x = x - h1 / (2 * n * h0)
    h0, h1 = np.ones_like(x), 2 * x
    for k in range(1, n - 1):
        h0, h1 = h1, 2 * x * h1 - 2 * k * h0
    fact = LD(1)
    for k in range(2, n + 1):
        fact *= k
    return x, LD(2) ** (n - 1) * fact * np.sqrt(4 * np.arctan(LD(1))) / (n * h1) ** 2


@functools.lru_cache(None)
def _gl(n):
    """Gauss-Legendre nodes and weights on [-1, 1], polished likewise on P_n."""
    x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for it in range(4):
        p0, p1 = np.ones_like(x), x                          # (k + 1) P_{k+1} = (2k + 1) x P_k - k P_{k-1}; (x^2 - 1) P_n' = n (x P_n - P_{n-1})
        for k in range(1, n):
            p0, p1 = p1, ((2 * k + 1) * x * p1 - k * p0) / (k + 1)
        dp = n * (x * p1 - p0) / (x * x - 1)
        if it < 3:
            x = x - p1 / dp
    return x, 2 / ((1 - x * x) * dp * dp)


def cart_components(l):
    return [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]


def _t_nodes(T, ngl):
    x, w = _gl(ngl)
    cut = min(LD(1), 8 / np.sqrt(T)) if T > 64.0 else LD(1)
    t, wt = 0.5 * cut * (x + 1.0), 0.5 * cut * w
    if cut < 1.0:
        t = np.concatenate([t, cut + 0.5 * (1.0 - cut) * (x + 1.0)]); wt = np.concatenate([wt, 0.5 * (1.0 - cut) * w])
    return t, wt


def primitive(a, A, la, b, B, lb, q, C, lp, order=0):
    """[ab|c] of three unnormalised primitive Cartesian shells: (ncart(la), ncart(lb), ncart(lp)), components in the order of cart_components, in
    extended precision (the contraction and the Cartesian -> spherical step of the callers stay in it; they round once, at the end)."""
    ngh, ngl = ORDERS[order]
    A, B, C = (np.asarray(v, dtype=float).astype(LD) for v in (A, B, C))
    a, b, q = LD(a), LD(b), LD(q)
    p = a + b
    AB = A - B
    PA, PB = -(b / p) * AB, (a / p) * AB          # P - A, P - B
    Cp = C - (A + (b / p) * (B - A))              # C - P
    rho = p * q / (p + q)
    T = rho * (Cp * Cp).sum()
    t, wt = _t_nodes(T, ngl)
    t2 = t * t
    z, wz = _gh(ngh)
    s11sq = (1.0 - t2) / p + t2 / (p + q)
    S11 = np.sqrt(s11sq); S21 = (t2 / (p + q)) / S11; S22 = np.sqrt((1.0 - t2) / (p * q * s11sq))
    G = []
    for d in range(3):
        y1 = (Cp[d] * q / (p + q)) * t2[:, None] + S11[:, None] * z[None, :]                                                  # (t, z1): x1 - P
        y2c = (-Cp[d] * p / (p + q)) * t2[:, None, None] + S21[:, None, None] * z[None, :, None] + S22[:, None, None] * z[None, None, :]   # x2 - C
        h = np.stack([(wz * y2c ** k).sum(axis=2) for k in range(lp + 1)])                                                     # (k, t, z1)
        f = np.stack([np.stack([wz * (y1 + PA[d]) ** i * (y1 + PB[d]) ** j for j in range(lb + 1)]) for i in range(la + 1)])     # (i, j, t, z1)
        G.append(np.einsum("ijtz,ktz->ijkt", f, h))
    ca, cb, cc = (np.array(cart_components(l)) for l in (la, lb, lp))
    pick = lambda d: G[d][ca[:, d][:, None, None], cb[:, d][None, :, None], cc[:, d][None, None, :]]                         # (ncA, ncB, ncP, t)
    val = (pick(0) * pick(1) * pick(2) * (wt * np.exp(-T * t2))).sum(axis=3)
    pi = 4 * np.arctan(LD(1))
    return ((2 / np.sqrt(pi)) * np.exp(-(a * b / p) * (AB * AB).sum()) * np.sqrt(rho) / (p * q * np.sqrt(p * q)) * val)


def _shell(mol, i):
    """(l, centre, exponents, coefficients (ncart, nprim), Cartesian range, AO range) of shell i from the records of Mole.bfs."""
    ia, l, ex, _, ao0, c0 = mol.shells[i]
    nc = (l + 1) * (l + 2) // 2
    assert [tuple(mol.bfs[c0 + k].lmn) for k in range(nc)] == cart_components(l)
    co = np.array([[mol.bfs[c0 + k].co[j] for j in range(len(ex))] for k in range(nc)])
    assert all(mol.bfs[c0 + k].ex[j] == ex[j] for k in range(nc) for j in range(len(ex)))
    return l, np.array(mol.bfs[c0].ctr[:]), np.asarray(ex, dtype=float), co, slice(c0, c0 + nc), slice(ao0, ao0 + 2 * l + 1)


def _laplacian(l):
    """The Laplacian from the degree-l monomials (order of cart_components) to the degree l - 2 ones, as an integer matrix."""
    comps = cart_components(l)
    lower = {c: i for i, c in enumerate(cart_components(l - 2))}
    lap = np.zeros((len(lower), len(comps)))
    for j, c in enumerate(comps):
        for d in range(3):
            if c[d] >= 2:
                cc = list(c); cc[d] -= 2
                lap[lower[tuple(cc)], j] += c[d] * (c[d] - 1)
    return lap


def harmonic(M, l, mp=None):
    """The Cartesian -> spherical matrix M of a shell (float64, integrals.cart2sph) with its non-harmonic residue projected out, M - L^T (L L^T)^-1 L M with
    L the Laplacian, in extended precision (or in mpmath when the module is passed).  The float64 matrix of a g shell is harmonic to 2e-14 only; the
    residue is a lower multipole, and through the Cartesian route of this reference it would put 2e-14 of the R^-1 part of the Cartesian integrals into a
    far block that falls like R^-5 or faster -- 7.6e-10 of the (d d|g) block at T = 1000.  The integrals meant are those of the solid harmonics (the host
    and device sources carry only the top Hermite term of an auxiliary shell, which evaluates exactly those), so the reference integrates them."""
    if l < 2:
        return M.astype(LD) if mp is None else mp.matrix(M.tolist())
    L = _laplacian(l)
    if mp is not None:
        Lm, Mm = mp.matrix(L.tolist()), mp.matrix(M.tolist())
        return Mm - Lm.T * (mp.inverse(Lm * Lm.T) * (Lm * Mm))
    L, M = L.astype(LD), M.astype(LD)
    G = (L @ L.T).astype(np.float64)                     # small integers: exact
    res = L @ M
    x = np.zeros_like(res)
    for _ in range(4):                                   # iterative refinement of the float64 solve
        x = x + np.linalg.solve(G, (res - (L @ L.T) @ x).astype(np.float64)).astype(LD)
    return M - L.T @ x


def block3c(mol, aux, i, j, k, order=0, prim=None):
    """(mu nu|P) for the orbital shells i, j of `mol` and the auxiliary shell k of `aux`: (2 l_i + 1, 2 l_j + 1, 2 l_k + 1), as integrals.aux_e2."""
    la, A, exa, coa, ca, sa = _shell(mol, i)
    lb, B, exb, cob, cb, sb = _shell(mol, j)
    lp, Cc, exc, coc, cc, sc = _shell(aux, k)
    acc = np.zeros((coa.shape[0], cob.shape[0], coc.shape[0]), dtype=LD)
    for x, a in enumerate(exa):
        for y, b in enumerate(exb):
            for w, q in enumerate(exc):
                acc += coa[:, x, None, None] * cob[None, :, y, None] * coc[None, None, :, w] * (prim or primitive)(a, A, la, b, B, lb, q, Cc, lp, order)
    return np.einsum("abc,ai,bj,ck->ijk", acc, harmonic(mol.c2s[ca, sa], la), harmonic(mol.c2s[cb, sb], lb), harmonic(aux.c2s[cc, sc], lp)).astype(np.float64)


def block2c(aux, i, k, order=0, prim=None):
    """(P|Q) for the shells i, k of `aux`: (2 l_i + 1, 2 l_k + 1), as integrals.int2c2e."""
    la, A, exa, coa, ca, sa = _shell(aux, i)
    lp, Cc, exc, coc, cc, sc = _shell(aux, k)
    acc = np.zeros((coa.shape[0], coc.shape[0]), dtype=LD)
    for x, a in enumerate(exa):
        for w, q in enumerate(exc):
            acc += coa[:, x, None] * coc[None, :, w] * (prim or primitive)(a, A, la, 0.0, A, 0, q, Cc, lp, order)[:, 0, :]
    return np.einsum("ac,ai,ck->ik", acc, harmonic(aux.c2s[ca, sa], la), harmonic(aux.c2s[cc, sc], lp)).astype(np.float64)


def converged_block(fn, *args):
    """The block at the first quadrature order and its deviation from the second one relative to its largest element; refused above SELF_CHECK."""
    r0, r1 = fn(*args, order=0), fn(*args, order=1)
    top = float(np.abs(r0).max())
    dev = float(np.abs(r0 - r1).max()) / top if top > 0 else 0.0
    if not dev <= SELF_CHECK:
        raise ArithmeticError(f"the two quadrature orders differ by {dev:.2e} of the block's largest element {top:.3e}")
    return r0, dev


# ---- mpmath: a third opinion on single primitives, and the Boys function -----------------------------------------------------------------------
@functools.lru_cache(None)
def _gh_mp(n, dps):
    import mpmath as mp
    with mp.workdps(dps + 10):
        x, w = np.polynomial.hermite.hermgauss(n)
        nodes = [mp.findroot(lambda v: mp.hermite(n, v), mp.mpf(float(v))) for v in x]
        wts = [2 ** (n - 1) * mp.factorial(n) * mp.sqrt(mp.pi) / (n * mp.hermite(n - 1, v)) ** 2 for v in nodes]
        return nodes, wts


def primitive_mp(a, A, la, b, B, lb, q, C, lp, order=None, dps=30, gl_degree=7, raw=False):
    """`primitive` in mpmath: scalar loops, Gauss-Hermite with just enough nodes, mpmath's Gauss-Legendre nodes (3 * 2^(gl_degree-1) per segment)."""
    import mpmath as mp
    from mpmath.calculus.quadrature import GaussLegendre
    with mp.workdps(dps):
        f = lambda v: mp.mpf(float(v))
        a, b, q = f(a), f(b), f(q)
        A, B, C = ([f(v) for v in X] for X in (A, B, C))
        p = a + b
        AB = [A[d] - B[d] for d in range(3)]
        PA = [-(b / p) * AB[d] for d in range(3)]; PB = [(a / p) * AB[d] for d in range(3)]
        Cp = [C[d] - (A[d] + (b / p) * (B[d] - A[d])) for d in range(3)]
        rho = p * q / (p + q)
        T = rho * sum(v * v for v in Cp)
        z, wz = _gh_mp((la + lb + lp) // 2 + 1, dps)
        xw = GaussLegendre(mp.mp).calc_nodes(gl_degree, mp.mp.prec)
        cut = min(mp.mpf(1), 8 / mp.sqrt(T)) if T > 64 else mp.mpf(1)
        nodes = [(cut * (x + 1) / 2, cut * w / 2) for x, w in xw]
        if cut < 1:
            nodes += [(cut + (1 - cut) * (x + 1) / 2, (1 - cut) * w / 2) for x, w in xw]
        comps = [cart_components(l) for l in (la, lb, lp)]
        out = [[[mp.mpf(0) for _ in comps[2]] for _ in comps[1]] for _ in comps[0]]
        for t, wt in nodes:
            t2 = t * t
            s11sq = (1 - t2) / p + t2 / (p + q)
            S11 = mp.sqrt(s11sq); S21 = (t2 / (p + q)) / S11; S22 = mp.sqrt((1 - t2) / (p * q * s11sq))
            G = []
            for d in range(3):
                g = [[[mp.mpf(0)] * (lp + 1) for _ in range(lb + 1)] for _ in range(la + 1)]
                for z1, w1 in zip(z, wz):
                    y1 = Cp[d] * q / (p + q) * t2 + S11 * z1
                    hk = [sum(w2 * (-Cp[d] * p / (p + q) * t2 + S21 * z1 + S22 * z2) ** k for z2, w2 in zip(z, wz)) for k in range(lp + 1)]
                    for i in range(la + 1):
                        for j in range(lb + 1):
                            fij = w1 * (y1 + PA[d]) ** i * (y1 + PB[d]) ** j
                            for k in range(lp + 1):
                                g[i][j][k] += fij * hk[k]
                G.append(g)
            e = wt * mp.exp(-T * t2)
            for ia, ca in enumerate(comps[0]):
                for ib, cb in enumerate(comps[1]):
                    for ic, cc in enumerate(comps[2]):
                        out[ia][ib][ic] += e * G[0][ca[0]][cb[0]][cc[0]] * G[1][ca[1]][cb[1]][cc[1]] * G[2][ca[2]][cb[2]][cc[2]]
        pref = 2 / mp.sqrt(mp.pi) * mp.exp(-(a * b / p) * sum(v * v for v in AB)) * mp.sqrt(rho) * (p * q) ** mp.mpf(-1.5)
        if raw:
            return [[[pref * v for v in r] for r in m] for m in out]
        return np.array([[[float(pref * v) for v in r] for r in m] for m in out])


def block_mp(mol, aux, i, j, k, dps=30):
    """block3c (j None: block2c of the shells i, k of `aux`) for SINGLE primitives entirely in mpmath, the Cartesian -> spherical step included: for far
    f / g blocks, which are 10^-5 ... 10^-6 of the Cartesian integrals they are formed from, so that extended precision leaves only 1e-13 of the block."""
    import mpmath as mp
    with mp.workdps(dps):
        two = j is None
        la, A, exa, coa, ca, sa = _shell(aux if two else mol, i)
        lb, B, exb, cob, cb, sb = (0, A, np.zeros(1), np.ones((1, 1)), None, None) if two else _shell(mol, j)
        lp, Cc, exc, coc, cc, sc = _shell(aux, k)
        assert len(exa) == len(exb) == len(exc) == 1
        V = primitive_mp(exa[0], A, la, exb[0], B, lb, exc[0], Cc, lp, dps=dps, raw=True)
        Ma = harmonic((aux if two else mol).c2s[ca, sa], la, mp)
        Mb = mp.matrix([[1]]) if two else harmonic(mol.c2s[cb, sb], lb, mp)
        Mc = harmonic(aux.c2s[cc, sc], lp, mp)
        na, nb, nc = len(V), len(V[0]), len(V[0][0])
        V = [[[V[x][y][z] * mp.mpf(float(coa[x, 0])) * mp.mpf(float(cob[y, 0])) * mp.mpf(float(coc[z, 0])) for z in range(nc)] for y in range(nb)] for x in range(na)]
        V = [[[sum(V[x][y][z] * Mc[z, m] for z in range(nc)) for m in range(Mc.cols)] for y in range(nb)] for x in range(na)]
        V = [[[sum(V[x][y][m] * Mb[y, n] for y in range(nb)) for m in range(Mc.cols)] for n in range(Mb.cols)] for x in range(na)]
        V = [[[sum(V[x][n][m] * Ma[x, o] for x in range(na)) for m in range(Mc.cols)] for n in range(Mb.cols)] for o in range(Ma.cols)]
        out = np.array([[[float(v) for v in r] for r in m] for m in V])
        return out[:, 0, :] if two else out


@functools.lru_cache(None)
def _boys_mp_row(x, m_max):
    import mpmath as mp
    with mp.workdps(40):
        if x == 0:
            return tuple(float(mp.mpf(1) / (2 * m + 1)) for m in range(m_max + 1))
        xm = mp.mpf(x)
        return tuple(float(mp.gammainc(m + mp.mpf(0.5), 0, xm) / (2 * xm ** (m + mp.mpf(0.5)))) for m in range(m_max + 1))


def boys_mp(xs, m_max=12):
    """F_m(x) = gamma(m + 1/2, x) / (2 x^(m + 1/2)), m = 0..m_max, rounded from 40 digits: (len(xs), m_max + 1)."""
    return np.array([_boys_mp_row(float(x), m_max) for x in xs])
