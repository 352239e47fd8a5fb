"""NumPy / Python-integer twin of the heat-bath selected CI behind solver="SCI-hip" (test infrastructure).

A determinant is a pair (alpha, beta) of Python integers, bit p set = fragment MO p occupied; alpha creators stand to the left of the beta ones, the creators of one
spin in ascending order: the order and sign convention of tests/fci_numpy.py, on which nothing here depends.  `hij` is the Slater-Condon rule on two
determinants; the Hamiltonian of a selected space is a dict of keys over connected pairs, diagonalised by numpy.linalg.eigh.  The selection rule:
  V0 = {HF}; a determinant a outside V joins when |H_ai c_i| >= eps for at least one i in V (singles and doubles, each product on its own), together with its
  spin-swapped partner; stop when a round adds nothing; results from the last diagonalisation.
`select` also reports margin = min |crit / eps - 1| over every candidate with crit = |H_ai c_i| > 0: how far the nearest decision was from the threshold."""
import numpy as np


def popcount(x):
    return bin(x).count("1")


def bits(x):
    out = []
    p = 0
    while x:
        if x & 1:
            out.append(p)
        x >>= 1
        p += 1
    return out


def _between(s, i, a):
    """parity of the occupied orbitals of s strictly between i and a"""
    lo, hi = (i, a) if i < a else (a, i)
    return popcount(s & (((1 << hi) - 1) & ~((1 << (lo + 1)) - 1))) & 1


def _single(h, V, s, other, i, a):
    """<a+ i S, O|H|S, O>: s the string that is excited (i -> a), other the string of the other spin"""
    x = h[a, i]
    for j in bits(s):
        x += V[a, i, j, j] - V[a, j, j, i]
    for j in bits(other):
        x += V[a, i, j, j]
    return -x if _between(s, i, a) else x


def hij(h, V, A, B):
    """<A|H|B> for A = (alpha, beta), B = (alpha, beta)"""
    da, db = A[0] ^ B[0], A[1] ^ B[1]
    na, nb = popcount(da) // 2, popcount(db) // 2
    if na + nb > 2:
        return 0.0
    if na + nb == 0:
        oa, ob = bits(B[0]), bits(B[1])
        e = sum(h[i, i] for i in oa) + sum(h[i, i] for i in ob)
        for occ in (oa, ob):
            for i in occ:
                for j in occ:
                    e += 0.5 * (V[i, i, j, j] - V[i, j, j, i])
        for i in oa:
            for j in ob:
                e += V[i, i, j, j]
        return float(e)
    if na + nb == 1:
        s, t, other = (B[0], A[0], B[1]) if na else (B[1], A[1], B[0])
        (i,), (a,) = bits(s & ~t), bits(t & ~s)
        return float(_single(h, V, s, other, i, a))
    if na == 1:      # one excitation in each spin
        (i,), (a,) = bits(B[0] & ~A[0]), bits(A[0] & ~B[0])
        (j,), (b,) = bits(B[1] & ~A[1]), bits(A[1] & ~B[1])
        sg = _between(B[0], i, a) ^ _between(B[1], j, b)
        return float(-V[a, i, b, j] if sg else V[a, i, b, j])
    s, t = (B[0], A[0]) if na == 2 else (B[1], A[1])
    (i, j), (a, b) = bits(s & ~t), bits(t & ~s)
    sg = _between(s, i, a) ^ _between(s ^ (1 << i) ^ (1 << a), j, b)
    x = V[a, i, b, j] - V[a, j, b, i]
    return float(-x if sg else x)


def connected(det, n):
    """every determinant one or two excitations away from det"""
    a, b = det
    full = (1 << n) - 1

    def singles(s):
        return [s ^ (1 << i) ^ (1 << p) for i in bits(s) for p in bits(full & ~s)]

    def doubles(s):
        occ, vir = bits(s), bits(full & ~s)
        return [s ^ (1 << occ[x]) ^ (1 << occ[y]) ^ (1 << vir[p]) ^ (1 << vir[q])
                for x in range(len(occ)) for y in range(x + 1, len(occ)) for p in range(len(vir)) for q in range(p + 1, len(vir))]

    sa, sb = singles(a), singles(b)
    out = [(x, b) for x in sa] + [(a, y) for y in sb]
    out += [(x, b) for x in doubles(a)] + [(a, y) for y in doubles(b)]
    out += [(x, y) for x in sa for y in sb]
    return out


def candidates(h, V, n, dets, c, eps):
    """(the sorted determinants outside `dets` that pass the rule, spin partners included; margin)"""
    inside = set(dets)
    new = set()
    margin = np.inf
    for d, ci in zip(dets, c):
        if ci == 0.0:
            continue
        for a in connected(d, n):
            if a in inside:
                continue
            crit = abs(hij(h, V, a, d) * ci)
            if crit > 0.0:
                margin = min(margin, abs(crit / eps - 1.0))
            if crit >= eps:
                new.add(a)
                new.add((a[1], a[0]))
    return sorted(new - inside), margin


_BYTE_BITS = np.array([popcount(x) for x in range(256)], dtype=np.int64)


def bit_count(x):
    """popcount of every uint64 word: numpy.bitwise_count (numpy >= 2.0), else a byte table"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.int64)
    return _BYTE_BITS[x.view(np.uint8).reshape(x.shape + (8,))].sum(axis=-1)


def differing_bits(words_a, words_b):
    """popcount(a ^ b) for every pair of two uint64 arrays, (len(a), len(b))"""
    x = np.asarray(words_a, dtype=np.uint64)[:, None] ^ np.asarray(words_b, dtype=np.uint64)[None, :]
    return bit_count(x)


def near_pairs(dets):
    """boolean (N, N): the pairs of `dets` at most two excitations apart (the pairs the Hamiltonian can connect)"""
    a = np.array([d[0] for d in dets], dtype=np.uint64)
    b = np.array([d[1] for d in dets], dtype=np.uint64)
    return differing_bits(a, a) + differing_bits(b, b) <= 4


def hamiltonian(h, V, dets, rows=None):
    """dense matrix of the dict of keys over the pairs of `dets` at most two excitations apart (found with numpy; each element is hij); rows: those rows only"""
    N = len(dets)
    H = np.zeros((N, N))
    near = near_pairs(dets)
    for x in (range(N) if rows is None else rows):
        for y in np.nonzero(near[x])[0]:
            if rows is not None or y >= x:
                H[x, y] = hij(h, V, dets[x], dets[int(y)])
                if rows is None:
                    H[y, x] = H[x, y]
    return H


# ---------------------------------------------------------------- the same rules on arrays of pairs (numpy on uint64 words), pinned to hij by the tests
_ONE = np.uint64(1)


def _lowest(x):
    """index of the lowest set bit of every (non-zero) word: the isolated bit is a power of two, which float64 holds exactly"""
    x = np.asarray(x, dtype=np.uint64)
    return np.log2((x & (~x + _ONE)).astype(np.float64)).astype(np.int64)


def _between_many(s, i, a):
    lo, hi = np.minimum(i, a).astype(np.uint64), np.maximum(i, a).astype(np.uint64)
    mask = ((_ONE << hi) - _ONE) & ~((_ONE << (lo + _ONE)) - _ONE)
    return bit_count(s & mask) & 1


def _occupations(s, n):
    return ((np.asarray(s, dtype=np.uint64)[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & _ONE).astype(np.float64)


def hij_many(h, V, Aa, Ab, Ba, Bb):
    """<(Aa, Ab)|H|(Ba, Bb)> for arrays of determinants: hij, class by class"""
    Aa, Ab, Ba, Bb = (np.asarray(x, dtype=np.uint64) for x in (Aa, Ab, Ba, Bb))
    n = h.shape[0]
    ar = np.arange(n)
    na = bit_count(Aa ^ Ba) // 2
    nb = bit_count(Ab ^ Bb) // 2
    out = np.zeros(Aa.shape[0])
    Jm, Km = np.einsum("iijj->ij", V), np.einsum("ijji->ij", V)
    k = np.nonzero(na + nb == 0)[0]
    if k.size:
        oa, ob = _occupations(Ba[k], n), _occupations(Bb[k], n)
        out[k] = (oa + ob) @ np.diag(h) + 0.5 * (np.einsum("ki,ij,kj->k", oa, Jm - Km, oa) + np.einsum("ki,ij,kj->k", ob, Jm - Km, ob)) + np.einsum("ki,ij,kj->k", oa, Jm, ob)
    for spin in (0, 1):      # one excitation, in the alpha or in the beta string
        k = np.nonzero((na == 1) & (nb == 0) if spin == 0 else (na == 0) & (nb == 1))[0]
        if k.size:
            s, t, other = (Ba[k], Aa[k], Bb[k]) if spin == 0 else (Bb[k], Ab[k], Ba[k])
            i, a = _lowest(s & ~t), _lowest(t & ~s)
            Jai = V[a[:, None], i[:, None], ar[None, :], ar[None, :]]
            Kai = V[a[:, None], ar[None, :], ar[None, :], i[:, None]]
            x = h[a, i] + (_occupations(s, n) * (Jai - Kai)).sum(axis=1) + (_occupations(other, n) * Jai).sum(axis=1)
            out[k] = np.where(_between_many(s, i, a) == 1, -x, x)
    k = np.nonzero((na == 1) & (nb == 1))[0]
    if k.size:
        i, a = _lowest(Ba[k] & ~Aa[k]), _lowest(Aa[k] & ~Ba[k])
        j, b = _lowest(Bb[k] & ~Ab[k]), _lowest(Ab[k] & ~Bb[k])
        x = V[a, i, b, j]
        out[k] = np.where(_between_many(Ba[k], i, a) ^ _between_many(Bb[k], j, b) == 1, -x, x)
    for spin in (0, 1):      # two excitations in one string
        k = np.nonzero((na == 2) & (nb == 0) if spin == 0 else (na == 0) & (nb == 2))[0]
        if k.size:
            s, t = (Ba[k], Aa[k]) if spin == 0 else (Bb[k], Ab[k])
            holes, parts = s & ~t, t & ~s
            i, a = _lowest(holes), _lowest(parts)
            j, b = _lowest(holes & (holes - _ONE)), _lowest(parts & (parts - _ONE))
            left = s ^ (_ONE << i.astype(np.uint64)) ^ (_ONE << a.astype(np.uint64))
            x = V[a, i, b, j] - V[a, j, b, i]
            out[k] = np.where(_between_many(s, i, a) ^ _between_many(left, j, b) == 1, -x, x)
    return out


def hamiltonian_many(h, V, dets):
    """the matrix of `hamiltonian`, every connected pair evaluated by hij_many"""
    a = np.array([d[0] for d in dets], dtype=np.uint64)
    b = np.array([d[1] for d in dets], dtype=np.uint64)
    N = len(dets)
    H = np.zeros((N, N))
    for r0 in range(0, N, 512):      # blocks of rows bound the temporaries
        x, y = np.nonzero(differing_bits(a[r0:r0 + 512], a) + differing_bits(b[r0:r0 + 512], b) <= 4)
        H[x + r0, y] = hij_many(h, V, a[x + r0], b[x + r0], a[y], b[y])
    return H


def _targets(s, n):
    """(single excitations, double excitations) of one string as uint64 arrays"""
    occ = np.array(bits(s), dtype=np.uint64)
    vir = np.array(bits(((1 << n) - 1) & ~s), dtype=np.uint64)
    s = np.uint64(s)
    single = (s ^ ((_ONE << occ)[:, None] ^ (_ONE << vir)[None, :])).reshape(-1)
    io, iv = np.triu_indices(len(occ), 1), np.triu_indices(len(vir), 1)
    oo = (_ONE << occ[io[0]]) ^ (_ONE << occ[io[1]])
    vv = (_ONE << vir[iv[0]]) ^ (_ONE << vir[iv[1]])
    return single, (s ^ (oo[:, None] ^ vv[None, :])).reshape(-1)


def candidates_many(h, V, n, dets, c, eps):
    """`candidates` with hij_many.  A determinant with |c_i| 2 max|V| < eps / 2 skips its double excitations: no double-excitation element exceeds 2 max|V|, so none
    of them can pass, and each of them is at least eps / 2 away from passing (the margin is capped at 1/2 accordingly)."""
    inside = set(dets)
    bound = 2.0 * np.abs(V).max()
    new, margin = set(), np.inf
    for d, ci in zip(dets, c):
        if ci == 0.0:
            continue
        sa, da = _targets(d[0], n)
        sb, db = _targets(d[1], n)
        A, B = np.uint64(d[0]), np.uint64(d[1])
        ta = [sa, np.full(sb.shape, A)]
        tb = [np.full(sa.shape, B), sb]
        if abs(ci) * bound >= 0.5 * eps:
            ta += [da, np.full(db.shape, A), np.repeat(sa, len(sb))]
            tb += [np.full(da.shape, B), db, np.tile(sb, len(sa))]
        else:
            margin = min(margin, 0.5)
        ta, tb = np.concatenate(ta), np.concatenate(tb)
        crit = np.abs(hij_many(h, V, ta, tb, np.full(ta.shape, A), np.full(ta.shape, B)) * ci)
        near = np.abs(crit / eps - 1.0)
        near[crit == 0.0] = np.inf
        for k in np.argsort(near):      # the nearest decision about a determinant outside the space
            if not near[k] < margin:
                break
            if (int(ta[k]), int(tb[k])) not in inside:
                margin = float(near[k])
                break
        for k in np.nonzero(crit >= eps)[0]:
            x, y = int(ta[k]), int(tb[k])
            if (x, y) not in inside:
                new.add((x, y)); new.add((y, x))
    return sorted(new - inside), margin


def fix_sign(c):
    c = np.asarray(c, dtype=float)
    c = c / np.linalg.norm(c)
    return c if c[int(np.argmax(np.abs(c)))] > 0 else -c


def select(h, V, o, eps, max_round=30):
    """the rule from the HF determinant: dict(dets, c, e, rounds, margin, converged, history); history[r] = (dets, c, joined) of round r"""
    n = h.shape[0]
    hf = (1 << o) - 1
    dets, c = [(hf, hf)], np.ones(1)
    e = hij(h, V, dets[0], dets[0])
    margin, history, converged, rounds = np.inf, [], False, 0
    for _ in range(max_round):
        new, m = candidates(h, V, n, dets, c, eps)
        margin = min(margin, m)
        history.append((list(dets), c.copy(), list(new)))
        if not new:
            converged = True
            break
        rounds += 1
        dets = sorted(dets + new)
        w, U = np.linalg.eigh(hamiltonian(h, V, dets))
        e, c = float(w[0]), fix_sign(U[:, 0])
    return dict(dets=dets, c=c, e=e, rounds=rounds, margin=margin, converged=converged, history=history)


def full_vector(dets, c, n, o):
    """the vector on the full (ns, ns) space of tests/fci_numpy.py, zeros outside the selected space"""
    st = [s for s in range(1 << n) if popcount(s) == o]
    pos = {s: k for k, s in enumerate(st)}
    out = np.zeros((len(st), len(st)))
    for (a, b), x in zip(dets, c):
        out[pos[a], pos[b]] = x
    return out


def rdm12(dets, c, n):
    """(dm1, dm2) of the selected vector from pairs of determinants: dm1[p,q] = <q+ p>, dm2[p,q,r,s] = <p+ r+ s q>, both summed over spin"""
    dm1 = np.zeros((n, n))
    dm2 = np.zeros((n, n, n, n))
    N = len(dets)
    for x in range(N):          # row I
        for y in range(N):      # column J: <I| ... |J> c_I c_J
            A, B = dets[x], dets[y]
            na, nb = popcount(A[0] ^ B[0]) // 2, popcount(A[1] ^ B[1]) // 2
            if na + nb > 2:
                continue
            w = c[x] * c[y]
            if na + nb == 0:
                occ = (bits(B[0]), bits(B[1]))
                for s1 in (0, 1):
                    for q in occ[s1]:
                        dm1[q, q] += w
                        for s2 in (0, 1):
                            for s in occ[s2]:
                                if s1 == s2 and q == s:
                                    continue
                                dm2[q, q, s, s] += w
                                if s1 == s2:
                                    dm2[s, q, q, s] -= w
            elif na + nb == 1:
                sp = 0 if na else 1
                s, t = B[sp], A[sp]
                (i,), (a,) = bits(s & ~t), bits(t & ~s)
                pw = -w if _between(s, i, a) else w
                dm1[i, a] += pw
                for s2 in (0, 1):
                    for k in bits(B[s2]):
                        if s2 == sp and k == i:
                            continue
                        dm2[a, i, k, k] += pw
                        dm2[k, k, a, i] += pw
                        if s2 == sp:
                            dm2[a, k, k, i] -= pw
                            dm2[k, i, a, k] -= pw
            elif na == 1:
                (i,), (a,) = bits(B[0] & ~A[0]), bits(A[0] & ~B[0])
                (j,), (b,) = bits(B[1] & ~A[1]), bits(A[1] & ~B[1])
                pw = -w if _between(B[0], i, a) ^ _between(B[1], j, b) else w
                dm2[a, i, b, j] += pw
                dm2[b, j, a, i] += pw
            else:
                s, t = (B[0], A[0]) if na == 2 else (B[1], A[1])
                (i, j), (a, b) = bits(s & ~t), bits(t & ~s)
                pw = -w if _between(s, i, a) ^ _between(s ^ (1 << i) ^ (1 << a), j, b) else w
                dm2[a, i, b, j] += pw
                dm2[b, j, a, i] += pw
                dm2[a, j, b, i] -= pw
                dm2[b, i, a, j] -= pw
    return 0.5 * (dm1 + dm1.T), dm2
