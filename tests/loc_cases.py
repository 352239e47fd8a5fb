"""Shared cases and checks of the localisation tests (csrc/loc_ops.hip: joint diagonalisation by Jacobi sweeps).  test_gpu_loc.py runs them on the device,
test_loc_hostlogic.py on the hostcheck mock; tests/loc_numpy.py is the independent twin.

The variants' limits (csrc/loc_core.h): the stack is kept in LDS when (K + 1) m^2 <= 7168 doubles (K = 3: m <= 42, K = 1: m <= 59, K = 7: m <= 29), otherwise one
launch pair per round with a workgroup per slab of 16 matrices.  The sizes below sit on and around those limits and across one slab (K = 16, 17, 33).

Bars (all from the issue that introduced the kernels):
  always      ||U^T U - 1||_2 <= 1e-13 m;  max |Q_out - U^T Q_0 U| <= 1e-12 max_k ||Q_0^k||_2;  f >= f(Q_0) (to the rounding of the two sums);  two calls, same bits
  K = 1       the diagonal equals eigvalsh to 1e-12 of the spectral norm
  commuting   off-diagonal <= 1e-10 ||Q||_F, U = V up to order and sign
  random      f = the twin's to 1e-10 relative;  max_pq |sum_k a_k (Q_pp - Q_qq)| <= 1e-8 sum_k ||Q^k||_F^2 (theta < 1e-10 and |R sin 4 theta| <= 4 theta sum ||Q||^2: a
              25 x margin);  sum d^2 >= sum a^2 - 1e-10 sum_k ||Q^k||_F^2 for every pair
A fully random Gaussian stack has no joint structure and the sweeps converge linearly, slowly as m grows; it is kept at m = 8: K = 3 in LDS, and K = 113 (seven
slabs and one matrix) on the launch-per-round variant.  The upper limit of that variant, m = 512 (and 511: the bye), runs one sweep through the always-checks on the device.  The larger random cases are a
commuting stack plus a symmetric Gaussian perturbation of 5 % per element: they do not commute, and converge in a few dozen sweeps."""
import ctypes as C

import numpy as np

import loc_numpy as ln

LDS_STACK_DOUBLES = 7168
QEMB_ERR_ARG, QEMB_ERR_ALLOC, QEMB_ERR_NUMERIC = -1, -2, -5


def in_lds(K, m):
    return K >= 1 and (K + 1) * m * m <= LDS_STACK_DOUBLES


def random_stack(K, m, seed):
    r = np.random.default_rng(seed)
    A = r.standard_normal((K, m, m))
    return A + A.transpose(0, 2, 1)


def commuting_stack(K, m, seed):
    r = np.random.default_rng(seed)
    V = np.linalg.qr(r.standard_normal((m, m)))[0]
    D = r.standard_normal((K, m))
    return np.array([(V * d) @ V.T for d in D]), V


def perturbed_stack(K, m, seed, eps=0.05):
    A, _ = commuting_stack(K, m, seed)
    return A + eps * random_stack(K, m, seed + 1)


# (K, m): tiny sizes (m = 3: the bye), the limits of the LDS variant and one past them, K across the slab of the rounds variant
SIZES = [(3, 1), (3, 2), (3, 3), (3, 4), (1, 6), (7, 5), (3, 41), (3, 42), (3, 43), (1, 58), (1, 59), (1, 60), (7, 29), (7, 30), (16, 21), (17, 21), (33, 15)]
RANDOM = [("gauss", 3, 8), ("gauss", 113, 8)] + [("perturbed", K, m) for K, m in SIZES if m >= 3]


def build(kind, K, m):
    seed = 1000 * K + m
    return random_stack(K, m, seed) if kind == "gauss" else perturbed_stack(K, m, seed)


def run(lib, Q0, **kw):
    from quemb_amd import lo
    return lo.joint_diag(Q0, lib=lib, **kw)


def check_always(lib, Q0, **kw):
    Q, U, info = run(lib, Q0, **kw)
    K, m = Q0.shape[0], Q0.shape[1]
    assert info["in_lds"] == in_lds(K, m)
    assert np.isfinite(Q).all() and np.isfinite(U).all()
    orth = np.linalg.norm(U.T @ U - np.eye(m), 2) if m else 0.0
    assert orth <= 1e-13 * max(m, 1), orth
    scale = max([np.linalg.norm(q, 2) for q in Q0], default=0.0)
    back = np.abs(Q - U.T @ Q0 @ U).max() if Q0.size else 0.0      # (matrix products: a three-operand einsum walks m^4 terms)
    assert back <= 1e-12 * scale, (back, scale)
    n2 = float((Q0 ** 2).sum())
    assert info["f"] >= ln.functional(Q0) - 1e-13 * n2
    assert abs(info["f"] - ln.functional(Q)) <= 1e-13 * n2
    Q2, U2, info2 = run(lib, Q0, **kw)
    assert np.array_equal(Q, Q2) and np.array_equal(U, U2) and info == info2, "two calls must give the same bits"
    return Q, U, info


def check_eigen(lib, m, seed):
    A = random_stack(1, m, seed)
    Q, U, info = check_always(lib, A)
    assert info["converged"]
    w = np.linalg.eigvalsh(A[0])
    err = np.abs(np.sort(np.diag(Q[0])) - w).max()
    assert err <= 1e-12 * np.abs(w).max(), err
    return info


def check_commuting(lib, K, m, seed):
    A, V = commuting_stack(K, m, seed)
    Q, U, info = check_always(lib, A)
    assert info["converged"]
    off = Q.copy()
    off[:, np.arange(m), np.arange(m)] = 0.0
    assert np.abs(off).max() <= 1e-10 * np.sqrt((A ** 2).sum())
    P = np.abs(U.T @ V)      # a permutation matrix: U = V up to order and sign
    assert np.abs(np.sort(P, axis=1)[:, -1] - 1.0).max() <= 1e-10 and np.abs(np.sort(P, axis=1)[:, :-1]).max() <= 1e-8
    assert sorted(P.argmax(axis=1)) == list(range(m))
    return info


def check_random(lib, kind, K, m):
    A = build(kind, K, m)
    Q, U, info = check_always(lib, A)
    Qt, Ut, sw_t, f_t, cv_t = ln.joint_diag(A)
    assert cv_t and info["converged"], (sw_t, info)
    print(f"{kind} K={K} m={m}: sweeps {info['sweeps']} (twin {sw_t}), f {info['f']:.15g} (twin {f_t:.15g})")
    assert abs(info["f"] - f_t) <= 1e-10 * abs(f_t)
    n2 = float((A ** 2).sum())
    g, h = ln.stationarity(Q)
    assert g <= 1e-8 * n2, g / n2
    assert h >= -1e-10 * n2, h / n2
    return info


def check_trivial(lib):
    for K, m in [(0, 4), (3, 1), (3, 0), (0, 0)]:
        A = random_stack(K, m, 5) if K and m else np.zeros((K, m, m))
        Q, U, info = run(lib, A)
        assert np.array_equal(U, np.eye(m)) and np.array_equal(Q, A) and info["sweeps"] == 0 and info["converged"]
        assert info["f"] == ln.functional(A)


def check_no_sweeps(lib):
    """max_sweeps = 0: nothing is rotated, f is that of the input, not converged"""
    for K, m in [(3, 6), (3, 43)]:
        A = random_stack(K, m, 6)
        Q, U, info = run(lib, A, max_sweeps=0)
        assert np.array_equal(U, np.eye(m)) and np.array_equal(Q, A) and info["sweeps"] == 0 and not info["converged"]
        assert abs(info["f"] - ln.functional(A)) <= 1e-13 * (A ** 2).sum()


def check_max_sweeps(lib):
    A = random_stack(3, 13, 7)      # linear convergence: three sweeps are not enough
    Q, U, info = check_always(lib, A, max_sweeps=3)
    assert info["sweeps"] == 3 and not info["converged"]


def check_diagonal_stack(lib):
    """an exactly diagonal stack is at its maximum: every pair's sums are below the noise floor (exactly zero), nothing is turned, one sweep, U = 1 to the bit.
    With degenerate diagonals (d = 0 and a = 0) atan2(0, 0) must not produce a turn either."""
    for K, m in [(3, 7), (3, 43)]:
        r = np.random.default_rng(K + m)
        D = r.standard_normal((K, m))
        D[:, 1] = D[:, 0]      # a degenerate pair
        A = np.array([np.diag(d) for d in D])
        Q, U, info = check_always(lib, A)
        assert info["sweeps"] == 1 and info["converged"] and np.array_equal(U, np.eye(m)) and np.array_equal(Q, A)


def check_rounds_limit(lib, m):
    """the launch-per-round variant at its largest m (512; 511 has the bye): one sweep, every always-check; the pair tables of the rotation kernel are full"""
    r = np.random.default_rng(m)
    A = np.diag(r.standard_normal(m))[None] + 1e-3 * random_stack(1, m, m + 1)
    Q, U, info = check_always(lib, A, max_sweeps=1)
    assert info["sweeps"] == 1 and not info["in_lds"]
    assert info["f"] > ln.functional(A)      # the sweep did turn: the diagonal gained weight


def check_guard(lib):
    """the guard, with a faked limit: refused before anything is allocated, naming K and m; lifted again, the same call passes"""
    from quemb_amd._lib import QembError
    A = perturbed_stack(3, 10, 8)
    need = C.c_int64()
    assert lib.qemb_op_joint_diag_bytes(3, 10, C.byref(need), None) == 0 and need.value >= 8 * (3 * 100 + 2 * 100)
    try:
        assert lib.qemb_op_joint_diag_mem_limit(need.value - 1) == 0
        try:
            run(lib, A)
            raise AssertionError("the guard did not refuse")
        except QembError as e:
            assert e.status == QEMB_ERR_ALLOC and "K = 3" in str(e) and "m = 10" in str(e)
        assert lib.qemb_op_joint_diag_mem_limit(need.value) == 0
        run(lib, A)
    finally:
        lib.qemb_op_joint_diag_mem_limit(-1)
    run(lib, A)


def check_refusals(lib):
    from quemb_amd._lib import DeviceBuffer
    b = DeviceBuffer(16, lib=lib)
    try:
        sw, f, cv = C.c_int(), C.c_double(), C.c_int()
        args = (C.byref(sw), C.byref(f), C.byref(cv))
        assert lib.qemb_op_joint_diag(1, 513, b.ptr, b.ptr, 1e-10, 1, *args) == -6      # beyond the rounds variant's m: QEMB_ERR_UNSUPPORTED naming the limit
        assert "m = 513" in lib.qemb_last_error().decode() and "m <= 512" in lib.qemb_last_error().decode()
        assert lib.qemb_op_joint_diag(-1, 2, b.ptr, b.ptr, 1e-10, 1, *args) == QEMB_ERR_ARG
        assert lib.qemb_op_joint_diag(1, 2, None, b.ptr, 1e-10, 1, *args) == QEMB_ERR_ARG
        assert lib.qemb_op_joint_diag(1, 2, b.ptr, b.ptr, -1.0, 1, *args) == QEMB_ERR_ARG
        assert lib.qemb_op_joint_diag(1, 2, b.ptr, b.ptr, 1e-10, -1, *args) == QEMB_ERR_ARG
    finally:
        b.free()
    from quemb_amd._lib import QembError
    for K, m in [(3, 5), (3, 43)]:
        A = random_stack(K, m, 9)
        A[1, 2, 2] = np.nan
        try:
            run(lib, A, max_sweeps=2)
            raise AssertionError("a NaN in the stack was not refused")
        except QembError as e:
            assert e.status == QEMB_ERR_NUMERIC


# ------------------------------------------------------------------------------------------------ dipole integrals
def check_dipole_class(la, lb, backend="host", lib=None):
    """every block of the three-shell molecules of one pair class (int1e_cases) against the Gauss-Hermite quadrature, symmetry to the bit, the origin shift"""
    import int1e_cases as ic
    import int4c_cases as c4
    from quemb_amd import integrals as I
    origin = (0.3, -0.2, 0.7)
    for prims in ((c4._EXP3, c4._EXP1, c4._EXP3), (c4._EXP1, c4._EXP3, c4._EXP1)):
        mol = ic.class_molecule(la, lb, prims)
        r = I.dipole(mol, origin, backend=backend, lib=lib)
        ref = ln.dipole_quadrature(mol, origin)
        na, nb = 2 * la + 1, 2 * lb + 1
        edges = [0, na, na + nb, na + 2 * nb]
        for i in range(3):
            for j in range(3):
                blk = (slice(None), slice(edges[i], edges[i + 1]), slice(edges[j], edges[j + 1]))
                top = np.abs(ref[blk]).max()
                if top <= 1e-12 * np.abs(ref).max():      # a block that parity makes zero (d with s on one centre) holds rounding only: it has no scale of its own
                    top = np.abs(ref).max()
                assert np.abs(r[blk] - ref[blk]).max() <= 1e-10 * top, (la, lb, i, j)
        assert np.array_equal(r, r.transpose(0, 2, 1))
        host = I.dipole(mol, origin)
        assert np.abs(r - host).max() <= 1e-13 * np.abs(host).max()
        S = mol.one_electron()[0]
        r0 = I.dipole(mol, backend=backend, lib=lib)
        assert np.abs(r - (r0 - np.asarray(origin)[:, None, None] * S)).max() <= 1e-13 * max(1.0, np.abs(r0).max())


def check_dipole_backends(lib):
    """host source and device kernel agree to 1e-13 (of the largest element) on the systems the localisation tests use; an f shell is refused as in qemb_int1e"""
    from quemb_amd import integrals as I
    from quemb_amd._lib import QembError
    for name in ("h8", "h8-dz", "octane"):
        mol = system(name)
        for origin in ((0.0, 0.0, 0.0), (0.4, 1.3, -2.2)):
            h, d = I.dipole(mol, origin), I.dipole(mol, origin, backend="hip", lib=lib)
            assert np.abs(h - d).max() <= 1e-13 * np.abs(h).max(), (name, np.abs(h - d).max())
            assert np.array_equal(d, d.transpose(0, 2, 1)) and np.array_equal(d, I.dipole(mol, origin, backend="hip", lib=lib))
    f = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]}, unit="Bohr")
    try:
        I.dipole(f, backend="hip", lib=lib)
        raise AssertionError("an f shell was not refused")
    except QembError as e:
        assert e.status == -6


# ------------------------------------------------------------------------------------------------ get_loc
def system(name):
    from helpers import GOLDEN
    from quemb_amd.integrals import Mole
    h8 = [["H", (0.0, 0.0, float(i))] for i in range(8)]
    return {"h8": lambda: Mole(h8), "h8-dz": lambda: Mole(h8, basis="cc-pvdz"), "octane": lambda: Mole(GOLDEN / "octane.xyz")}[name]()


def lowdin_columns(mol):
    """an orthonormal set to localise that needs no mean field: the first half of the symmetrically orthogonalised AOs, mixed by a fixed orthogonal matrix"""
    S = mol.intor("int1e_ovlp")
    w, v = np.linalg.eigh(S)
    W = (v / np.sqrt(w)) @ v.T
    m = mol.nao // 2
    R = np.linalg.qr(np.random.default_rng(mol.nao).standard_normal((m, m)))[0]
    return S, W[:, :m] @ R


_CONTEXTS = {}


def dense_context(lib, name, kind="cholesky"):
    """a dense 3-index context of a system, made once per library: the Cholesky factor of the AO integrals (tol 1e-8) or the tensor fitted in an even-tempered basis"""
    from quemb_amd import eri_transform as et
    from quemb_amd import integrals as I
    key = (id(lib), name, kind)
    if key not in _CONTEXTS:
        mol = system(name)
        if kind == "cholesky":
            _CONTEXTS[key] = et.DFContext.from_cholesky(mol, tol=1e-8, lib=lib)
        else:
            auxmol = I.make_auxmol(mol, "etb")
            j2c, pqL = I.int2c2e(auxmol), I.aux_e2(mol, auxmol)
            df = et.DFContext(j2c=j2c, lib=lib)
            df.set_ints(pqL, mol.nao, "pqL")
            df.host_ints = (pqL, j2c)      # for the checks: the fitted integrals formed again on the host
            _CONTEXTS[key] = df
    return _CONTEXTS[key]


def context_tensor(lib, df):
    out, ident = np.empty((df.naux, df.nao, df.nao)), C.c_int()
    assert lib.qemb_op_df_get_ints(df.h, out.ctypes.data, C.byref(ident)) == 0
    return out, bool(ident.value)


def check_get_loc(lib, name, method, pop_method=None, df=None):
    import warnings
    from quemb_amd import lo
    mol = system(name)
    S, C0 = lowdin_columns(mol)
    m = C0.shape[1]
    st = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # not converged in max_sweeps is a valid answer: the checks below hold for any rotation
        Cl = lo.get_loc(mol, C0, method, pop_method=pop_method, lib=lib, stats=st, df=df)
    assert np.abs(Cl.T @ S @ Cl - np.eye(m)).max() <= 1e-12
    assert np.abs(Cl @ Cl.T - C0 @ C0.T).max() <= 1e-12
    if method == "cholesky":
        return st
    print(f"get_loc {name} {method} {pop_method}: K = {st['K']}, m = {st['m']}, sweeps {st['sweeps']}, f {st['f_before']:.6f} -> {st['f_after']:.6f}, converged {st['converged']}")
    assert st["f_after"] >= st["f_before"] * (1.0 - 1e-13)
    if method == "PM":
        Q = lo.population_stack(mol, Cl, S, pop_method or "lowdin")
        assert Q.shape[0] == mol.natm and np.abs(Q.sum(axis=0) - np.eye(m)).max() <= 1e-12
        assert abs(np.einsum("kii,kii->", Q, Q) - st["f_after"]) <= 1e-10 * st["f_after"]
    elif method == "ER":
        assert st["K"] == df.naux
        B, identity = context_tensor(lib, df)
        if identity:      # a Cholesky factor is the 3-index factor itself: sum_i (ii|ii) = sum_P sum_i (C^T B^P C)_ii^2, formed here on the host
            for Cx, key in ((C0, "f_before"), (Cl, "f_after")):
                d = np.einsum("mi,Pmn,ni->Pi", Cx, B, Cx)
                assert abs((d ** 2).sum() - st[key]) <= 1e-10 * st[key], (key, (d ** 2).sum(), st[key])
        else:             # a fitted tensor: (ii|ii) = d^T J^-1 d with d_P = (P|ii), formed here on the host from the same 3- and 2-centre integrals
            pqL, j2c = df.host_ints
            for Cx, key in ((C0, "f_before"), (Cl, "f_after")):
                d = np.einsum("mi,mnP,ni->Pi", Cx, pqL, Cx)
                ref = float(np.einsum("Pi,Pi->", d, np.linalg.solve(j2c, d)))
                assert abs(ref - st[key]) <= 1e-10 * ref, (key, ref, st[key])
    else:
        from quemb_amd import integrals
        for origin in ((0.0, 0.0, 0.0), (1.0, -2.0, 3.0)):      # the functional's differences do not depend on the origin
            r = integrals.dipole(mol, origin)
            d0 = np.array([np.diag(C0.T @ x @ C0) for x in r])
            d1 = np.array([np.diag(Cl.T @ x @ Cl) for x in r])
            spread_gain = (d1 ** 2).sum() - (d0 ** 2).sum()
            assert abs(spread_gain - (st["f_after"] - st["f_before"])) <= 1e-9 * st["f_after"]
    return st


def check_get_loc_refusals(lib):
    import pytest
    from quemb_amd import lo
    mol = system("h8")
    S, C0 = lowdin_columns(mol)
    with pytest.raises(ValueError, match="df"):
        lo.get_loc(mol, C0, "ER", lib=lib)
    with pytest.raises(ValueError, match="df"):
        lo.get_loc(mol, C0, lib=lib)                                  # the default method is ER
    with pytest.raises(ValueError, match="df"):
        lo.get_loc(system("h8-dz"), lowdin_columns(system("h8-dz"))[1], "ER", df=dense_context(lib, "h8"), lib=lib)      # a context of another basis
    with pytest.raises(NotImplementedError, match="meta-lowdin"):
        lo.get_loc(mol, C0, "PM", pop_method="meta-lowdin", lib=lib)
    with pytest.raises(NotImplementedError):
        lo.get_loc(mol, C0, "boys", init_guess=np.eye(4), lib=lib)
    with pytest.raises(NotImplementedError):
        lo.get_loc(mol, C0, "IAO", lib=lib)
    with pytest.raises(ValueError):
        lo.get_loc(mol, C0, "boys", pop_method="lowdin", lib=lib)
    for g in (None, "atomic"):
        assert np.array_equal(lo.get_loc(mol, C0, "cholesky", init_guess=g, lib=lib), lo.cholesky_mos(C0))
    with pytest.warns(RuntimeWarning, match="sweeps"):
        lo.get_loc(mol, C0, "boys", max_sweeps=1, lib=lib)


def check_cholesky_mos():
    from quemb_amd import lo
    r = np.random.default_rng(4)
    C0 = np.linalg.qr(r.standard_normal((9, 4)))[0]
    L = lo.cholesky_mos(C0)
    assert np.abs(L @ L.T - C0 @ C0.T).max() <= 1e-14
    piv = [int(np.abs(L[:, j]).argmax()) for j in range(4)]
    assert len(set(piv)) == 4 and all(np.abs(L[piv[j], j + 1:]).max(initial=0.0) <= 1e-14 for j in range(4))      # lower trapezoidal in pivot order
    E = np.zeros((6, 3)); E[[1, 4, 5], [0, 1, 2]] = 1.0      # equal diagonals: ties go to the lowest index
    assert np.array_equal(lo.cholesky_mos(E @ np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0.0]])), E)


# ------------------------------------------------------------------------------------------------ BE
import functools

FRAG_KEYS = {"h8": "test_autogen_h_linear_be2", "octane": "test_autogen_octane_be2"}


@functools.lru_cache(maxsize=None)
def mean_field(name):
    from quemb_amd.integrals import RHF
    mf = RHF(system(name))
    mf.kernel()
    return mf


def tight(lib):
    from quemb_amd.fragsolver import default_opts
    return default_opts(lib, cc_conv_tol=1e-12, cc_conv_tol_normt=1e-10, scf_conv_tol=1e-13, scf_conv_tol_grad=1e-9)


def make_be(lib, name, frozen=False, **kw):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mf = mean_field(name)
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", FRAG_KEYS[name])
    if frozen:
        fobj = fobj.freeze_core(mf.mol)
    return BE(mf, fobj, distribute=False, lib=lib, solver_opts=tight(lib), **kw)


_REFERENCE = {}


CHOLESKY_ROUTE = dict(int_transform="cholesky-hip", integral_backend="hip")


def reference_run(lib, name, **route):
    """the unlocalised run of a system on a route, computed once per library: the driver, and its one-shot CCSD and MP2 correlation energies"""
    key = (id(lib), name, tuple(sorted(route.items())))
    if key not in _REFERENCE:
        be = make_be(lib, name, **route)
        _REFERENCE[key] = (be, {s: be.oneshot(solver=s)[0] for s in ("CCSD", "MP2")})
    return _REFERENCE[key]


def check_be_bath(lib, name, method):
    """a bath rotation is a unitary change inside the embedding space: fragment columns untouched to the bit, the bath's span, HF-in-HF and the one-shot energies kept"""
    route = CHOLESKY_ROUTE if method == "ER" else {}      # ER reads the factor of the Cholesky route; its reference is the unlocalised run on the same route
    be0, e0 = reference_run(lib, name, **route)
    be1 = make_be(lib, name, lo_bath_post_schmidt=method, **route)
    S = be0.S
    moved = 0.0
    for f0, f1 in zip(be0.Fobjs, be1.Fobjs):
        assert f0.n_f == f1.n_f and f0.TA.shape == f1.TA.shape
        assert np.array_equal(f0.TA[:, :f0.n_f], f1.TA[:, :f1.n_f])
        B0, B1 = f0.TA[:, f0.n_f:], f1.TA[:, f1.n_f:]
        assert np.abs(B0 @ B0.T - B1 @ B1.T).max() <= 1e-12
        assert np.abs(B1.T @ S @ B1 - np.eye(B1.shape[1])).max() <= 1e-12
        moved = max(moved, np.abs(B0 - B1).max())
    assert moved > 1e-3, "the bath was not rotated at all"
    assert abs(be1.ebe_hf - be0.ebe_hf) <= 1e-10, be1.ebe_hf - be0.ebe_hf
    for s in ("CCSD", "MP2"):
        e1 = be1.oneshot(solver=s)[0]
        print(f"{name} bath {method} {s}: E_corr {e1:.12f}, unlocalised {e0[s]:.12f}, difference {e1 - e0[s]:.2e}")
        assert abs(e1 - e0[s]) <= 1e-9, (s, e1 - e0[s])
    return be1


def check_be_lo_method(lib, name, method, frozen=False, hf_bar=1e-7, **kw):
    """lo_method boys / PM / ER: W orthonormal, HF-in-HF within the bar of the existing HF-in-HF cases (1e-7), finite energies, the same on a second run.  kw: further
    BE keywords (pop_method="mulliken": a PM run that really rotates the Loewdin orbitals; the Cholesky route for ER, whose HF-in-HF bar the caller sets from cd_tol)"""
    be = make_be(lib, name, frozen=frozen, lo_method=method, **kw)
    n = be.W.shape[1]
    assert n == be.S.shape[0] - be.ncore
    assert np.abs(be.W.T @ be.S @ be.W - np.eye(n)).max() <= 1e-12
    assert abs(be.ebe_hf - mean_field(name).e_tot) <= hf_bar, be.ebe_hf - mean_field(name).e_tot
    e = be.oneshot(solver="MP2")[0]
    assert np.isfinite(e) and e < 0.0
    be2 = make_be(lib, name, frozen=frozen, lo_method=method, **kw)
    assert np.array_equal(be.W, be2.W) and be2.ebe_hf == be.ebe_hf and be2.oneshot(solver="MP2")[0] == e
    print(f"{name} lo_method {method} frozen {frozen}: HF-in-HF {be.ebe_hf - mean_field(name).e_tot:.2e}, MP2 E_corr {e:.10f}, sweeps {be.lo_stats['W']['sweeps']}")
    return be


def check_be_defaults(lib, name):
    """the new keywords at their defaults change nothing: bit-identical to a run that does not pass them"""
    be0 = make_be(lib, name)      # a fresh driver each: a one-shot energy is compared with one from the same starting state
    be1 = make_be(lib, name, lo_method="lowdin", pop_method=None, init_guess="atomic", lo_bath_post_schmidt=None)
    assert np.array_equal(be0.W, be1.W) and be0.ebe_hf == be1.ebe_hf
    for f0, f1 in zip(be0.Fobjs, be1.Fobjs):
        assert np.array_equal(f0.TA, f1.TA) and np.array_equal(f0.fock, f1.fock)
    assert be1.oneshot(solver="MP2")[0] == be0.oneshot(solver="MP2")[0]


def check_be_refusals(lib):
    import pytest
    with pytest.raises(NotImplementedError):
        make_be(lib, "h8", lo_method="IAO")
    for kw in (dict(lo_method="ER"), dict(lo_bath_post_schmidt="ER"), dict(lo_method="ER", int_transform="int-direct-DF-hip")):
        with pytest.raises(ValueError, match="dense 3-index context"):      # the in-core route, and a DF route without an auxiliary basis, hold none
            make_be(lib, "h8", **kw)
    with pytest.raises(ValueError):
        make_be(lib, "h8", lo_bath_post_schmidt="lowdin")
