"""Shared cases of the DF-integral tests (test_gpu_int3c.py on the device, test_int3c_hostlogic.py through the scalar twin): every check takes the
library handle, so the same comparison runs on both -- against the host integral source, and against the independent quadrature reference of
int3c_reference.py, whose cases and blocks are stored in golden/int3c_ref.npz (written by golden/make_golden_int3c_ref.py)."""
import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np

from quemb_amd import _lib
from quemb_amd import integrals as I

BAR = 1e-10                      # max |dev - host| <= BAR * max(1, max |host|): ten times inside the 1e-9 of the DF transform comparisons
BAR_REL = 1e-10                  # max |dev - ref| <= BAR_REL * max |ref| per block against the quadrature reference: BAR, relative to the block itself
MIN_BLOCK = 1e-8                 # every reference block has an element at least this large (asserted when the fixture is written)
BOYS_SWITCH = 35.0               # series below, asymptotic form from here on (int3c_core.h)
BOYS_POINTS = [0.0, 1e-12, 1e-6, 0.1, 1.0, 5.0, 15.0, 25.0, 30.0, 35.0, 60.0, 200.0, BOYS_SWITCH * (1 - 1e-9), BOYS_SWITCH * (1 + 1e-9), 34.5, 35.5,
               745.0, 1e3, 1e4, 1e5]            # from 745 on exp(-x) underflows
BOYS_M_MAX = 12                  # dev_boys accepts 0..12; the kernels use 0..8
REF_NPZ = Path(__file__).resolve().parent / "golden" / "int3c_ref.npz"

# 2-3 primitives per shell, exponents of ordinary valence / fitting functions
_EXP = {0: ([2.3, 0.7, 0.25], [0.3, 0.5, 0.4]), 1: ([1.6, 0.45], [0.55, 0.6]), 2: ([1.2, 0.5, 0.3], [0.4, 0.5, 0.3]), 3: ([1.4, 0.6], [0.6, 0.5]),
        4: ([1.1, 0.55], [0.5, 0.6])}
GEOMETRIES = {      # centres of shell a, shell b, auxiliary shell (Bohr): distinct, non-collinear, off the axes; one atom; a = b != P
    "three": ((0.13, -0.21, 0.32), (0.94, 0.55, -0.47), (-0.38, 0.81, 0.66)),
    "one": ((0.13, -0.21, 0.32),) * 3,
    "ab": ((0.13, -0.21, 0.32), (0.13, -0.21, 0.32), (-0.38, 0.81, 0.66)),
}
CLASSES = [(la, lb, lp) for lb in range(3) for la in range(lb + 1) for lp in range(5)]


def close(dev, host):
    d = float(np.abs(np.asarray(dev) - np.asarray(host)).max()) if np.size(host) else 0.0
    return d, d <= BAR * max(1.0, float(np.abs(host).max()) if np.size(host) else 0.0)


@functools.lru_cache(None)
def boys_xs():
    return np.concatenate([BOYS_POINTS, np.random.default_rng(20261017).uniform(0.0, 60.0, 200)])


@functools.lru_cache(None)
def boys_reference():
    """F_0..F_12 at boys_xs() from mpmath's incomplete gamma function at 40 digits (computed once per process)."""
    from int3c_reference import boys_mp
    return boys_mp(boys_xs(), BOYS_M_MAX)


def check_boys(lib, on_device, m_max=8):
    """One call with this m_max: the series of the x < 35 branch starts at F[m_max], the upward recursion of the other branch ends there."""
    xs = boys_xs()
    out = np.empty((len(xs), m_max + 1))
    if on_device:
        dx = _lib.DeviceBuffer.from_numpy(xs, lib=lib); do = _lib.DeviceBuffer(out.size, lib=lib)
        _lib.check(lib.qemb_op_boys(m_max, len(xs), dx.ptr, do.ptr), "qemb_op_boys", lib)
        out = do.numpy(out.shape)
        dx.free(); do.free()
    else:
        _lib.check(lib.qemb_op_boys(m_max, len(xs), xs.ctypes.data, out.ctypes.data), "qemb_op_boys", lib)
    rel = np.abs(out / boys_reference()[:, : m_max + 1] - 1.0)
    i, m = np.unravel_index(rel.argmax(), rel.shape)
    print(f"boys m_max = {m_max}: max relative deviation {rel.max():.2e} at x = {xs[i]!r}, m = {m}")
    assert rel.max() <= 1e-13, rel.max(axis=1)
    assert (out[0] == 1.0 / (2 * np.arange(m_max + 1) + 1)).all()


def class_block(lib, la, lb, lp, geom):
    """(device block, host block) of one angular class on explicit shells."""
    ra, rb, rp = GEOMETRIES[geom]
    mol = I.Mole([("H", ra), ("C", rb)], basis={"H": [(la, *_EXP[la])], "C": [(lb, *_EXP[lb])]}, unit="Bohr")
    aux = I.Mole([("H", rp)], basis={"H": [(lp, *_EXP[lp])]}, unit="Bohr")
    na, nb, npp = 2 * la + 1, 2 * lb + 1, 2 * lp + 1
    host = I.aux_e2(mol, aux)[:na, na:, :]
    out = np.empty((na, nb, npp))
    rec = [mol.bfs[mol.shells[0][5]], mol.bfs[mol.shells[1][5]], aux.bfs[0]]
    tab = I.c2s_table()
    _lib.check(lib.qemb_op_int3c_class(la, lb, lp, C.addressof(rec[0]), C.addressof(rec[1]), C.addressof(rec[2]), tab.ctypes.data, out.ctypes.data),
               "qemb_op_int3c_class", lib)
    return out, host


def check_class(lib, la, lb, lp):
    for geom in GEOMETRIES:
        dev, host = class_block(lib, la, lb, lp, geom)
        d, ok = close(dev, host)
        print(f"class ({la},{lb}|{lp}) {geom}: max |dev - host| = {d:.2e}, max |host| = {np.abs(host).max():.3e}")
        assert ok, (la, lb, lp, geom, d)
        assert np.abs(host).max() > 0 or geom == "one"      # (on one centre most classes vanish by parity: the zeros must come out as zeros too)


# ---- the quadrature reference (golden/int3c_ref.npz) ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def reference():
    """(cases, arrays): the case definitions (name, family, kind "3c" / "2c", shells a, b, p as {l, ex, co, r}) and the npz with "ref/<name>" blocks."""
    z = np.load(REF_NPZ)
    return json.loads(str(z["cases"])), z


def reference_cases(kind=None, family=None):
    return [c for c in reference()[0] if kind in (None, c["kind"]) and family in (None, c["family"])]


def reference_families():
    return sorted({c["family"] for c in reference()[0]})


def case_moles(case):
    """3c: (mol with the shells a, b; aux with the shell p).  2c: (aux with the shells a, p,)."""
    sh = lambda k: (case[k]["l"], case[k]["ex"], case[k]["co"])
    if case["kind"] == "2c":
        return (I.Mole([("H", case["a"]["r"]), ("C", case["p"]["r"])], basis={"H": [sh("a")], "C": [sh("p")]}, unit="Bohr"),)
    return (I.Mole([("H", case["a"]["r"]), ("C", case["b"]["r"])], basis={"H": [sh("a")], "C": [sh("b")]}, unit="Bohr"),
            I.Mole([("H", case["p"]["r"])], basis={"H": [sh("p")]}, unit="Bohr"))


def case_block(case, lib=None):
    """The block of a case from the host source (lib None), or from `lib`: qemb_op_int3c_class in the case's shell order, qemb_int2c2e for the metric."""
    na = 2 * case["a"]["l"] + 1
    if case["kind"] == "2c":
        aux, = case_moles(case)
        return (I.int2c2e(aux) if lib is None else I.int2c2e(aux, backend="hip", lib=lib))[:na, na:]
    mol, aux = case_moles(case)
    if lib is None:
        return I.aux_e2(mol, aux)[:na, na:, :]
    la, lb, lp = (case[k]["l"] for k in "abp")
    out = np.empty((na, 2 * lb + 1, 2 * lp + 1))
    rec = [mol.bfs[mol.shells[0][5]], mol.bfs[mol.shells[1][5]], aux.bfs[0]]
    tab = I.c2s_table()
    _lib.check(lib.qemb_op_int3c_class(la, lb, lp, C.addressof(rec[0]), C.addressof(rec[1]), C.addressof(rec[2]), tab.ctypes.data, out.ctypes.data),
               "qemb_op_int3c_class", lib)
    return out


def rel_dev(got, ref):
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def check_class_against_reference(lib, case):
    """lib None: the host source."""
    ref = reference()[1]["ref/" + case["name"]]
    got = case_block(case, lib)
    assert got.shape == ref.shape and np.abs(ref).max() >= MIN_BLOCK
    d = rel_dev(got, ref)
    print(f"{case['name']}: max |got - ref| = {d:.2e} of max |ref| = {np.abs(ref).max():.3e}")
    assert d <= BAR_REL, (case["name"], d)
    return d


def h3_layout_case():
    """H3 / cc-pVDZ, N = 15, with an auxiliary basis whose shell counts per l (17, 13, 5) are coprime to the shell-pair counts per class (21, 18, 6) and no
    multiple of a workgroup: the etb basis on the first two atoms and 1 s, 1 p, 3 d shells on the third (the etb basis on all three would give 24, 18, 3,
    which share factors with the pair counts).  naux = 81."""
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(3)], basis="cc-pvdz")
    etb = I.etb_auxbasis(mol)["H"]
    third = [(0, [0.9], [1.0]), (1, [1.3], [1.0]), (2, [0.7], [1.0]), (2, [1.454], [1.0]), (2, [2.9], [1.0])]
    aux = I.Mole([("H", mol.atom[0][1]), ("H", mol.atom[1][1]), ("C", mol.atom[2][1])], basis={"H": etb, "C": third}, unit="Bohr")
    npair = {}                                                   # shell pairs I >= J per class (larger l, smaller l): what qemb_int3c2e launches
    for i in range(mol.nbas):
        for j in range(i + 1):
            key = tuple(sorted((mol.shells[i][1], mol.shells[j][1]), reverse=True))
            npair[key] = npair.get(key, 0) + 1
    assert npair == {(1, 1): 6, (1, 0): 18, (0, 0): 21} and mol.nao == 15 and aux.nao == 81
    naux_sh = [sum(1 for s in aux.shells if s[1] == l) for l in range(3)]
    assert naux_sh == [17, 13, 5]
    assert all(np.gcd(a, b) == 1 and a % 64 and b % 64 for a in npair.values() for b in naux_sh)
    return mol, aux


def check_layouts_on(lib):
    """The three dense layouts from `lib` agree bit for bit, and the pqL one meets the reference block by block."""
    mol, aux = h3_layout_case()
    pql = I.aux_e2(mol, aux, backend="hip", lib=lib)
    lpq = I._int3c_hip(mol, aux, "Lpq", lib=lib)
    packed = I._int3c_hip(mol, aux, "packed", lib=lib)
    assert (lpq == pql.transpose(2, 0, 1)).all()
    il = np.tril_indices(mol.nao)
    assert (packed == lpq[:, il[0], il[1]]).all()
    check_h3_against_reference(pql)


def check_h3_against_reference(j3):
    """Every (shell pair | auxiliary shell) block of the H3 case that the fixture holds (largest element >= MIN_BLOCK), to BAR_REL of the block."""
    mol, aux = h3_layout_case()
    z = reference()[1]
    ref, blocks = z["h3/ref"], z["h3/blocks"]
    il = np.tril_indices(mol.nao)
    got = j3[il[0], il[1]]
    assert got.shape == ref.shape
    lo, la = mol.ao_loc_nr(), aux.ao_loc_nr()
    pair_shell = np.searchsorted(lo, il[0], side="right") - 1, np.searchsorted(lo, il[1], side="right") - 1
    worst = 0.0
    for i, j, k in blocks:
        rows = (pair_shell[0] == i) & (pair_shell[1] == j)
        r = ref[rows, la[k]: la[k + 1]]
        assert np.abs(r).max() >= MIN_BLOCK
        d = rel_dev(got[rows, la[k]: la[k + 1]], r)
        worst = max(worst, d)
        assert d <= BAR_REL, (i, j, k, d)
    print(f"H3 / cc-pVDZ: {len(blocks)} blocks, worst deviation {worst:.2e} of a block's largest element")
    assert len(blocks) == 1451                     # of 1575: the others hold no element of 3e-8


def h8(basis="sto-3g", n=8):
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(n)], basis=basis)
    return mol, I.make_auxmol(mol, "etb")


def octane12():
    from helpers import GOLDEN
    mol = I.Mole(I.read_xyz(GOLDEN / "octane.xyz")[:12])
    return mol, I.make_auxmol(mol, "etb")


def check_molecule(lib, mol, aux, name):
    host3, host2 = I.aux_e2(mol, aux), I.int2c2e(aux)
    dev3, dev2 = I.aux_e2(mol, aux, backend="hip", lib=lib), I.int2c2e(aux, backend="hip", lib=lib)
    d3, ok3 = close(dev3, host3); d2, ok2 = close(dev2, host2)
    print(f"{name}: N = {mol.nao}, naux = {aux.nao}, aux l up to {max(s[1] for s in aux.shells)}: (mu nu|P) {d3:.2e}, (P|Q) {d2:.2e}")
    assert ok3 and ok2, (d3, d2)
    assert (dev3 == dev3.transpose(1, 0, 2)).all() and (dev2 == dev2.T).all()                       # the mirror is a copy
    again3, again2 = I.aux_e2(mol, aux, backend="hip", lib=lib), I.int2c2e(aux, backend="hip", lib=lib)
    assert again3.tobytes() == dev3.tobytes() and again2.tobytes() == dev2.tobytes()               # every element written once: the same bits
    return host3, host2


def check_pair_list(lib):
    """The stored pairs of the H8 semi-sparse case (H8 / cc-pVDZ, N = 40, so that shells hold several functions and a pair inside one shell can be
    off-diagonal; AO screening at 1e-2 so that the list is a proper subset of the triangle), plus explicit corner pairs."""
    from quemb_amd import eri_sparse_DF as sdf
    mol, aux = h8("cc-pvdz", 8)
    assert mol.natm == 8 and mol.nao == 40
    S_abs = sdf.approx_S_abs(mol, lib=lib)
    t = sdf.get_sparse_P_mu_nu(mol, aux, sdf._get_AO_per_AO(S_abs, 1e-2, None, lib=lib), fill=False)
    pairs = sorted(((mu, nu) for mu, r in enumerate(t.exch_reachable_unique) for nu in r), key=lambda pq: t.offsets[(pq[0] * (pq[0] + 1)) // 2 + pq[1]])
    assert 0 < len(pairs) < mol.nao * (mol.nao + 1) // 2, "the list must be screened"
    last = (mol.nao - 1, mol.nao - 1)
    inside = (mol.nao - 1, mol.nao - 3)                       # two different p functions of the last shell
    assert last in pairs
    pairs = pairs + [inside, (2, 9), (9, 2)] if inside not in pairs else pairs + [(2, 9), (9, 2)]
    host = I.aux_e2_pairs(mol, aux, pairs)
    dev = I.aux_e2_pairs(mol, aux, pairs, backend="hip", lib=lib)
    d, ok = close(dev, host)
    print(f"pair list: {len(pairs)} pairs of {mol.nao * (mol.nao + 1) // 2}, max |dev - host| = {d:.2e}")
    assert ok, d
    assert (dev[-1] == dev[-2]).all()


def check_inplace_fill(lib, mol, aux, alloc_stats):
    from quemb_amd import eri_transform as et
    rng = np.random.default_rng(7)
    TA = np.linalg.qr(rng.standard_normal((mol.nao, mol.nao)))[0][:, : min(6, mol.nao)]
    df_h = et.DFContext(j2c=I.int2c2e(aux), lib=lib)
    df_h.set_ints(I.aux_e2(mol, aux), mol.nao, "pqL")
    ref = df_h.transform(TA)
    df_h.free()
    df = et.DFContext.empty(lib=lib)
    if alloc_stats:
        n, nf, ms, gb = C.c_longlong(), C.c_longlong(), C.c_double(), C.c_double()
        lib.qemb_trim_all()
        lib.qemb_alloc_stats(C.byref(n), C.byref(nf), C.byref(ms), C.byref(gb), 1)
    df.set_ints_from_mol(mol, aux)
    if alloc_stats:
        lib.qemb_alloc_stats(C.byref(n), C.byref(nf), C.byref(ms), C.byref(gb), 0)
        tensor = 8.0 * aux.nao * mol.nao * mol.nao
        got = gb.value * 1e9                                   # qemb_alloc_stats reports bytes * 1e-9
        # what a fill without staging allocates: the tensor, three naux^2 images (the metric that becomes its factor, the inverse, the work space of the
        # inversion), the shells and index lists (256 KiB is generous for them) and 25 % of the tensor for the allocator's rounding.  A staging copy of
        # the tensor would add `tensor` bytes: 2 x tensor + the rest, well above the bound when the tensor dominates the naux^2 terms (both figures are printed)
        bound = 1.25 * tensor + 8.0 * 3 * aux.nao ** 2 + 2 ** 18
        print(f"in-place fill: {got:.0f} bytes allocated for a tensor of {tensor:.0f}, bound {bound:.0f}, with a staging copy at least {2 * tensor + 8.0 * 3 * aux.nao ** 2:.0f}")
        assert got <= bound
    out = df.transform(TA)
    df.free()
    rel = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"in-place fill: transform deviates by {rel:.2e} relative")
    assert rel <= 1e-9


def be_energies(lib, int_transform, solver, integral_backend, **kw):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
    mf = be_energies.mf = getattr(be_energies, "mf", None) or I.RHF(mol)
    if mf.e_tot is None:
        mf.kernel()
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    be = BE(mf, fobj, lib=lib, distribute=False, int_transform=int_transform, auxbasis="etb", integral_backend=integral_backend, **kw)
    e, comp = be.oneshot(solver=solver)[:2]
    return np.array([e, *comp])


def check_end_to_end(lib, int_transform, solver, **kw):
    host = be_energies(lib, int_transform, solver, "host", **kw)
    dev = be_energies(lib, int_transform, solver, "hip", **kw)
    print(f"{int_transform} {solver}: E_corr host {host[0]:.12f} hip {dev[0]:.12f}, pieces differ by {np.abs(host - dev).max():.2e}")
    assert np.abs(host - dev).max() <= 1e-9, (host, dev)
