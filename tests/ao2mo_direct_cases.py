"""Shared cases of the integral-direct AO -> fragment transform (test_gpu_ao2mo_direct.py on the device, test_ao2mo_direct_hostlogic.py through the scalar twin):
every check takes the library handle, so the same comparison runs on both.  References: the stored 4-fold packed integrals of the same kernels
(integrals.eri(mol, 4, backend="hip"), itself held to the host source by int4c_cases) for the tiles and the identity transform -- compared with ==, the tile form
stores the same values -- and the stored route AOEri.from_basis(...).transform(TA) for the transformed blocks, to BAR of the block's largest element."""
import ctypes as C
import functools

import numpy as np

import int4c_cases as c4
import jk_direct_cases as cj
from quemb_amd import _lib
from quemb_amd import eri_transform as et
from quemb_amd import integrals as I

BAR = c4.BAR                     # 1e-10 of the block's largest element: the project's bar for the integrals themselves
TILE_BAR = 1e-12                 # of the largest element: two tile sizes sum the same products in another grouping (rounding alone, far above 1e-16 x sqrt(terms))
BE_BAR = c4.BE_BAR               # 1e-9 Eh


def molecules():
    m = dict(c4.molecules())
    m["h8_far"] = lambda: I.Mole([["H", (0.0, 0.0, 2.5 * i)] for i in range(8)])      # the stretched chain of int4c_cases.check_screening
    return m


@functools.lru_cache(None)
def mole(name):
    return molecules()[name]()


# ---- the slabs, restated: whole canonical shell pairs (I >= J, I outer), at most tile_pairs AO pairs, a larger shell pair alone -------------------------------
def pair_size(mol, I_, J_):
    na, nb = 2 * mol.shells[I_][1] + 1, 2 * mol.shells[J_][1] + 1
    return na * (na + 1) // 2 if I_ == J_ else na * nb


def slabs(mol, tile_pairs):
    out, cur, rows = [], [], 0
    for I_ in range(mol.nbas):
        for J_ in range(I_ + 1):
            sz = pair_size(mol, I_, J_)
            if cur and rows + sz > tile_pairs:
                out.append(cur)
                cur, rows = [], 0
            cur.append((I_, J_))
            rows += sz
    out.append(cur)
    return out


def ao_pairs(mol, pairs):
    """the AO pair indices ij = mu (mu + 1) / 2 + nu of the rows of a tile side: list order, inside a shell pair increasing"""
    ij = []
    for I_, J_ in pairs:
        a0, b0 = mol.shells[I_][4], mol.shells[J_][4]
        for a in range(2 * mol.shells[I_][1] + 1):
            for b in range(a + 1 if I_ == J_ else 2 * mol.shells[J_][1] + 1):
                mu, nu = a0 + a, b0 + b
                ij.append(mu * (mu + 1) // 2 + nu)
    return np.array(ij)


def pair_class(mol, pr):
    la, lb = sorted((mol.shells[pr[0]][1], mol.shells[pr[1]][1]), reverse=True)
    return la * (la + 1) // 2 + lb


def dev_tile(basis, mol, R, S, thresh=0.0):
    r, s = np.ascontiguousarray(R, dtype=np.int32), np.ascontiguousarray(S, dtype=np.int32)
    out = np.full((len(ao_pairs(mol, R)), len(ao_pairs(mol, S))), np.nan)
    _lib.check(basis.lib.qemb_op_int4c_tile(basis.h, r.ctypes.data, len(r), s.ctypes.data, len(s), float(thresh), out.ctypes.data), "qemb_op_int4c_tile", basis.lib)
    return out


_STORED = {}


def stored_s4(lib, name):
    """the stored 4-fold packed integrals of a molecule on this library, computed once and shared (left unchanged by the checks)"""
    if (id(lib), name) not in _STORED:
        e = I.eri(mole(name), 4, backend="hip", lib=lib)
        e.setflags(write=False)
        _STORED[(id(lib), name)] = (lib, e)
    return _STORED[(id(lib), name)][1]


# ---- 1. tiles are the stored integrals --------------------------------------------------------------------------------------------------------------------
def check_tiles(lib, name, tile_pairs):
    mol, E = mole(name), stored_s4(lib, name)
    npair = mol.nao * (mol.nao + 1) // 2
    sl = slabs(mol, tile_pairs)
    rows = [ao_pairs(mol, s) for s in sl]
    assert sorted(np.concatenate(rows)) == list(range(npair))      # every AO pair in exactly one slab
    cover = np.zeros((npair, npair), dtype=np.int64)
    same_slab = np.zeros((npair, npair), dtype=np.int64)
    n_transposed = n_big = 0
    b = I.DeviceBasis(mol, lib)
    try:
        for r, R in enumerate(sl):
            big = len(R) == 1 and len(rows[r]) > tile_pairs
            n_big += big
            assert len(rows[r]) <= tile_pairs or big
            for s in range(r + 1):
                S = sl[s]
                t = dev_tile(b, mol, R, S)
                assert (t == E[np.ix_(rows[r], rows[s])]).all(), (name, tile_pairs, r, s)
                cover[np.ix_(rows[r], rows[s])] += 1
                if r == s:
                    same_slab[np.ix_(rows[r], rows[r])] = 1
                elif max(pair_class(mol, p) for p in S) > min(pair_class(mol, p) for p in R):
                    n_transposed += 1      # a quartet whose higher-class pair sits in the column set: computed as (S|R), stored transposed
    finally:
        b.free()
    assert (cover + cover.T - same_slab == 1).all()      # the union of the tiles R >= S: every (ij, kl) once per triangle
    print(f"{name}, tile_pairs = {tile_pairs}: {len(sl)} slabs, {len(sl) * (len(sl) + 1) // 2} tiles equal the stored integrals; {n_transposed} with a transposed "
          f"class, {n_big} shell pairs larger than the tile")
    return n_transposed, n_big


# ---- 2. identity transform --------------------------------------------------------------------------------------------------------------------------------
def check_identity(lib, name, tiles=(7, 40)):
    mol, E = mole(name), stored_s4(lib, name)
    b = I.DeviceBasis(mol, lib)
    try:
        for t in tiles:
            G, = b.ao2mo([np.eye(mol.nao)], tile_pairs=t)
            assert (G == E).all(), (name, t, float(np.abs(G - E).max()))      # only zeros are added and ones multiplied
            assert b.eri_stats()[1] == 0
    finally:
        b.free()


# ---- 3. against the stored route --------------------------------------------------------------------------------------------------------------------------
def random_ta(N, n, seed):
    return np.random.default_rng(seed).standard_normal((N, n)) / np.sqrt(N)


_REF = {}


def stored_transform(lib, name, key, TA):
    """AOEri.from_basis(...).transform(TA): computed once per (library, molecule, key) and shared"""
    k = (id(lib), name, key)
    if k not in _REF:
        b = I.DeviceBasis(mole(name), lib)
        try:
            ao = et.AOEri.from_basis(b)
            try:
                ref = ao.transform(TA)
            finally:
                ao.free()
        finally:
            b.free()
        ref.setflags(write=False)
        _REF[k] = (lib, ref)
    return _REF[k][1]


def rel(a, ref):
    return float(np.abs(a - ref).max()) / float(np.abs(ref).max())


def compare(label, G, ref):
    d = rel(G, ref)
    print(f"{label}: max |direct - stored| = {d:.2e} of max |stored| = {np.abs(ref).max():.3e}")
    assert G.shape == ref.shape and d <= BAR, (label, d)
    assert (G == G.T).all(), label      # G = A + A^T
    return d


def check_random(lib, name, tile_pairs=40):
    mol = mole(name)
    b = I.DeviceBasis(mol, lib)
    try:
        for n in (5, mol.nao - 1):
            TA = random_ta(mol.nao, n, 100 + n)
            G, = b.ao2mo([TA], tile_pairs=tile_pairs)
            compare(f"{name} random TA, n = {n}, tile_pairs = {tile_pairs}", G, stored_transform(lib, name, n, TA))
    finally:
        b.free()


_H8_TAS = {}


def h8_be2_tas(lib):
    """the embedding coefficients of the BE2 fragments of H8 / STO-3G"""
    if id(lib) not in _H8_TAS:
        _, be = c4.be_energies(lib, "MP2", True)
        _H8_TAS[id(lib)] = (lib, [np.array(f.TA) for f in be.Fobjs])
    return _H8_TAS[id(lib)][1]


def check_h8_fragments(lib, tile_pairs=7):
    tas = h8_be2_tas(lib)
    b = I.DeviceBasis(mole("h8_sto3g"), lib)
    try:
        Gs = b.ao2mo(tas, tile_pairs=tile_pairs)
    finally:
        b.free()
    for k, (G, TA) in enumerate(zip(Gs, tas)):
        compare(f"H8 BE2 fragment {k} (n = {TA.shape[1]})", G, stored_transform(lib, "h8_sto3g", ("be2", k), TA))


# ---- 4. many fragments, one pass --------------------------------------------------------------------------------------------------------------------------
def check_many(lib, name="spd3", tile_pairs=40):
    mol = mole(name)
    tas = [random_ta(mol.nao, n, 200 + n) for n in (3, 5, mol.nao - 1)]
    nsp = mol.nbas * (mol.nbas + 1) // 2
    b = I.DeviceBasis(mol, lib)
    try:
        joint = b.ao2mo(tas, tile_pairs=tile_pairs)
        nq_joint, _ = b.eri_stats()
        single = []
        for t in tas:
            single.append(b.ao2mo([t], tile_pairs=tile_pairs)[0])
            assert b.eri_stats()[0] == nq_joint
    finally:
        b.free()
    assert nq_joint == nsp * (nsp + 1) // 2      # every canonical shell quartet once, not once per fragment
    for g, s in zip(joint, single):
        assert g.tobytes() == s.tobytes()


# ---- 5. tile-size independence and reproducibility ----------------------------------------------------------------------------------------------------------
def check_tile_independence(lib, name="spd3", tiles=(7, 40)):
    mol = mole(name)
    TA = random_ta(mol.nao, 5, 105)
    b = I.DeviceBasis(mol, lib)
    try:
        Ga, = b.ao2mo([TA], tile_pairs=tiles[0])
        va, _ = b.tile_stats()
        Gb, = b.ao2mo([TA], tile_pairs=tiles[1])
        vb, _ = b.tile_stats()
        Gb2, = b.ao2mo([TA], tile_pairs=tiles[1])
        Gd, = b.ao2mo([TA])      # the default tile, chosen from the free memory
    finally:
        b.free()
    d = rel(Ga, Gb)
    print(f"{name}: tile_pairs {tiles[0]} ({va} tiles) against {tiles[1]} ({vb} tiles): {d:.2e} of the largest element; default tile {rel(Gd, Gb):.2e}")
    assert va == len(slabs(mol, tiles[0])) * (len(slabs(mol, tiles[0])) + 1) // 2 and vb == len(slabs(mol, tiles[1])) * (len(slabs(mol, tiles[1])) + 1) // 2 and va > vb
    assert d <= TILE_BAR and rel(Gd, Gb) <= TILE_BAR
    assert Gb.tobytes() == Gb2.tobytes()


# ---- 6. memory ----------------------------------------------------------------------------------------------------------------------------------------------
def check_memory(lib, name="spd3", tile_pairs=40):
    mol = mole(name)
    N, n = mol.nao, 5
    npair = N * (N + 1) // 2
    TA = random_ta(N, n, 100 + n)
    ref = stored_transform(lib, name, n, TA)
    b = I.DeviceBasis(mol, lib)
    try:
        need = b.ao2mo_bytes([n], tile_pairs)
        limit = 8 * npair * npair - 1
        print(f"{name}: N = {N}, the direct transform (n = {n}, tile_pairs = {tile_pairs}) takes {need} bytes on the device, the stored integrals alone {8 * npair ** 2}")
        assert need < limit
        assert lib.qemb_int4c_mem_limit(b.h, limit) == 0
        try:
            et.AOEri.from_basis(b)
            raise AssertionError("the stored integrals were accepted under the limit")
        except _lib.QembError as err:
            assert err.status == _lib.QEMB_ERR_ALLOC
        G, = b.ao2mo([TA], tile_pairs=tile_pairs)
        compare(f"{name} under the memory limit", G, ref)
    finally:
        b.free()
    # below the footprint of the smallest tile: refused with the bytes in the message, before the pair stage or anything else is allocated
    b = I.DeviceBasis(mol, lib)
    try:
        small = b.ao2mo_bytes([n], 1)
        assert lib.qemb_int4c_mem_limit(b.h, small - 1) == 0
        out = np.empty((n * (n + 1) // 2,) * 2)
        ta, ns, op = (C.c_void_p * 1)(TA.ctypes.data), (C.c_int * 1)(n), (C.c_void_p * 1)(out.ctypes.data)
        assert lib.qemb_ao2mo_direct(b.h, 1, ta, ns, op, None, 1, 0.0) == _lib.QEMB_ERR_ALLOC
        msg = lib.qemb_last_error()
        assert str(small).encode() in msg and f"N = {N}".encode() in msg, msg
        assert lib.qemb_int4c_mem_limit(b.h, small) == 0
        assert lib.qemb_ao2mo_direct(b.h, 1, ta, ns, op, None, 1, 0.0) == 0      # the figure is the call's own: at the limit it runs
        assert rel(out, ref) <= BAR
    finally:
        b.free()


def check_bytes_do_not_follow_npair_squared(lib, tile_pairs=40, n=5):
    """for a fixed tile and n the footprint is the pair stage and lists (what jk_bytes counts, O(npair)), three int32 tables of npair entries, the tile and the
    three tile-row operands (a tile holds at most max(tile_pairs, 25) AO pairs: a d-d shell pair alone), the block, the coefficients and 4 KiB"""
    figs = {}
    for name in ("h8_sto3g", "h4_ccpvdz", "spd3"):
        mol = mole(name)
        N, npq, rows = mol.nao, n * (n + 1) // 2, max(tile_pairs, 25)
        npair = N * (N + 1) // 2
        b = I.DeviceBasis(mol, lib)
        try:
            got, jk = b.ao2mo_bytes([n], tile_pairs), b.jk_bytes()
        finally:
            b.free()
        bound = jk + 12 * npair + 8 * (rows * rows + 3 * rows * npq + npq * npq + N * n) + 4096
        figs[name] = (npair, got, bound)
        assert got <= bound, (name, got, bound)
    print("ao2mo_bytes at tile_pairs = 40, n = 5: " + ", ".join(f"{k}: npair {v[0]}, {v[1]} bytes (bound {v[2]})" for k, v in figs.items()))
    (p0, b0, _), (p1, b1, _) = figs["h8_sto3g"], figs["spd3"]
    assert 8 * (p1 * p1 - p0 * p0) > 4 * (b1 - b0)      # npair grows 10-fold: 8 npair^2 by 1.1 MB, the footprint by less than a quarter of that


# ---- 7. screening -------------------------------------------------------------------------------------------------------------------------------------------
def check_screening(lib, thresh=1e-12):
    """the stretched H8 chain of int4c_cases.check_screening, every shell pair a slab of its own: distant pairs fall below the threshold, and a tile of two of them
    is skipped as a whole"""
    mol = mole("h8_far")
    TA = random_ta(mol.nao, 5, 300)
    b = I.DeviceBasis(mol, lib)
    try:
        G0, = b.ao2mo([TA], tile_pairs=1)
        nq0, nz0 = b.eri_stats()
        v0, s0 = b.tile_stats()
        G1, = b.ao2mo([TA], tile_pairs=1, thresh=thresh)
        nq1, nz1 = b.eri_stats()
        v1, s1 = b.tile_stats()
        b.eri(8, thresh=thresh)
        _, nz_fill = b.eri_stats()
    finally:
        b.free()
    d = rel(G1, G0)
    print(f"screening at {thresh:g}: {nz1} of {nq1} canonical quartets screened (the fill: {nz_fill}), {s1} of {v1 + s1} tiles skipped, result moves by {d:.2e}")
    assert (nz0, s0) == (0, 0) and nq0 == nq1 == 36 * 37 // 2 and v0 == v1 + s1 == 36 * 37 // 2
    assert nz1 == nz_fill > 0 and s1 >= 1
    assert d <= BAR


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------------------------
def be_pair(lib, mf, frag, solver, tile):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    out = {}
    for route in ("in-core-hip", "int-direct-hip"):
        fobj = FragPart.from_json(GOLDEN / "fragmentation.json", frag)
        kw = dict(int_direct_tile=tile) if route == "int-direct-hip" else {}
        be = BE(mf, fobj, lib=lib, distribute=False, int_transform=route, integral_backend="hip", **kw)
        assert be._eri_from_geometry and mf._eri is None
        e1 = be.oneshot(solver=solver)[0]
        be.optimize(solver=solver)
        out[route] = (np.array([e1, be.e_corr, be.hf_err]), be)
    a, b = out["in-core-hip"][0], out["int-direct-hip"][0]
    print(f"{frag} {solver}: oneshot E_corr {a[0]:.12f} / {b[0]:.12f}, optimize E_corr {a[1]:.12f} / {b[1]:.12f}, HF-in-HF error {a[2]:.3e} / {b[2]:.3e} "
          f"(in-core-hip / int-direct-hip), largest difference {np.abs(a - b).max():.2e}")
    assert np.abs(a - b).max() <= BE_BAR, (a, b)
    return out["int-direct-hip"][1]


def check_end_to_end_h8(lib, solver="MP2"):
    """H8 / STO-3G BE2 on a direct mean field.  (At N = 8 an array of N^4 / 8 doubles is 4 KiB, less than the pair stage of any route: the comparison of the
    footprint with N^4 / 8 is made on octane, check_end_to_end_octane.)"""
    mf = cj.direct_h8_mf(lib)
    be = be_pair(lib, mf, "test_autogen_h_linear_be2", solver, 7)
    assert mf._eri is None and be.int_direct_bytes > 0


def check_end_to_end_octane(lib, solver="MP2", tile=128):
    """octane / STO-3G BE2 (N = 58, fragments of 42).  No array of N^4 / 8 doubles: the mean field holds none (`_eri` None, every array of a J / K call is part of
    jk_bytes), and every array of the transform is either one fragment's block (npair(n)^2 doubles, which the fragment keeps on every route) or part of the rest
    of the footprint of a call for the largest fragment."""
    from helpers import GOLDEN
    mol = I.Mole(GOLDEN / "octane.xyz")
    mf = I.RHF(mol, integral_backend="hip", lib=lib, direct=True)
    try:
        mf.kernel()
        be = be_pair(lib, mf, "test_autogen_octane_be2", solver, tile)
        N, nmax = mol.nao, max(f.TA.shape[1] for f in be.Fobjs)
        block = 8 * (nmax * (nmax + 1) // 2) ** 2
        b = I.DeviceBasis(mol, lib)
        try:
            rest, jk = b.ao2mo_bytes([nmax], tile) - block, b.jk_bytes()
        finally:
            b.free()
        print(f"octane: N^4 / 8 doubles = {N ** 4} bytes; largest fragment block {block}, the rest of a transform call {rest}, a J / K call {jk}; "
              f"the whole transform call of BE {be.int_direct_bytes}")
        assert mf._eri is None and max(block, rest, jk) < N ** 4
    finally:
        mf.free()


# ---- 9. argument errors -------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    fobj = lambda: FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    mf = c4.h8_mf()
    with np.testing.assert_raises(ValueError):
        BE(mf, fobj(), lib=lib, distribute=False, int_transform="int-direct-hip", integral_backend="host")
    with np.testing.assert_raises(ValueError):
        BE(mf, fobj(), lib=lib, distribute=False, int_transform="int-direct-hip")

    class NoMol:
        mol = None

        def __init__(self, m):
            self._m = m

        def __getattr__(self, k):
            return getattr(self._m, k)

    with np.testing.assert_raises(ValueError):
        BE(NoMol(mf), fobj(), lib=lib, distribute=False, int_transform="int-direct-hip", integral_backend="hip")
    assert "int-direct-hip" in et.HIP_INT_TRANSFORMS
    mol = mole("h8_sto3g")
    b = I.DeviceBasis(mol, lib)
    TA = random_ta(mol.nao, 3, 1)
    out = np.empty((6, 6))
    ta, ns, op = (C.c_void_p * 1)(TA.ctypes.data), (C.c_int * 1)(3), (C.c_void_p * 1)(out.ctypes.data)
    try:
        assert lib.qemb_ao2mo_direct(b.h, 1, ta, ns, op, None, 7, -1.0) == _lib.QEMB_ERR_ARG
        assert lib.qemb_ao2mo_direct(b.h, 0, ta, ns, op, None, 7, 0.0) == _lib.QEMB_ERR_ARG
        assert lib.qemb_ao2mo_direct(b.h, 1, None, ns, op, None, 7, 0.0) == _lib.QEMB_ERR_ARG
        assert lib.qemb_ao2mo_direct(b.h, 1, ta, (C.c_int * 1)(mol.nao + 1), op, None, 7, 0.0) == _lib.QEMB_ERR_ARG
        assert lib.qemb_ao2mo_direct_bytes(b.h, 1, ns, 7, None) == _lib.QEMB_ERR_ARG
        with np.testing.assert_raises(ValueError):
            b.ao2mo([TA[:-1]])
        # tiles: a non-canonical pair, a pair twice, two lists that overlap without being the same
        t = np.empty(64)

        def tile(R, S):
            r, s = np.array(R, dtype=np.int32), np.array(S, dtype=np.int32)
            return lib.qemb_op_int4c_tile(b.h, r.ctypes.data, len(r), s.ctypes.data, len(s), 0.0, t.ctypes.data)

        assert tile([(0, 1)], [(0, 0)]) == _lib.QEMB_ERR_ARG
        assert tile([(1, 0), (1, 0)], [(0, 0)]) == _lib.QEMB_ERR_ARG
        assert tile([(1, 0), (1, 1)], [(1, 1)]) == _lib.QEMB_ERR_ARG
        assert tile([(1, 0), (1, 1)], [(0, 0)]) == 0
        assert lib.qemb_ao2mo_direct(b.h, 1, ta, ns, op, None, 7, 0.0) == 0
        dead = C.c_void_p(b.h.value)
    finally:
        b.free()
    assert lib.qemb_ao2mo_direct(dead, 1, ta, ns, op, None, 7, 0.0) == _lib.QEMB_ERR_ARG and b"live basis handle" in lib.qemb_last_error()
    assert lib.qemb_ao2mo_direct_bytes(dead, 1, ns, 7, C.byref(C.c_int64())) == _lib.QEMB_ERR_ARG
    assert lib.qemb_int4c_tile_stats(dead, None, None) == _lib.QEMB_ERR_ARG
    assert lib.qemb_op_int4c_tile(dead, None, 0, None, 0, 0.0, None) == _lib.QEMB_ERR_ARG
    # an f orbital shell: the basis uploads, the transform names the shell
    fmol = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]})
    fb = I.DeviceBasis(fmol, lib)
    try:
        fta = random_ta(fmol.nao, 2, 2)
        fo = np.empty((3, 3))
        args = ((C.c_void_p * 1)(fta.ctypes.data), (C.c_int * 1)(2), (C.c_void_p * 1)(fo.ctypes.data))
        assert lib.qemb_ao2mo_direct(fb.h, 1, *args, None, 7, 0.0) == _lib.QEMB_ERR_UNSUPPORTED
        assert b"orbital shell 1" in lib.qemb_last_error() and b"l = 3" in lib.qemb_last_error()
        assert lib.qemb_ao2mo_direct_bytes(fb.h, 1, args[1], 7, C.byref(C.c_int64())) == _lib.QEMB_ERR_UNSUPPORTED
        try:
            fb.ao2mo([fta])
            raise AssertionError("an f shell was accepted")
        except _lib.QembError as err:
            assert err.status == _lib.QEMB_ERR_UNSUPPORTED
    finally:
        fb.free()
