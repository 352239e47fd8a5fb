// int3c.h -- the integral source of density fitting on the device: (mu nu|P) and (P|Q) from a basis uploaded once (what integrals.aux_e2, aux_e2_pairs and
// int2c2e obtain from the host library; the reference asks libcint: molbe/eri_onthefly.py:64-108, eri_sparse_DF.py:410-494).  The driver groups shell
// pairs and auxiliary shells by angular momentum and issues one launch per class (dev_int3c_class); results go straight to the layout the consumer reads.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "dev_ops.h"
#include "int3c_core.h"
#include "tensor_utils.h"

namespace qemb {

class DfContext;
struct PairCache;      // int4c.cpp: the resident pair stage, pair lists and Schwarz factors of a basis

// the record integrals.py builds per Cartesian contracted function (`_BF`; csrc_host/gto_ints.c bf_t)
struct BfRecord {
  double ctr[3];
  int lmn[3];
  int nprim;
  double ex[int3c::kMaxPrim], co[int3c::kMaxPrim];
};

class IntBasis {
 public:
  int nshell = 0, nao = 0;
  std::vector<int3c::Shell> shells;      // host copy: the driver sorts work by it
  DBuf dshells, dc2s;                    // dshells: the nshell shells and, at index nshell, a unit s function (role B of the metric blocks)
  // records: n_bf Cartesian functions, shell after shell, the components of a shell in libcint order with one set of exponents / coefficients;
  // c2s: int3c::kC2sLen doubles, integrals.cart2sph(l) for l = 0..4; the matrices of l = 0, 1 must be the identity (QEMB_ERR_UNSUPPORTED otherwise)
  int create(int n_bf, const BfRecord* records, const double* c2s_host);
  const int3c::Shell* dev() const { return reinterpret_cast<const int3c::Shell*>(dshells.p); }
  // the four-centre integrals of the basis (int4c.cpp): Schwarz factors sqrt(max (ab|ab)) per shell pair of each of the six pair classes (ss ps pp ds dp dd; filled
  // by the first screened call), the device bytes a call may take (< 0: the free memory) and [canonical shell quartets, of which screened] of the last fill
  std::vector<double> schwarz[6];
  int64_t int4c_mem_limit = -1;
  int64_t int4c_stats[2] = {0, 0};
  int64_t int4c_tiles[2] = {0, 0};      // tiles visited / skipped by the last integral-direct AO -> fragment transform (int4c_ao2mo_direct)
  int64_t cd_stats[3] = {0, 0, 0};      // the last Cholesky decomposition of the basis (int4c_cholesky): rank, panels, integral columns evaluated
  double cd_dmax = 0.0;                 // ... and the largest residual diagonal it ended with
  // pair lists, pair stage and Schwarz factors resident on the device, from the first call that needs them (direct J / K, the direct AO -> fragment transform,
  // the explicit tile) to the end of the basis
  std::shared_ptr<PairCache> pair_cache;
};

// The refusals the DF and the four-centre drivers share; who: the entry point, for the messages.
int check_orbital(const IntBasis& orb, const char* who);       // an orbital shell beyond d: QEMB_ERR_UNSUPPORTED naming the shell and its l
int check_c2s(const double* c2s_host, const char* who);        // the kernels skip the Cartesian -> spherical step of s and p shells: QEMB_ERR_UNSUPPORTED unless identity
int check_thresh(double thresh, const char* who);              // a screening threshold must be >= 0 (QEMB_ERR_ARG)
// the shell of angular momentum l that starts at record r (1 to 8 primitives: QEMB_ERR_ARG otherwise)
int shell_of(const BfRecord& r, int l, int ao0, const std::string& who, int3c::Shell* s);

enum { INT_LAYOUT_PQL = 0, INT_LAYOUT_LPQ = 1, INT_LAYOUT_PACKED = 2, INT_LAYOUT_PAIRS = 3 };

// (mu nu|P) into out_dev: (N, N, naux), (naux, N, N), (naux, npair(N)) or, with a pair list (n_pairs x 2 AO indices, host), (n_pairs, naux).
// Orbital shells beyond d: QEMB_ERR_UNSUPPORTED naming the shell.
int int3c_fill(const IntBasis& orb, const IntBasis& aux, int layout, const int64_t* pairs_host, int64_t n_pairs, double* out_dev);
// (P|Q) into out_dev (naux x naux): the lower triangle of shell pairs is computed, the upper one copied
int int2c_fill(const IntBasis& aux, double* out_dev);
// S, T and V = sum_C -Z_C <a|1/r_C|b> of the orbital basis into host arrays (N x N each; a null one is skipped): same normalisation, component order and
// Cartesian -> spherical matrices as Mole.one_electron().  natm nuclei at xyz_host (3 natm, Bohr) with charges Z_host.  Orbital shells beyond d: QEMB_ERR_UNSUPPORTED.
int int1e_fill(const IntBasis& orb, int natm, const double* xyz_host, const double* Z_host, double* S_host, double* T_host, double* V_host);
// the dipole integrals <a|r - origin|b> of the same basis, out_host[3][N][N]: the same shell-pair ownership, every element stored once with its mirror image
int int1e_dipole_fill(const IntBasis& orb, const double* origin, double* out_host);
// one explicit block (qemb_op_int3c_class): out_host[(a * (2 lb + 1) + b) * (2 lP + 1) + m]
int int3c_block(int la, int lb, int lp, const BfRecord* A, const BfRecord* B, const BfRecord* P, const double* c2s_host, double* out_host);

}  // namespace qemb
