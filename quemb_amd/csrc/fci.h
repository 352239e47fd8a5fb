// fci.h -- determinant-space FCI of one embedding problem on the device: what `fci.FCI(mf, mo_coeff).kernel()`, make_rdm1 and make_rdm2 do for
// solver == "FCI" of be_func (molbe/solver.py:339-342, :507-528).  Occupation strings and link tables on the host (once per (n, nsocc), kept on the device),
// the Hamiltonian in Knowles-Handy form -- two gather passes around one FP64 product (fci_ops.hip, dev_gemm) --, a Davidson-Liu iteration with the basis on
// the device and the small eigenproblem on the host, the 1- and 2-RDM from one more product of D with itself.  Plain C++ over dev_ops.h.
#pragma once
#include <cstdint>
#include <vector>
#include "tensor_utils.h"

namespace qemb {

struct FciOptions {
  double conv_tol = 1e-9;      // ||H c - E c||_2
  int max_cycle = 100;         // applications of H
  int max_space = 12;          // basis vectors before the collapse to the Ritz vector
  double lindep = 1e-14;       // a correction whose norm falls below this after orthogonalisation is dropped
};

// strings of one spin in lexical order and, for every string I, the nlink = nsocc (n - nsocc + 1) pairs (p,q) with <I|E_pq|J> = +-1 (the diagonal ones included);
// device copies in the layouts of dev_ops.h
struct FciTables {
  int n = 0, nsocc = 0, nlink = 0;
  int64_t ns = 0;
  std::vector<int32_t> strings, links;      // host: strings[I]; links[l * ns + I]
  int32_t* strings_dev = nullptr;
  int32_t* links_dev = nullptr;
  int64_t ndet() const { return ns * ns; }
};
// built on first use, uploaded once and kept for the life of the process (one table per (n, nsocc); any execution context may read it)
int fci_tables(int n, int nsocc, const FciTables** out);
int64_t fci_string_count(int n, int nsocc);
// device bytes of a solve: D and G (2 x 8 n^2 N_det), the Davidson basis, its images and four work vectors ((2 max_space + 4) x 8 N_det), the tables and the n^4 pieces
int64_t fci_bytes(int n, int nsocc, int max_space);
// Slabs: D and G hold the columns of `rows` alpha strings at a time (all beta strings: rows * ns determinants, contiguous in c), and one application of H, or
// one RDM build, walks the ceil(ns / rows) slabs in ascending order.  rows <= 0 (and rows >= ns in the byte count) is the whole space.
//   fci_bytes_slab: fci_bytes with D and G at 2 x 8 n^2 min(rows, ns) ns;  fci_slab_count: ceil(ns / rows), 1 when rows <= 0
//   fci_rows_that_fit: the largest rows <= ns whose fci_bytes_slab is at most `room` bytes; 0 when not even one row fits
int64_t fci_bytes_slab(int n, int nsocc, int max_space, int64_t rows);
int64_t fci_slab_count(int64_t ns, int64_t rows);
int64_t fci_rows_that_fit(int n, int nsocc, int max_space, double room);

// k_pq = h_pq - 1/2 sum_r (pr|rq) on the host (h, V: [n][n] and [n^2][n^2] host arrays)
void fci_one_body(int n, const double* h, const double* V, double* k);

// one application of H: sigma = H c.  k_dev [n^2], V_dev [n^2][n^2]; D, G: n^2 N_det doubles of work space each.  rows > 0: in slabs of that many alpha rows
// through the slab kernels (rows >= ns: one slab), D and G n^2 min(rows, ns) ns doubles each; for a given rows two calls give the same bits
int fci_apply(const FciTables& T, const double* k_dev, const double* V_dev, const double* c, double* D, double* G, double* sigma, int64_t rows = 0);

struct FciResult { double e = 0.0, residual = 0.0; int n_iter = 0; bool converged = false; };
// lowest state of the M_s = 0 space of H(h, V) with nelec = (nsocc, nsocc); c (N_det doubles, device) receives the normalised vector, largest-magnitude component
// positive.  h_host: [n][n]; V_dev: [n^2][n^2] on the device.  rows: the slab height of every application of H (0: none); the working set is fci_bytes_slab.
int fci_davidson(const FciTables& T, const double* h_host, const double* V_dev, const FciOptions& opt, double* c, FciResult* res, int64_t rows = 0);

// the host side of the Davidson iteration, shared with sci.cpp: the small symmetric eigenproblem (cyclic Jacobi; A [m][m] is overwritten, w ascending, eigenvectors
// in the columns of V), host[j] = <x, ys[j]> and out = sum_j coef[j] xs[j] (+ out) eight vectors per pass (scratch: >= 8 doubles on the device)
namespace fci_detail {
void small_eigh(int m, std::vector<double>& A, std::vector<double>& w, std::vector<double>& V);
int dots(int64_t N, const double* x, const std::vector<const double*>& ys, double* scratch, double* host);
int combine(int64_t N, const std::vector<double>& coef, const std::vector<const double*>& xs, bool accumulate, double* out);
}  // namespace fci_detail

// dm1[p,q] = sum_I c_I D[pq][I] (host, symmetrised) and, when dm2_dev != null, dm2[p,q,r,s] = <p+ r+ s q> (n^4 doubles, device); o_cum >= 0: minus the mean-field part.
// rows > 0: slab by slab (dm1 += D_s c_s, A += D_s D_s^T), D at n^2 min(rows, ns) ns doubles
int fci_rdm12(const FciTables& T, const double* c, int o_cum, double* dm1_host, double* dm2_dev, int64_t rows = 0);

}  // namespace qemb
