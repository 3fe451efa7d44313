// Device-resident CSR matrix: product, diagonal and a preconditioned conjugate-gradient iteration that never leaves the device
// (the vendor-backend slot of the reference: matrix/_mkl.py multiplies and solves with the library that owns the data; here the
// triplet that the assembly kernels leave in HBM is used where it lies).
//
//   * k_csr_spmv<L, Idx, DOT>: y = mask(alpha A x + beta b).  L lanes own a row (L = 1 .. 64, a power of two); consecutive lane groups
//     of a wave take consecutive rows, so a wave reads one contiguous span of values / column indices; rows longer than L are walked
//     in strides of L and the L partial sums are folded with __shfl_xor in a fixed order.  A workgroup strides over the rows, the grid
//     is a function of (nrows, L) only, nothing is atomic: repeated calls are bit-identical.  Column indices are int32 (narrowed once
//     per matrix by nh_csr_compact: 12 instead of 16 bytes per entry) or the int64 of the assembly; rowptr stays int64.
//     DOT = 1: additionally the workgroup's share of x . y goes to partial[blockIdx.x] (the p . Ap of a CG step).
//     DOT = 2: the shares of w . y and y . y, w a vector of its own, go to partial[blockIdx.x] and partial2[blockIdx.x] (the two products of a BiCGStab
//     step); the kernel does nothing at all when *skip != 0 (the iteration has stopped).
//     DOT = 3: no dots, only the skip cell (the product of a GMRES step, whose dots are the Gram-Schmidt kernels').
//   * k_csr_support<L, Idx>: the support of the matrix above a tolerance, by the product's mapping (L lanes per row, a wave reads one contiguous span):
//     a lane that meets |a| > tol stores the byte 1 to colsupp[col] and remembers it for the row, whose L lanes are folded with __shfl_xor before lane 0
//     stores rowsupp[row].  Lanes that meet the same column store the same byte to the same address: plain vector byte stores, nothing atomic, and since
//     the result is a set it does not depend on who comes first.  The arrays are zeroed before the launch.
//   * k_cg_update / k_cg_direction: the vector half of a CG step.  Every workgroup sums the partials of the kernel before it in the
//     same order and so holds the same alpha / beta; scalars that cross an iteration live in two cells each, one written and one read
//     per kernel, so no kernel reads a cell that one of its own workgroups writes.
//   * k_bicgstab_half / k_bicgstab_update / k_bicgstab_direction: the vector part of a right-preconditioned BiCGStab step for general square matrices, by
//     the same rules (the cells and who writes them: the B_ enum below).
//   * k_minres_lanczos / k_minres_update: the vector part of a MINRES step for symmetric indefinite matrices, one product and three launches a step, by the
//     same rules (the M_ enum below).
#include "nh_common.h"
#include <algorithm>
#include <climits>
#include <cstdint>
#include <initializer_list>

namespace {

#include "nh_krylov.inc"  // WG, the grid caps, block_sum, partial_sum, check_csr, spmv_grid, vec_grid, and the cells W_RR, W_FLAG_B, W_STOP: shared with nh_amg.hip

// the other cells of the CG work array (doubles)
enum { W_FLAG_A = 3, W_RZ_A = 4, W_RZ_B = 5, W_PQ = 8, W_RZP = W_PQ + SPMV_MAX_WGS, W_RRP = W_RZP + VEC_MAX_WGS, W_END = W_RRP + VEC_MAX_WGS };

template <int L, class Idx, int DOT>
__global__ __launch_bounds__(WG) void k_csr_spmv(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                                 const double *__restrict__ x, double alpha, double beta, const double *b, const unsigned char *__restrict__ mask, double *y,
                                                 double *partial, const double *__restrict__ w, double *partial2, const double *skip) {
  if (DOT >= 2 && skip && *skip != 0.) return;
  constexpr int G = WG / L;  // rows per workgroup and step
  const int lane = threadIdx.x & (L - 1);
  double dot = 0, dot2 = 0;
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the shuffles)
    const i64 row = base + threadIdx.x / L;
    const bool live = row < nrows;
    const bool on = live && (!mask || mask[row]);
    double s = 0;
    if (on) {
      const i64 k1 = rowptr[row + 1];
#pragma unroll 2
      for (i64 k = rowptr[row] + lane; k < k1; k += L) s += values[k] * x[col[k]];
    }
#pragma unroll
    for (int o = L >> 1; o; o >>= 1) s += __shfl_xor(s, o, L);
    if (live && lane == 0) {
      double v = 0;
      if (on) {
        v = alpha * s;
        if (b) v += beta * b[row];
      }
      y[row] = v;
      if (DOT == 1) dot += x[row] * v;
      if (DOT == 2 && on) {
        dot += w[row] * v;
        dot2 += v * v;
      }
    }
  }
  if (DOT == 1 || DOT == 2) {
    __shared__ double lds[4];
    dot = block_sum(dot, lds);
    if (DOT == 2) dot2 = block_sum(dot2, lds);
    if (threadIdx.x == 0) {
      partial[blockIdx.x] = dot;
      if (DOT == 2) partial2[blockIdx.x] = dot2;
    }
  }
}

template <int L, class Idx>
__global__ __launch_bounds__(WG) void k_csr_support(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values, double tol,
                                                    unsigned char *__restrict__ rowsupp, unsigned char *__restrict__ colsupp) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the shuffles)
    const i64 row = base + threadIdx.x / L;
    const bool live = row < nrows;
    int any = 0;
    if (live) {
      const i64 k1 = rowptr[row + 1];
      for (i64 k = rowptr[row] + lane; k < k1; k += L)
        if (fabs(values[k]) > tol) {  // (strict; false for NaN)
          any = 1;
          if (colsupp) colsupp[col[k]] = 1;
        }
    }
#pragma unroll
    for (int o = L >> 1; o; o >>= 1) any |= __shfl_xor(any, o, L);
    if (rowsupp && live && lane == 0 && any) rowsupp[row] = 1;
  }
}

__global__ void k_csr_compact(i64 nnz, const i64 *__restrict__ col, int32_t *__restrict__ col32) {
  for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (i64)gridDim.x * blockDim.x) col32[k] = (int32_t)col[k];
}

template <class Idx>
__global__ void k_csr_diagonal(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values, double *__restrict__ diag) {
  const i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrows) return;
  double d = 0;
  for (i64 k = rowptr[row], k1 = rowptr[row + 1]; k < k1; ++k)
    if ((i64)col[k] == row) d += values[k];
  diag[row] = d;
}

// z = dinv r (or r), p = z, partials of r . z and r . r
__global__ __launch_bounds__(WG) void k_cg_init(i64 n, double *work, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ p) {
  __shared__ double lds[4];
  double rz = 0, rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double ri = r[i], zi = dinv ? dinv[i] * ri : ri;
    p[i] = zi;
    rz += ri * zi;
    rr += ri * ri;
  }
  rz = block_sum(rz, lds);
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) {
    work[W_RZP + blockIdx.x] = rz;
    work[W_RRP + blockIdx.x] = rr;
  }
}

__global__ __launch_bounds__(WG) void k_cg_init_scalars(int nparts, double *work) {
  __shared__ double lds[4];
  const double rz = partial_sum(work + W_RZP, nparts, lds);
  const double rr = partial_sum(work + W_RRP, nparts, lds);
  if (threadIdx.x == 0) {
    work[W_RR] = rr;
    work[W_RZ_B] = rz;
    work[W_RZ_A] = rz;
    work[W_FLAG_A] = 0.;
    work[W_FLAG_B] = 0.;
    work[W_STOP] = 0.;
  }
}

// alpha = r.z / p.q;  x += alpha p;  r -= alpha q;  partials of r . z and r . r with z = dinv r.
// reads RR, RZ_B, FLAG_A, STOP, the p.q partials; writes RZ_A, FLAG_B, the r.z / r.r partials (not when done: r has not moved, they stand)
__global__ __launch_bounds__(WG) void k_cg_update(i64 n, int npq, double *work, const double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r,
                                                  const double *__restrict__ p, const double *__restrict__ q) {
  __shared__ double lds[4];
  const double pq = partial_sum(work + W_PQ, npq, lds);
  const double rz = work[W_RZ_B], rr = work[W_RR];
  bool bad = work[W_FLAG_A] != 0.;
  // within the bound (0. without one: the residual vanished): nothing left to do, and p . q = 0 is no breakdown.  Iterated past convergence r . r falls
  // through the subnormal range, where r . z or p . q underflow to 0 before r . r does: a false breakdown
  const bool done = rr <= work[W_STOP];
  if (!done && !bad) bad = !(rz > 0. && rz <= 1.7976931348623157e308 && pq > 0. && pq <= 1.7976931348623157e308);
  const bool move = !done && !bad;
  const double alpha = move ? rz / pq : 0.;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[W_RZ_A] = rz;
    work[W_FLAG_B] = bad ? 1. : 0.;
  }
  if (done) return;
  double srz = 0, srr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    double ri = r[i];
    if (move) {  // (a stalled iteration does no arithmetic on x and r: no 0 * inf)
      x[i] += alpha * p[i];
      ri -= alpha * q[i];
      r[i] = ri;
    }
    const double zi = dinv ? dinv[i] * ri : ri;
    srz += ri * zi;
    srr += ri * ri;
  }
  srz = block_sum(srz, lds);
  srr = block_sum(srr, lds);
  if (threadIdx.x == 0) {
    work[W_RZP + blockIdx.x] = srz;
    work[W_RRP + blockIdx.x] = srr;
  }
}

// beta = r.z (new) / r.z (old);  p = z + beta p (not once r . r is within the bound: no iteration will read p).  reads RZ_A, FLAG_B, STOP, the partials;
// writes RR, RZ_B, FLAG_A
__global__ __launch_bounds__(WG) void k_cg_direction(i64 n, int nparts, double *work, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ p) {
  __shared__ double lds[4];
  const double rz = partial_sum(work + W_RZP, nparts, lds);
  const double rr = partial_sum(work + W_RRP, nparts, lds);
  const double rz_old = work[W_RZ_A];
  const bool bad = work[W_FLAG_B] != 0.;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[W_RR] = rr;
    work[W_RZ_B] = bad ? rz_old : rz;
    work[W_FLAG_A] = bad ? 1. : 0.;
  }
  if (bad || rr <= work[W_STOP]) return;
  const double beta = rz_old != 0. ? rz / rz_old : 0.;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double zi = dinv ? dinv[i] * r[i] : r[i];
    p[i] = zi + beta * p[i];
  }
}

// ---- BiCGStab: right-preconditioned, M^-1 = dinv or the identity; all vectors vanish on masked rows.  An iteration is
//   v = mask(A phat), partials of rhat . v                                          (k_csr_spmv, DOT = 2, w = rhat)
//   half:      alpha = rho / rhat.v;  s = r - alpha v;  shat = dinv s;  partials of s . s
//   t = mask(A shat), partials of t . s and t . t                                   (k_csr_spmv, DOT = 2, w = s)
//   update:    omega = t.s / t.t;  x += alpha phat + omega shat;  r = s - omega t;  partials of rhat . r and r . r
//   direction: rho' = rhat . r;  beta = (rho' / rho) (alpha / omega);  p = r + beta (p - omega v);  phat = dinv p
// (the direction of the first iteration, p = r, is set by k_bicgstab_init).  Cells of the work array; after "<-" the kernel that writes a cell, every other
// kernel only reads it.  B_RR, B_FLAG, B_COUNT are what the host looks at.  A status is 0 (iterate), ST_DONE (r . r <= stop_rr) or ST_BAD (breakdown); it
// travels direction -> product, half -> product, update -> direction, and a kernel that receives a non-zero status passes it on and does nothing else.
enum {
  B_RR = 0,      // r . r of the recurrence        <- direction
  B_FLAG = 1,    // 1. after a breakdown           <- direction
  B_COUNT = 2,   // iterations that moved x        <- direction
  B_ST = 3,      // status for product 1 and half  <- direction
  B_ST_H = 4,    // status for product 2 and update <- half
  B_ST_U = 5,    // status for direction           <- update
  B_RHO = 6,     // rhat . r                       <- direction
  B_RHO_OLD = 7, // the rho that alpha was made of <- half
  B_ALPHA = 8,   //                                <- half
  B_OMEGA = 9,   //                                <- update
  B_COUNT_U = 10,  // B_COUNT, plus one if x moved <- update
  B_WY = 16,                   // partials of w . y of a product
  B_YY = B_WY + SPMV_MAX_WGS,  // partials of y . y of a product
  B_SS = B_YY + SPMV_MAX_WGS,  // partials of s . s    <- half
  B_RHOP = B_SS + VEC_MAX_WGS, // partials of rhat . r <- update
  B_RRP = B_RHOP + VEC_MAX_WGS,  // partials of r . r  <- update, init
  B_END = B_RRP + VEC_MAX_WGS
};
constexpr double ST_DONE = 1., ST_BAD = 2.;

__device__ __forceinline__ bool finite(double a) { return a >= -1.7976931348623157e308 && a <= 1.7976931348623157e308; }

// rhat = p = r, phat = dinv r, partials of r . r
__global__ __launch_bounds__(WG) void k_bicgstab_init(i64 n, double *work, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ rhat,
                                                      double *__restrict__ p, double *__restrict__ phat) {
  __shared__ double lds[4];
  double rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double ri = r[i];
    rhat[i] = ri;
    p[i] = ri;
    if (dinv) phat[i] = dinv[i] * ri;
    rr += ri * ri;
  }
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) work[B_RRP + blockIdx.x] = rr;
}

__global__ __launch_bounds__(WG) void k_bicgstab_init_scalars(int nparts, double *work) {
  __shared__ double lds[4];
  const double rr = partial_sum(work + B_RRP, nparts, lds);
  if (threadIdx.x == 0) {
    const bool bad = !finite(rr);
    work[B_RR] = rr;
    work[B_FLAG] = bad ? 1. : 0.;
    work[B_COUNT] = 0.;
    work[B_ST] = bad ? ST_BAD : rr == 0. ? ST_DONE : 0.;  // (a residual of zero: nothing to do, and rhat . v = 0 would be no breakdown)
    work[B_RHO] = rr;                                     // rhat = r
    work[B_RHO_OLD] = work[B_ALPHA] = work[B_OMEGA] = 1.;
  }
}

// reads ST, RHO, the rhat . v partials; writes ST_H, RHO_OLD, ALPHA, the s . s partials.  shat is not written without a preconditioner (it is s).
__global__ __launch_bounds__(WG) void k_bicgstab_half(i64 n, int nwy, double *work, const double *__restrict__ dinv, const double *__restrict__ r, const double *__restrict__ v,
                                                      double *__restrict__ s, double *__restrict__ shat) {
  __shared__ double lds[4];
  const double st = work[B_ST];
  if (st != 0.) {
    if (blockIdx.x == 0 && threadIdx.x == 0) work[B_ST_H] = st;
    return;
  }
  const double rv = partial_sum(work + B_WY, nwy, lds);
  const double rho = work[B_RHO];
  const double alpha = rv != 0. ? rho / rv : 0.;
  const bool bad = !(rv != 0. && finite(rv) && finite(alpha));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[B_ST_H] = bad ? ST_BAD : 0.;
    work[B_RHO_OLD] = rho;
    work[B_ALPHA] = alpha;
  }
  if (bad) return;
  double ss = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double si = r[i] - alpha * v[i];
    s[i] = si;
    if (dinv) shat[i] = dinv[i] * si;
    ss += si * si;
  }
  ss = block_sum(ss, lds);
  if (threadIdx.x == 0) work[B_SS + blockIdx.x] = ss;
}

// reads ST_H, ALPHA, COUNT, the t . s, t . t and s . s partials; writes ST_U, OMEGA, COUNT_U, the rhat . r and r . r partials
__global__ __launch_bounds__(WG) void k_bicgstab_update(i64 n, int nwy, int nparts, double stop_rr, double *work, double *__restrict__ x, double *__restrict__ r,
                                                        const double *__restrict__ rhat, const double *phat, const double *shat, const double *s,
                                                        const double *__restrict__ t) {
  __shared__ double lds[4];
  const double st = work[B_ST_H], count = work[B_COUNT];
  if (st != 0.) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      work[B_ST_U] = st;
      work[B_COUNT_U] = count;
    }
    return;
  }
  const double ts = partial_sum(work + B_WY, nwy, lds);
  const double tt = partial_sum(work + B_YY, nwy, lds);
  const double ss = partial_sum(work + B_SS, nparts, lds);
  const double alpha = work[B_ALPHA];
  double omega = tt != 0. ? ts / tt : 0.;
  bool bad = false;
  if (!(omega != 0. && finite(omega))) {  // no second half: with s within the bound that is convergence at the half step, x += alpha phat, r = s
    omega = 0.;
    bad = !(ss <= stop_rr);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[B_ST_U] = bad ? ST_BAD : 0.;
    work[B_OMEGA] = omega;
    work[B_COUNT_U] = bad ? count : count + 1.;
  }
  if (bad) return;
  double rho = 0, rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    x[i] += alpha * phat[i] + omega * shat[i];
    const double ri = s[i] - omega * t[i];
    r[i] = ri;
    rho += rhat[i] * ri;
    rr += ri * ri;
  }
  rho = block_sum(rho, lds);
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) {
    work[B_RHOP + blockIdx.x] = rho;
    work[B_RRP + blockIdx.x] = rr;
  }
}

// reads ST_U, RHO_OLD, ALPHA, OMEGA, COUNT_U, the rhat . r and r . r partials; writes RR, FLAG, COUNT, ST, RHO.  phat is not written without a
// preconditioner (it is p).
__global__ __launch_bounds__(WG) void k_bicgstab_direction(i64 n, int nparts, double stop_rr, double *work, const double *__restrict__ dinv, const double *__restrict__ r,
                                                           const double *__restrict__ v, double *__restrict__ p, double *__restrict__ phat) {
  __shared__ double lds[4];
  const double st = work[B_ST_U], count = work[B_COUNT_U];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (st != 0.) {
    if (first) {
      work[B_ST] = st;
      work[B_COUNT] = count;
      if (st == ST_BAD) work[B_FLAG] = 1.;
    }
    return;
  }
  const double rho = partial_sum(work + B_RHOP, nparts, lds);
  const double rr = partial_sum(work + B_RRP, nparts, lds);
  const double omega = work[B_OMEGA];
  const bool done = rr <= stop_rr;
  const double beta = done || omega == 0. ? 0. : (rho / work[B_RHO_OLD]) * (work[B_ALPHA] / omega);
  const bool bad = !done && !(rho != 0. && finite(rho) && omega != 0. && finite(beta));
  if (first) {
    work[B_RR] = rr;
    work[B_COUNT] = count;
    work[B_ST] = done ? ST_DONE : bad ? ST_BAD : 0.;
    if (bad) work[B_FLAG] = 1.;
    work[B_RHO] = rho;
  }
  if (done || bad) return;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double pi = r[i] + beta * (p[i] - omega * v[i]);
    p[i] = pi;
    if (dinv) phat[i] = dinv[i] * pi;
  }
}

// work[0] = w . y, work[1] = y . y from the partials of a product, summed in the order the solver's kernels use
__global__ __launch_bounds__(WG) void k_spmv_dots_sum(int nwy, double *work) {
  __shared__ double lds[4];
  const double wy = partial_sum(work + B_WY, nwy, lds);
  const double yy = partial_sum(work + B_YY, nwy, lds);
  if (threadIdx.x == 0) {
    work[0] = wy;
    work[1] = yy;
  }
}

// ---- MINRES (Paige and Saunders) for symmetric matrices, definite or not, in the variable names of scipy.sparse.linalg.minres; M^-1 = dinv > 0 or the identity;
// all vectors vanish on masked rows.  The y of the textbook is not stored: it is dinv r2.  An iteration is
//   q = mask(A v), partials of v . q                                                (k_csr_spmv, DOT = 2, w = v)
//   lanczos:   alpha = v . q;  r1 <- r2;  r2 <- q - (beta / oldb) r1 - (alpha / beta) r2 (no r1 term in the first step);  partials of r2 . dinv r2
//   update:    beta' = sqrt(r2 . dinv r2);  the rotation (delta, gbar, epsln, dbar, gamma, cs, sn, phi, phibar);  w1 <- w2;  w2 <- (v - oldeps w1 - delta w2) / gamma;
//              x += phi w2;  r <- sn^2 r - (phibar cs / beta') r2;  v <- dinv r2 / beta';  partials of r . r
// and every nh_minres_iterate ends with k_minres_finish, one workgroup that sums the partials of r . r for the host.  phibar is the residual norm in the M^-1-norm;
// r carries the residual itself, whose 2-norm the stopping rule is about.  It is the lanczos kernel that finds r . r <= stop_rr, one product late: that product
// writes q and nothing else.  Cells of the work array; after "<-" the kernel that writes a cell, every other kernel only reads it (the init writes all).  What
// crosses an iteration is written by update and relayed by lanczos to the cell that update reads.  A status is 0 (iterate), ST_DONE (r . r <= stop_rr, or beta' =
// 0: the Krylov space is exhausted, the step taken) or ST_BAD (a scalar that is not finite, r2 . dinv r2 < 0, gamma = 0); it travels update -> product and
// lanczos, lanczos -> update, and a kernel that receives a non-zero status passes it on and does nothing else.
enum {
  M_RR = 0,      // r . r of the recurrence        <- finish
  M_FLAG = 1,    // 1. after ST_BAD                <- finish
  M_COUNT = 2,   // iterations that moved x        <- finish
  M_ST = 3,      // status for product and lanczos <- update
  M_BETA = 4,    // the beta that v was divided by <- update
  M_OLDB = 5,    // the beta before it             <- update
  M_DBAR = 6,    //                                <- update
  M_EPSLN = 7,   //                                <- update
  M_PHIBAR = 8,  //                                <- update
  M_CS = 9,      //                                <- update
  M_SN = 10,     //                                <- update
  M_COUNT_U = 11,  // iterations that moved x      <- update
  M_FLAG_U = 12,   // 1. after ST_BAD              <- update
  M_ST_L = 16,   // status for update              <- lanczos
  M_ALPHA = 17,  // v . q                          <- lanczos
  M_RELAY = 18,  // M_BETA .. M_COUNT_U, relayed   <- lanczos
  M_NRELAY = M_COUNT_U - M_BETA + 1,
  M_VQ = 32,                    // partials of v . q of the product
  M_QQ = M_VQ + SPMV_MAX_WGS,   // partials of q . q of the product (not read)
  M_RYP = M_QQ + SPMV_MAX_WGS,  // partials of r2 . dinv r2 <- lanczos
  M_RRP = M_RYP + VEC_MAX_WGS,  // partials of r . r        <- update
  M_END = M_RRP + VEC_MAX_WGS
};

// r1 = r2 = r, w1 = w2 = 0, partials of r . dinv r and r . r
__global__ __launch_bounds__(WG) void k_minres_init(i64 n, double *work, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ r1,
                                                    double *__restrict__ r2, double *__restrict__ w1, double *__restrict__ w2) {
  __shared__ double lds[4];
  double ry = 0, rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double ri = r[i];
    r1[i] = r2[i] = ri;
    w1[i] = w2[i] = 0.;
    ry += ri * (dinv ? dinv[i] * ri : ri);
    rr += ri * ri;
  }
  ry = block_sum(ry, lds);
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) {
    work[M_RYP + blockIdx.x] = ry;
    work[M_RRP + blockIdx.x] = rr;
  }
}

__global__ __launch_bounds__(WG) void k_minres_init_scalars(int nparts, double *work) {
  __shared__ double lds[4];
  const double ry = partial_sum(work + M_RYP, nparts, lds);
  const double rr = partial_sum(work + M_RRP, nparts, lds);
  if (threadIdx.x == 0) {
    const bool bad = !(finite(rr) && finite(ry) && (ry > 0. || (ry == 0. && rr == 0.)));  // (r . dinv r <= 0 with r != 0: the preconditioner is not positive)
    const double beta = bad ? 0. : sqrt(ry);
    work[M_RR] = rr;
    work[M_FLAG] = work[M_FLAG_U] = bad ? 1. : 0.;
    work[M_COUNT] = work[M_COUNT_U] = 0.;
    work[M_ST] = bad ? ST_BAD : rr == 0. ? ST_DONE : 0.;  // (a residual of zero: nothing to do, and nothing to normalise)
    work[M_BETA] = work[M_PHIBAR] = beta;
    work[M_OLDB] = work[M_DBAR] = work[M_EPSLN] = work[M_SN] = 0.;
    work[M_CS] = -1.;
  }
}

// v = dinv r / beta: the first Lanczos vector
__global__ __launch_bounds__(WG) void k_minres_first(i64 n, const double *__restrict__ work, const double *__restrict__ dinv, const double *__restrict__ r,
                                                     double *__restrict__ v) {
  if (work[M_ST] != 0.) return;
  const double beta = work[M_BETA];
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) v[i] = (dinv ? dinv[i] * r[i] : r[i]) / beta;
}

// reads ST, BETA .. COUNT_U, the v . q and r . r partials; writes ST_L, ALPHA, the relay, the r2 . dinv r2 partials
__global__ __launch_bounds__(WG) void k_minres_lanczos(i64 n, int nvq, int nparts, double stop_rr, double *work, const double *__restrict__ dinv,
                                                       const double *__restrict__ q, double *__restrict__ r1, double *__restrict__ r2) {
  __shared__ double lds[4];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  double st = work[M_ST];
  double alpha = 0;
  if (st == 0.) {  // (the same sums in every workgroup: the branches are uniform over the grid)
    if (partial_sum(work + M_RRP, nparts, lds) <= stop_rr) {
      st = ST_DONE;
    } else {
      alpha = partial_sum(work + M_VQ, nvq, lds);
      if (!finite(alpha)) st = ST_BAD;
    }
  }
  if (first) work[M_ST_L] = st;
  if (st != 0.) return;
  const double beta = work[M_BETA], oldb = work[M_OLDB];
  if (first) {
    work[M_ALPHA] = alpha;
    for (int c = 0; c < M_NRELAY; ++c) work[M_RELAY + c] = work[M_BETA + c];
  }
  const bool second = oldb != 0.;  // from the second step on: r1 of the first is r2
  const double c1 = second ? beta / oldb : 0., c2 = alpha / beta;
  double ry = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double r2i = r2[i];
    double yi = q[i];
    if (second) yi -= c1 * r1[i];
    yi -= c2 * r2i;
    r1[i] = r2i;
    r2[i] = yi;
    ry += yi * (dinv ? dinv[i] * yi : yi);
  }
  ry = block_sum(ry, lds);
  if (threadIdx.x == 0) work[M_RYP + blockIdx.x] = ry;
}

// reads ST_L, ALPHA, the relay, the r2 . dinv r2 partials; writes ST, BETA .. COUNT_U, FLAG_U, the r . r partials
__global__ __launch_bounds__(WG) void k_minres_update(i64 n, int nparts, double *work, const double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r,
                                                      const double *__restrict__ r2, double *__restrict__ v, double *__restrict__ w1, double *__restrict__ w2) {
  __shared__ double lds[4];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const double st = work[M_ST_L];
  if (st != 0.) {
    if (first) {
      work[M_ST] = st;
      if (st == ST_BAD) work[M_FLAG_U] = 1.;
    }
    return;
  }
  const double ry = partial_sum(work + M_RYP, nparts, lds);
  const double *relay = work + M_RELAY - M_BETA;
  const double alpha = work[M_ALPHA], beta = relay[M_BETA], cs_old = relay[M_CS], sn_old = relay[M_SN], dbar_old = relay[M_DBAR], oldeps = relay[M_EPSLN];
  bool bad = !(finite(ry) && ry >= 0.);
  const double betan = bad ? 0. : sqrt(ry);
  const double delta = cs_old * dbar_old + sn_old * alpha, gbar = sn_old * dbar_old - cs_old * alpha;
  const double gamma = hypot(gbar, betan);
  bad = bad || !(gamma > 0. && finite(gamma));
  double cs = 0, sn = 0, phi = 0, phibar = 0;
  if (!bad) {
    cs = gbar / gamma;
    sn = betan / gamma;
    phi = cs * relay[M_PHIBAR];
    phibar = sn * relay[M_PHIBAR];
    bad = !(finite(phi) && finite(delta));
  }
  if (bad) {
    if (first) {
      work[M_ST] = ST_BAD;
      work[M_FLAG_U] = 1.;
    }
    return;
  }
  const bool more = betan != 0.;  // (beta' = 0 with gamma > 0: the Krylov space is exhausted; the step is taken, r becomes 0, and there is no next v)
  if (first) {
    work[M_ST] = more ? 0. : ST_DONE;
    work[M_BETA] = betan;
    work[M_OLDB] = beta;
    work[M_DBAR] = -cs_old * betan;
    work[M_EPSLN] = sn_old * betan;
    work[M_PHIBAR] = phibar;
    work[M_CS] = cs;
    work[M_SN] = sn;
    work[M_COUNT_U] = relay[M_COUNT_U] + 1.;
  }
  const double s2 = sn * sn, c3 = more ? phibar * cs / betan : 0.;
  double rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double w2i = w2[i];
    const double wi = (v[i] - oldeps * w1[i] - delta * w2i) / gamma;
    w1[i] = w2i;
    w2[i] = wi;
    x[i] += phi * wi;
    double ri = s2 * r[i];
    if (more) {
      const double r2i = r2[i];
      ri -= c3 * r2i;
      v[i] = (dinv ? dinv[i] * r2i : r2i) / betan;
    }
    r[i] = ri;
    rr += ri * ri;
  }
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) work[M_RRP + blockIdx.x] = rr;
}

// what the host reads, after the last iteration of a call: r . r from the partials in the order of k_minres_lanczos, the flag and the count
__global__ __launch_bounds__(WG) void k_minres_finish(int nparts, double *work) {
  __shared__ double lds[4];
  const double rr = partial_sum(work + M_RRP, nparts, lds);
  if (threadIdx.x == 0) {
    work[M_RR] = rr;
    work[M_FLAG] = work[M_FLAG_U];
    work[M_COUNT] = work[M_COUNT_U];
  }
}

// ---- restarted GMRES: right-preconditioned, M^-1 = dinv or the identity (with a fixed M flexible and right-preconditioned GMRES are one iteration); all
// vectors vanish on masked rows.  V holds restart + 1 basis vectors of n doubles, one after the other.  Arnoldi step j (j = G_COUNT, read on the device:
// the host does not know where in a cycle it enqueues) is
//   w = mask(A z)                                                                       (k_csr_spmv, DOT = 3)
//   twice (classical Gram-Schmidt; one pass leaves V^T V - I at 2e-9 after 72 steps on a 1480-row matrix, at 7e-6 by the time an unrestarted solve has converged):
//     dots:     partials of v_k . w, k = 0 .. j, the basis vectors taken GS_CHUNK at a time with one accumulator each
//     dots_sum: h[k] = the partials summed, workgroup k sums those of v_k               (G_H1 in the first pass, G_H2 in the second)
//     axpy:     w -= sum_k h[k] v_k, k ascending; in the second pass also the partials of w . w
//   scalars:    one workgroup: column j of the Hessenberg matrix is h1 + h2 above h_(j+1,j) = |w|; the stored rotations are applied to it, a new one
//               annihilates h_(j+1,j), g is rotated, G_RR = g_(j+1)^2 is the squared residual norm of the least-squares problem; status and count
//   normalize:  v_(j+1) = w / h_(j+1,j), z = dinv v_(j+1)                               (also the v_0 = r / |r| of nh_gmres_init)
// Every kernel reads the status G_ST first and does nothing unless it is 0; k_gmres_scalars (and the init) is its only writer, as of every cell of the
// head.  A status is 0 (iterate), ST_DONE (G_RR <= stop_rr, or the new direction vanished with a pivot left: the lucky breakdown), ST_BAD (the column
// cannot be taken: no pivot, or not finite) or ST_FULL (restart columns taken).  A direction "vanishes" when |w| after the two passes is within GS_VANISH
// of the norm of the column, sqrt(sum h^2 + |w|^2) = |A z| before them: what is left of w is then rounding noise, whose normalisation would be a basis
// vector of noise.  G_FLAG is raised with every vanished or non-finite direction; what it means is the host's to decide from the true residual.
enum {
  G_RR = 0,     // g_(j+1)^2 (after init: r . r)       <- scalars, init
  G_FLAG = 1,   // 1. after a vanished or non-finite direction
  G_COUNT = 2,  // columns taken in this cycle: the j of the next step
  G_ST = 3,     // status
  G_HN = 4,     // the divisor of normalize: |r| or h_(j+1,j)
  G_HEAD = 8
};
constexpr double ST_FULL = 3.;
constexpr int GS_CHUNK = 8;            // basis vectors per pass over w in the Gram-Schmidt kernels (kernels.GMRES_CHUNK)
constexpr double GS_VANISH = 0x1p-40;  // (the rounding of a two-pass Gram-Schmidt step is (j + n) u |A z| at the very most: 2^-33 of it for 2^20 rows)

// where the arrays of the work array start, m = restart: h1, h2 (the two passes' dots), cs, sn (rotations), g, y (m + 1 each), r (the triangular factor, column j
// at r + j (m + 1)), wwp (partials of w . w or r . r), hp (partials of v_k . w at hp + k VEC_MAX_WGS)
struct GmresCells {
  i64 h1, h2, cs, sn, g, y, r, wwp, hp, end;
};
__host__ __device__ inline GmresCells gmres_cells(int m) {
  GmresCells c;
  const i64 m1 = (i64)m + 1;
  c.h1 = G_HEAD;
  c.h2 = c.h1 + m1;
  c.cs = c.h2 + m1;
  c.sn = c.cs + m1;
  c.g = c.sn + m1;
  c.y = c.g + m1;
  c.r = c.y + m1;
  c.wwp = c.r + m1 * m;
  c.hp = c.wwp + VEC_MAX_WGS;
  c.end = c.hp + (i64)m * VEC_MAX_WGS;
  return c;
}

// VW doubles of a vector in one load or store (VW = 2: 16 bytes, for vectors of even length on 16-byte boundaries)
template <int VW>
struct Pack {
  double v[VW];
};
template <int VW>
__device__ __forceinline__ Pack<VW> ld(const double *p) {
  Pack<VW> a;
  if constexpr (VW == 2) {
    const double2 t = *reinterpret_cast<const double2 *>(p);
    a.v[0] = t.x;
    a.v[1] = t.y;
  } else
    a.v[0] = *p;
  return a;
}
template <int VW>
__device__ __forceinline__ void st(double *p, const Pack<VW> &a) {
  if constexpr (VW == 2)
    *reinterpret_cast<double2 *>(p) = make_double2(a.v[0], a.v[1]);
  else
    *p = a.v[0];
}

// the column the step works on: G_COUNT, kept inside the basis whatever the cell holds
__device__ __forceinline__ int gmres_column(const double *work, int m) { return max(0, min((int)work[G_COUNT], m - 1)); }

#define NH_GS_ROWS(i) for (i64 i = ((i64)blockIdx.x * WG + threadIdx.x) * VW; i < n; i += (i64)gridDim.x * WG * VW)

// partials of r . r
__global__ __launch_bounds__(WG) void k_gmres_norm(i64 n, int m, const double *__restrict__ r, double *work) {
  __shared__ double lds[4];
  double rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) rr += r[i] * r[i];
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) work[gmres_cells(m).wwp + blockIdx.x] = rr;
}

__global__ __launch_bounds__(WG) void k_gmres_init_scalars(int nparts, int m, double *work) {
  __shared__ double lds[4];
  const GmresCells c = gmres_cells(m);
  const double rr = partial_sum(work + c.wwp, nparts, lds);
  if (threadIdx.x == 0) {
    const bool bad = !finite(rr);
    const double beta = sqrt(rr);
    work[G_RR] = rr;
    work[G_FLAG] = bad ? 1. : 0.;
    work[G_COUNT] = 0.;
    work[G_ST] = bad ? ST_BAD : rr == 0. ? ST_DONE : 0.;  // (a residual of zero: nothing to do, and nothing to normalise)
    work[G_HN] = beta;
    work[c.g] = beta;
  }
}

// v_count = src / G_HN, z = dinv v_count (or v_count); src is w, or r at the start of a cycle
template <int VW>
__global__ __launch_bounds__(WG) void k_gmres_normalize(i64 n, int m, const double *__restrict__ dinv, const double *__restrict__ src, double *__restrict__ V,
                                                        double *__restrict__ z, const double *__restrict__ work) {
  if (work[G_ST] != 0.) return;
  const double hn = work[G_HN];
  double *v = V + (i64)max(0, min((int)work[G_COUNT], m)) * n;
  NH_GS_ROWS(i) {
    Pack<VW> a = ld<VW>(src + i);
#pragma unroll
    for (int e = 0; e < VW; ++e) a.v[e] /= hn;
    st<VW>(v + i, a);
    if (dinv) {
      const Pack<VW> d = ld<VW>(dinv + i);
#pragma unroll
      for (int e = 0; e < VW; ++e) a.v[e] *= d.v[e];
    }
    st<VW>(z + i, a);
  }
}

// partials of v_k . w, k = 0 .. j: w and every basis vector are read once per chunk of C vectors
template <int C, int VW>
__global__ __launch_bounds__(WG) void k_gmres_dots(i64 n, int m, const double *__restrict__ V, const double *__restrict__ w, double *work) {
  if (work[G_ST] != 0.) return;
  __shared__ double lds[4 * C];
  const int j = gmres_column(work, m);
  double *hp = work + gmres_cells(m).hp + blockIdx.x;
  for (int k0 = 0; k0 <= j; k0 += C) {
    const int nk = min(C, j + 1 - k0);
    const double *v0 = V + (i64)k0 * n;
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0;
    NH_GS_ROWS(i) {
      const Pack<VW> wi = ld<VW>(w + i);
      Pack<VW> vi[C];
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk) vi[c] = ld<VW>(v0 + (i64)c * n + i);
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk)
#pragma unroll
          for (int e = 0; e < VW; ++e) acc[c] += vi[c].v[e] * wi.v[e];
    }
    block_sum_n<C>(acc, lds);
    if (threadIdx.x == 0)
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk) hp[(i64)(k0 + c) * VEC_MAX_WGS] = acc[c];
  }
}

// h[k] = the partials of v_k . w in a fixed order; a workgroup per k
__global__ __launch_bounds__(WG) void k_gmres_dots_sum(int nparts, int m, int second, double *work) {
  if (work[G_ST] != 0.) return;
  __shared__ double lds[4];
  const GmresCells c = gmres_cells(m);
  const int j = gmres_column(work, m);
  for (int k = blockIdx.x; k <= j; k += gridDim.x) {
    const double h = partial_sum(work + c.hp + (i64)k * VEC_MAX_WGS, nparts, lds);
    if (threadIdx.x == 0) work[(second ? c.h2 : c.h1) + k] = h;
  }
}

// w -= sum_k h[k] v_k, k ascending; WW: the partials of the new w . w
template <int C, int VW, bool WW>
__global__ __launch_bounds__(WG) void k_gmres_axpy(i64 n, int m, int second, const double *__restrict__ V, double *__restrict__ w, double *work) {
  if (work[G_ST] != 0.) return;
  __shared__ double lds[4];
  const GmresCells cells = gmres_cells(m);
  const int j = gmres_column(work, m);
  const double *h = work + (second ? cells.h2 : cells.h1);
  double ww = 0;
  NH_GS_ROWS(i) {
    Pack<VW> wi = ld<VW>(w + i);
    for (int k0 = 0; k0 <= j; k0 += C) {
      const int nk = min(C, j + 1 - k0);
      Pack<VW> vi[C];
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk) vi[c] = ld<VW>(V + (i64)(k0 + c) * n + i);
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk)
#pragma unroll
          for (int e = 0; e < VW; ++e) wi.v[e] -= h[k0 + c] * vi[c].v[e];
    }
    st<VW>(w + i, wi);
    if (WW)
#pragma unroll
      for (int e = 0; e < VW; ++e) ww += wi.v[e] * wi.v[e];
  }
  if (WW) {
    ww = block_sum(ww, lds);
    if (threadIdx.x == 0) work[cells.wwp + blockIdx.x] = ww;
  }
}

// the scalar work of step j, by one thread after the workgroup has summed the partials of w . w
__global__ __launch_bounds__(WG) void k_gmres_scalars(int nparts, int m, double stop_rr, double *work) {
  __shared__ double lds[4];
  if (work[G_ST] != 0.) return;
  const GmresCells c = gmres_cells(m);
  const double ww = partial_sum(work + c.wwp, nparts, lds);
  if (threadIdx.x) return;
  const int j = gmres_column(work, m);
  const double *h1 = work + c.h1, *h2 = work + c.h2;
  double *cs = work + c.cs, *sn = work + c.sn, *g = work + c.g, *R = work + c.r + (i64)j * (m + 1);
  double p = h1[0] + h2[0], col2 = p * p;
  for (int k = 0; k < j; ++k) {  // the stored rotations, on (h_k, h_(k+1))
    const double q = h1[k + 1] + h2[k + 1];
    col2 += q * q;
    R[k] = cs[k] * p + sn[k] * q;
    p = cs[k] * q - sn[k] * p;
  }
  col2 += ww;
  const bool vanish = !(ww > (GS_VANISH * GS_VANISH) * col2);
  double st = ST_BAD, flag = 1., count = j;
  if (finite(col2) && !(vanish && !(fabs(p) > GS_VANISH * sqrt(col2)))) {
    const double q = vanish ? 0. : sqrt(ww);
    const double d = fmax(hypot(p, q), fmax(fabs(p), q));  // (never below either: |sn| <= 1 and the estimate cannot rise, whatever hypot rounds to)
    const double cj = p / d, sj = q / d, gj = g[j], gn = -sj * gj, rr = gn * gn;
    if (finite(rr)) {
      R[j] = d;
      cs[j] = cj;
      sn[j] = sj;
      g[j] = cj * gj;
      g[j + 1] = gn;
      work[G_RR] = rr;
      work[G_HN] = q;
      count = j + 1;
      flag = vanish ? 1. : 0.;
      st = vanish || rr <= stop_rr ? ST_DONE : j + 1 >= m ? ST_FULL : 0.;
    }
  }
  work[G_FLAG] = flag;
  work[G_COUNT] = count;
  work[G_ST] = st;
}

// y = R^-1 g for the columns taken, by one workgroup: column by column from the last, every thread owning the entries it updates
__global__ __launch_bounds__(WG) void k_gmres_solve(int m, double *work) {
  const GmresCells c = gmres_cells(m);
  const int count = max(0, min((int)work[G_COUNT], m));
  double *y = work + c.y;
  for (int i = threadIdx.x; i < count; i += WG) y[i] = work[c.g + i];
  __syncthreads();
  for (int k = count - 1; k >= 0; --k) {
    const double *col = work + c.r + (i64)k * (m + 1);
    if (threadIdx.x == 0) y[k] = y[k] / col[k];
    __syncthreads();
    const double yk = y[k];
    for (int i = threadIdx.x; i < k; i += WG) y[i] -= col[i] * yk;
    __syncthreads();
  }
}

// x += dinv sum_k y[k] v_k, k ascending over the columns taken
template <int C, int VW>
__global__ __launch_bounds__(WG) void k_gmres_xupdate(i64 n, int m, const double *__restrict__ dinv, const double *__restrict__ V, double *__restrict__ x,
                                                      const double *__restrict__ work) {
  const int count = max(0, min((int)work[G_COUNT], m));
  if (!count) return;
  const double *y = work + gmres_cells(m).y;
  NH_GS_ROWS(i) {
    Pack<VW> s;
#pragma unroll
    for (int e = 0; e < VW; ++e) s.v[e] = 0;
    for (int k0 = 0; k0 < count; k0 += C) {
      const int nk = min(C, count - k0);
      Pack<VW> vi[C];
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk) vi[c] = ld<VW>(V + (i64)(k0 + c) * n + i);
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < nk)
#pragma unroll
          for (int e = 0; e < VW; ++e) s.v[e] += y[k0 + c] * vi[c].v[e];
    }
    Pack<VW> xi = ld<VW>(x + i);
    if (dinv) {
      const Pack<VW> d = ld<VW>(dinv + i);
#pragma unroll
      for (int e = 0; e < VW; ++e) xi.v[e] += d.v[e] * s.v[e];
    } else
#pragma unroll
      for (int e = 0; e < VW; ++e) xi.v[e] += s.v[e];
    st<VW>(x + i, xi);
  }
}

// Z_count = t: the column of the flexible method, what the preconditioner returned for v_count (count = G_COUNT, as the step that follows reads it)
template <int VW>
__global__ __launch_bounds__(WG) void k_gmres_keep(i64 n, int m, const double *__restrict__ t, double *__restrict__ Z, const double *__restrict__ work) {
  if (work[G_ST] != 0.) return;
  double *zc = Z + (i64)gmres_column(work, m) * n;
  NH_GS_ROWS(i) st<VW>(zc + i, ld<VW>(t + i));
}
#undef NH_GS_ROWS

// what a product leaves besides y: nothing (partial == NULL), the partials of x . y (w == NULL), or those of w . y and y . y; with a skip cell and no
// partials the plain product, not done when the cell is set
struct Epilogue {
  double *partial = nullptr;
  const double *w = nullptr;
  double *partial2 = nullptr;
  const double *skip = nullptr;
};

template <int L, class Idx>
void launch_lanes(const nh_csr *A, const Idx *col, double alpha, const double *x, double beta, const double *b, const unsigned char *mask, double *y, const Epilogue &e,
                  hipStream_t s) {
  const dim3 grid(spmv_grid(A->nrows, L));
  if (e.w)
    hipLaunchKernelGGL((k_csr_spmv<L, Idx, 2>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, x, alpha, beta, b, mask, y, e.partial, e.w,
                       e.partial2, e.skip);
  else if (e.partial)
    hipLaunchKernelGGL((k_csr_spmv<L, Idx, 1>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, x, alpha, beta, b, mask, y, e.partial, e.w,
                       e.partial2, e.skip);
  else if (e.skip)
    hipLaunchKernelGGL((k_csr_spmv<L, Idx, 3>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, x, alpha, beta, b, mask, y, e.partial, e.w,
                       e.partial2, e.skip);
  else
    hipLaunchKernelGGL((k_csr_spmv<L, Idx, 0>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, x, alpha, beta, b, mask, y, e.partial, e.w,
                       e.partial2, e.skip);
}

template <class Idx>
void launch_idx(int L, const nh_csr *A, const Idx *col, double alpha, const double *x, double beta, const double *b, const unsigned char *mask, double *y, const Epilogue &e,
                hipStream_t s) {
  switch (L) {
    case 1: launch_lanes<1>(A, col, alpha, x, beta, b, mask, y, e, s); break;
    case 2: launch_lanes<2>(A, col, alpha, x, beta, b, mask, y, e, s); break;
    case 4: launch_lanes<4>(A, col, alpha, x, beta, b, mask, y, e, s); break;
    case 8: launch_lanes<8>(A, col, alpha, x, beta, b, mask, y, e, s); break;
    case 16: launch_lanes<16>(A, col, alpha, x, beta, b, mask, y, e, s); break;
    case 32: launch_lanes<32>(A, col, alpha, x, beta, b, mask, y, e, s); break;
    default: launch_lanes<64>(A, col, alpha, x, beta, b, mask, y, e, s); break;
  }
}

int spmv(const nh_csr *A, double alpha, const double *x, double beta, const double *b, const unsigned char *mask, double *y, const Epilogue &e, hipStream_t s) {
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (A->col32_dev)
    launch_idx(L, A, A->col32_dev, alpha, x, beta, b, mask, y, e, s);
  else
    launch_idx(L, A, (const i64 *)A->colidx_dev, alpha, x, beta, b, mask, y, e, s);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

template <class Idx>
void launch_support(int L, const nh_csr *A, const Idx *col, double tol, unsigned char *rowsupp, unsigned char *colsupp, hipStream_t s) {
#define NH_SUPPORT(LL)                                                                                                                                            \
  case LL:                                                                                                                                                        \
    hipLaunchKernelGGL((k_csr_support<LL, Idx>), dim3(spmv_grid(A->nrows, LL)), dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, tol, rowsupp, \
                       colsupp);                                                                                                                                  \
    break;
  switch (L) {
    NH_SUPPORT(1)
    NH_SUPPORT(2)
    NH_SUPPORT(4)
    NH_SUPPORT(8)
    NH_SUPPORT(16)
    NH_SUPPORT(32)
    default:
    NH_SUPPORT(64)
  }
#undef NH_SUPPORT
}

// the Gram-Schmidt kernels take two doubles per load when every vector of V starts on a 16-byte boundary; they stride from the row count of the other vector kernels on
bool gs_pairs(i64 n, std::initializer_list<const void *> vectors) {
  if (n & 1) return false;
  for (const void *p : vectors)
    if ((uintptr_t)p & 15) return false;
  return true;
}
unsigned gs_grid(i64 n, int vw) { return (unsigned)std::min<i64>((n + WG * vw - 1) / (WG * vw), VEC_MAX_WGS / vw); }

// One Arnoldi step from the product input p: nine launches.  With Z (the flexible method: p = M z is not a function of the basis alone) p is first kept
// as column G_COUNT of Z, a tenth launch.
template <int VW>
int gmres_step(const nh_csr *B, const unsigned char *rowmask, const double *dinv, const double *p, double *Z, double *V, double *z, double *w, double *work, int m,
               double stop_rr, hipStream_t s) {
  const i64 n = B->nrows;
  const dim3 grid(gs_grid(n, VW)), block(WG), sums((unsigned)std::min(m, 1024));
  Epilogue e;
  e.skip = work + G_ST;
  if (Z) {
    hipLaunchKernelGGL(k_gmres_keep<VW>, grid, block, 0, s, n, m, p, Z, (const double *)work);
    NH_LAUNCH_CHECK();
  }
  if (int rc = spmv(B, 1., p, 0., nullptr, rowmask, w, e, s)) return rc;
  for (int second = 0; second < 2; ++second) {
    hipLaunchKernelGGL((k_gmres_dots<GS_CHUNK, VW>), grid, block, 0, s, n, m, (const double *)V, (const double *)w, work);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gmres_dots_sum, sums, block, 0, s, (int)grid.x, m, second, work);
    NH_LAUNCH_CHECK();
    if (second)
      hipLaunchKernelGGL((k_gmres_axpy<GS_CHUNK, VW, true>), grid, block, 0, s, n, m, second, (const double *)V, w, work);
    else
      hipLaunchKernelGGL((k_gmres_axpy<GS_CHUNK, VW, false>), grid, block, 0, s, n, m, second, (const double *)V, w, work);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_gmres_scalars, dim3(1), block, 0, s, (int)grid.x, m, stop_rr, work);
  NH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gmres_normalize<VW>, grid, block, 0, s, n, m, dinv, (const double *)w, V, z, (const double *)work);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

// niter Arnoldi steps with the fixed preconditioner: the product input of each is the z its predecessor left
template <int VW>
int gmres_steps(const nh_csr *B, const unsigned char *rowmask, const double *dinv, double *V, double *z, double *w, double *work, int m, double stop_rr, int niter,
                hipStream_t s) {
  for (int it = 0; it < niter; ++it)
    if (int rc = gmres_step<VW>(B, rowmask, dinv, z, nullptr, V, z, w, work, m, stop_rr, s)) return rc;
  return NH_OK;
}

}  // namespace

int nh_csr_spmv_pq(const nh_csr *A, const double *p_dev, const unsigned char *rowmask_dev, double *q_dev, double *partial_dev, int max_partials, int *npartials,
                   hipStream_t s) {
  if (int rc = check_csr("nh_csr_spmv_pq", A)) return rc;
  NH_REQUIRE(partial_dev && npartials && (!A->nrows || (p_dev && q_dev)), "nh_csr_spmv_pq: NULL vector");
  NH_REQUIRE(max_partials >= SPMV_MAX_WGS, "nh_csr_spmv_pq: room for %d partials, a product may leave %d", max_partials, SPMV_MAX_WGS);
  *npartials = 0;
  if (!A->nrows) return NH_OK;
  nh_csr B = *A;
  B.lanes = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  *npartials = (int)spmv_grid(A->nrows, B.lanes);
  Epilogue pq;
  pq.partial = partial_dev;
  return spmv(&B, 1., p_dev, 0., nullptr, rowmask_dev, q_dev, pq, s);
}

int nh_gmres_step_from(const nh_csr *A, const unsigned char *rowmask_dev, const double *t_dev, double *Z_dev, double *V_dev, double *z_dev, double *w_dev, double *work_dev,
                       int restart, double stop_rr, hipStream_t s) {
  if (int rc = check_csr("nh_gmres_step_from", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_gmres_step_from: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(restart >= 1, "nh_gmres_step_from: restart must be at least 1 (got %d)", restart);
  NH_REQUIRE(stop_rr >= 0., "nh_gmres_step_from: the bound on r . r must not be negative");
  NH_REQUIRE(work_dev && (!A->nrows || (t_dev && Z_dev && V_dev && z_dev && w_dev)), "nh_gmres_step_from: NULL vector");
  if (!A->nrows) return NH_OK;
  nh_csr B = *A;
  B.lanes = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (gs_pairs(A->nrows, {t_dev, Z_dev, V_dev, z_dev, w_dev})) return gmres_step<2>(&B, rowmask_dev, nullptr, t_dev, Z_dev, V_dev, z_dev, w_dev, work_dev, restart, stop_rr, s);
  return gmres_step<1>(&B, rowmask_dev, nullptr, t_dev, Z_dev, V_dev, z_dev, w_dev, work_dev, restart, stop_rr, s);
}

extern "C" {

int nh_csr_lanes(int64_t nrows, int64_t nnz) {
  if (nrows <= 0 || nnz <= 0) return 1;
  const i64 target = 2 * nnz / (3 * nrows);  // two thirds of the mean row length, rounded down to a power of two, at most 32 (the sweep of profiles/matrix_backend.md)
  int L = 1;
  while (L < 32 && 2 * L <= target) L *= 2;
  return L;
}

int64_t nh_cg_work_doubles(void) { return W_END; }

int nh_csr_compact(int64_t nnz, int64_t ncols, const int64_t *colidx_dev, int32_t *col32_dev, void *stream) {
  NH_REQUIRE(nnz >= 0 && ncols >= 0, "nh_csr_compact: negative size");
  NH_REQUIRE(ncols <= INT32_MAX, "nh_csr_compact: int32 column indices cannot address %lld columns", (long long)ncols);
  NH_REQUIRE(!nnz || (colidx_dev && col32_dev), "nh_csr_compact: NULL column indices");
  if (!nnz) return NH_OK;
  hipLaunchKernelGGL(k_csr_compact, dim3((unsigned)std::min<i64>((nnz + WG - 1) / WG, 256 * 32)), dim3(WG), 0, nh_stream(stream), (i64)nnz, (const i64 *)colidx_dev, col32_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_csr_spmv(const nh_csr *A, double alpha, const double *x_dev, double beta, const double *b_dev, const unsigned char *rowmask_dev, double *y_dev, void *stream) {
  if (int rc = check_csr("nh_csr_spmv", A)) return rc;
  NH_REQUIRE(!A->nrows || y_dev, "nh_csr_spmv: NULL result vector");
  NH_REQUIRE(!A->nnz || x_dev, "nh_csr_spmv: NULL argument vector");
  if (!A->nrows) return NH_OK;
  if (!A->nnz && !b_dev) {  // nothing to multiply: the result is zero, no launch
    NH_CHECK_HIP(hipMemsetAsync(y_dev, 0, sizeof(double) * (size_t)A->nrows, nh_stream(stream)));
    return NH_OK;
  }
  return spmv(A, alpha, x_dev, beta, b_dev, rowmask_dev, y_dev, Epilogue(), nh_stream(stream));
}

int nh_csr_diagonal(const nh_csr *A, double *diag_dev, void *stream) {
  if (int rc = check_csr("nh_csr_diagonal", A)) return rc;
  NH_REQUIRE(!A->nrows || diag_dev, "nh_csr_diagonal: NULL result vector");
  if (!A->nrows) return NH_OK;
  if (!A->nnz) {
    NH_CHECK_HIP(hipMemsetAsync(diag_dev, 0, sizeof(double) * (size_t)A->nrows, nh_stream(stream)));
    return NH_OK;
  }
  const dim3 grid((unsigned)((A->nrows + WG - 1) / WG));
  if (A->col32_dev)
    hipLaunchKernelGGL(k_csr_diagonal<int32_t>, grid, dim3(WG), 0, nh_stream(stream), (i64)A->nrows, (const i64 *)A->rowptr_dev, A->col32_dev, A->values_dev, diag_dev);
  else
    hipLaunchKernelGGL(k_csr_diagonal<i64>, grid, dim3(WG), 0, nh_stream(stream), (i64)A->nrows, (const i64 *)A->rowptr_dev, (const i64 *)A->colidx_dev, A->values_dev, diag_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_csr_support(const nh_csr *A, double tol, unsigned char *rowsupp_dev, unsigned char *colsupp_dev, void *stream) {
  if (int rc = check_csr("nh_csr_support", A)) return rc;
  NH_REQUIRE(tol >= 0., "nh_csr_support: the tolerance must not be negative");
  hipStream_t s = nh_stream(stream);
  if (rowsupp_dev && A->nrows) NH_CHECK_HIP(hipMemsetAsync(rowsupp_dev, 0, (size_t)A->nrows, s));
  if (colsupp_dev && A->ncols) NH_CHECK_HIP(hipMemsetAsync(colsupp_dev, 0, (size_t)A->ncols, s));
  if (!A->nrows || !A->nnz || !(rowsupp_dev || colsupp_dev)) return NH_OK;  // an empty matrix has an empty support: no launch
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (A->col32_dev)
    launch_support(L, A, A->col32_dev, tol, rowsupp_dev, colsupp_dev, s);
  else
    launch_support(L, A, (const i64 *)A->colidx_dev, tol, rowsupp_dev, colsupp_dev, s);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_cg_init(int64_t n, const double *dinv_dev, const double *r_dev, double *p_dev, double *work_dev, void *stream) {
  NH_REQUIRE(n >= 0, "nh_cg_init: negative size");
  NH_REQUIRE(work_dev && (!n || (r_dev && p_dev)), "nh_cg_init: NULL vector");
  const unsigned grid = vec_grid(n);
  if (n) {
    hipLaunchKernelGGL(k_cg_init, dim3(grid), dim3(WG), 0, nh_stream(stream), (i64)n, work_dev, dinv_dev, r_dev, p_dev);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_cg_init_scalars, dim3(1), dim3(WG), 0, nh_stream(stream), (int)grid, work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_cg_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, double *p_dev, double *q_dev, double *work_dev,
                  int niter, void *stream) {
  if (int rc = check_csr("nh_cg_iterate", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_cg_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(niter >= 0, "nh_cg_iterate: negative iteration count");
  NH_REQUIRE(work_dev && (!A->nrows || (x_dev && r_dev && p_dev && q_dev)), "nh_cg_iterate: NULL vector");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  const i64 n = A->nrows;
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  const int npq = (int)spmv_grid(n, L);
  const unsigned grid = vec_grid(n);
  nh_csr B = *A;
  B.lanes = L;
  Epilogue pq;
  pq.partial = work_dev + W_PQ;
  for (int it = 0; it < niter; ++it) {
    if (int rc = spmv(&B, 1., p_dev, 0., nullptr, rowmask_dev, q_dev, pq, s)) return rc;
    hipLaunchKernelGGL(k_cg_update, dim3(grid), dim3(WG), 0, s, n, npq, work_dev, dinv_dev, x_dev, r_dev, (const double *)p_dev, (const double *)q_dev);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cg_direction, dim3(grid), dim3(WG), 0, s, n, (int)grid, work_dev, dinv_dev, (const double *)r_dev, p_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

int64_t nh_bicgstab_work_doubles(void) { return B_END; }

int nh_csr_spmv_dots(const nh_csr *A, const double *x_dev, const double *w_dev, const unsigned char *rowmask_dev, double *y_dev, double *work_dev, void *stream) {
  if (int rc = check_csr("nh_csr_spmv_dots", A)) return rc;
  NH_REQUIRE(work_dev && (!A->nrows || (x_dev && w_dev && y_dev)), "nh_csr_spmv_dots: NULL vector");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  nh_csr B = *A;
  B.lanes = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  Epilogue e;
  e.partial = work_dev + B_WY;
  e.w = w_dev;
  e.partial2 = work_dev + B_YY;
  if (int rc = spmv(&B, 1., x_dev, 0., nullptr, rowmask_dev, y_dev, e, s)) return rc;
  hipLaunchKernelGGL(k_spmv_dots_sum, dim3(1), dim3(WG), 0, s, (int)spmv_grid(A->nrows, B.lanes), work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_bicgstab_init(int64_t n, const double *dinv_dev, const double *r_dev, double *rhat_dev, double *p_dev, double *phat_dev, double *work_dev, void *stream) {
  NH_REQUIRE(n >= 0, "nh_bicgstab_init: negative size");
  NH_REQUIRE(work_dev && (!n || (r_dev && rhat_dev && p_dev && (!dinv_dev || phat_dev))), "nh_bicgstab_init: NULL vector");
  const unsigned grid = vec_grid(n);
  if (n) {
    hipLaunchKernelGGL(k_bicgstab_init, dim3(grid), dim3(WG), 0, nh_stream(stream), (i64)n, work_dev, dinv_dev, r_dev, rhat_dev, p_dev, phat_dev);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_bicgstab_init_scalars, dim3(1), dim3(WG), 0, nh_stream(stream), (int)grid, work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_bicgstab_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, const double *rhat_dev, double *p_dev,
                        double *v_dev, double *s_dev, double *t_dev, double *phat_dev, double *shat_dev, double *work_dev, double stop_rr, int niter, void *stream) {
  if (int rc = check_csr("nh_bicgstab_iterate", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_bicgstab_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(niter >= 0, "nh_bicgstab_iterate: negative iteration count");
  NH_REQUIRE(stop_rr >= 0., "nh_bicgstab_iterate: the bound on r . r must not be negative");
  NH_REQUIRE(work_dev && (!A->nrows || (x_dev && r_dev && rhat_dev && p_dev && v_dev && s_dev && t_dev && (!dinv_dev || (phat_dev && shat_dev)))),
             "nh_bicgstab_iterate: NULL vector");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  const i64 n = A->nrows;
  nh_csr B = *A;
  B.lanes = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  const int nwy = (int)spmv_grid(n, B.lanes);
  const unsigned grid = vec_grid(n);
  const double *ph = dinv_dev ? phat_dev : p_dev, *sh = dinv_dev ? shat_dev : s_dev;  // without a preconditioner phat is p and shat is s
  Epilogue rv, ts;
  rv.partial = ts.partial = work_dev + B_WY;
  rv.partial2 = ts.partial2 = work_dev + B_YY;
  rv.w = rhat_dev;
  rv.skip = work_dev + B_ST;
  ts.w = s_dev;
  ts.skip = work_dev + B_ST_H;
  for (int it = 0; it < niter; ++it) {
    if (int rc = spmv(&B, 1., ph, 0., nullptr, rowmask_dev, v_dev, rv, s)) return rc;
    hipLaunchKernelGGL(k_bicgstab_half, dim3(grid), dim3(WG), 0, s, n, nwy, work_dev, dinv_dev, (const double *)r_dev, (const double *)v_dev, s_dev, shat_dev);
    NH_LAUNCH_CHECK();
    if (int rc = spmv(&B, 1., sh, 0., nullptr, rowmask_dev, t_dev, ts, s)) return rc;
    hipLaunchKernelGGL(k_bicgstab_update, dim3(grid), dim3(WG), 0, s, n, nwy, (int)grid, stop_rr, work_dev, x_dev, r_dev, rhat_dev, ph, sh, (const double *)s_dev,
                       (const double *)t_dev);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bicgstab_direction, dim3(grid), dim3(WG), 0, s, n, (int)grid, stop_rr, work_dev, dinv_dev, (const double *)r_dev, (const double *)v_dev, p_dev, phat_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

int64_t nh_minres_work_doubles(void) { return M_END; }

int nh_minres_init(int64_t n, const double *dinv_dev, const double *r_dev, double *r1_dev, double *r2_dev, double *v_dev, double *w1_dev, double *w2_dev, double *work_dev,
                   void *stream) {
  NH_REQUIRE(n >= 0, "nh_minres_init: negative size");
  NH_REQUIRE(work_dev && (!n || (r_dev && r1_dev && r2_dev && v_dev && w1_dev && w2_dev)), "nh_minres_init: NULL vector");
  hipStream_t s = nh_stream(stream);
  const unsigned grid = vec_grid(n);
  if (n) {
    hipLaunchKernelGGL(k_minres_init, dim3(grid), dim3(WG), 0, s, (i64)n, work_dev, dinv_dev, r_dev, r1_dev, r2_dev, w1_dev, w2_dev);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_minres_init_scalars, dim3(1), dim3(WG), 0, s, (int)grid, work_dev);
  NH_LAUNCH_CHECK();
  if (n) {
    hipLaunchKernelGGL(k_minres_first, dim3(grid), dim3(WG), 0, s, (i64)n, (const double *)work_dev, dinv_dev, r_dev, v_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

int nh_minres_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, double *r1_dev, double *r2_dev, double *v_dev,
                      double *q_dev, double *w1_dev, double *w2_dev, double *work_dev, double stop_rr, int niter, void *stream) {
  if (int rc = check_csr("nh_minres_iterate", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_minres_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(niter >= 0, "nh_minres_iterate: negative iteration count");
  NH_REQUIRE(stop_rr >= 0., "nh_minres_iterate: the bound on r . r must not be negative");
  NH_REQUIRE(work_dev && (!A->nrows || (x_dev && r_dev && r1_dev && r2_dev && v_dev && q_dev && w1_dev && w2_dev)), "nh_minres_iterate: NULL vector");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  const i64 n = A->nrows;
  nh_csr B = *A;
  B.lanes = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  const int nvq = (int)spmv_grid(n, B.lanes);
  const unsigned grid = vec_grid(n);
  Epilogue vq;  // w = x = v: the partials of v . q (and of q . q, which nothing reads)
  vq.partial = work_dev + M_VQ;
  vq.partial2 = work_dev + M_QQ;
  vq.w = v_dev;
  vq.skip = work_dev + M_ST;
  for (int it = 0; it < niter; ++it) {
    if (int rc = spmv(&B, 1., v_dev, 0., nullptr, rowmask_dev, q_dev, vq, s)) return rc;
    hipLaunchKernelGGL(k_minres_lanczos, dim3(grid), dim3(WG), 0, s, n, nvq, (int)grid, stop_rr, work_dev, dinv_dev, (const double *)q_dev, r1_dev, r2_dev);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_minres_update, dim3(grid), dim3(WG), 0, s, n, (int)grid, work_dev, dinv_dev, x_dev, r_dev, (const double *)r2_dev, v_dev, w1_dev, w2_dev);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_minres_finish, dim3(1), dim3(WG), 0, s, (int)grid, work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int64_t nh_gmres_work_doubles(int restart) {
  if (restart < 1) {
    nh_set_error("nh_gmres_work_doubles: restart must be at least 1 (got %d)", restart);
    return -1;
  }
  return gmres_cells(restart).end;
}

int nh_gmres_init(int64_t n, int restart, const double *dinv_dev, const double *r_dev, double *V_dev, double *z_dev, double *work_dev, void *stream) {
  NH_REQUIRE(n >= 0, "nh_gmres_init: negative size");
  NH_REQUIRE(restart >= 1, "nh_gmres_init: restart must be at least 1 (got %d)", restart);
  NH_REQUIRE(work_dev && (!n || (r_dev && V_dev && z_dev)), "nh_gmres_init: NULL vector");
  hipStream_t s = nh_stream(stream);
  const unsigned grid = vec_grid(n);
  if (n) {
    hipLaunchKernelGGL(k_gmres_norm, dim3(grid), dim3(WG), 0, s, (i64)n, restart, r_dev, work_dev);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_gmres_init_scalars, dim3(1), dim3(WG), 0, s, (int)grid, restart, work_dev);
  NH_LAUNCH_CHECK();
  if (n) {
    if (gs_pairs(n, {dinv_dev, r_dev, V_dev, z_dev}))
      hipLaunchKernelGGL(k_gmres_normalize<2>, dim3(gs_grid(n, 2)), dim3(WG), 0, s, (i64)n, restart, dinv_dev, r_dev, V_dev, z_dev, (const double *)work_dev);
    else
      hipLaunchKernelGGL(k_gmres_normalize<1>, dim3(gs_grid(n, 1)), dim3(WG), 0, s, (i64)n, restart, dinv_dev, r_dev, V_dev, z_dev, (const double *)work_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

int nh_gmres_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *V_dev, double *z_dev, double *w_dev, double *work_dev, int restart,
                     double stop_rr, int niter, void *stream) {
  if (int rc = check_csr("nh_gmres_iterate", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_gmres_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(restart >= 1, "nh_gmres_iterate: restart must be at least 1 (got %d)", restart);
  NH_REQUIRE(niter >= 0, "nh_gmres_iterate: negative iteration count");
  NH_REQUIRE(stop_rr >= 0., "nh_gmres_iterate: the bound on r . r must not be negative");
  NH_REQUIRE(work_dev && (!A->nrows || (V_dev && z_dev && w_dev)), "nh_gmres_iterate: NULL vector");
  if (!A->nrows) return NH_OK;
  nh_csr B = *A;
  B.lanes = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (gs_pairs(A->nrows, {dinv_dev, V_dev, z_dev, w_dev}))
    return gmres_steps<2>(&B, rowmask_dev, dinv_dev, V_dev, z_dev, w_dev, work_dev, restart, stop_rr, niter, nh_stream(stream));
  return gmres_steps<1>(&B, rowmask_dev, dinv_dev, V_dev, z_dev, w_dev, work_dev, restart, stop_rr, niter, nh_stream(stream));
}

int nh_gmres_update(int64_t n, int restart, const double *dinv_dev, const double *V_dev, double *x_dev, double *work_dev, void *stream) {
  NH_REQUIRE(n >= 0, "nh_gmres_update: negative size");
  NH_REQUIRE(restart >= 1, "nh_gmres_update: restart must be at least 1 (got %d)", restart);
  NH_REQUIRE(work_dev && (!n || (V_dev && x_dev)), "nh_gmres_update: NULL vector");
  if (!n) return NH_OK;
  hipStream_t s = nh_stream(stream);
  hipLaunchKernelGGL(k_gmres_solve, dim3(1), dim3(WG), 0, s, restart, work_dev);
  NH_LAUNCH_CHECK();
  if (gs_pairs(n, {dinv_dev, V_dev, x_dev}))
    hipLaunchKernelGGL((k_gmres_xupdate<GS_CHUNK, 2>), dim3(gs_grid(n, 2)), dim3(WG), 0, s, (i64)n, restart, dinv_dev, V_dev, x_dev, (const double *)work_dev);
  else
    hipLaunchKernelGGL((k_gmres_xupdate<GS_CHUNK, 1>), dim3(gs_grid(n, 1)), dim3(WG), 0, s, (i64)n, restart, dinv_dev, V_dev, x_dev, (const double *)work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

}  // extern "C"
