// Device-resident CSR matrix: product, diagonal and a preconditioned conjugate-gradient iteration that never leaves the device
// (the vendor-backend slot of the reference: matrix/_mkl.py multiplies and solves with the library that owns the data; here the
// triplet that the assembly kernels leave in HBM is used where it lies).
//
//   * k_csr_spmv<L, Idx, DOT>: y = mask(alpha A x + beta b).  L lanes own a row (L = 1 .. 64, a power of two); consecutive lane groups
//     of a wave take consecutive rows, so a wave reads one contiguous span of values / column indices; rows longer than L are walked
//     in strides of L and the L partial sums are folded with __shfl_xor in a fixed order.  A workgroup strides over the rows, the grid
//     is a function of (nrows, L) only, nothing is atomic: repeated calls are bit-identical.  Column indices are int32 (narrowed once
//     per matrix by nh_csr_compact: 12 instead of 16 bytes per entry) or the int64 of the assembly; rowptr stays int64.
//     DOT: additionally the workgroup's share of x . y goes to partial[blockIdx.x] (the p . Ap of a CG step).
//   * k_cg_update / k_cg_direction: the vector half of a CG step.  Every workgroup sums the partials of the kernel before it in the
//     same order and so holds the same alpha / beta; scalars that cross an iteration live in two cells each, one written and one read
//     per kernel, so no kernel reads a cell that one of its own workgroups writes.
#include "nh_common.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int WG = 256;
constexpr int SPMV_MAX_WGS = 2048;  // 8 waves per SIMD on 256 CUs; also the number of p . Ap partials every workgroup of k_cg_update sums
constexpr int VEC_MAX_WGS = 1024;

// cells of the CG work array (doubles)
enum { W_RR = 0, W_FLAG_B = 1, W_FLAG_A = 2, W_RZ_A = 3, W_RZ_B = 4, W_PQ = 8, W_RZP = W_PQ + SPMV_MAX_WGS, W_RRP = W_RZP + VEC_MAX_WGS, W_END = W_RRP + VEC_MAX_WGS };

// sum over the workgroup in a fixed order; every thread returns the total
__device__ __forceinline__ double block_sum(double s, double *lds) {
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();  // (lds may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// sum of n partials, the same order in every workgroup
__device__ __forceinline__ double partial_sum(const double *part, int n, double *lds) {
  double s = 0;
  for (int j = threadIdx.x; j < n; j += WG) s += part[j];
  return block_sum(s, lds);
}

template <int L, class Idx, bool DOT>
__global__ __launch_bounds__(WG) void k_csr_spmv(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                                 const double *__restrict__ x, double alpha, double beta, const double *b, const unsigned char *__restrict__ mask, double *y,
                                                 double *partial) {
  constexpr int G = WG / L;  // rows per workgroup and step
  const int lane = threadIdx.x & (L - 1);
  double dot = 0;
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
      if (DOT) dot += x[row] * v;
    }
  }
  if (DOT) {
    __shared__ double lds[4];
    dot = block_sum(dot, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = dot;
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
  }
}

// alpha = r.z / p.q;  x += alpha p;  r -= alpha q;  partials of r . z and r . r with z = dinv r.
// reads RR, RZ_B, FLAG_A, the p.q partials; writes RZ_A, FLAG_B, the r.z / r.r partials
__global__ __launch_bounds__(WG) void k_cg_update(i64 n, int npq, double *work, const double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r,
                                                  const double *__restrict__ p, const double *__restrict__ q) {
  __shared__ double lds[4];
  const double pq = partial_sum(work + W_PQ, npq, lds);
  const double rz = work[W_RZ_B], rr = work[W_RR];
  bool bad = work[W_FLAG_A] != 0.;
  const bool done = rr == 0.;  // the residual vanished: nothing left to do, and p . q = 0 is no breakdown
  if (!done && !bad) bad = !(rz > 0. && rz <= 1.7976931348623157e308 && pq > 0. && pq <= 1.7976931348623157e308);
  const bool move = !done && !bad;
  const double alpha = move ? rz / pq : 0.;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[W_RZ_A] = rz;
    work[W_FLAG_B] = bad ? 1. : 0.;
  }
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

// beta = r.z (new) / r.z (old);  p = z + beta p.  reads RZ_A, FLAG_B, the partials; writes RR, RZ_B, FLAG_A
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
  if (bad) return;
  const double beta = rz_old != 0. ? rz / rz_old : 0.;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double zi = dinv ? dinv[i] * r[i] : r[i];
    p[i] = zi + beta * p[i];
  }
}

bool lanes_ok(int lanes) { return lanes >= 0 && lanes <= 64 && (lanes & (lanes - 1)) == 0; }

int check_csr(const char *who, const nh_csr *A) {
  NH_REQUIRE(A, "%s: NULL matrix", who);
  NH_REQUIRE(A->nrows >= 0 && A->ncols >= 0 && A->nnz >= 0, "%s: negative size (%lld x %lld, %lld entries)", who, (long long)A->nrows, (long long)A->ncols, (long long)A->nnz);
  NH_REQUIRE(lanes_ok(A->lanes), "%s: lanes per row must be 0 or a power of two <= 64 (got %d)", who, A->lanes);
  NH_REQUIRE(!A->nrows || A->rowptr_dev, "%s: NULL row pointers", who);
  NH_REQUIRE(!A->nnz || (A->values_dev && (A->colidx_dev || A->col32_dev)), "%s: NULL values or column indices", who);
  NH_REQUIRE(!A->col32_dev || A->ncols <= INT32_MAX, "%s: int32 column indices cannot address %lld columns", who, (long long)A->ncols);
  return NH_OK;
}

unsigned spmv_grid(i64 nrows, int L) { return (unsigned)std::min<i64>((nrows + WG / L - 1) / (WG / L), SPMV_MAX_WGS); }
unsigned vec_grid(i64 n) { return (unsigned)std::min<i64>((n + WG - 1) / WG, VEC_MAX_WGS); }

template <int L, class Idx>
void launch_lanes(const nh_csr *A, const Idx *col, double alpha, const double *x, double beta, const double *b, const unsigned char *mask, double *y, double *partial,
                  hipStream_t s) {
  const dim3 grid(spmv_grid(A->nrows, L));
  if (partial)
    hipLaunchKernelGGL((k_csr_spmv<L, Idx, true>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, x, alpha, beta, b, mask, y, partial);
  else
    hipLaunchKernelGGL((k_csr_spmv<L, Idx, false>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, x, alpha, beta, b, mask, y, partial);
}

template <class Idx>
void launch_idx(int L, const nh_csr *A, const Idx *col, double alpha, const double *x, double beta, const double *b, const unsigned char *mask, double *y, double *partial,
                hipStream_t s) {
  switch (L) {
    case 1: launch_lanes<1>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
    case 2: launch_lanes<2>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
    case 4: launch_lanes<4>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
    case 8: launch_lanes<8>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
    case 16: launch_lanes<16>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
    case 32: launch_lanes<32>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
    default: launch_lanes<64>(A, col, alpha, x, beta, b, mask, y, partial, s); break;
  }
}

int spmv(const nh_csr *A, double alpha, const double *x, double beta, const double *b, const unsigned char *mask, double *y, double *partial, hipStream_t s) {
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (A->col32_dev)
    launch_idx(L, A, A->col32_dev, alpha, x, beta, b, mask, y, partial, s);
  else
    launch_idx(L, A, (const i64 *)A->colidx_dev, alpha, x, beta, b, mask, y, partial, s);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

}  // namespace

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
  return spmv(A, alpha, x_dev, beta, b_dev, rowmask_dev, y_dev, nullptr, nh_stream(stream));
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
  for (int it = 0; it < niter; ++it) {
    if (int rc = spmv(&B, 1., p_dev, 0., nullptr, rowmask_dev, q_dev, work_dev + W_PQ, s)) return rc;
    hipLaunchKernelGGL(k_cg_update, dim3(grid), dim3(WG), 0, s, n, npq, work_dev, dinv_dev, x_dev, r_dev, (const double *)p_dev, (const double *)q_dev);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cg_direction, dim3(grid), dim3(WG), 0, s, n, (int)grid, work_dev, dinv_dev, (const double *)r_dev, p_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

}  // extern "C"
