// Smoothed-aggregation algebraic multigrid as the preconditioner of the device CG solve: the numeric phase of the setup, the V-cycle, and a conjugate-gradient
// iteration whose preconditioner is that cycle.  The symbolic phase (aggregates, patterns, expand-sort-compress plans) is torch plumbing (nutils_amd/amg.py);
// what is here reads value arrays.  The rules are those of nh_csr.hip: nothing atomic, every sum in a fixed order, launch geometry a function of sizes only,
// repeated calls bit-identical.
//
//   * k_segment_dot<L>: out[s] = sum_k a[ia[k]] b[ib[k]] over k = ptr[s] .. ptr[s+1] - 1 (b == NULL: a plain segment sum) -- a sparse product whose
//     products have been listed and sorted by output entry beforehand.  L lanes own a segment, consecutive lane groups take consecutive segments (so a
//     wave reads one contiguous span of the index arrays), segments longer than L are walked in strides of L and folded with __shfl_xor: the mapping
//     of k_csr_spmv.  It evaluates A T, A P and R (A P) of every level.
//   * k_block_segment_dot<K, PK, QK>: the same products stated over blocks, for a hierarchy with a near-nullspace of K vectors: a segment is an output block
//     (P x K), the sum of products of a block (P x Q) with a block (Q x K), P and Q each 1 or K; the blocks lie in scalar CSR value arrays and are found by
//     their first entry and their row stride.  One lane per entry of an output block walks the segment; the index arrays are read once per block product.
//   * k_aggregate_qr<L>: the aggregate-wise thin QR of a near-nullspace B [n x k], k <= 6, by Gram-Schmidt in two passes: Q [n x k] holds the values of the
//     tentative prolongator, the triangles R are the near-nullspace of the next level.  L lanes own an aggregate (chosen from the mean size as above), rows
//     strided over them, norms and dots folded with __shfl_xor.  Once per hierarchy build.
//   * k_jacobi<L, Idx>: y = x + w (b - A x) on the rows the mask keeps, 0 elsewhere, in one launch (k_csr_spmv with another epilogue; y != x).
//   * k_chebyshev<L, Idx, FIRST>: a step of the Chebyshev smoother, dout = c1 d + c2 dinv (b - A x), y = x + dout, on the mapping of k_jacobi; k_chebyshev_start
//     is the step from x = 0.  The coefficient pairs of a level's polynomial are a small device array the host computed from its eigenvalue bounds.
//   * k_lanczos_*: the Lanczos recurrence on S A_f S that estimates the largest eigenvalue of D^-1 A_f for those bounds: three launches a step (product with the
//     partials of q . w; update with the partials of w . w; normalisation, which stores alpha and beta), a pair of status cells that makes later steps idle.
//   * k_scale: y = w b, the sweep that starts from zero, and the solve of a diagonal terminal level.
//   * k_dense: z = Ainv b for the coarsest level, one workgroup, a wave per row, lanes over the columns.
//   * the cycle (amg_cycle) is a host loop over the level descriptions that enqueues those kernels and nh_csr_spmv (residual, restriction,
//     prolongate-and-add); with one sweep that is five launches per level and one for the coarsest.
//   * nh_fgmres_iterate: flexible GMRES with the cycle as its preconditioner: t = M z by amg_cycle, then the Arnoldi step of nh_csr.hip from the product input t
//     (nh_gmres_step_from), which keeps t as a column of Z.  No kernel of its own here.
//   * the block preconditioner of a saddle point K = [[A, Bt], [B, C]] (nh_schur_*): k_schur_diagonal<L, Idx> forms the SIMPLE diagonal of the approximate Schur
//     complement on the mapping of k_csr_spmv; the application z2 = sinv r (k_schur_scale), t = mask1(r - K z2) (nh_csr_spmv), z1 = cycle(t) (amg_cycle on the
//     hierarchy of the first block), z = z1 + z2 (k_schur_merge) is a host sequence; nh_fgmres_iterate_schur is nh_fgmres_iterate with that application.
//   * k_pcg_*: CG with z = M r handed in.  An iteration: q = mask(A p) with the partials of p . q (the DOT = 1 product of nh_csr.hip); update (alpha, x,
//     r, partials of r . r); the cycle; partials of r . z; direction (beta, p = z + beta p).  The cell discipline is that of k_cg_update / k_cg_direction.
#include "nh_common.h"
#include <algorithm>
#include <climits>
#include <cstdint>
#include <new>
#include <vector>

struct nh_amg {
  std::vector<nh_amg_level> levels;
};

// views, like nh_amg: the hierarchy of the first block, the matrix the operator was built on, the mask of the first field, the inverse Schur diagonal (0 off the
// second field) and two scratch vectors
struct nh_schur {
  const nh_amg *first;
  nh_csr K;
  const unsigned char *mask1;
  const double *sinv;
  double *z2, *t;
};

namespace {

#include "nh_krylov.inc"  // WG, the grid caps, block_sum, partial_sum, check_csr, spmv_grid, vec_grid, and the cells W_RR, W_FLAG_B, W_STOP: shared with nh_csr.hip

constexpr int DENSE_WG = 1024;

// the other cells of the work array of nh_pcg_* (the first three are W_RR, W_FLAG_B, W_STOP, as in nh_cg_*)
enum { P_FLAG_A = 3, P_RZ_A = 4, P_RZ_B = 5, P_PQ = 8, P_RZP = P_PQ + SPMV_MAX_WGS, P_RRP = P_RZP + VEC_MAX_WGS, P_END = P_RRP + VEC_MAX_WGS };

template <int L>
__global__ __launch_bounds__(WG) void k_segment_dot(i64 nseg, const i64 *__restrict__ ptr, const int32_t *__restrict__ ia, const int32_t *__restrict__ ib,
                                                    const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  for (i64 base = (i64)blockIdx.x * G; base < nseg; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the shuffles)
    const i64 seg = base + threadIdx.x / L;
    const bool live = seg < nseg;
    double s = 0;
    if (live) {
      const i64 k1 = ptr[seg + 1];
      if (b) {
#pragma unroll 2
        for (i64 k = ptr[seg] + lane; k < k1; k += L) s += a[ia[k]] * b[ib[k]];
      } else {
#pragma unroll 2
        for (i64 k = ptr[seg] + lane; k < k1; k += L) s += a[ia[k]];
      }
    }
#pragma unroll
    for (int o = L >> 1; o; o >>= 1) s += __shfl_xor(s, o, L);
    if (live && lane == 0) out[seg] = s;
  }
}

constexpr int QR_MAXK = 6;

// The sparse products of a hierarchy with a near-nullspace of K vectors, stated over blocks: segment s is the output block (P x K) at out[of[s] + r os[s] + c],
// the sum over its products k of the block (P x Q) at a[ia[k] + r sa[s] + t] times the block (Q x K) at b[ib[k] + t sb[k] + c] (sb NULL: the stride bstride
// for every product, the rows of Q [n x K]).  P and Q are 1 or K.  One lane owns one entry (r, c) of one output block and walks the products of its segment
// in the order of the plan, t ascending within a product: one accumulator, nothing crosses lanes.  The P K lanes of a segment are neighbours, so they read the
// same index words (one request) and the K consecutive doubles of a row of the second factor; the index arrays are read once per block product, where
// k_segment_dot reads a pair for every multiply-add.
template <int K, bool PK, bool QK>
__global__ __launch_bounds__(WG) void k_block_segment_dot(i64 nseg, const i64 *__restrict__ ptr, const int32_t *__restrict__ ia, const int32_t *__restrict__ ib,
                                                          const int32_t *__restrict__ sa, const int32_t *__restrict__ sb, int bstride,
                                                          const int32_t *__restrict__ of, const int32_t *__restrict__ os, const double *__restrict__ a,
                                                          const double *__restrict__ b, double *__restrict__ out) {
  constexpr int P = PK ? K : 1, Q = QK ? K : 1, E = P * K;
  const i64 total = nseg * E;
  for (i64 g = (i64)blockIdx.x * WG + threadIdx.x; g < total; g += (i64)gridDim.x * WG) {
    const i64 seg = g / E;
    const int e = (int)(g - seg * E), r = e / K, c = e - r * K;
    const i64 k1 = ptr[seg + 1];
    const i64 arow = P > 1 ? (i64)r * sa[seg] : 0;
    double s = 0;
#pragma unroll 2
    for (i64 k = ptr[seg]; k < k1; ++k) {
      const double *ap = a + (ia[k] + arow);
      const double *bp = b + ((i64)ib[k] + c);
      const i64 st = Q > 1 ? (sb ? sb[k] : bstride) : 0;
#pragma unroll
      for (int t = 0; t < Q; ++t) s += ap[t] * bp[t * st];
    }
    out[of[seg] + (P > 1 ? (i64)r * os[seg] : 0) + c] = s;
  }
}

template <int L>
__device__ __forceinline__ double group_sum(double s) {
#pragma unroll
  for (int o = L >> 1; o; o >>= 1) s += __shfl_xor(s, o, L);
  return s;  // (the same bits on every lane of the group: each fold adds the same two numbers)
}

// Thin QR of B on the rows of every aggregate.  L lanes own an aggregate, its rows midx[mptr[a]] .. are strided over them; Q is the working storage (a lane
// only ever revisits its own rows, what crosses lanes goes through the folds), every control decision around a fold is uniform over the wave (k is, and a
// dropped column changes values, not the path).  Column j: n0 from B; the second Gram-Schmidt pass against q_0 .. q_(j-1), one after the other (the first
// was made when each of them was finished); n1; drop or normalise; and in the same pass over the rows the k - j - 1 dots of q_j with the columns to come,
// whose first pass that is.  Lane 0 keeps R in Rc: the first coefficient is stored, the second added to it.
template <int L>
__global__ __launch_bounds__(WG) void k_aggregate_qr(i64 nagg, const i64 *__restrict__ mptr, const int32_t *__restrict__ midx, int k, const double *__restrict__ B,
                                                     double *__restrict__ Q, double *__restrict__ Rc) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  for (i64 base = (i64)blockIdx.x * G; base < nagg; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the folds)
    const i64 a = base + threadIdx.x / L;
    const bool live = a < nagg;
    const i64 m0 = live ? mptr[a] + lane : 0, m1 = live ? mptr[a + 1] : 0;
    const bool writer = live && lane == 0;
    double *R = Rc + a * k * k;
    for (i64 m = m0; m < m1; m += L) {
      const i64 i = (i64)midx[m] * k;
      for (int j = 0; j < k; ++j) Q[i + j] = B[i + j];
    }
    for (int j = 0; j < k; ++j) {
      double s = 0;
      for (i64 m = m0; m < m1; m += L) {
        const double v = B[(i64)midx[m] * k + j];
        s += v * v;
      }
      const double n0 = sqrt(group_sum<L>(s));
      for (int l = 0; l < j; ++l) {
        double c = 0;
        for (i64 m = m0; m < m1; m += L) {
          const i64 i = (i64)midx[m] * k;
          c += Q[i + l] * Q[i + j];
        }
        c = group_sum<L>(c);
        for (i64 m = m0; m < m1; m += L) {
          const i64 i = (i64)midx[m] * k;
          Q[i + j] -= c * Q[i + l];
        }
        if (writer) R[l * k + j] += c;
      }
      s = 0;
      for (i64 m = m0; m < m1; m += L) {
        const double v = Q[(i64)midx[m] * k + j];
        s += v * v;
      }
      const double n1 = sqrt(group_sum<L>(s));
      const bool keep = n1 > 0x1p-26 * n0;  // below a relative sqrt(u) nothing of the column is left that is not rounding
      double c[QR_MAXK - 1];
#pragma unroll
      for (int t = 0; t < QR_MAXK - 1; ++t) c[t] = 0;
      for (i64 m = m0; m < m1; m += L) {
        const i64 i = (i64)midx[m] * k;
        const double q = keep ? Q[i + j] / n1 : 0.;
        Q[i + j] = q;
#pragma unroll
        for (int t = 0; t < QR_MAXK - 1; ++t)
          if (j + 1 + t < k) c[t] += q * Q[i + j + 1 + t];
      }
#pragma unroll
      for (int t = 0; t < QR_MAXK - 1; ++t)
        if (j + 1 + t < k) c[t] = group_sum<L>(c[t]);
      for (i64 m = m0; m < m1; m += L) {
        const i64 i = (i64)midx[m] * k;
        const double q = Q[i + j];
#pragma unroll
        for (int t = 0; t < QR_MAXK - 1; ++t)
          if (j + 1 + t < k) Q[i + j + 1 + t] -= c[t] * q;
      }
      if (writer) {
        for (int l = 0; l < j; ++l) R[j * k + l] = 0.;
        R[j * k + j] = keep ? n1 : 0.;
#pragma unroll
        for (int t = 0; t < QR_MAXK - 1; ++t)
          if (j + 1 + t < k) R[j * k + j + 1 + t] = c[t];
      }
    }
  }
}

template <int L, class Idx>
__global__ __launch_bounds__(WG) void k_jacobi(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                               const double *__restrict__ x, const double *__restrict__ w, const double *__restrict__ b,
                                               const unsigned char *__restrict__ mask, double *__restrict__ y) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {
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
    if (live && lane == 0) y[row] = on ? x[row] + w[row] * (b[row] - s) : 0.;
  }
}

__global__ __launch_bounds__(WG) void k_scale(i64 n, const double *__restrict__ w, const double *__restrict__ b, double *__restrict__ y) {
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) y[i] = w[i] * b[i];
}

// out[row] = A[row, row] - sum over the entries k of the row with first[col[k]] of values[k] vt[k] dinv[col[k]]: the diagonal of C - B diag(A)^-1 Bt on the rows of
// the second field when vt holds the values of the transpose on the same pattern, first marks the first field and dinv = 1 / diag there.  The mapping and the
// fold of k_csr_spmv, for the two sums.
template <int L, class Idx>
__global__ __launch_bounds__(WG) void k_schur_diagonal(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                                       const double *__restrict__ vt, const unsigned char *__restrict__ first, const double *__restrict__ dinv,
                                                       double *__restrict__ out) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the shuffles)
    const i64 row = base + threadIdx.x / L;
    const bool live = row < nrows;
    double d = 0, s = 0;
    if (live) {
      const i64 k1 = rowptr[row + 1];
      for (i64 k = rowptr[row] + lane; k < k1; k += L) {
        const i64 c = (i64)col[k];
        if (c == row) d += values[k];
        if (first[c]) s += values[k] * vt[k] * dinv[c];
      }
    }
#pragma unroll
    for (int o = L >> 1; o; o >>= 1) {
      d += __shfl_xor(d, o, L);
      s += __shfl_xor(s, o, L);
    }
    if (live && lane == 0) out[row] = d - s;
  }
}

// z2 = sinv r where sinv != 0 (the second field), +0 elsewhere: r is not read off the second field
__global__ __launch_bounds__(WG) void k_schur_scale(i64 n, const double *__restrict__ sinv, const double *__restrict__ r, double *__restrict__ z2) {
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double w = sinv[i];
    z2[i] = w != 0. ? w * r[i] : 0.;
  }
}

// z += z2: the two parts have disjoint supports
__global__ __launch_bounds__(WG) void k_schur_merge(i64 n, const double *__restrict__ z2, double *__restrict__ z) {
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) z[i] += z2[i];
}

// One step of the Chebyshev smoother: dout = c1 d + c2 dinv (b - A x), y = x + dout on the rows the mask keeps, +0 in both elsewhere (k_jacobi with another
// epilogue; y != x).  coef = (c1, c2) on the device.  FIRST: the first step of a polynomial, which has no d term: neither d nor c1 is read.  d and dout are not
// restrict: a row reads d[row] before it writes dout[row] and no other row does either, so the update may be in place.
template <int L, class Idx, bool FIRST>
__global__ __launch_bounds__(WG) void k_chebyshev(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                                  const double *__restrict__ x, const double *d, const double *__restrict__ dinv, const double *__restrict__ b,
                                                  const double *__restrict__ coef, const unsigned char *__restrict__ mask, double *__restrict__ y, double *dout) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  const double c1 = FIRST ? 0. : coef[0], c2 = coef[1];
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {
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
      double v = 0., xi = 0.;
      if (on) {
        v = c2 * dinv[row] * (b[row] - s);
        if (!FIRST) v += c1 * d[row];
        xi = x[row] + v;
      }
      dout[row] = v;
      y[row] = xi;
    }
  }
}

// x = d = c2 w b: step 0 of the polynomial from x = 0, which needs no product
__global__ __launch_bounds__(WG) void k_chebyshev_start(i64 n, const double *__restrict__ coef, const double *__restrict__ w, const double *__restrict__ b,
                                                        double *__restrict__ d, double *__restrict__ x) {
  const double c2 = coef[1];
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double v = c2 * w[i] * b[i];
    d[i] = v;
    x[i] = v;
  }
}

// The Lanczos recurrence on S A_f S (nh_csr_lanczos).  The cells of its work array: who stopped (two cells, one read and one written per kernel, as in the CG
// kernels: ST_B is read by the product and the update, which copies it to ST_A; ST_A is read by the normalisation, which writes ST_B), alpha of the step (written
// by the update, read by the normalisation), beta (written by the normalisation, read by the next update), and the partials of the two dots.
enum { Z_ST_A = 0, Z_ST_B = 1, Z_ALPHA = 2, Z_BETA = 3, Z_PA = 8, Z_PB = Z_PA + SPMV_MAX_WGS, Z_END = Z_PB + VEC_MAX_WGS };
static_assert(Z_END <= NH_LANCZOS_CELLS, "the cells of nh_csr_lanczos outgrow what the header promises");

__device__ __forceinline__ bool positive_finite(double v) { return v > 0. && v <= 1.7976931348623157e308; }

// q = u on the rows that take part (mask, s != 0), 0 elsewhere; partials of q . q
__global__ __launch_bounds__(WG) void k_lanczos_start(i64 n, const double *__restrict__ u, const double *__restrict__ s, const unsigned char *__restrict__ mask,
                                                      double *__restrict__ q, double *work) {
  __shared__ double lds[4];
  double acc = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double v = (!mask || mask[i]) && s[i] != 0. ? u[i] : 0.;
    q[i] = v;
    acc += v * v;
  }
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) work[Z_PB + blockIdx.x] = acc;
}

// q_0 = q / |q|, sq = s q_0, the cells; a start vector without a finite positive norm stops the recurrence before its first step
__global__ __launch_bounds__(WG) void k_lanczos_first(i64 n, int nparts, const double *__restrict__ s, double *__restrict__ q, double *__restrict__ sq, double *work) {
  __shared__ double lds[4];
  const double norm = sqrt(partial_sum(work + Z_PB, nparts, lds));
  const bool stop = !positive_finite(norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[Z_ST_A] = work[Z_ST_B] = stop ? 1. : 0.;
    work[Z_ALPHA] = work[Z_BETA] = 0.;
  }
  if (stop) return;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double v = q[i] / norm;
    q[i] = v;
    sq[i] = s[i] * v;
  }
}

// w = s mask(A sq), partials of q . w (k_csr_spmv with DOT = 1 and another epilogue)
template <int L, class Idx>
__global__ __launch_bounds__(WG) void k_lanczos_product(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                                        const double *__restrict__ sq, const double *__restrict__ s, const double *__restrict__ q,
                                                        const unsigned char *__restrict__ mask, double *__restrict__ w, double *work) {
  if (work[Z_ST_B] != 0.) return;
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  double dot = 0;
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {
    const i64 row = base + threadIdx.x / L;
    const bool live = row < nrows;
    const bool on = live && (!mask || mask[row]);
    double t = 0;
    if (on) {
      const i64 k1 = rowptr[row + 1];
#pragma unroll 2
      for (i64 k = rowptr[row] + lane; k < k1; k += L) t += values[k] * sq[col[k]];
    }
#pragma unroll
    for (int o = L >> 1; o; o >>= 1) t += __shfl_xor(t, o, L);
    if (live && lane == 0) {
      const double v = on ? s[row] * t : 0.;
      w[row] = v;
      dot += q[row] * v;
    }
  }
  __shared__ double lds[4];
  dot = block_sum(dot, lds);
  if (threadIdx.x == 0) work[Z_PA + blockIdx.x] = dot;
}

// alpha = q . w; w -= alpha q + beta qprev (first: beta = 0 and qprev is not read); partials of w . w
__global__ __launch_bounds__(WG) void k_lanczos_update(i64 n, int npa, int first, const double *__restrict__ q, const double *__restrict__ qprev, double *__restrict__ w,
                                                       double *work) {
  __shared__ double lds[4];
  const bool stopped = work[Z_ST_B] != 0.;
  if (blockIdx.x == 0 && threadIdx.x == 0) work[Z_ST_A] = stopped ? 1. : 0.;
  if (stopped) return;
  const double alpha = partial_sum(work + Z_PA, npa, lds), beta = work[Z_BETA];
  if (blockIdx.x == 0 && threadIdx.x == 0) work[Z_ALPHA] = alpha;
  double acc = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    double v = w[i] - alpha * q[i];
    if (!first) v -= beta * qprev[i];
    w[i] = v;
    acc += v * v;
  }
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) work[Z_PB + blockIdx.x] = acc;
}

// beta = |w|; alpha_j, beta_(j+1) and the count to `out`; q_(j+1) = w / beta in place, sq = s q_(j+1).  beta = 0 or not finite: the recurrence ends here
__global__ __launch_bounds__(WG) void k_lanczos_normalize(i64 n, int nparts, int j, int steps, const double *__restrict__ s, double *__restrict__ w, double *__restrict__ sq,
                                                          double *work, double *__restrict__ out) {
  __shared__ double lds[4];
  const bool stopped = work[Z_ST_A] != 0.;
  if (stopped) {
    if (blockIdx.x == 0 && threadIdx.x == 0) work[Z_ST_B] = 1.;
    return;
  }
  const double beta = sqrt(partial_sum(work + Z_PB, nparts, lds));
  const bool stop = !positive_finite(beta);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[2 * j] = work[Z_ALPHA];
    out[2 * j + 1] = beta;
    out[2 * steps] = j + 1;
    work[Z_BETA] = beta;
    work[Z_ST_B] = stop ? 1. : 0.;
  }
  if (stop) return;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double v = w[i] / beta;
    w[i] = v;
    sq[i] = s[i] * v;
  }
}

// z[idx[i]] = sum_j Ainv[i][j] b[idx[j]], i < m (idx == NULL: the identity); other rows of z are not touched (the caller has zeroed them).  One workgroup: a
// wave per row, its lanes stride over the columns and are folded in a fixed order.
__global__ __launch_bounds__(DENSE_WG) void k_dense(int m, const double *__restrict__ Ainv, const double *__restrict__ b, const int32_t *__restrict__ idx,
                                                    double *__restrict__ z) {
  __shared__ double bs[1024];
  for (int j = threadIdx.x; j < m; j += DENSE_WG) bs[j] = b[idx ? idx[j] : j];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < m; i += DENSE_WG / 64) {
    const double *row = Ainv + (i64)i * m;
    double s = 0;
    for (int j = lane; j < m; j += 64) s += row[j] * bs[j];
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) z[idx ? idx[i] : i] = s;
  }
}

// p = z, partials of r . z and r . r
__global__ __launch_bounds__(WG) void k_pcg_init(i64 n, double *work, const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ p) {
  __shared__ double lds[4];
  double rz = 0, rr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    const double ri = r[i], zi = z[i];
    p[i] = zi;
    rz += ri * zi;
    rr += ri * ri;
  }
  rz = block_sum(rz, lds);
  rr = block_sum(rr, lds);
  if (threadIdx.x == 0) {
    work[P_RZP + blockIdx.x] = rz;
    work[P_RRP + blockIdx.x] = rr;
  }
}

__global__ __launch_bounds__(WG) void k_pcg_init_scalars(int nparts, double *work) {
  __shared__ double lds[4];
  const double rz = partial_sum(work + P_RZP, nparts, lds);
  const double rr = partial_sum(work + P_RRP, nparts, lds);
  if (threadIdx.x == 0) {
    work[W_RR] = rr;
    work[P_RZ_B] = rz;
    work[P_RZ_A] = rz;
    work[P_FLAG_A] = 0.;
    work[W_FLAG_B] = 0.;
    work[W_STOP] = 0.;
  }
}

// alpha = r.z / p.q;  x += alpha p;  r -= alpha q;  partials of r . r.  reads RR, RZ_B, FLAG_A, STOP, the p.q partials; writes RZ_A, FLAG_B, the r.r partials
// (not when done or stalled: r has not moved, they stand)
__global__ __launch_bounds__(WG) void k_pcg_update(i64 n, int npq, double *work, double *__restrict__ x, double *__restrict__ r, const double *__restrict__ p,
                                                   const double *__restrict__ q) {
  __shared__ double lds[4];
  const double pq = partial_sum(work + P_PQ, npq, lds);
  const double rz = work[P_RZ_B], rr = work[W_RR];
  bool bad = work[P_FLAG_A] != 0.;
  const bool done = rr <= work[W_STOP];  // (within the bound: nothing left to do, and p . q = 0 is no breakdown)
  if (!done && !bad) bad = !(rz > 0. && rz <= 1.7976931348623157e308 && pq > 0. && pq <= 1.7976931348623157e308);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[P_RZ_A] = rz;
    work[W_FLAG_B] = bad ? 1. : 0.;
  }
  if (done || bad) return;
  const double alpha = rz / pq;
  double srr = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    srr += ri * ri;
  }
  srr = block_sum(srr, lds);
  if (threadIdx.x == 0) work[P_RRP + blockIdx.x] = srr;
}

// partials of r . z, z = M r of the cycle just run
__global__ __launch_bounds__(WG) void k_pcg_dot(i64 n, double *work, const double *__restrict__ r, const double *__restrict__ z) {
  __shared__ double lds[4];
  double rz = 0;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) rz += r[i] * z[i];
  rz = block_sum(rz, lds);
  if (threadIdx.x == 0) work[P_RZP + blockIdx.x] = rz;
}

// beta = r.z (new) / r.z (old);  p = z + beta p (not once r . r is within the bound, nor after a breakdown).  reads RZ_A, FLAG_B, STOP, the partials; writes RR,
// RZ_B, FLAG_A
__global__ __launch_bounds__(WG) void k_pcg_direction(i64 n, int nparts, double *work, const double *__restrict__ z, double *__restrict__ p) {
  __shared__ double lds[4];
  const double rz = partial_sum(work + P_RZP, nparts, lds);
  const double rr = partial_sum(work + P_RRP, nparts, lds);
  const double rz_old = work[P_RZ_A];
  const bool bad = work[W_FLAG_B] != 0.;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    work[W_RR] = rr;
    work[P_RZ_B] = bad ? rz_old : rz;
    work[P_FLAG_A] = bad ? 1. : 0.;
  }
  if (bad || rr <= work[W_STOP]) return;
  const double beta = rz_old != 0. ? rz / rz_old : 0.;
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) p[i] = z[i] + beta * p[i];
}

template <class Idx>
void launch_jacobi(int L, const nh_csr &A, const Idx *col, const double *x, const double *w, const double *b, const unsigned char *mask, double *y, hipStream_t s) {
#define NH_JACOBI(LL)                                                                                                                                                    \
  case LL:                                                                                                                                                               \
    hipLaunchKernelGGL((k_jacobi<LL, Idx>), dim3(spmv_grid(A.nrows, LL)), dim3(WG), 0, s, (i64)A.nrows, (const i64 *)A.rowptr_dev, col, A.values_dev, x, w, b, mask, y); \
    break;
  switch (L) {
    NH_JACOBI(1)
    NH_JACOBI(2)
    NH_JACOBI(4)
    NH_JACOBI(8)
    NH_JACOBI(16)
    NH_JACOBI(32)
    default:
    NH_JACOBI(64)
  }
#undef NH_JACOBI
}

// y = mask(x + w (b - A x)); the caller has checked the view
int jacobi(const nh_csr &A, const double *x, const double *w, const double *b, const unsigned char *mask, double *y, hipStream_t s) {
  if (!A.nrows) return NH_OK;
  const int L = A.lanes ? A.lanes : nh_csr_lanes(A.nrows, A.nnz);
  if (A.col32_dev)
    launch_jacobi(L, A, A.col32_dev, x, w, b, mask, y, s);
  else
    launch_jacobi(L, A, (const i64 *)A.colidx_dev, x, w, b, mask, y, s);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int scale(i64 n, const double *w, const double *b, double *y, hipStream_t s) {
  if (!n) return NH_OK;
  hipLaunchKernelGGL(k_scale, dim3(vec_grid(n)), dim3(WG), 0, s, n, w, b, y);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

template <class Idx, bool FIRST>
void launch_chebyshev(int L, const nh_csr &A, const Idx *col, const double *x, const double *d, const double *dinv, const double *b, const double *coef,
                      const unsigned char *mask, double *y, double *dout, hipStream_t s) {
#define NH_CHEBYSHEV(LL)                                                                                                                                             \
  case LL:                                                                                                                                                           \
    hipLaunchKernelGGL((k_chebyshev<LL, Idx, FIRST>), dim3(spmv_grid(A.nrows, LL)), dim3(WG), 0, s, (i64)A.nrows, (const i64 *)A.rowptr_dev, col, A.values_dev, x, d, dinv, \
                       b, coef, mask, y, dout);                                                                                                                      \
    break;
  switch (L) {
    NH_CHEBYSHEV(1)
    NH_CHEBYSHEV(2)
    NH_CHEBYSHEV(4)
    NH_CHEBYSHEV(8)
    NH_CHEBYSHEV(16)
    NH_CHEBYSHEV(32)
    default:
    NH_CHEBYSHEV(64)
  }
#undef NH_CHEBYSHEV
}

// dout = c1 d + c2 dinv (b - A x), y = mask(x + dout); d == NULL: the first step, without d; the caller has checked the view
int chebyshev(const nh_csr &A, const double *x, const double *d, const double *dinv, const double *b, const double *coef, const unsigned char *mask, double *y,
              double *dout, hipStream_t s) {
  if (!A.nrows) return NH_OK;
  const int L = A.lanes ? A.lanes : nh_csr_lanes(A.nrows, A.nnz);
  if (A.col32_dev) {
    if (d)
      launch_chebyshev<int32_t, false>(L, A, A.col32_dev, x, d, dinv, b, coef, mask, y, dout, s);
    else
      launch_chebyshev<int32_t, true>(L, A, A.col32_dev, x, d, dinv, b, coef, mask, y, dout, s);
  } else {
    if (d)
      launch_chebyshev<i64, false>(L, A, (const i64 *)A.colidx_dev, x, d, dinv, b, coef, mask, y, dout, s);
    else
      launch_chebyshev<i64, true>(L, A, (const i64 *)A.colidx_dev, x, d, dinv, b, coef, mask, y, dout, s);
  }
  NH_LAUNCH_CHECK();
  return NH_OK;
}

template <class Idx>
void launch_lanczos_product(int L, const nh_csr &A, const Idx *col, const double *sq, const double *sc, const double *q, const unsigned char *mask, double *w,
                            double *work, hipStream_t s) {
#define NH_LANCZOS(LL)                                                                                                                                              \
  case LL:                                                                                                                                                          \
    hipLaunchKernelGGL((k_lanczos_product<LL, Idx>), dim3(spmv_grid(A.nrows, LL)), dim3(WG), 0, s, (i64)A.nrows, (const i64 *)A.rowptr_dev, col, A.values_dev, sq, sc, q, \
                       mask, w, work);                                                                                                                              \
    break;
  switch (L) {
    NH_LANCZOS(1)
    NH_LANCZOS(2)
    NH_LANCZOS(4)
    NH_LANCZOS(8)
    NH_LANCZOS(16)
    NH_LANCZOS(32)
    default:
    NH_LANCZOS(64)
  }
#undef NH_LANCZOS
}

// x = M b on level l.  The sweeps alternate between the level's two vectors: there are 2 sweeps - 1 that swap, so the cycle starts in t and ends in x.  A
// Chebyshev level of degree d takes the launches of a Jacobi level with d sweeps: the step that starts from zero needs no product, the others are one launch each.
int amg_cycle(const nh_amg *h, size_t l, const double *b, double *x, hipStream_t s) {
  const nh_amg_level &lv = h->levels[l];
  const i64 n = lv.A.nrows;
  if (!n) return NH_OK;
  if (lv.kind == NH_AMG_DENSE) {
    if (lv.ndense < n) NH_CHECK_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)n, s));  // (a masked level 0: the rows the dense block does not reach are 0)
    if (!lv.ndense) return NH_OK;
    hipLaunchKernelGGL(k_dense, dim3(1), dim3(DENSE_WG), 0, s, (int)lv.ndense, lv.Ainv_dev, b, lv.idx_dev, x);
    NH_LAUNCH_CHECK();
    return NH_OK;
  }
  if (lv.kind == NH_AMG_DIAGONAL) return scale(n, lv.w_dev, b, x, s);
  const nh_amg_level &next = h->levels[l + 1];
  double *cur = lv.t_dev, *other = x;
  const bool cheb = lv.smoother == NH_AMG_CHEBYSHEV;
  const int sweeps = cheb ? lv.degree : lv.sweeps;
  if (cheb) {
    hipLaunchKernelGGL(k_chebyshev_start, dim3(vec_grid(n)), dim3(WG), 0, s, n, lv.coef_dev, lv.w_dev, b, lv.d_dev, cur);
    NH_LAUNCH_CHECK();
  } else if (int rc = scale(n, lv.w_dev, b, cur, s))
    return rc;
  for (int k = 1; k < sweeps; ++k) {
    if (int rc = cheb ? chebyshev(lv.A, cur, lv.d_dev, lv.w_dev, b, lv.coef_dev + 2 * k, lv.rowmask_dev, other, lv.d_dev, s)
                      : jacobi(lv.A, cur, lv.w_dev, b, lv.rowmask_dev, other, s))
      return rc;
    std::swap(cur, other);
  }
  if (int rc = nh_csr_spmv(&lv.A, -1., cur, 1., b, lv.rowmask_dev, lv.r_dev, s)) return rc;
  if (int rc = nh_csr_spmv(&lv.R, 1., lv.r_dev, 0., nullptr, nullptr, next.b_dev, s)) return rc;
  if (int rc = amg_cycle(h, l + 1, next.b_dev, next.x_dev, s)) return rc;
  if (int rc = nh_csr_spmv(&lv.P, 1., next.x_dev, 1., cur, nullptr, cur, s)) return rc;
  for (int k = 0; k < sweeps; ++k) {
    if (int rc = cheb ? chebyshev(lv.A, cur, k ? lv.d_dev : nullptr, lv.w_dev, b, lv.coef_dev + 2 * k, lv.rowmask_dev, other, lv.d_dev, s)
                      : jacobi(lv.A, cur, lv.w_dev, b, lv.rowmask_dev, other, s))
      return rc;
    std::swap(cur, other);
  }
  return NH_OK;  // (cur == x)
}

template <class Idx>
void launch_schur_diagonal(int L, const nh_csr &A, const Idx *col, const double *vt, const unsigned char *first, const double *dinv, double *out, hipStream_t s) {
#define NH_SCHURDIAG(LL)                                                                                                                                          \
  case LL:                                                                                                                                                        \
    hipLaunchKernelGGL((k_schur_diagonal<LL, Idx>), dim3(spmv_grid(A.nrows, LL)), dim3(WG), 0, s, (i64)A.nrows, (const i64 *)A.rowptr_dev, col, A.values_dev, vt, \
                       first, dinv, out);                                                                                                                         \
    break;
  switch (L) {
    NH_SCHURDIAG(1)
    NH_SCHURDIAG(2)
    NH_SCHURDIAG(4)
    NH_SCHURDIAG(8)
    NH_SCHURDIAG(16)
    NH_SCHURDIAG(32)
    default:
    NH_SCHURDIAG(64)
  }
#undef NH_SCHURDIAG
}

// z = M r, the block upper-triangular solve: four steps on full-length vectors, the cycle in between
int schur_apply(const nh_schur *h, const double *r, double *z, hipStream_t s) {
  const i64 n = h->K.nrows;
  if (!n) return NH_OK;
  const unsigned grid = vec_grid(n);
  hipLaunchKernelGGL(k_schur_scale, dim3(grid), dim3(WG), 0, s, n, h->sinv, r, h->z2);
  NH_LAUNCH_CHECK();
  if (int rc = nh_csr_spmv(&h->K, -1., h->z2, 1., r, h->mask1, h->t, s)) return rc;
  if (int rc = amg_cycle(h->first, 0, h->t, z, s)) return rc;
  hipLaunchKernelGGL(k_schur_merge, dim3(grid), dim3(WG), 0, s, n, (const double *)h->z2, z);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

}  // namespace

extern "C" {

int nh_segment_dot(int64_t nseg, const int64_t *ptr_dev, const int32_t *ia_dev, const int32_t *ib_dev, const double *a_dev, const double *b_dev, int64_t nprod,
                   double *out_dev, void *stream) {
  NH_REQUIRE(nseg >= 0 && nprod >= 0, "nh_segment_dot: negative size");
  NH_REQUIRE(!nseg || (ptr_dev && out_dev), "nh_segment_dot: NULL segment pointers or result");
  NH_REQUIRE(!nprod || (ia_dev && a_dev), "nh_segment_dot: NULL first factor");
  NH_REQUIRE(!b_dev || !nprod || ib_dev, "nh_segment_dot: a second factor without its indices");
  if (!nseg) return NH_OK;
  hipStream_t s = nh_stream(stream);
  const i64 *ptr = (const i64 *)ptr_dev;
#define NH_SEGDOT(LL)                                                                                                                          \
  case LL:                                                                                                                                     \
    hipLaunchKernelGGL(k_segment_dot<LL>, dim3(spmv_grid(nseg, LL)), dim3(WG), 0, s, (i64)nseg, ptr, ia_dev, ib_dev, a_dev, b_dev, out_dev); \
    break;
  switch (nh_csr_lanes(nseg, nprod)) {
    NH_SEGDOT(1)
    NH_SEGDOT(2)
    NH_SEGDOT(4)
    NH_SEGDOT(8)
    NH_SEGDOT(16)
    default:
    NH_SEGDOT(32)
  }
#undef NH_SEGDOT
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_block_segment_dot(int k, int p, int q, int64_t nseg, const int64_t *ptr_dev, int64_t nprod, const int32_t *ia_dev, const int32_t *ib_dev,
                         const int32_t *sa_dev, const int32_t *sb_dev, int bstride, const int32_t *of_dev, const int32_t *os_dev, const double *a_dev,
                         const double *b_dev, double *out_dev, void *stream) {
  NH_REQUIRE(k >= 1 && k <= QR_MAXK, "nh_block_segment_dot: k must be between 1 and %d (got %d)", QR_MAXK, k);
  NH_REQUIRE((p == 1 || p == k) && (q == 1 || q == k), "nh_block_segment_dot: the blocks are p x q and q x k with p and q either 1 or k = %d (got p = %d, q = %d)", k, p, q);
  NH_REQUIRE(nseg >= 0 && nprod >= 0, "nh_block_segment_dot: negative size");
  NH_REQUIRE(!nseg || (ptr_dev && of_dev && out_dev), "nh_block_segment_dot: NULL segment pointers, result offsets or result");
  NH_REQUIRE(!nseg || p == 1 || (sa_dev && os_dev), "nh_block_segment_dot: blocks of %d rows without the row strides of the first factor and of the result", p);
  NH_REQUIRE(!nprod || (ia_dev && a_dev), "nh_block_segment_dot: NULL first factor");
  NH_REQUIRE(!nprod || (ib_dev && b_dev), "nh_block_segment_dot: NULL second factor");
  NH_REQUIRE(!nprod || q == 1 || sb_dev || bstride >= k, "nh_block_segment_dot: without its row strides the second factor needs a common one of at least k = %d (got %d)", k, bstride);
  if (!nseg) return NH_OK;
  hipStream_t s = nh_stream(stream);
  const i64 *ptr = (const i64 *)ptr_dev;
  const i64 total = (i64)nseg * p * k;
  const unsigned grid = (unsigned)std::min<i64>((total + WG - 1) / WG, SPMV_MAX_WGS);
  const bool pk = p > 1, qk = q > 1;
#define NH_BLOCKDOT_AT(KK, PK, QK)                                                                                                                      \
  hipLaunchKernelGGL((k_block_segment_dot<KK, PK, QK>), dim3(grid), dim3(WG), 0, s, (i64)nseg, ptr, ia_dev, ib_dev, sa_dev, sb_dev, bstride, of_dev, os_dev, \
                     a_dev, b_dev, out_dev)
#define NH_BLOCKDOT(KK)                    \
  case KK:                                 \
    if (pk && qk)                          \
      NH_BLOCKDOT_AT(KK, true, true);      \
    else if (pk)                           \
      NH_BLOCKDOT_AT(KK, true, false);     \
    else if (qk)                           \
      NH_BLOCKDOT_AT(KK, false, true);     \
    else                                   \
      NH_BLOCKDOT_AT(KK, false, false);    \
    break;
  switch (k) {
    NH_BLOCKDOT(1)
    NH_BLOCKDOT(2)
    NH_BLOCKDOT(3)
    NH_BLOCKDOT(4)
    NH_BLOCKDOT(5)
    default:
    NH_BLOCKDOT(6)
  }
#undef NH_BLOCKDOT
#undef NH_BLOCKDOT_AT
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_aggregate_qr(int64_t nagg, const int64_t *mptr_dev, const int32_t *midx_dev, int64_t nmembers, int k, int64_t n, const double *B_dev, double *Q_dev,
                    double *Rc_dev, void *stream) {
  NH_REQUIRE(nagg >= 0 && nmembers >= 0 && n >= 0, "nh_aggregate_qr: negative size");
  NH_REQUIRE(k >= 1 && k <= QR_MAXK, "nh_aggregate_qr: k must be between 1 and %d (got %d)", QR_MAXK, k);
  NH_REQUIRE(nmembers <= n, "nh_aggregate_qr: %lld members of %lld rows: a row is in at most one aggregate", (long long)nmembers, (long long)n);
  NH_REQUIRE(!nagg || (mptr_dev && Rc_dev), "nh_aggregate_qr: NULL aggregate pointers or coarse vectors");
  NH_REQUIRE(!nmembers || midx_dev, "nh_aggregate_qr: NULL member list");
  NH_REQUIRE(!n || (B_dev && Q_dev && B_dev != Q_dev), "nh_aggregate_qr: NULL vectors, or the result is the argument");
  hipStream_t s = nh_stream(stream);
  if (n) NH_CHECK_HIP(hipMemsetAsync(Q_dev, 0, sizeof(double) * (size_t)n * (size_t)k, s));  // (rows in no aggregate)
  if (!nagg) return NH_OK;
  NH_CHECK_HIP(hipMemsetAsync(Rc_dev, 0, sizeof(double) * (size_t)nagg * (size_t)(k * k), s));  // (the first Gram-Schmidt coefficient is added to, not stored)
  const i64 *mptr = (const i64 *)mptr_dev;
#define NH_AGGQR(LL)                                                                                                                  \
  case LL:                                                                                                                            \
    hipLaunchKernelGGL(k_aggregate_qr<LL>, dim3(spmv_grid(nagg, LL)), dim3(WG), 0, s, (i64)nagg, mptr, midx_dev, k, B_dev, Q_dev, Rc_dev); \
    break;
  switch (nh_csr_lanes(nagg, nmembers)) {
    NH_AGGQR(1)
    NH_AGGQR(2)
    NH_AGGQR(4)
    NH_AGGQR(8)
    NH_AGGQR(16)
    default:
    NH_AGGQR(32)
  }
#undef NH_AGGQR
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_csr_jacobi(const nh_csr *A, const double *x_dev, const double *w_dev, const double *b_dev, const unsigned char *rowmask_dev, double *y_dev, void *stream) {
  if (int rc = check_csr("nh_csr_jacobi", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_csr_jacobi: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(!A->nrows || (x_dev && w_dev && b_dev && y_dev), "nh_csr_jacobi: NULL vector");
  NH_REQUIRE(!A->nrows || x_dev != y_dev, "nh_csr_jacobi: the result must not be the argument");
  return jacobi(*A, x_dev, w_dev, b_dev, rowmask_dev, y_dev, nh_stream(stream));
}

int nh_csr_chebyshev(const nh_csr *A, const double *x_dev, const double *d_dev, const double *dinv_dev, const double *b_dev, const double *coef_dev,
                     const unsigned char *rowmask_dev, double *y_dev, double *dout_dev, void *stream) {
  if (int rc = check_csr("nh_csr_chebyshev", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_csr_chebyshev: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(!A->nrows || (x_dev && dinv_dev && b_dev && coef_dev && y_dev && dout_dev), "nh_csr_chebyshev: NULL vector or coefficients");
  NH_REQUIRE(!A->nrows || (x_dev != y_dev && x_dev != dout_dev && y_dev != dout_dev && y_dev != d_dev),
             "nh_csr_chebyshev: the result must not be the argument, nor the two results each other");
  return chebyshev(*A, x_dev, d_dev, dinv_dev, b_dev, coef_dev, rowmask_dev, y_dev, dout_dev, nh_stream(stream));
}

int nh_csr_lanczos(const nh_csr *A, const double *s_dev, const unsigned char *rowmask_dev, const double *u_dev, int steps, double *work_dev, double *out_dev,
                   void *stream) {
  if (int rc = check_csr("nh_csr_lanczos", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_csr_lanczos: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(steps >= 1 && steps <= 1 << 20, "nh_csr_lanczos: steps must be at least 1 (got %d)", steps);
  NH_REQUIRE(out_dev, "nh_csr_lanczos: nowhere to put the coefficients");
  NH_REQUIRE(!A->nrows || (s_dev && u_dev && work_dev), "nh_csr_lanczos: NULL vector or work array");
  hipStream_t s = nh_stream(stream);
  NH_CHECK_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * (size_t)(2 * steps + 1), s));
  const i64 n = A->nrows;
  if (!n) return NH_OK;
  const int L = A->lanes ? A->lanes : nh_csr_lanes(n, A->nnz);
  const int npa = (int)spmv_grid(n, L);
  const unsigned grid = vec_grid(n);
  double *q = work_dev + NH_LANCZOS_CELLS, *qprev = q + n, *w = qprev + n, *sq = w + n;
  hipLaunchKernelGGL(k_lanczos_start, dim3(grid), dim3(WG), 0, s, n, u_dev, s_dev, rowmask_dev, q, work_dev);
  NH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lanczos_first, dim3(grid), dim3(WG), 0, s, n, (int)grid, s_dev, q, sq, work_dev);
  NH_LAUNCH_CHECK();
  for (int j = 0; j < steps; ++j) {
    if (A->col32_dev)
      launch_lanczos_product(L, *A, A->col32_dev, sq, s_dev, q, rowmask_dev, w, work_dev, s);
    else
      launch_lanczos_product(L, *A, (const i64 *)A->colidx_dev, sq, s_dev, q, rowmask_dev, w, work_dev, s);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lanczos_update, dim3(grid), dim3(WG), 0, s, n, npa, (int)(j == 0), (const double *)q, (const double *)qprev, w, work_dev);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lanczos_normalize, dim3(grid), dim3(WG), 0, s, n, (int)grid, j, steps, s_dev, w, sq, work_dev, out_dev);
    NH_LAUNCH_CHECK();
    double *t = qprev;  // (the vectors rotate whether or not the recurrence has stopped: the launches are a function of sizes only)
    qprev = q;
    q = w;
    w = t;
  }
  return NH_OK;
}

int nh_amg_create(const nh_amg_level *levels, int nlevels, nh_amg **out) {
  NH_REQUIRE(levels && nlevels >= 1 && out, "nh_amg_create: no levels, or nowhere to put the handle");
  for (int l = 0; l < nlevels; ++l) {
    const nh_amg_level &lv = levels[l];
    const bool last = l == nlevels - 1;
    const i64 n = lv.A.nrows;
    if (int rc = check_csr("nh_amg_create (a level matrix)", &lv.A)) return rc;
    NH_REQUIRE(n == lv.A.ncols, "nh_amg_create: level %d is not square", l);
    NH_REQUIRE(lv.kind == NH_AMG_COARSEN || lv.kind == NH_AMG_DENSE || lv.kind == NH_AMG_DIAGONAL, "nh_amg_create: level %d has an unknown kind %d", l, lv.kind);
    NH_REQUIRE((lv.kind == NH_AMG_COARSEN) == !last, "nh_amg_create: every level but the last is coarsened, the last is not (level %d)", l);
    NH_REQUIRE(l == 0 || !n || (lv.b_dev && lv.x_dev), "nh_amg_create: level %d lacks its right-hand side or solution vector", l);
    if (lv.kind == NH_AMG_DENSE) {
      NH_REQUIRE(lv.ndense >= 0 && lv.ndense <= 1024 && lv.ndense <= n, "nh_amg_create: the dense level has %lld unknowns (at most 1024, and no more than rows)", (long long)lv.ndense);
      NH_REQUIRE(!lv.ndense || lv.Ainv_dev, "nh_amg_create: NULL dense inverse");
      NH_REQUIRE(lv.ndense == n || lv.idx_dev || !lv.ndense, "nh_amg_create: a dense level smaller than its vectors needs its index list");
    } else {
      NH_REQUIRE(!n || lv.w_dev, "nh_amg_create: level %d lacks its weights", l);
    }
    if (lv.kind == NH_AMG_COARSEN) {
      const i64 nc = levels[l + 1].A.nrows;
      NH_REQUIRE(lv.smoother == NH_AMG_JACOBI || lv.smoother == NH_AMG_CHEBYSHEV, "nh_amg_create: level %d has an unknown smoother %d", l, lv.smoother);
      if (lv.smoother == NH_AMG_CHEBYSHEV) {
        NH_REQUIRE(lv.degree >= 1, "nh_amg_create: level %d: degree must be at least 1 (got %d)", l, lv.degree);
        NH_REQUIRE(!n || (lv.coef_dev && lv.d_dev), "nh_amg_create: level %d lacks the coefficients or the vector d of its Chebyshev smoother", l);
      } else
        NH_REQUIRE(lv.sweeps >= 1, "nh_amg_create: level %d: sweeps must be at least 1 (got %d)", l, lv.sweeps);
      NH_REQUIRE(!n || (lv.t_dev && lv.r_dev), "nh_amg_create: level %d lacks its work vectors", l);
      if (int rc = check_csr("nh_amg_create (a prolongator)", &lv.P)) return rc;
      if (int rc = check_csr("nh_amg_create (a restriction)", &lv.R)) return rc;
      NH_REQUIRE(lv.P.nrows == n && lv.P.ncols == nc && lv.R.nrows == nc && lv.R.ncols == n, "nh_amg_create: level %d: P is %lld x %lld and R %lld x %lld between %lld and %lld dofs", l,
                 (long long)lv.P.nrows, (long long)lv.P.ncols, (long long)lv.R.nrows, (long long)lv.R.ncols, (long long)n, (long long)nc);
    }
  }
  nh_amg *h = new (std::nothrow) nh_amg;
  NH_REQUIRE(h, "nh_amg_create: out of memory");
  h->levels.assign(levels, levels + nlevels);
  *out = h;
  return NH_OK;
}

int nh_amg_free(nh_amg *amg) {
  delete amg;
  return NH_OK;
}

int nh_amg_apply(const nh_amg *amg, const double *r_dev, double *z_dev, void *stream) {
  NH_REQUIRE(amg, "nh_amg_apply: NULL hierarchy");
  NH_REQUIRE(!amg->levels[0].A.nrows || (r_dev && z_dev && r_dev != z_dev), "nh_amg_apply: NULL vector, or the result is the argument");
  return amg_cycle(amg, 0, r_dev, z_dev, nh_stream(stream));
}

int64_t nh_pcg_work_doubles(void) { return P_END; }

int nh_pcg_init(int64_t n, const nh_amg *amg, const double *r_dev, double *z_dev, double *p_dev, double *work_dev, void *stream) {
  NH_REQUIRE(n >= 0, "nh_pcg_init: negative size");
  NH_REQUIRE(amg && amg->levels[0].A.nrows == n, "nh_pcg_init: NULL hierarchy, or one of another size");
  NH_REQUIRE(work_dev && (!n || (r_dev && z_dev && p_dev && r_dev != z_dev)), "nh_pcg_init: NULL vector");
  hipStream_t s = nh_stream(stream);
  const unsigned grid = vec_grid(n);
  if (n) {
    if (int rc = amg_cycle(amg, 0, r_dev, z_dev, s)) return rc;
    hipLaunchKernelGGL(k_pcg_init, dim3(grid), dim3(WG), 0, s, (i64)n, work_dev, r_dev, (const double *)z_dev, p_dev);
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pcg_init_scalars, dim3(1), dim3(WG), 0, s, (int)grid, work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_pcg_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const nh_amg *amg, double *x_dev, double *r_dev, double *z_dev, double *p_dev, double *q_dev,
                   double *work_dev, int niter, void *stream) {
  NH_REQUIRE(A, "nh_pcg_iterate: NULL matrix");
  NH_REQUIRE(A->nrows == A->ncols, "nh_pcg_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(niter >= 0, "nh_pcg_iterate: negative iteration count");
  NH_REQUIRE(amg && amg->levels[0].A.nrows == A->nrows, "nh_pcg_iterate: NULL hierarchy, or one of another size");
  NH_REQUIRE(work_dev && (!A->nrows || (x_dev && r_dev && z_dev && p_dev && q_dev)), "nh_pcg_iterate: NULL vector");
  hipStream_t s = nh_stream(stream);
  const i64 n = A->nrows;
  const unsigned grid = vec_grid(n);
  for (int it = 0; it < niter; ++it) {
    int npq = 0;
    if (int rc = nh_csr_spmv_pq(A, p_dev, rowmask_dev, q_dev, work_dev + P_PQ, SPMV_MAX_WGS, &npq, s)) return rc;
    if (!n) return NH_OK;
    hipLaunchKernelGGL(k_pcg_update, dim3(grid), dim3(WG), 0, s, n, npq, work_dev, x_dev, r_dev, (const double *)p_dev, (const double *)q_dev);
    NH_LAUNCH_CHECK();
    if (int rc = amg_cycle(amg, 0, r_dev, z_dev, s)) return rc;
    hipLaunchKernelGGL(k_pcg_dot, dim3(grid), dim3(WG), 0, s, n, work_dev, (const double *)r_dev, (const double *)z_dev);
    NH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pcg_direction, dim3(grid), dim3(WG), 0, s, n, (int)grid, work_dev, (const double *)z_dev, p_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

int nh_fgmres_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const nh_amg *amg, double *V_dev, double *Z_dev, double *z_dev, double *t_dev, double *w_dev,
                      double *work_dev, int restart, double stop_rr, int niter, void *stream) {
  if (int rc = check_csr("nh_fgmres_iterate", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_fgmres_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(restart >= 1, "nh_fgmres_iterate: restart must be at least 1 (got %d)", restart);
  NH_REQUIRE(niter >= 0, "nh_fgmres_iterate: negative iteration count");
  NH_REQUIRE(stop_rr >= 0., "nh_fgmres_iterate: the bound on r . r must not be negative");
  NH_REQUIRE(amg && amg->levels[0].A.nrows == A->nrows, "nh_fgmres_iterate: NULL hierarchy, or one of another size");
  NH_REQUIRE(work_dev && (!A->nrows || (V_dev && Z_dev && z_dev && t_dev && w_dev && z_dev != t_dev)), "nh_fgmres_iterate: NULL vector, or the cycle's result is its argument");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  for (int it = 0; it < niter; ++it) {
    if (int rc = amg_cycle(amg, 0, z_dev, t_dev, s)) return rc;  // (also past a stop: the cycle reads no status, its result then goes nowhere)
    if (int rc = nh_gmres_step_from(A, rowmask_dev, t_dev, Z_dev, V_dev, z_dev, w_dev, work_dev, restart, stop_rr, s)) return rc;
  }
  return NH_OK;
}

int nh_csr_schur_diagonal(const nh_csr *A, const double *vt_dev, const unsigned char *first_dev, const double *dinv_dev, double *out_dev, void *stream) {
  if (int rc = check_csr("nh_csr_schur_diagonal", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_csr_schur_diagonal: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(!A->nrows || out_dev, "nh_csr_schur_diagonal: NULL result vector");
  NH_REQUIRE(!A->nnz || (vt_dev && first_dev && dinv_dev), "nh_csr_schur_diagonal: NULL transposed values, field mask or inverse diagonal");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  if (!A->nnz) {
    NH_CHECK_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * (size_t)A->nrows, s));
    return NH_OK;
  }
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (A->col32_dev)
    launch_schur_diagonal(L, *A, A->col32_dev, vt_dev, first_dev, dinv_dev, out_dev, s);
  else
    launch_schur_diagonal(L, *A, (const i64 *)A->colidx_dev, vt_dev, first_dev, dinv_dev, out_dev, s);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_schur_create(const nh_amg *first, const nh_csr *K, const unsigned char *mask1_dev, const double *sinv_dev, double *z2_dev, double *t_dev, nh_schur **out) {
  NH_REQUIRE(out, "nh_schur_create: nowhere to put the handle");
  NH_REQUIRE(first, "nh_schur_create: NULL hierarchy of the first block");
  if (int rc = check_csr("nh_schur_create", K)) return rc;
  NH_REQUIRE(K->nrows == K->ncols, "nh_schur_create: the matrix must be square (got %lld x %lld)", (long long)K->nrows, (long long)K->ncols);
  NH_REQUIRE(first->levels[0].A.nrows == K->nrows, "nh_schur_create: a hierarchy of another size (%lld rows, the matrix has %lld)", (long long)first->levels[0].A.nrows,
             (long long)K->nrows);
  NH_REQUIRE(!K->nrows || (mask1_dev && sinv_dev && z2_dev && t_dev), "nh_schur_create: NULL mask, Schur diagonal or scratch vector");
  NH_REQUIRE(!K->nrows || z2_dev != t_dev, "nh_schur_create: the two scratch vectors must be distinct");
  nh_schur *h = new (std::nothrow) nh_schur{first, *K, mask1_dev, sinv_dev, z2_dev, t_dev};
  NH_REQUIRE(h, "nh_schur_create: out of memory");
  *out = h;
  return NH_OK;
}

int nh_schur_free(nh_schur *schur) {
  delete schur;
  return NH_OK;
}

int nh_schur_apply(const nh_schur *schur, const double *r_dev, double *z_dev, void *stream) {
  NH_REQUIRE(schur, "nh_schur_apply: NULL preconditioner");
  NH_REQUIRE(!schur->K.nrows || (r_dev && z_dev && r_dev != z_dev), "nh_schur_apply: NULL vector, or the result is the argument");
  NH_REQUIRE(!schur->K.nrows || (z_dev != schur->z2 && z_dev != schur->t && r_dev != schur->z2 && r_dev != schur->t), "nh_schur_apply: a vector is one of the handle's scratch vectors");
  return schur_apply(schur, r_dev, z_dev, nh_stream(stream));
}

int nh_fgmres_iterate_schur(const nh_csr *A, const unsigned char *rowmask_dev, const nh_schur *schur, double *V_dev, double *Z_dev, double *z_dev, double *t_dev,
                            double *w_dev, double *work_dev, int restart, double stop_rr, int niter, void *stream) {
  if (int rc = check_csr("nh_fgmres_iterate_schur", A)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_fgmres_iterate_schur: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(restart >= 1, "nh_fgmres_iterate_schur: restart must be at least 1 (got %d)", restart);
  NH_REQUIRE(niter >= 0, "nh_fgmres_iterate_schur: negative iteration count");
  NH_REQUIRE(stop_rr >= 0., "nh_fgmres_iterate_schur: the bound on r . r must not be negative");
  NH_REQUIRE(schur && schur->K.nrows == A->nrows, "nh_fgmres_iterate_schur: NULL preconditioner, or one of another size");
  NH_REQUIRE(work_dev && (!A->nrows || (V_dev && Z_dev && z_dev && t_dev && w_dev && z_dev != t_dev)),
             "nh_fgmres_iterate_schur: NULL vector, or the preconditioner's result is its argument");
  NH_REQUIRE(!A->nrows || (z_dev != schur->z2 && z_dev != schur->t && t_dev != schur->z2 && t_dev != schur->t), "nh_fgmres_iterate_schur: a vector is one of the handle's scratch vectors");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  for (int it = 0; it < niter; ++it) {
    if (int rc = schur_apply(schur, z_dev, t_dev, s)) return rc;  // (also past a stop, as the cycle of nh_fgmres_iterate: its result then goes nowhere)
    if (int rc = nh_gmres_step_from(A, rowmask_dev, t_dev, Z_dev, V_dev, z_dev, w_dev, work_dev, restart, stop_rr, s)) return rc;
  }
  return NH_OK;
}

}  // extern "C"
