// Several vectors at once on a device-resident CSR matrix: the product with a block of vectors and a batched conjugate-gradient iteration, beside the
// single-vector kernels of nh_csr.hip and by their rules.  A block of vectors is row-major [n][k] with a leading dimension ld >= k in doubles (numpy's C order
// of an (n, k) array; a column slice of a wider block is a view).
//
//   * k_csr_spmm<L, Idx, KC, VW, DOT>: Y = mask(alpha A X + beta B) for a group of kc <= KC columns, by the mapping of k_csr_spmv: L lanes own a row, consecutive
//     lane groups take consecutive rows, a row is walked in strides of L, the L partial sums are folded with __shfl_xor in the same order, the grid is
//     spmv_grid(nrows, L), nothing is atomic.  A lane loads values[k] and col[k] once and updates kc accumulators from the kc contiguous doubles at
//     x + col[k] ldx, two per load (VW = 2) where ldx is even and x lies on a 16-byte boundary.  For every column the sums are formed by the expressions of
//     k_csr_spmv in its order: column j of the result is, bit for bit, the single-vector product of column j.
//     DOT = 1: additionally the workgroup's share of x_j . y_j goes to partial[j PSTRIDE + blockIdx.x] (the p . q of a batched CG step).
//   * k_cgm_init / k_cgm_init_scalars / k_cgm_update / k_cgm_direction<K>: K independent CG recurrences on one matrix, every launch covering all columns.  A thread
//     owns the rows k_cg_* give it when it comes to the sums, so each column's partials are summed in the single-vector order (the elementwise work runs over
//     contiguous doubles, and the new r reaches the row's thread through LDS); every workgroup sums the partials of the kernel before it in the same order;
//     scalars that cross an iteration live in two cells per column, one written and one read per kernel.
//     A column whose r . r is within its bound idles as a single solve does (no arithmetic, no flag), a flagged column does no arithmetic either; the product
//     still covers them, their p does not move and so their q does not.
#include "nh_common.h"
#include <algorithm>
#include <climits>
#include <cstdint>

namespace {

#include "nh_krylov.inc"  // WG, the grid caps, block_sum, block_sum_n, partial_sum, check_csr, spmv_grid, vec_grid

constexpr int KM = NH_MULTI_MAX;  // columns per group of the product (16 VGPRs of accumulators), and the most a batched CG takes

// the cells of the work array of a batched CG on k columns.  The head is the caller's: r . r at [0, k), the breakdown flags at [k, 2k), the counts of the
// iterations that moved a column at [2k, 3k), the bounds at [3k, 4k).  After "<-" the kernel that writes a cell, every other kernel only reads it.
enum {
  C_FLAG_A = 4 * KM,   // + j: the flag for update            <- direction
  C_RZ_A = 5 * KM,     // + j: the r . z that alpha was made of <- update
  C_RZ_B = 6 * KM,     // + j: r . z                           <- direction
  C_COUNT_A = 7 * KM,  // + j: the count, plus one if x moved <- update
  C_PQ = 8 * KM,                      // + j SPMV_MAX_WGS: partials of p_j . q_j  <- product
  C_RZP = C_PQ + KM * SPMV_MAX_WGS,   // + j VEC_MAX_WGS: partials of r_j . z_j   <- update, init
  C_RRP = C_RZP + KM * VEC_MAX_WGS,   // + j VEC_MAX_WGS: partials of r_j . r_j   <- update, init
  C_END = C_RRP + KM * VEC_MAX_WGS
};
// head cells (k: the columns of the solve): RR + j <- direction, FLAG_B + j <- update, COUNT + j <- direction, STOP + j: the host's
__host__ __device__ inline int h_rr(int) { return 0; }
__host__ __device__ inline int h_flag(int k) { return k; }
__host__ __device__ inline int h_count(int k) { return 2 * k; }
__host__ __device__ inline int h_stop(int k) { return 3 * k; }

template <int L, class Idx, int KC, int VW, int DOT>
__global__ __launch_bounds__(WG) void k_csr_spmm(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values, int kc,
                                                 const double *__restrict__ x, i64 ldx, double alpha, double beta, const double *b, i64 ldb,
                                                 const unsigned char *__restrict__ mask, double *y, i64 ldy, double *partial, int pstride) {
  constexpr int G = WG / L;  // rows per workgroup and step
  const int lane = threadIdx.x & (L - 1);
  double dot[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) dot[c] = 0;
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the shuffles)
    const i64 row = base + threadIdx.x / L;
    const bool live = row < nrows;
    const bool on = live && (!mask || mask[row]);
    double s[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) s[c] = 0;
    if (on) {
      const i64 k1 = rowptr[row + 1];
      for (i64 k = rowptr[row] + lane; k < k1; k += L) {
        const double a = values[k];
        const double *__restrict__ xr = x + (i64)col[k] * ldx;
#pragma unroll
        for (int c = 0; c < KC; c += VW) {  // (kc is uniform: the guards are scalar branches; nothing is read past column kc)
          if (VW == 2 && c + 1 < kc) {
            const double2 t = *reinterpret_cast<const double2 *>(xr + c);
            s[c] += a * t.x;
            s[c + 1] += a * t.y;
          } else if (c < kc)
            s[c] += a * xr[c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < kc)
#pragma unroll
        for (int o = L >> 1; o; o >>= 1) s[c] += __shfl_xor(s[c], o, L);
    if (live && lane == 0) {
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (c < kc) {
          double v = 0;
          if (on) {
            v = alpha * s[c];
            if (b) v += beta * b[row * ldb + c];
          }
          y[row * ldy + c] = v;
          if (DOT == 1) dot[c] += x[row * ldx + c] * v;
        }
    }
  }
  if (DOT == 1) {
    __shared__ double lds[4 * KC];
    block_sum_n<KC>(dot, lds);
    if (threadIdx.x == 0)
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (c < kc) partial[(i64)c * pstride + blockIdx.x] = dot[c];
  }
}

// The vector kernels take the blocks a tile of WG rows at a time.  The elementwise work runs over the tile's WG K contiguous doubles, consecutive threads on
// consecutive doubles (a thread that walked its own row would touch a cache line per lane and load); the new r goes through an LDS tile, from which thread t
// reads row t -- the row k_cg_* give it -- and adds its terms to the column's partials, in the single-vector order.  The tile's leading dimension is odd: the
// rows of a wave fall into different banks.
#define NH_TILES(base) for (i64 base = (i64)blockIdx.x * WG; base < n; base += (i64)gridDim.x * WG)  // (uniform over the workgroup: the loop holds barriers)
template <int K>
struct Tile {
  static constexpr int LD = K | 1;
  int ne;  // doubles of the tile
  i64 e0;  // the first of them in the block
  __device__ Tile(i64 base, i64 n) : ne((int)(n - base < WG ? n - base : WG) * K), e0(base * K) {}
};
// the elements of a tile that a thread takes: f = threadIdx.x + m WG, row f / K of the tile, column f % K
#define NH_TILE_ELEMENTS(t, f, row, c)                                                      \
  _Pragma("unroll") for (int m_ = 0, f = threadIdx.x, row, c; m_ < K; ++m_, f += WG)        \
    if (f < t.ne && (row = f / K, c = f - row * K, true))

// z = dinv r (or r), p = z, partials of r . z and r . r, per column
template <int K>
__global__ __launch_bounds__(WG) void k_cgm_init(i64 n, double *work, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ p) {
  constexpr int LD = Tile<K>::LD;
  __shared__ double lds[4 * K];
  __shared__ double tile[WG * LD];
  double rz[K], rr[K];
#pragma unroll
  for (int c = 0; c < K; ++c) rz[c] = rr[c] = 0;
  NH_TILES(base) {
    const Tile<K> t(base, n);
    NH_TILE_ELEMENTS(t, f, row, c) {
      const double ri = r[t.e0 + f], zi = dinv ? dinv[base + row] * ri : ri;
      p[t.e0 + f] = zi;
      tile[row * LD + c] = ri;
    }
    __syncthreads();
    const i64 i = base + threadIdx.x;
    if (i < n) {
      const double d = dinv ? dinv[i] : 0.;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const double ri = tile[threadIdx.x * LD + c], zi = dinv ? d * ri : ri;
        rz[c] += ri * zi;
        rr[c] += ri * ri;
      }
    }
    __syncthreads();
  }
  block_sum_n<K>(rz, lds);
  block_sum_n<K>(rr, lds);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      work[C_RZP + c * VEC_MAX_WGS + blockIdx.x] = rz[c];
      work[C_RRP + c * VEC_MAX_WGS + blockIdx.x] = rr[c];
    }
}

__global__ __launch_bounds__(WG) void k_cgm_init_scalars(int nparts, int k, double *work) {
  __shared__ double lds[4];
  for (int c = 0; c < k; ++c) {
    const double rz = partial_sum(work + C_RZP + c * VEC_MAX_WGS, nparts, lds);
    const double rr = partial_sum(work + C_RRP + c * VEC_MAX_WGS, nparts, lds);
    if (threadIdx.x == 0) {
      work[h_rr(k) + c] = rr;
      work[h_flag(k) + c] = 0.;
      work[h_count(k) + c] = 0.;
      work[h_stop(k) + c] = 0.;
      work[C_FLAG_A + c] = 0.;
      work[C_RZ_A + c] = rz;
      work[C_RZ_B + c] = rz;
      work[C_COUNT_A + c] = 0.;
    }
  }
}

// per column: alpha = r.z / p.q;  x += alpha p;  r -= alpha q;  partials of r . z and r . r with z = dinv r.
// reads RR, RZ_B, FLAG_A, STOP, COUNT, the p.q partials; writes RZ_A, FLAG_B, COUNT_A, the r.z / r.r partials (not of a column within its bound: its r has not
// moved, they stand)
template <int K>
__global__ __launch_bounds__(WG) void k_cgm_update(i64 n, int npq, double *work, const double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r,
                                                   const double *__restrict__ p, const double *__restrict__ q) {
  constexpr int LD = Tile<K>::LD;
  __shared__ double lds[4 * K];
  __shared__ double tile[WG * LD];
  __shared__ double alphas[K];
  unsigned open = 0, moving = 0;  // bit c: column c is above its bound / takes a step
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const double pq = partial_sum(work + C_PQ + c * SPMV_MAX_WGS, npq, lds);
    const double rz = work[C_RZ_B + c], rr = work[h_rr(K) + c];
    bool bad = work[C_FLAG_A + c] != 0.;
    const bool done = rr <= work[h_stop(K) + c];  // (the idle rule of k_cg_update: nothing left to do, and p . q = 0 is no breakdown)
    if (!done && !bad) bad = !(rz > 0. && rz <= 1.7976931348623157e308 && pq > 0. && pq <= 1.7976931348623157e308);
    const bool move = !done && !bad;
    if (!done) open |= 1u << c;
    if (move) moving |= 1u << c;
    if (threadIdx.x == 0) {
      alphas[c] = move ? rz / pq : 0.;
      if (blockIdx.x == 0) {
        work[C_RZ_A + c] = rz;
        work[h_flag(K) + c] = bad ? 1. : 0.;
        work[C_COUNT_A + c] = work[h_count(K) + c] + (move ? 1. : 0.);
      }
    }
  }
  if (!open) return;
  __syncthreads();
  double srz[K], srr[K];
#pragma unroll
  for (int c = 0; c < K; ++c) srz[c] = srr[c] = 0;
  NH_TILES(base) {
    const Tile<K> t(base, n);
    NH_TILE_ELEMENTS(t, f, row, c) {
      if (open >> c & 1) {
        double ri = r[t.e0 + f];
        if (moving >> c & 1) {  // (a stalled column does no arithmetic on x and r: no 0 * inf)
          const double alpha = alphas[c];
          x[t.e0 + f] += alpha * p[t.e0 + f];
          ri -= alpha * q[t.e0 + f];
          r[t.e0 + f] = ri;
        }
        tile[row * LD + c] = ri;
      }
    }
    __syncthreads();
    const i64 i = base + threadIdx.x;
    if (i < n) {
      const double d = dinv ? dinv[i] : 0.;
#pragma unroll
      for (int c = 0; c < K; ++c)
        if (open >> c & 1) {
          const double ri = tile[threadIdx.x * LD + c], zi = dinv ? d * ri : ri;
          srz[c] += ri * zi;
          srr[c] += ri * ri;
        }
    }
    __syncthreads();
  }
  block_sum_n<K>(srz, lds);
  block_sum_n<K>(srr, lds);
  if (threadIdx.x == 0)
#pragma unroll
    for (int c = 0; c < K; ++c)
      if (open >> c & 1) {
        work[C_RZP + c * VEC_MAX_WGS + blockIdx.x] = srz[c];
        work[C_RRP + c * VEC_MAX_WGS + blockIdx.x] = srr[c];
      }
}

// per column: beta = r.z (new) / r.z (old);  p = z + beta p (not once r . r is within the bound).  reads RZ_A, FLAG_B, COUNT_A, STOP, the partials; writes RR,
// RZ_B, FLAG_A, COUNT
template <int K>
__global__ __launch_bounds__(WG) void k_cgm_direction(i64 n, int nparts, double *work, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ p) {
  __shared__ double lds[4];
  __shared__ double betas[K];
  unsigned turning = 0;  // bit c: column c gets a new direction
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const double rz = partial_sum(work + C_RZP + c * VEC_MAX_WGS, nparts, lds);
    const double rr = partial_sum(work + C_RRP + c * VEC_MAX_WGS, nparts, lds);
    const double rz_old = work[C_RZ_A + c];
    const bool bad = work[h_flag(K) + c] != 0.;
    if (threadIdx.x == 0) {
      betas[c] = rz_old != 0. ? rz / rz_old : 0.;
      if (blockIdx.x == 0) {
        work[h_rr(K) + c] = rr;
        work[C_RZ_B + c] = bad ? rz_old : rz;
        work[C_FLAG_A + c] = bad ? 1. : 0.;
        work[h_count(K) + c] = work[C_COUNT_A + c];
      }
    }
    if (!(bad || rr <= work[h_stop(K) + c])) turning |= 1u << c;
  }
  if (!turning) return;
  __syncthreads();
  NH_TILES(base) {
    const Tile<K> t(base, n);
    NH_TILE_ELEMENTS(t, f, row, c) {
      if (turning >> c & 1) {
        const double ri = r[t.e0 + f], zi = dinv ? dinv[base + row] * ri : ri;
        p[t.e0 + f] = zi + betas[c] * p[t.e0 + f];
      }
    }
  }
}
#undef NH_TILE_ELEMENTS
#undef NH_TILES

// one group of kc <= KM columns of a block product
struct Group {
  int kc;
  const double *x;
  i64 ldx;
  double alpha, beta;
  const double *b;
  i64 ldb;
  const unsigned char *mask;
  double *y;
  i64 ldy;
  double *partial;  // NULL, or where the partials of x_j . y_j go (C_PQ of a work array)
};

template <int L, class Idx, int VW>
void launch_lanes(const nh_csr *A, const Idx *col, const Group &g, hipStream_t s) {
  const dim3 grid(spmv_grid(A->nrows, L));
  if (g.partial)
    hipLaunchKernelGGL((k_csr_spmm<L, Idx, KM, VW, 1>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, g.kc, g.x, g.ldx, g.alpha, g.beta, g.b,
                       g.ldb, g.mask, g.y, g.ldy, g.partial, (int)SPMV_MAX_WGS);
  else
    hipLaunchKernelGGL((k_csr_spmm<L, Idx, KM, VW, 0>), grid, dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, g.kc, g.x, g.ldx, g.alpha, g.beta, g.b,
                       g.ldb, g.mask, g.y, g.ldy, g.partial, (int)SPMV_MAX_WGS);
}

template <class Idx, int VW>
void launch_idx(int L, const nh_csr *A, const Idx *col, const Group &g, hipStream_t s) {
  switch (L) {
    case 1: launch_lanes<1, Idx, VW>(A, col, g, s); break;
    case 2: launch_lanes<2, Idx, VW>(A, col, g, s); break;
    case 4: launch_lanes<4, Idx, VW>(A, col, g, s); break;
    case 8: launch_lanes<8, Idx, VW>(A, col, g, s); break;
    case 16: launch_lanes<16, Idx, VW>(A, col, g, s); break;
    case 32: launch_lanes<32, Idx, VW>(A, col, g, s); break;
    default: launch_lanes<64, Idx, VW>(A, col, g, s); break;
  }
}

template <int VW>
void launch_vw(int L, const nh_csr *A, const Group &g, hipStream_t s) {
  if (A->col32_dev)
    launch_idx<int32_t, VW>(L, A, A->col32_dev, g, s);
  else
    launch_idx<i64, VW>(L, A, (const i64 *)A->colidx_dev, g, s);
}

// L: the lanes per row, resolved by the caller
int spmm_group(int L, const nh_csr *A, const Group &g, hipStream_t s) {
  if (!(g.ldx & 1) && !((uintptr_t)g.x & 15))  // two doubles per load: every row of the group starts on a 16-byte boundary
    launch_vw<2>(L, A, g, s);
  else
    launch_vw<1>(L, A, g, s);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int check_columns(const char *who, int k) {
  NH_REQUIRE(k >= 1, "%s: at least one column (got %d)", who, k);
  if (k > KM) {
    nh_set_error("%s: at most %d columns at once (got %d)", who, KM, k);
    return NH_ELIMIT;
  }
  return NH_OK;
}

#define NH_COLUMNS(k, LAUNCH) \
  switch (k) {                \
    case 1: LAUNCH(1); break; \
    case 2: LAUNCH(2); break; \
    case 3: LAUNCH(3); break; \
    case 4: LAUNCH(4); break; \
    case 5: LAUNCH(5); break; \
    case 6: LAUNCH(6); break; \
    case 7: LAUNCH(7); break; \
    default: LAUNCH(8); break; \
  }
static_assert(KM == 8, "NH_COLUMNS instantiates the vector kernels for 1 .. 8 columns");

}  // namespace

extern "C" {

int nh_csr_spmm(const nh_csr *A, int k, double alpha, const double *x_dev, int64_t ldx, double beta, const double *b_dev, int64_t ldb, const unsigned char *rowmask_dev,
                double *y_dev, int64_t ldy, void *stream) {
  if (int rc = check_csr("nh_csr_spmm", A)) return rc;
  NH_REQUIRE(k >= 1, "nh_csr_spmm: at least one column (got %d)", k);
  NH_REQUIRE(ldx >= k && ldy >= k && (!b_dev || ldb >= k), "nh_csr_spmm: a leading dimension is below the %d columns (x %lld, b %lld, y %lld)", k, (long long)ldx,
             (long long)ldb, (long long)ldy);
  NH_REQUIRE(!A->nrows || y_dev, "nh_csr_spmm: NULL result block");
  NH_REQUIRE(!A->nnz || x_dev, "nh_csr_spmm: NULL argument block");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  if (!A->nnz && !b_dev) {  // nothing to multiply: the k columns of every row are zero, no launch
    NH_CHECK_HIP(hipMemset2DAsync(y_dev, sizeof(double) * (size_t)ldy, 0, sizeof(double) * (size_t)k, (size_t)A->nrows, s));
    return NH_OK;
  }
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  for (int k0 = 0; k0 < k; k0 += KM) {  // groups of KM columns and a remnant group
    const Group g{std::min(KM, k - k0), x_dev ? x_dev + k0 : nullptr, ldx, alpha, beta, b_dev ? b_dev + k0 : nullptr, ldb, rowmask_dev, y_dev + k0, ldy, nullptr};
    if (int rc = spmm_group(L, A, g, s)) return rc;
  }
  return NH_OK;
}

int64_t nh_cgm_work_doubles(int k) {
  if (check_columns("nh_cgm_work_doubles", k)) return -1;
  return C_END;
}

int nh_cgm_init(int64_t n, int k, const double *dinv_dev, const double *r_dev, double *p_dev, double *work_dev, void *stream) {
  NH_REQUIRE(n >= 0, "nh_cgm_init: negative size");
  if (int rc = check_columns("nh_cgm_init", k)) return rc;
  NH_REQUIRE(work_dev && (!n || (r_dev && p_dev)), "nh_cgm_init: NULL vector");
  hipStream_t s = nh_stream(stream);
  const unsigned grid = vec_grid(n);
  if (n) {
#define NH_LAUNCH(K) hipLaunchKernelGGL(k_cgm_init<K>, dim3(grid), dim3(WG), 0, s, (i64)n, work_dev, dinv_dev, r_dev, p_dev)
    NH_COLUMNS(k, NH_LAUNCH)
#undef NH_LAUNCH
    NH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_cgm_init_scalars, dim3(1), dim3(WG), 0, s, (int)grid, k, work_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_cgm_iterate(const nh_csr *A, int k, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, double *p_dev, double *q_dev,
                   double *work_dev, int niter, void *stream) {
  if (int rc = check_csr("nh_cgm_iterate", A)) return rc;
  if (int rc = check_columns("nh_cgm_iterate", k)) return rc;
  NH_REQUIRE(A->nrows == A->ncols, "nh_cgm_iterate: the matrix must be square (got %lld x %lld)", (long long)A->nrows, (long long)A->ncols);
  NH_REQUIRE(niter >= 0, "nh_cgm_iterate: negative iteration count");
  NH_REQUIRE(work_dev && (!A->nrows || (x_dev && r_dev && p_dev && q_dev)), "nh_cgm_iterate: NULL vector");
  if (!A->nrows) return NH_OK;
  hipStream_t s = nh_stream(stream);
  const i64 n = A->nrows;
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  const int npq = (int)spmv_grid(n, L);
  const unsigned grid = vec_grid(n);
  const Group pq{k, p_dev, k, 1., 0., nullptr, 0, rowmask_dev, q_dev, k, work_dev + C_PQ};
  for (int it = 0; it < niter; ++it) {
    if (int rc = spmm_group(L, A, pq, s)) return rc;
#define NH_LAUNCH(K) hipLaunchKernelGGL(k_cgm_update<K>, dim3(grid), dim3(WG), 0, s, n, npq, work_dev, dinv_dev, x_dev, r_dev, (const double *)p_dev, (const double *)q_dev)
    NH_COLUMNS(k, NH_LAUNCH)
#undef NH_LAUNCH
    NH_LAUNCH_CHECK();
#define NH_LAUNCH(K) hipLaunchKernelGGL(k_cgm_direction<K>, dim3(grid), dim3(WG), 0, s, n, (int)grid, work_dev, dinv_dev, (const double *)r_dev, p_dev)
    NH_COLUMNS(k, NH_LAUNCH)
#undef NH_LAUNCH
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

}  // extern "C"
