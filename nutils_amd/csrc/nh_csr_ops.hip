// Matrix algebra of the device-resident CSR matrix: transpose, selection (submatrix, pruning of zeros) and the values of a sum of two patterns
// (Matrix.T, Matrix.submatrix, Matrix.__add__ of the reference, matrix/_base.py; there scipy does them on one core of the host).  Every result
// is index arrays plus `pos`, the position in the operand of every entry of the result: the values follow by one nh_index_copy, and the next
// matrix on the same pattern needs only that copy.  Every output is a pure function of the input: repeated calls give identical arrays.
//
//   * Transpose, four phases.  k_tr_count: a histogram of the column indices, one thread per entry (int32 atomicAdd: a sum of ones does not
//     depend on the order).  nh_scan_exclusive: the row pointers of the transpose.  k_tr_place: one thread per entry claims a slot of its output
//     row with an int32 atomicAdd and stores its own position k there; which slot it gets depends on the order, the SET of positions an output
//     row holds does not.  k_tr_sort: every output row is sorted by k, which is sorted by source row since k rises with the row (and, should a
//     row of the operand repeat a column, keeps those entries in their order); the keys are unique, so the sorted row does not depend on the
//     claimed slots.  The source row of a sorted key, the column index of the transpose, is a binary search of k in the operand's row pointers.
//     Sorting: a workgroup of four waves takes four consecutive output rows at a time.  A row of at most 64 entries is sorted by ONE WAVE IN
//     REGISTERS (one key a lane, a bitonic network of __shfl_xor: no LDS, no barrier).  A row of 65 .. TR_CAP = 2048 entries is sorted by the
//     WHOLE WORKGROUP IN LDS (bitonic, 16 KiB).  A row of more than TR_CAP entries takes the slow path: the workgroup sorts it in pieces of TR_CAP,
//     writes them back, and every entry finds its rank as its place in its piece plus, by binary search, the number of smaller keys in every other
//     piece: O(n^2 / TR_CAP log TR_CAP), meant for the odd dense column, not for a matrix of them.
//   * Selection.  k_select<L, Idx, FILL>: the product's mapping (L lanes per row, a wave reads one contiguous span).  Entry k of row i is kept iff
//     rowkeep[i], colkeep[col[k]] and, with drop_zeros, values[k] != 0 (true for NaN, false for -0.0).  Per stride of L entries the lanes vote
//     with __ballot (a 64-bit mask on this wave64 hardware); a lane group shifts its own L bits out of it, and an entry's rank in its row is
//     the running count plus the population of the group's bits below its lane, so entries keep their order.  No atomics.  The count pass stores
//     the length of every kept row at its new index (the exclusive scan of rowkeep), the fill pass the new column indices (the scan of colkeep)
//     and pos.
//   * Sum.  k_place / k_add_at: out = 0, out[pos_a[k]] = a[k], out[pos_b[k]] += sign b[k]: positions are unique within a part, plain stores.
#include "nh_common.h"
#include <algorithm>
#include <climits>
#include <cstdint>

namespace {

#include "nh_krylov.inc"  // WG, the grid caps, lanes_ok, spmv_grid, vec_grid

constexpr int TR_CAP = 2048;  // entries of an output row of the transpose that one workgroup sorts in LDS; longer rows take the slow path
constexpr i64 KEY_MAX = INT64_MAX;

struct Scratch {  // device memory that lives as long as the call (hipFree waits for the device)
  void *p = nullptr;
  ~Scratch() {
    if (p) hipFree(p);
  }
};

// the row of the operand that holds entry k: the last r with rowptr[r] <= k (rows without entries are stepped over: their successor has the same pointer)
__device__ __forceinline__ i64 row_of(const i64 *__restrict__ rowptr, i64 nrows, i64 k) {
  i64 lo = 0, hi = nrows;
  while (hi - lo > 1) {
    const i64 mid = (lo + hi) >> 1;
    if (rowptr[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}

template <class Idx>
__global__ __launch_bounds__(WG) void k_tr_count(i64 nnz, const Idx *__restrict__ col, int32_t *cnt) {
  for (i64 k = (i64)blockIdx.x * WG + threadIdx.x; k < nnz; k += (i64)gridDim.x * WG) atomicAdd(&cnt[col[k]], 1);
}

template <class Idx>
__global__ __launch_bounds__(WG) void k_tr_place(i64 nnz, const Idx *__restrict__ col, const i64 *__restrict__ rowptr_t, int32_t *cursor, i64 *__restrict__ key) {
  for (i64 k = (i64)blockIdx.x * WG + threadIdx.x; k < nnz; k += (i64)gridDim.x * WG) {
    const i64 c = col[k];
    key[rowptr_t[c] + atomicAdd(&cursor[c], 1)] = k;
  }
}

// bitonic sort of P = 2^m keys in LDS by the whole workgroup, ascending
__device__ __forceinline__ void lds_sort(i64 *lds, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += WG) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const i64 a = lds[i], b = lds[ixj];
          if ((a > b) == ((i & k) == 0)) lds[i] = b, lds[ixj] = a;
        }
      }
      __syncthreads();
    }
}

// key: in, the positions every output row holds, in any order; out, the source rows (the column indices of the transpose).  pos: out, the positions sorted.
__global__ __launch_bounds__(WG) void k_tr_sort(i64 ncols, i64 nrows, const i64 *__restrict__ rowptr, const i64 *__restrict__ rowptr_t, i64 *key, i64 *pos) {
  __shared__ i64 lds[TR_CAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int R = WG / 64;  // output rows per workgroup and step
  for (i64 base = (i64)blockIdx.x * R; base < ncols; base += (i64)gridDim.x * R) {  // (uniform in the workgroup: it meets at barriers below)
    {  // short rows: one wave each, in registers
      const i64 r = base + wave;
      const i64 a = r < ncols ? rowptr_t[r] : 0;
      const i64 n = r < ncols ? rowptr_t[r + 1] - a : 0;
      if (n > 0 && n <= 64) {  // (uniform in the wave)
        i64 v = lane < n ? key[a + lane] : KEY_MAX;
        for (int k = 2; k < 2 * n; k <<= 1)  // (the lanes from the next power of two on hold KEY_MAX and trade it among themselves)
          for (int j = k >> 1; j > 0; j >>= 1) {
            const i64 o = __shfl_xor(v, j, 64);
            const bool low = ((lane & j) == 0) == ((lane & k) == 0);
            v = low ? (o < v ? o : v) : (o > v ? o : v);
          }
        if (lane < n) {
          pos[a + lane] = v;
          key[a + lane] = row_of(rowptr, nrows, v);
        }
      }
    }
    for (int w = 0; w < R && base + w < ncols; ++w) {  // long rows: the workgroup, one after the other
      const i64 a = rowptr_t[base + w], n = rowptr_t[base + w + 1] - a;
      if (n <= 64) continue;  // (uniform in the workgroup)
      const i64 npieces = (n + TR_CAP - 1) / TR_CAP;
      for (i64 p = 0; p < npieces; ++p) {
        const i64 a0 = a + p * TR_CAP;
        const int m = n - p * TR_CAP < TR_CAP ? (int)(n - p * TR_CAP) : TR_CAP;
        int P = 64;
        while (P < m) P <<= 1;
        for (int i = threadIdx.x; i < P; i += WG) lds[i] = i < m ? key[a0 + i] : KEY_MAX;
        __syncthreads();
        lds_sort(lds, P);
        if (npieces == 1) {
          for (int i = threadIdx.x; i < m; i += WG) {
            const i64 v = lds[i];
            pos[a0 + i] = v;
            key[a0 + i] = row_of(rowptr, nrows, v);
          }
        } else {
          for (int i = threadIdx.x; i < m; i += WG) key[a0 + i] = lds[i];
        }
        __syncthreads();  // (lds is loaded again; the pieces written above are read below)
      }
      if (npieces > 1) {  // slow path: the rank of a key is its place in its piece and the number of smaller keys in every other piece
        for (i64 i = threadIdx.x; i < n; i += WG) {
          const i64 v = key[a + i], mine = i / TR_CAP;
          i64 rank = i - mine * TR_CAP;
          for (i64 p = 0; p < npieces; ++p) {
            if (p == mine) continue;
            i64 lo = p * TR_CAP, hi = lo + TR_CAP < n ? lo + TR_CAP : n;  // the first key of the piece that is not below v
            while (lo < hi) {
              const i64 mid = (lo + hi) >> 1;
              if (key[a + mid] < v) lo = mid + 1; else hi = mid;
            }
            rank += lo - p * TR_CAP;
          }
          pos[a + rank] = v;
        }
        __syncthreads();
        for (i64 i = threadIdx.x; i < n; i += WG) key[a + i] = row_of(rowptr, nrows, pos[a + i]);
        __syncthreads();
      }
    }
  }
}

__global__ __launch_bounds__(WG) void k_mask_i32(i64 n, const unsigned char *__restrict__ mask, int32_t *__restrict__ out) {
  for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < n; i += (i64)gridDim.x * WG) out[i] = mask[i] != 0;
}

template <int L, class Idx, bool FILL>
__global__ __launch_bounds__(WG) void k_select(i64 nrows, const i64 *__restrict__ rowptr, const Idx *__restrict__ col, const double *__restrict__ values,
                                               const unsigned char *__restrict__ rowkeep, const unsigned char *__restrict__ colkeep, int drop_zeros,
                                               const i64 *__restrict__ newrow, const i64 *__restrict__ newcol, int32_t *__restrict__ cnt, const i64 *__restrict__ rowptr_s,
                                               i64 *__restrict__ colidx_s, i64 *__restrict__ pos) {
  constexpr int G = WG / L;
  const int lane = threadIdx.x & (L - 1);
  const int shift = (threadIdx.x & 63) & ~(L - 1);  // where the bits of this lane group start in the wave's vote
  const unsigned long long group = L == 64 ? ~0ull : (1ull << (L & 63)) - 1, below = (1ull << lane) - 1;
  for (i64 base = (i64)blockIdx.x * G; base < nrows; base += (i64)gridDim.x * G) {  // (uniform trip count: every lane takes part in the votes)
    const i64 row = base + threadIdx.x / L;
    const bool live = row < nrows && (!rowkeep || rowkeep[row]);
    i64 k0 = 0, k1 = 0, orow = 0, out = 0;
    int n = 0;
    if (live) {
      k0 = rowptr[row], k1 = rowptr[row + 1];
      orow = newrow ? newrow[row] : row;
      if (FILL) out = rowptr_s[orow];
    }
    while (__any(k0 < k1)) {  // (uniform in the wave: the longest row of the wave sets the number of votes)
      const i64 k = k0 + lane;
      bool keep = false;
      i64 c = 0;
      if (k < k1) {
        c = col[k];
        keep = (!colkeep || colkeep[c]) && (!drop_zeros || values[k] != 0.);
      }
      const unsigned long long bits = (__ballot(keep) >> shift) & group;
      if (FILL) {
        if (keep) {
          const i64 at = out + __popcll(bits & below);
          colidx_s[at] = newcol ? newcol[c] : c;
          pos[at] = k;
        }
        out += __popcll(bits);
      } else {
        n += __popcll(bits);
      }
      k0 += L;
    }
    if (!FILL && live && lane == 0) cnt[orow] = n;
  }
}

template <class Idx, bool FILL>
void launch_select(int L, const nh_csr *A, const Idx *col, const unsigned char *rowkeep, const unsigned char *colkeep, int drop_zeros, const i64 *newrow, const i64 *newcol,
                   int32_t *cnt, const i64 *rowptr_s, i64 *colidx_s, i64 *pos, hipStream_t s) {
#define NH_SELECT(LL)                                                                                                                                                    \
  case LL:                                                                                                                                                               \
    hipLaunchKernelGGL((k_select<LL, Idx, FILL>), dim3(spmv_grid(A->nrows, LL)), dim3(WG), 0, s, (i64)A->nrows, (const i64 *)A->rowptr_dev, col, A->values_dev, rowkeep, \
                       colkeep, drop_zeros, newrow, newcol, cnt, rowptr_s, colidx_s, pos);                                                                               \
    break;
  switch (L) {
    NH_SELECT(1)
    NH_SELECT(2)
    NH_SELECT(4)
    NH_SELECT(8)
    NH_SELECT(16)
    NH_SELECT(32)
    default:
    NH_SELECT(64)
  }
#undef NH_SELECT
}

template <bool FILL>
void select(const nh_csr *A, const unsigned char *rowkeep, const unsigned char *colkeep, int drop_zeros, const i64 *newrow, const i64 *newcol, int32_t *cnt,
            const i64 *rowptr_s, i64 *colidx_s, i64 *pos, hipStream_t s) {
  const int L = A->lanes ? A->lanes : nh_csr_lanes(A->nrows, A->nnz);
  if (A->col32_dev)
    launch_select<int32_t, FILL>(L, A, A->col32_dev, rowkeep, colkeep, drop_zeros, newrow, newcol, cnt, rowptr_s, colidx_s, pos, s);
  else
    launch_select<i64, FILL>(L, A, (const i64 *)A->colidx_dev, rowkeep, colkeep, drop_zeros, newrow, newcol, cnt, rowptr_s, colidx_s, pos, s);
}

// new[i] = the number of kept indices below i (new[n]: how many are kept, returned in *kept); tmp: n int32
int renumber(const unsigned char *keep, i64 n, int32_t *tmp, i64 *renum, i64 *kept, hipStream_t s) {
  if (n) {
    hipLaunchKernelGGL(k_mask_i32, dim3(vec_grid(n)), dim3(WG), 0, s, n, keep, tmp);
    NH_LAUNCH_CHECK();
  }
  if (int rc = nh_scan_exclusive(tmp, renum, n, s)) return rc;
  NH_CHECK_HIP(hipMemcpyAsync(kept, renum + n, sizeof(i64), hipMemcpyDeviceToHost, s));
  NH_CHECK_HIP(hipStreamSynchronize(s));
  return NH_OK;
}

int check_select(const char *who, const nh_csr *A, const unsigned char *rowkeep, const unsigned char *colkeep, const int64_t *newrow, const int64_t *newcol) {
  if (int rc = check_csr(who, A)) return rc;
  NH_REQUIRE((rowkeep != nullptr) == (newrow != nullptr) && (colkeep != nullptr) == (newcol != nullptr), "%s: a mask and its renumbering go together", who);
  return NH_OK;
}

__global__ __launch_bounds__(WG) void k_place(i64 n, const double *__restrict__ a, const i64 *__restrict__ pos, double *__restrict__ out) {
  for (i64 k = (i64)blockIdx.x * WG + threadIdx.x; k < n; k += (i64)gridDim.x * WG) out[pos[k]] = a[k];
}

__global__ __launch_bounds__(WG) void k_add_at(i64 n, const double *__restrict__ b, const i64 *__restrict__ pos, double sign, double *__restrict__ out) {
  for (i64 k = (i64)blockIdx.x * WG + threadIdx.x; k < n; k += (i64)gridDim.x * WG) out[pos[k]] += sign * b[k];
}

}  // namespace

extern "C" {

int nh_csr_transpose(const nh_csr *A, int64_t *rowptr_t_dev, int64_t *colidx_t_dev, int64_t *pos_dev, void *stream) {
  NH_REQUIRE(A, "nh_csr_transpose: NULL matrix");
  NH_REQUIRE(A->nrows >= 0 && A->ncols >= 0 && A->nnz >= 0, "nh_csr_transpose: negative size");
  NH_REQUIRE(A->nrows <= INT32_MAX, "nh_csr_transpose: the column histogram is int32: at most %d rows", INT32_MAX);
  NH_REQUIRE(rowptr_t_dev, "nh_csr_transpose: NULL row pointers of the result");
  NH_REQUIRE(!A->nnz || (A->rowptr_dev && (A->colidx_dev || A->col32_dev) && colidx_t_dev && pos_dev), "nh_csr_transpose: NULL index array");
  NH_REQUIRE(!A->col32_dev || A->ncols <= INT32_MAX, "nh_csr_transpose: int32 column indices cannot address %lld columns", (long long)A->ncols);
  hipStream_t s = nh_stream(stream);
  if (!A->nnz) {
    NH_CHECK_HIP(hipMemsetAsync(rowptr_t_dev, 0, sizeof(i64) * (size_t)(A->ncols + 1), s));
    return NH_OK;
  }
  const i64 nnz = A->nnz, ncols = A->ncols;
  // the histogram and the slot cursors, ncols int32: in `pos`, which nothing needs before the sort, where they fit
  Scratch scratch;
  int32_t *cnt = (int32_t *)pos_dev;
  if ((ncols + 1) / 2 > nnz) {
    NH_CHECK_HIP(hipMalloc(&scratch.p, sizeof(int32_t) * (size_t)ncols));
    cnt = (int32_t *)scratch.p;
  }
  const dim3 entries(vec_grid(nnz)), block(WG);
  NH_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)ncols, s));
  if (A->col32_dev)
    hipLaunchKernelGGL(k_tr_count<int32_t>, entries, block, 0, s, nnz, A->col32_dev, cnt);
  else
    hipLaunchKernelGGL(k_tr_count<i64>, entries, block, 0, s, nnz, (const i64 *)A->colidx_dev, cnt);
  NH_LAUNCH_CHECK();
  if (int rc = nh_scan_exclusive(cnt, (i64 *)rowptr_t_dev, ncols, s)) return rc;
  NH_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)ncols, s));
  if (A->col32_dev)
    hipLaunchKernelGGL(k_tr_place<int32_t>, entries, block, 0, s, nnz, A->col32_dev, (const i64 *)rowptr_t_dev, cnt, (i64 *)colidx_t_dev);
  else
    hipLaunchKernelGGL(k_tr_place<i64>, entries, block, 0, s, nnz, (const i64 *)A->colidx_dev, (const i64 *)rowptr_t_dev, cnt, (i64 *)colidx_t_dev);
  NH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tr_sort, dim3(spmv_grid(ncols, 64)), block, 0, s, ncols, (i64)A->nrows, (const i64 *)A->rowptr_dev, (const i64 *)rowptr_t_dev, (i64 *)colidx_t_dev,
                     (i64 *)pos_dev);
  NH_LAUNCH_CHECK();
  if (scratch.p) NH_CHECK_HIP(hipStreamSynchronize(s));
  return NH_OK;
}

int nh_csr_select_count(const nh_csr *A, const unsigned char *rowkeep_dev, const unsigned char *colkeep_dev, int drop_zeros, int64_t nrows_s, int64_t ncols_s,
                        int64_t *newrow_dev, int64_t *newcol_dev, int64_t *rowptr_s_dev, int64_t *nnz, void *stream) {
  if (int rc = check_select("nh_csr_select_count", A, rowkeep_dev, colkeep_dev, newrow_dev, newcol_dev)) return rc;
  NH_REQUIRE(rowptr_s_dev && nnz, "nh_csr_select_count: NULL result");
  NH_REQUIRE(nrows_s >= 0 && nrows_s <= A->nrows && ncols_s >= 0 && ncols_s <= A->ncols, "nh_csr_select_count: the selection cannot have more rows or columns than the matrix");
  hipStream_t s = nh_stream(stream);
  *nnz = 0;
  Scratch scratch;
  NH_CHECK_HIP(hipMalloc(&scratch.p, sizeof(int32_t) * (size_t)(std::max(A->nrows, A->ncols) + 1)));
  int32_t *tmp = (int32_t *)scratch.p;
  i64 kept = A->nrows;
  if (rowkeep_dev)
    if (int rc = renumber(rowkeep_dev, A->nrows, tmp, (i64 *)newrow_dev, &kept, s)) return rc;
  NH_REQUIRE(kept == nrows_s, "nh_csr_select_count: the row mask keeps %lld rows, the caller made room for %lld", (long long)kept, (long long)nrows_s);
  kept = A->ncols;
  if (colkeep_dev)
    if (int rc = renumber(colkeep_dev, A->ncols, tmp, (i64 *)newcol_dev, &kept, s)) return rc;
  NH_REQUIRE(kept == ncols_s, "nh_csr_select_count: the column mask keeps %lld columns, the caller expects %lld", (long long)kept, (long long)ncols_s);
  if (!nrows_s || !A->nnz) {  // nothing to count: no launch
    NH_CHECK_HIP(hipMemsetAsync(rowptr_s_dev, 0, sizeof(i64) * (size_t)(nrows_s + 1), s));
    return NH_OK;
  }
  select<false>(A, rowkeep_dev, colkeep_dev, drop_zeros, (const i64 *)newrow_dev, (const i64 *)newcol_dev, tmp, nullptr, nullptr, nullptr, s);
  NH_LAUNCH_CHECK();
  if (int rc = nh_scan_exclusive(tmp, (i64 *)rowptr_s_dev, nrows_s, s)) return rc;
  NH_CHECK_HIP(hipMemcpyAsync(nnz, (i64 *)rowptr_s_dev + nrows_s, sizeof(i64), hipMemcpyDeviceToHost, s));
  NH_CHECK_HIP(hipStreamSynchronize(s));
  return NH_OK;
}

int nh_csr_select_fill(const nh_csr *A, const unsigned char *rowkeep_dev, const unsigned char *colkeep_dev, int drop_zeros, const int64_t *newrow_dev,
                       const int64_t *newcol_dev, const int64_t *rowptr_s_dev, int64_t *colidx_s_dev, int64_t *pos_dev, void *stream) {
  if (int rc = check_select("nh_csr_select_fill", A, rowkeep_dev, colkeep_dev, newrow_dev, newcol_dev)) return rc;
  if (!A->nrows || !A->nnz) return NH_OK;
  NH_REQUIRE(rowptr_s_dev && colidx_s_dev && pos_dev, "nh_csr_select_fill: NULL result");
  select<true>(A, rowkeep_dev, colkeep_dev, drop_zeros, (const i64 *)newrow_dev, (const i64 *)newcol_dev, nullptr, (const i64 *)rowptr_s_dev, (i64 *)colidx_s_dev,
               (i64 *)pos_dev, nh_stream(stream));
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_csr_add_values(int64_t nnz_a, const double *a_dev, const int64_t *pos_a_dev, int64_t nnz_b, const double *b_dev, const int64_t *pos_b_dev, double sign, int64_t nnz_u,
                      double *out_dev, void *stream) {
  NH_REQUIRE(nnz_a >= 0 && nnz_b >= 0 && nnz_u >= 0 && nnz_a <= nnz_u && nnz_b <= nnz_u, "nh_csr_add_values: a part has more entries than the union");
  NH_REQUIRE(sign == 1. || sign == -1., "nh_csr_add_values: the sign is 1 or -1");
  NH_REQUIRE(!nnz_a || (a_dev && pos_a_dev), "nh_csr_add_values: NULL first part");
  NH_REQUIRE(!nnz_b || (b_dev && pos_b_dev), "nh_csr_add_values: NULL second part");
  NH_REQUIRE(!nnz_u || out_dev, "nh_csr_add_values: NULL result");
  if (!nnz_u) return NH_OK;
  hipStream_t s = nh_stream(stream);
  NH_CHECK_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * (size_t)nnz_u, s));
  if (nnz_a) {
    hipLaunchKernelGGL(k_place, dim3(vec_grid(nnz_a)), dim3(WG), 0, s, (i64)nnz_a, a_dev, (const i64 *)pos_a_dev, out_dev);
    NH_LAUNCH_CHECK();
  }
  if (nnz_b) {
    hipLaunchKernelGGL(k_add_at, dim3(vec_grid(nnz_b)), dim3(WG), 0, s, (i64)nnz_b, b_dev, (const i64 *)pos_b_dev, sign, out_dev);
    NH_LAUNCH_CHECK();
  }
  return NH_OK;
}

}  // extern "C"
