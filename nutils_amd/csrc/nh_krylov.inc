// What the Krylov solvers of nh_csr.hip, nh_csr_multi.hip and nh_amg.hip share, so that the files cannot drift apart: the workgroup size and grid caps, the sums over a
// workgroup and over the partials of the kernel before, the checks of a CSR view, and the head of a CG work array.  Included inside the anonymous namespace of
// each file.

constexpr int WG = 256;
constexpr int SPMV_MAX_WGS = 2048;  // 8 waves per SIMD on 256 CUs; also the number of p . Ap partials every workgroup of a CG update sums
constexpr int VEC_MAX_WGS = 1024;

// the cells of a CG work array (nh_cg_*, nh_pcg_*) that are the caller's to read (RR, FLAG_B) and to write (STOP: the init clears it, the kernels only read it)
enum { W_RR = 0, W_FLAG_B = 1, W_STOP = 2 };

// sum over the workgroup in a fixed order; every thread returns the total
__device__ __forceinline__ double block_sum(double s, double *lds) {
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();  // (lds may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// block_sum of C numbers at once (lds: 4 C doubles), each added in block_sum's order
template <int C>
__device__ __forceinline__ void block_sum_n(double (&s)[C], double *lds) {
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int o = 32; o; o >>= 1) s[c] += __shfl_xor(s[c], o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < C; ++c) lds[4 * c + (threadIdx.x >> 6)] = s[c];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = ((lds[4 * c] + lds[4 * c + 1]) + lds[4 * c + 2]) + lds[4 * c + 3];
}

// sum of n partials, the same order in every workgroup
__device__ __forceinline__ double partial_sum(const double *part, int n, double *lds) {
  double s = 0;
  for (int j = threadIdx.x; j < n; j += WG) s += part[j];
  return block_sum(s, lds);
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
