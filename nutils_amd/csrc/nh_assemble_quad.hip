// Write-once assembly for structured 2-D tensor-product bases on quadrilaterals: the C0 'std' basis of degree 1 or 2 and the quadratic
// spline basis, 1 or 2 components, constant-coefficient bilinear forms (examples/laplace.py, poisson.py, elasticity.py).
//
// Replaces, for these bases, the generated element loop + einsum (evaluable.py:6773-6786, 1885-1886) and the sparse dedup / accumulate of
// its result (evaluable.py:588-616, 5560-5682; numeric.py:434-460): same CSR layout as nh_pattern_expand (rows / cols lexicographic,
// structural zeros kept, flat dof = node * ncomp + comp), each value formed once and stored once.
//
// Pattern.  Along an axis with n elements, dof X of the 'std' basis of degree p couples to [X-p, X+p] if X % p == 0, else to
// [p (X/p), p (X/p) + p], clipped to [0, n p]; dof X of the spline basis to [max(0, X-p), min(n+p-1, X+p)].  A 2-D row is the Kronecker
// product of the two 1-D ranges (axis 0 slowest), so row pointers and column positions are arithmetic (Axis below).
//
// Formulation.  With R_m[q] = (value, d/dxi_0, d/dxi_1) of local function m at point q (the class table of the element), Ji = J^-1 and
// wd = w_q |det J|, the physical slots are D_m = (R_m0, sum_a R_m(1+a) Ji[a][b]) and
//     A[(m,c),(n,d)] = sum_q sum_{a,b} wd D_m[a] C[c][a][d][b] D_n[b] = sum_q h_d . R_n,
//     g_d[b] = sum_a wd D_m[a] C[c][a][d][b],   h_d = (g_d[0], sum_b Ji[a][b] g_d[1+b])
// so a row costs 3 FMAs per (point, trial function, component) beyond the per-point h.
//
// Ownership.  A workgroup owns a tile of TX node lines (axis 0) x TY nodes (axis 1); a thread owns one row (node, component) of it.
// Phase 1: the geometric factors (Ji, wd) of every (element, point) touching the tile, into LDS (thread per (element, point)).
// Phase 2: each thread sums its row over the (up to (p+1)^2) elements that contain its node, in registers laid out as the row's band --
// the element's column offset within the band is (element - first element of the node) * step, a compile-time index once the element
// loop is unrolled.  Phase 3: the rows of every line of the tile go to LDS laid out exactly like the CSR (a line's rows are contiguous in
// the value array), and are streamed out with coalesced stores.  No global atomics, no zero-fill, no element map; every value is stored
// by one lane, and every sum is formed in a fixed order: repeated assemblies are bit-identical.  Elements on tile borders are evaluated
// (phase 1 only) by every tile they touch.
#include "nh_common.h"

#include <algorithm>

namespace {

#include "nh_geom.inc"

// one axis of the structured basis: n elements, degree p, 'std' (C0, step p) or spline (maximal smoothness, step 1)
struct Axis {
  int n, p, spline;
  __host__ __device__ int ndofs() const { return spline ? n + p : n * p + 1; }
  __host__ __device__ int step() const { return spline ? 1 : p; }
  __host__ __device__ int elo(int X) const { return spline ? max(0, X - p) : (X % p == 0 ? max(0, X / p - 1) : X / p); }
  __host__ __device__ int ehi(int X) const { return spline ? min(n - 1, X) : min(n - 1, X / p); }
  __host__ __device__ int lo(int X) const { return elo(X) * step(); }
  __host__ __device__ int len(int X) const { return ehi(X) * step() + p - lo(X) + 1; }
  // sum of len(X') over X' < X, 0 <= X <= ndofs()
  __host__ __device__ i64 pre(int X) const {
    if (spline) {
      const i64 a = min(X, p), b = max(0, X - n);
      return (i64)X * (2 * p + 1) - (a * p - a * (a - 1) / 2) - b * (b + 1) / 2;
    }
    const i64 kv = (X + p - 1) / p;  // vertices in front of X
    return kv * (2 * p + 1) - (kv >= 1 ? p : 0) - (kv >= n + 1 ? p : 0) + (X - kv) * (p + 1);
  }
};

static Axis make_axis(int n, int btype, int degree) { return Axis{n, degree, btype == 1}; }

// ---- closed-form pattern: thread per row (node, component) ----
__global__ void k_quad_pattern(Axis a0, Axis a1, int nc, i64 *rowptr, i64 *colidx) {
  const int N1 = a1.ndofs();
  const i64 nrows = (i64)a0.ndofs() * N1 * nc;
  const i64 T1 = a1.pre(N1);
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r <= nrows; r += (i64)gridDim.x * blockDim.x) {
    if (r == nrows) {
      rowptr[r] = (i64)nc * nc * a0.pre(a0.ndofs()) * T1;
      continue;
    }
    const int c = (int)(r % nc);
    const i64 node = r / nc;
    const int X = (int)(node / N1), Y = (int)(node % N1);
    const int l0 = a0.len(X), l1 = a1.len(Y), lo0 = a0.lo(X), lo1 = a1.lo(Y);
    const i64 start = (i64)nc * nc * (a0.pre(X) * T1 + l0 * a1.pre(Y)) + (i64)c * nc * l0 * l1;
    rowptr[r] = start;
    i64 k = start;
    for (int u = 0; u < l0; ++u)
      for (int v = 0; v < l1; ++v)
        for (int d = 0; d < nc; ++d) colidx[k++] = ((i64)(lo0 + u) * N1 + lo1 + v) * nc + d;
  }
}

struct QuadK {
  Axis a0, a1;
  int nq;
  const double *w;        // [nq]
  int gkind;              // NH_GEOM_ISO or NH_GEOM_BOX
  const double *gT;       // ISO: [4][nq][3]
  const double *verts;    // ISO: [(n0+1)(n1+1)][2]
  const double *origin, *size;  // BOX: [nelems][2]
  const double *T;        // [nclass][nb][nq][3]
  const int32_t *cls0, *cls1;
  int ncls1, ncls;
  int nograd;
  double C[2][3][2][3];
  double *values;
  int ntx, nty;           // tiles per axis
};

// tile sizes (TX lines x TY nodes x NC components = threads) per instantiation: LDS for the factors of the elements of a tile and for its rows
template <int P, bool SPL, int NC> struct QuadTile;
template <> struct QuadTile<1, false, 1> { static constexpr int TX = 4, TY = 64; };
template <> struct QuadTile<1, false, 2> { static constexpr int TX = 2, TY = 64; };
template <> struct QuadTile<2, false, 1> { static constexpr int TX = 4, TY = 64; };
template <> struct QuadTile<2, false, 2> { static constexpr int TX = 1, TY = 64; };
template <> struct QuadTile<2, true, 1> { static constexpr int TX = 4, TY = 32; };
template <> struct QuadTile<2, true, 2> { static constexpr int TX = 2, TY = 32; };

template <int P, bool SPL, int NC> struct QuadCfg {
  static constexpr int TX = QuadTile<P, SPL, NC>::TX, TY = QuadTile<P, SPL, NC>::TY;
  static constexpr int NT = TX * TY * NC;
  static constexpr int STEP = SPL ? 1 : P;
  static constexpr int NB1 = P + 1, NB = NB1 * NB1;
  static constexpr int BW = 2 * P + 1;           // widest 1-D band
  static constexpr int AMAX = SPL ? P + 1 : 2;   // elements per axis containing one node
  static constexpr int EX = SPL ? TX + P : (TX - 1) / P + 2;  // elements per axis touching a tile
  static constexpr int EY = SPL ? TY + P : (TY - 1) / P + 2;
  static constexpr int LINE = NC * NC * BW * BW * TY;  // doubles of one line's rows (bound)
  static constexpr int GS = EX * EY + 1;  // one (point, factor) plane of the factor table: the tile's elements + a zero slot for absent elements
  static size_t gf_doubles(int nq) { return (size_t)5 * nq * GS; }
  __host__ __device__ static size_t tab_doubles(int nq, int ncls) { return ((size_t)ncls * NB * nq * 3 + nq + 1) & ~(size_t)1; }  // class tables and weights (16-byte aligned)
  static size_t lds_bytes(int nq, int ncls) { return 8 * (tab_doubles(nq, ncls) + std::max(gf_doubles(nq), (size_t)TX * LINE)); }
};

template <int P, bool SPL, int NC>
__global__ void __launch_bounds__((QuadCfg<P, SPL, NC>::NT)) k_quad(QuadK k) {
  using Q = QuadCfg<P, SPL, NC>;
  const Axis A0{k.a0.n, P, SPL}, A1{k.a1.n, P, SPL};  // (degree and type as constants: the divisions by p fold)
  extern __shared__ double lds_all[];
  const int tid = threadIdx.x, nq = k.nq;
  // class tables and weights stay in LDS for the whole launch (read by every row at every point: broadcast reads), transposed to [class][point][function][3]
  // so that the functions of one point are at compile-time offsets from one address
  const int ntab = k.ncls * Q::NB * nq * 3;
  double *tab = lds_all, *wq = lds_all + ntab;
  double *lds = lds_all + Q::tab_doubles(nq, k.ncls);
  for (int i = tid; i < ntab; i += Q::NT) {
    const int s = i % 3, q = (i / 3) % nq, n = (i / (3 * nq)) % Q::NB, cl = i / (3 * nq * Q::NB);
    tab[((cl * nq + q) * Q::NB + n) * 3 + s] = nh_g(k.T)[i];
  }
  for (int i = tid; i < nq; i += Q::NT) wq[i] = nh_g(k.w)[i];
  const int N0 = A0.ndofs(), N1 = A1.ndofs();
  const i64 T1 = A1.pre(N1);
  constexpr int GS = Q::GS;
  // this thread's row within a tile
  const int c = tid % NC, y = (tid / NC) % Q::TY, x = tid / (NC * Q::TY);
  // (the form tensor goes through LDS: read from the argument block by every lane, it would hold 2 NC^2 9 scalar registers)
  __shared__ double Cs[NC][3][NC][3];
  if (tid < NC * 9 * NC) (&Cs[0][0][0][0])[tid] = k.C[tid / (9 * NC)][(tid / (3 * NC)) % 3][(tid / 3) % NC][tid % 3];
  __syncthreads();
  double Cc[3][NC][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int d = 0; d < NC; ++d)
#pragma unroll
      for (int b = 0; b < 3; ++b) Cc[a][d][b] = Cs[c][a][d][b];

  for (int tile = blockIdx.x; tile < k.ntx * k.nty; tile += gridDim.x) {
    const int X0 = (tile / k.nty) * Q::TX, Y0 = (tile % k.nty) * Q::TY;
    const int Xe = min(X0 + Q::TX, N0), Ye = min(Y0 + Q::TY, N1);
    const int e0lo = A0.elo(X0), e1lo = A1.elo(Y0);
    const int E0 = A0.ehi(Xe - 1) - e0lo + 1, E1 = A1.ehi(Ye - 1) - e1lo + 1;
    // phase 1: geometric factors of the elements touching the tile (and the zero slot of absent elements)
    for (int i = tid; i < 5 * nq; i += Q::NT) lds[(size_t)i * GS + Q::EX * Q::EY] = 0.;
    for (int i = tid; i < E0 * E1 * nq; i += Q::NT) {
      const int q = i % nq, eb = (i / nq) % E1, ea = i / (nq * E1);
      const int e0 = e0lo + ea, e1 = e1lo + eb;
      double J[2][2], Ji[2][2], det;
      if (k.gkind == NH_GEOM_ISO) {
        J[0][0] = J[0][1] = J[1][0] = J[1][1] = 0.;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const i64 v = (i64)(e0 + (a >> 1)) * (A1.n + 1) + e1 + (a & 1);
          const auto t = nh_g(k.gT) + ((i64)a * nq + q) * 3;
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const double xr = nh_g(k.verts)[v * 2 + r];
#pragma unroll
            for (int s = 0; s < 2; ++s) J[r][s] += xr * t[1 + s];
          }
        }
      } else {
        const i64 e = (i64)e0 * A1.n + e1;
        J[0][0] = nh_g(k.size)[e * 2];
        J[1][1] = nh_g(k.size)[e * 2 + 1];
        J[0][1] = J[1][0] = 0.;
      }
      invert<2>(J, Ji, det);
      if (k.nograd) Ji[0][0] = Ji[0][1] = Ji[1][0] = Ji[1][1] = 0.;
      double *g = lds + (size_t)q * 5 * GS + ea * Q::EY + eb;
      g[0] = Ji[0][0];
      g[GS] = Ji[0][1];
      g[2 * GS] = Ji[1][0];
      g[3 * GS] = Ji[1][1];
      g[4 * GS] = wq[q] * fabs(det);
    }
    __syncthreads();
    // phase 2: the row of (X, Y, c) in registers, as its band
    const int X = X0 + x, Y = Y0 + y;
    const bool own = X < N0 && Y < N1;
    double acc[Q::BW][Q::BW][NC];
#pragma unroll
    for (int u = 0; u < Q::BW; ++u)
#pragma unroll
      for (int v = 0; v < Q::BW; ++v)
#pragma unroll
        for (int d = 0; d < NC; ++d) acc[u][v][d] = 0.;
    int l0 = 0, l1 = 0;
    if (own) {
      const int f0 = A0.elo(X), f1 = A1.elo(Y);
      const int cnt0 = A0.ehi(X) - f0 + 1, cnt1 = A1.ehi(Y) - f1 + 1;
      l0 = A0.len(X);
      l1 = A1.len(Y);
      // (branch-free over the element slots: an absent element -- a node on the mesh border, inner nodes of a 'std' element -- reads the zero
      // factors of slot EX * EY and adds exact zeros to band positions that are not written out)
#pragma unroll
      for (int a0 = 0; a0 < Q::AMAX; ++a0) {
        const int e0 = f0 + a0, i = X - e0 * Q::STEP;
#pragma unroll
        for (int a1 = 0; a1 < Q::AMAX; ++a1) {
          const int e1 = f1 + a1, j = Y - e1 * Q::STEP;
          const bool ok = a0 < cnt0 && a1 < cnt1;
          const int m = ok ? i * Q::NB1 + j : 0;
          const int cls = ok ? (k.cls0 ? nh_g(k.cls0)[e0] * k.ncls1 : 0) + (k.cls1 ? nh_g(k.cls1)[e1] : 0) : 0;
          const double *Tc = tab + (size_t)cls * nq * Q::NB * 3;
          const double *g = lds + (ok ? (e0 - e0lo) * Q::EY + (e1 - e1lo) : Q::EX * Q::EY);
          for (int q = 0; q < nq; ++q) {
            const double *gq = g + (size_t)q * 5 * GS;
            const double J00 = gq[0], J01 = gq[GS], J10 = gq[2 * GS], J11 = gq[3 * GS], wd = gq[4 * GS];
            const double *Tq = Tc + (size_t)q * Q::NB * 3;
            const double *Rm = Tq + m * 3;
            const double D[3] = {Rm[0] * wd, (Rm[1] * J00 + Rm[2] * J10) * wd, (Rm[1] * J01 + Rm[2] * J11) * wd};
            double h[NC][3];
#pragma unroll
            for (int d = 0; d < NC; ++d) {
              double gd[3];
#pragma unroll
              for (int b = 0; b < 3; ++b) gd[b] = D[0] * Cc[0][d][b] + D[1] * Cc[1][d][b] + D[2] * Cc[2][d][b];
              h[d][0] = gd[0];
              h[d][1] = J00 * gd[1] + J01 * gd[2];
              h[d][2] = J10 * gd[1] + J11 * gd[2];
            }
#pragma unroll
            for (int kk = 0; kk < Q::NB1; ++kk)
#pragma unroll
              for (int ll = 0; ll < Q::NB1; ++ll) {
                const double *Rn = Tq + (kk * Q::NB1 + ll) * 3;
                const double r0 = Rn[0], r1 = Rn[1], r2 = Rn[2];
#pragma unroll
                for (int d = 0; d < NC; ++d) acc[a0 * Q::STEP + kk][a1 * Q::STEP + ll][d] += h[d][0] * r0 + h[d][1] * r1 + h[d][2] * r2;
              }
          }
        }
      }
    }
    __syncthreads();  // (the factor table is dead: the row buffers take its place)
    // phase 3: rows into LDS laid out like the CSR lines of the tile, then streamed out
    if (own) {
      const i64 rel = (i64)NC * NC * l0 * (A1.pre(Y) - A1.pre(Y0)) + (i64)c * NC * l0 * l1;
      double *row = lds + (size_t)x * Q::LINE + rel;
#pragma unroll
      for (int u = 0; u < Q::BW; ++u)
#pragma unroll
        for (int v = 0; v < Q::BW; ++v)
          if (u < l0 && v < l1)
#pragma unroll
            for (int d = 0; d < NC; ++d) row[(u * l1 + v) * NC + d] = acc[u][v][d];
    }
    __syncthreads();
    for (int xx = 0; xx < Q::TX && X0 + xx < N0; ++xx) {
      const int Xl = X0 + xx, ll0 = A0.len(Xl);
      const i64 base = (i64)NC * NC * (A0.pre(Xl) * T1 + ll0 * A1.pre(Y0));
      const int n = NC * NC * ll0 * (int)(A1.pre(Ye) - A1.pre(Y0));
      const double *src = lds + (size_t)xx * Q::LINE;
      for (int i = tid; i < n; i += Q::NT) __builtin_nontemporal_store(src[i], nh_gw(k.values) + base + i);
    }
    __syncthreads();
  }
}

template <int P, bool SPL, int NC>
hipError_t launch_quad(const QuadK &k, int max_wg, size_t *lds_out, hipStream_t s) {
  using Q = QuadCfg<P, SPL, NC>;
  QuadK p = k;
  p.ntx = (k.a0.ndofs() + Q::TX - 1) / Q::TX;
  p.nty = (k.a1.ndofs() + Q::TY - 1) / Q::TY;
  const size_t ldsb = Q::lds_bytes(k.nq, k.ncls);
  *lds_out = ldsb;
  if (ldsb > 160 * 1024) return hipErrorInvalidValue;
  const i64 ntiles = (i64)p.ntx * p.nty;
  const unsigned grid = (unsigned)std::min<i64>(ntiles, max_wg > 0 ? max_wg : 1 << 20);
  auto kern = k_quad<P, SPL, NC>;
  // the LDS limit of this instantiation is raised once per device (to the largest request so far), not on every re-assembly
  static size_t granted[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (ldsb > granted[dev]) {
    e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb);
    if (e != hipSuccess) return e;
    granted[dev] = ldsb;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(Q::NT), ldsb, s, p);
  return hipGetLastError();
}

// ---- uniform cells: replicate the rows of a small mesh ----
// Per axis the dofs fall into a head of H dofs, a periodic interior of period PER and a tail of TL dofs; with uniform cells the rows of a dof
// depend only on its place in that structure, and the small mesh holds the head, ONE period and the tail.
struct UAxis {
  Axis big, small;
  int H, PER, TL;  // H = ndofs: identity (the small mesh is the mesh)
};

static UAxis uniform_axis(int n, int btype, int degree) {
  UAxis u;
  u.big = make_axis(n, btype, degree);
  const int ns = btype == 1 ? 3 * degree - 1 : 2;  // spline: the first and last p-1 elements have tables of their own
  if (n <= ns) {
    u.small = u.big;
    u.H = u.big.ndofs(), u.PER = 1, u.TL = 0;
  } else {
    u.small = make_axis(ns, btype, degree);
    if (btype == 1) u.H = 2 * degree - 1, u.PER = 1, u.TL = 2 * degree - 1;
    else u.H = 1, u.PER = degree, u.TL = 1;
  }
  return u;
}

// small-mesh dof representing dof X of the big mesh
__device__ __forceinline__ int urep(const UAxis &u, int X) {
  const int N = u.big.ndofs(), Ns = u.small.ndofs();
  if (X < u.H) return X;
  if (X >= N - u.TL) return X - N + Ns;
  return u.H + (X - u.H) % u.PER;
}

// one workgroup per line X of axis 0 (grid-stride): the line's values are head | periodic middle | tail of the small line
__global__ void __launch_bounds__(256) k_quad_rows_uniform(UAxis u0, UAxis u1, int nc, const double *__restrict__ small, double *__restrict__ values) {
  const int N0 = u0.big.ndofs(), N1 = u1.big.ndofs(), N1s = u1.small.ndofs();
  const i64 T1 = u1.big.pre(N1), T1s = u1.small.pre(N1s);
  const int nc2 = nc * nc;
  for (int X = blockIdx.x; X < N0; X += gridDim.x) {
    const int Xs = urep(u0, X), l0 = u0.big.len(X);
    const i64 dst = (i64)nc2 * u0.big.pre(X) * T1, src = (i64)nc2 * u0.small.pre(Xs) * T1s;
    const i64 n = (i64)nc2 * l0 * T1, ns = (i64)nc2 * l0 * T1s;
    const i64 head = (i64)nc2 * l0 * u1.big.pre(min(u1.H, N1));
    const i64 tail = (i64)nc2 * l0 * (T1 - u1.big.pre(N1 - u1.TL));
    const int per = nc2 * l0 * (int)(u1.small.pre(u1.H + u1.PER) - u1.small.pre(u1.H));
    for (i64 i = threadIdx.x; i < n; i += blockDim.x) {
      i64 j;
      if (i < head) j = i;
      else if (i >= n - tail) j = i - n + ns;
      else j = head + (unsigned)(i - head) % (unsigned)per;
      __builtin_nontemporal_store(nh_g(small)[src + j], nh_gw(values) + dst + i);
    }
  }
}

}  // namespace

extern "C" {

int nh_quad_nnz(const int *shape, int btype, int degree, int ncomp, int64_t *nnz) {
  NH_REQUIRE(shape && nnz, "nh_quad_nnz: NULL argument");
  NH_REQUIRE(shape[0] >= 1 && shape[1] >= 1 && (btype == 0 || btype == 1) && degree >= 1 && degree <= 4 && ncomp >= 1 && ncomp <= 3,
             "nh_quad_nnz: shape / btype / degree / ncomp");
  const Axis a0 = make_axis(shape[0], btype, degree), a1 = make_axis(shape[1], btype, degree);
  *nnz = (int64_t)ncomp * ncomp * a0.pre(a0.ndofs()) * a1.pre(a1.ndofs());
  return NH_OK;
}

int nh_quad_pattern(const int *shape, int btype, int degree, int ncomp, int64_t *rowptr_dev, int64_t *colidx_dev, void *stream) {
  NH_REQUIRE(shape && rowptr_dev && colidx_dev, "nh_quad_pattern: NULL argument");
  int64_t nnz;
  int rc = nh_quad_nnz(shape, btype, degree, ncomp, &nnz);
  if (rc) return rc;
  const Axis a0 = make_axis(shape[0], btype, degree), a1 = make_axis(shape[1], btype, degree);
  const i64 nrows = (i64)a0.ndofs() * a1.ndofs() * ncomp;
  const unsigned grid = (unsigned)std::min<i64>((nrows + 256) / 256, 256 * 64);
  hipLaunchKernelGGL(k_quad_pattern, dim3(grid), dim3(256), 0, nh_stream(stream), a0, a1, ncomp, (i64 *)rowptr_dev, (i64 *)colidx_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_quad_matrix(const nh_quad_args *a, void *stream) {
  NH_REQUIRE(a, "nh_quad_matrix: NULL args");
  NH_REQUIRE(a->shape[0] >= 1 && a->shape[1] >= 1, "nh_quad_matrix: shape");
  const bool spl = a->btype == 1;
  NH_REQUIRE((a->btype == 0 && (a->degree == 1 || a->degree == 2)) || (spl && a->degree == 2),
             "nh_quad_matrix: bases 'std' degree 1 or 2, 'spline' degree 2 (btype %d degree %d)", a->btype, a->degree);
  NH_REQUIRE(a->ncomp == 1 || a->ncomp == 2, "nh_quad_matrix: ncomp %d", a->ncomp);
  NH_REQUIRE(a->nq >= 1 && a->weights_dev && a->T_dev && a->values_dev && a->C_host, "nh_quad_matrix: NULL argument");
  NH_REQUIRE((a->geom.kind == NH_GEOM_ISO && a->geom.gT_dev && a->geom.verts_dev) || (a->geom.kind == NH_GEOM_BOX && a->geom.size_dev),
             "nh_quad_matrix: geometry must be ISO (P1 table and vertices) or BOX");
  NH_REQUIRE(a->geom.bnd_axis < 0, "nh_quad_matrix: volume samples only");
  NH_REQUIRE(a->nclass[0] >= 1 && a->nclass[1] >= 1 && (a->nclass[0] == 1 || a->class0_dev) && (a->nclass[1] == 1 || a->class1_dev),
             "nh_quad_matrix: classes");
  QuadK k{};
  k.a0 = make_axis(a->shape[0], a->btype, a->degree);
  k.a1 = make_axis(a->shape[1], a->btype, a->degree);
  k.nq = a->nq;
  k.w = a->weights_dev;
  k.gkind = a->geom.kind;
  k.gT = a->geom.gT_dev;
  k.verts = a->geom.verts_dev;
  k.origin = a->geom.origin_dev;
  k.size = a->geom.size_dev;
  k.T = a->T_dev;
  k.cls0 = a->nclass[0] > 1 ? a->class0_dev : nullptr;
  k.cls1 = a->nclass[1] > 1 ? a->class1_dev : nullptr;
  k.ncls1 = a->nclass[1];
  k.ncls = a->nclass[0] * a->nclass[1];
  const int nc = a->ncomp;
  for (int c = 0; c < nc; ++c)
    for (int s = 0; s < 3; ++s)
      for (int d = 0; d < nc; ++d)
        for (int t = 0; t < 3; ++t) k.C[c][s][d][t] = a->C_host[((c * 3 + s) * nc + d) * 3 + t];
  k.nograd = !uses_gradients(a->C_host, nc, 3, nc);
  k.values = a->values_dev;
  hipStream_t s = nh_stream(stream);
  size_t ldsb = 0;
  hipError_t e;
  if (!spl && a->degree == 1) e = nc == 1 ? launch_quad<1, false, 1>(k, a->max_workgroups, &ldsb, s) : launch_quad<1, false, 2>(k, a->max_workgroups, &ldsb, s);
  else if (!spl) e = nc == 1 ? launch_quad<2, false, 1>(k, a->max_workgroups, &ldsb, s) : launch_quad<2, false, 2>(k, a->max_workgroups, &ldsb, s);
  else e = nc == 1 ? launch_quad<2, true, 1>(k, a->max_workgroups, &ldsb, s) : launch_quad<2, true, 2>(k, a->max_workgroups, &ldsb, s);
  if (ldsb > 160 * 1024) {
    nh_set_error("nh_quad_matrix: %d quadrature points need %zu bytes of LDS per workgroup (limit 160 KiB)", a->nq, ldsb);
    return NH_ELIMIT;
  }
  NH_CHECK_HIP(e);
  return NH_OK;
}

int nh_quad_uniform_shape(const int *shape, int btype, int degree, int *small_shape) {
  NH_REQUIRE(shape && small_shape && shape[0] >= 1 && shape[1] >= 1 && (btype == 0 || btype == 1) && degree >= 1, "nh_quad_uniform_shape: arguments");
  for (int i = 0; i < 2; ++i) small_shape[i] = uniform_axis(shape[i], btype, degree).small.n;
  return NH_OK;
}

int nh_quad_rows_uniform(const int *shape, int btype, int degree, int ncomp, const double *small_values_dev, double *values_dev, void *stream) {
  NH_REQUIRE(shape && small_values_dev && values_dev, "nh_quad_rows_uniform: NULL argument");
  NH_REQUIRE(shape[0] >= 1 && shape[1] >= 1 && (btype == 0 || btype == 1) && degree >= 1 && degree <= 2 && ncomp >= 1 && ncomp <= 2,
             "nh_quad_rows_uniform: shape / btype / degree / ncomp");
  const UAxis u0 = uniform_axis(shape[0], btype, degree), u1 = uniform_axis(shape[1], btype, degree);
  const unsigned grid = (unsigned)std::min(u0.big.ndofs(), 256 * 16);
  hipLaunchKernelGGL(k_quad_rows_uniform, dim3(grid), dim3(256), 0, nh_stream(stream), u0, u1, ncomp, small_values_dev, values_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

}  // extern "C"
