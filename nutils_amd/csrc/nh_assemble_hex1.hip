// Write-once assembly for the trilinear 'std' basis of a full 3-D structured topology (no periodic axis), 1-3 components, constant-coefficient
// bilinear forms: 3-D linear elasticity on hexahedra, anisotropic diffusion with a full tensor, vector mass + stiffness.
//
// Replaces, for this basis, the generated element loop + einsum (evaluable.py:6773-6786, 1885-1886) and the sparse dedup / accumulate of
// its result (evaluable.py:588-616, 5560-5682; numeric.py:434-460): same CSR layout as nh_pattern_expand (rows / cols lexicographic,
// structural zeros kept, flat dof = node * ncomp + comp), each value formed once and stored once.
//
// Pattern.  Along an axis of N = n + 1 nodes, node X couples to [max(0, X-1), min(N-1, X+1)]; a row is the Kronecker product of the three
// 1-D ranges (axis 0 slowest), so row pointers and column positions are arithmetic (Axis below).
//
// Formulation.  With D_m = (phi_m, grad phi_m) the physical slots of local function m at point q and wd = w_q |det J|, the element matrix is
//     A[(m,c),(n,d)] = sum_{a,b} C[c][a][d][b] G_mn[a][b],   G_mn[a][b] = sum_q wd D_m[a] D_n[b]
// and, C being constant, the assembled value of a node pair is C applied to the SUM of the element Grams of the elements that contain both
// nodes.  The Gram does not depend on C or the component count: per element 36 symmetric node pairs x nq x (S + S^2) FMAs (S = 3 slots when C
// has no value slot, else 4), per CSR value S^2 FMAs.
//
// Ownership.  A workgroup owns a column of 2 x 2 nodes (axes 1, 2) over a chunk of HX node planes along axis 0, and sweeps the chunk plane by
// plane.  Per element layer L (the 3 x 3 elements under the column between planes L and L+1): the physical slots of its elements (thread per
// (element, point), into LDS), then their Grams (thread per (element, node pair), into a ring of two layers in LDS); plane L is then final:
// thread per (node, neighbour, component) sums the Grams of the (up to 8) elements of layers L-1 and L that contain both nodes, in a fixed
// order, applies C, and puts the row values into LDS laid out like the CSR (the rows of one node line are contiguous in the value array);
// the plane's two lines are streamed out with coalesced stores.  No global atomics, no zero-fill, no element map; every value is stored by
// one lane and every sum is formed in a fixed order: repeated assemblies are bit-identical.  Elements next to a column are evaluated by
// every column they touch (9 elements per 4 nodes), the first layer of a chunk by both chunks.
#include "nh_common.h"

#include <algorithm>

namespace {

#include "nh_geom.inc"

// one axis of the trilinear basis: N nodes (n + 1)
struct Axis {
  int N;
  __host__ __device__ int lo(int X) const { return max(X - 1, 0); }
  __host__ __device__ int len(int X) const { return min(X + 1, N - 1) - lo(X) + 1; }
  // sum of len(X') over X' < X, 0 <= X <= N
  __host__ __device__ i64 pre(int X) const { return 3 * (i64)X - (X >= 1) - (X >= N); }
};

// ---- closed-form pattern: thread per row (node, component) ----
__global__ void k_hex1_pattern(Axis a0, Axis a1, Axis a2, int nc, i64 *rowptr, i64 *colidx) {
  const i64 nrows = (i64)a0.N * a1.N * a2.N * nc;
  const i64 T1 = a1.pre(a1.N), T2 = a2.pre(a2.N);
  for (i64 r = blockIdx.x * (i64)blockDim.x + threadIdx.x; r <= nrows; r += (i64)gridDim.x * blockDim.x) {
    if (r == nrows) {
      rowptr[r] = (i64)nc * nc * a0.pre(a0.N) * T1 * T2;
      continue;
    }
    const int c = (int)(r % nc);
    const i64 node = r / nc;
    const int Z = (int)(node % a2.N), Y = (int)((node / a2.N) % a1.N), X = (int)(node / ((i64)a2.N * a1.N));
    const int l0 = a0.len(X), l1 = a1.len(Y), l2 = a2.len(Z);
    const i64 start = (i64)nc * nc * (a0.pre(X) * T1 * T2 + l0 * (a1.pre(Y) * T2 + (i64)l1 * a2.pre(Z))) + (i64)c * nc * l0 * l1 * l2;
    rowptr[r] = start;
    i64 k = start;
    for (int u = 0; u < l0; ++u)
      for (int v = 0; v < l1; ++v)
        for (int w = 0; w < l2; ++w)
          for (int d = 0; d < nc; ++d) colidx[k++] = (((i64)(a0.lo(X) + u) * a1.N + a1.lo(Y) + v) * a2.N + a2.lo(Z) + w) * nc + d;
  }
}

struct Hex1K {
  Axis a0, a1, a2;
  int nq;
  const double *w;        // [nq]
  int gkind;              // NH_GEOM_ISO or NH_GEOM_BOX
  const double *verts;    // ISO: [N0 N1 N2][3]
  const double *size;     // BOX: [nelems][3]
  const double *T;        // [8][nq][4]
  int nograd;
  double C[3][4][3][4];
  double *values;
  int nty, ntz, nxc;      // columns per axis 1, 2; chunks along axis 0 (one workgroup each)
};

constexpr int HY = 2, HZ = 2;                  // nodes of a column per axis 1, 2
constexpr int EY = HY + 1, EZ = HZ + 1, EL = EY * EZ;  // elements of one layer under a column
constexpr int HX = 8;                          // node planes per chunk
constexpr int NP = 36;                         // node pairs m <= n of one element
constexpr int QC = 8;                          // points per pass of the slot table
constexpr int NT = 384;                        // threads (>= EL * NP = 324 Gram tasks, >= 4 * 27 * 3 row tasks)

__host__ __device__ constexpr int pair_index(int m, int n) { return m * 8 - m * (m - 1) / 2 + (n - m); }  // m <= n

template <int S> struct Hex1Cfg {
  static constexpr int LINE = 9 * 3 * 3 * 3 * HZ;  // doubles of one line's rows within a column (bound: nc^2 l0 l1 (3 HZ))
  static constexpr int SLOTS = QC * EL * (8 * S + 1);
  static constexpr int GRAM = 2 * EL * NP * S * S;
  __host__ __device__ static size_t tab_doubles(int nq) { return ((size_t)33 * nq + 1) & ~(size_t)1; }
  static constexpr int GEO = (HX + 2) * (EY + 1) * (EZ + 1) * 3;  // vertices (ISO) or element sizes (BOX) of a column chunk
  static size_t lds_bytes(int nq) { return 8 * (tab_doubles(nq) + SLOTS + GRAM + HY * LINE + GEO); }
};

template <int NC, int S>
__global__ void __launch_bounds__(NT) k_hex1(Hex1K k) {
  using Q = Hex1Cfg<S>;
  constexpr int S0 = 4 - S;  // first slot of C used (S = 3: gradients only)
  extern __shared__ double lds_all[];
  const int tid = threadIdx.x, nq = k.nq;
  // reference table transposed to [point][function][4], and weights: read by every element of every layer
  double *tab = lds_all, *wq = lds_all + 32 * nq;
  double *slot = lds_all + Q::tab_doubles(nq);  // [QC][EL][8][S] physical slots, then [QC][EL] wd
  double *wdl = slot + QC * EL * 8 * S;
  double *gram = slot + Q::SLOTS;               // [2][EL][NP][S][S]
  double *stage = gram + Q::GRAM;               // [HY][LINE]
  double *geo = stage + HY * Q::LINE;           // ISO: [HX + 2][EY + 1][EZ + 1][3] vertices; BOX: [HX + 1][EY][EZ][3] sizes
  for (int i = tid; i < 32 * nq; i += NT) {
    const int s = i % 4, m = (i / 4) % 8, q = i / 32;
    tab[i] = nh_g(k.T)[(m * nq + q) * 4 + s];
  }
  for (int i = tid; i < nq; i += NT) wq[i] = nh_g(k.w)[i];
  __shared__ double Cs[NC][S][NC][S];
  __shared__ unsigned char pm[NP], pn[NP];
  for (int i = tid; i < NC * S * NC * S; i += NT) {
    const int b = i % S, d = (i / S) % NC, a = (i / (S * NC)) % S, c = i / (S * NC * S);
    Cs[c][a][d][b] = k.C[c][S0 + a][d][S0 + b];
  }
  if (tid < 8)
    for (int n = tid; n < 8; ++n) pm[pair_index(tid, n)] = tid, pn[pair_index(tid, n)] = n;
  __syncthreads();
  const int n0 = k.a0.N - 1, n1 = k.a1.N - 1, n2 = k.a2.N - 1;
  const i64 T1 = k.a1.pre(k.a1.N), T2 = k.a2.pre(k.a2.N);

  {
    const int wg = blockIdx.x;
    const int Z0 = (wg % k.ntz) * HZ, Y0 = ((wg / k.ntz) % k.nty) * HY, X0 = (wg / (k.ntz * k.nty)) * HX;
    const int Xe = min(X0 + HX, k.a0.N), Ze = min(Z0 + HZ, k.a2.N);
    // the geometry of the whole chunk into LDS at once: one memory latency per workgroup instead of one per element layer
    if (k.gkind == NH_GEOM_ISO) {
      for (int i = tid; i < Q::GEO; i += NT) {
        const int r = i % 3, zz = (i / 3) % (EZ + 1), yy = (i / (3 * (EZ + 1))) % (EY + 1), pl = i / (3 * (EZ + 1) * (EY + 1));
        const int X = X0 - 1 + pl, Y = Y0 - 1 + yy, Z = Z0 - 1 + zz;
        geo[i] = X >= 0 && X < k.a0.N && Y >= 0 && Y < k.a1.N && Z >= 0 && Z < k.a2.N ? nh_g(k.verts)[(((i64)X * k.a1.N + Y) * k.a2.N + Z) * 3 + r] : 0.;
      }
    } else {
      for (int i = tid; i < (HX + 1) * EL * 3; i += NT) {
        const int r = i % 3, ez = Z0 - 1 + (i / 3) % EZ, ey = Y0 - 1 + (i / (3 * EZ)) % EY, ex = X0 - 1 + i / (3 * EL);
        geo[i] = ex >= 0 && ex < n0 && ey >= 0 && ey < n1 && ez >= 0 && ez < n2 ? nh_g(k.size)[(((i64)ex * n1 + ey) * n2 + ez) * 3 + r] : 0.;
      }
    }
    __syncthreads();
    for (int L = X0 - 1; L < Xe; ++L) {
      // ---- element layer L (if any): slots, then Grams into ring slot L & 1 ----
      if (L >= 0 && L < n0) {
        const int te = tid / NP, p = tid % NP;
        const int gy = Y0 - 1 + te / EZ, gz = Z0 - 1 + te % EZ;
        const bool gram_task = tid < EL * NP && gy >= 0 && gy < n1 && gz >= 0 && gz < n2;
        const int m = pm[p % NP], n = pn[p % NP];
        double G[S][S];
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
          for (int b = 0; b < S; ++b) G[a][b] = 0.;
        for (int q0 = 0; q0 < nq; q0 += QC) {
          const int qc = min(QC, nq - q0);
          for (int i = tid; i < EL * qc; i += NT) {
            const int e = i / qc, qq = i % qc, q = q0 + qq;
            const int ey = Y0 - 1 + e / EZ, ez = Z0 - 1 + e % EZ;
            if (ey < 0 || ey >= n1 || ez < 0 || ez >= n2) continue;
            double J[3][3], Ji[3][3], det;
            if (k.gkind == NH_GEOM_ISO) {
#pragma unroll
              for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) J[r][s] = 0.;
#pragma unroll 2
              for (int a = 0; a < 8; ++a) {
                const double *xa = geo + (((L - X0 + 1 + (a >> 2)) * (EY + 1) + ey - Y0 + 1 + ((a >> 1) & 1)) * (EZ + 1) + ez - Z0 + 1 + (a & 1)) * 3;
                const double *t = tab + ((size_t)q * 8 + a) * 4;  // (the geometry basis is the basis: the same table)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                  const double xr = xa[r];
#pragma unroll
                  for (int s = 0; s < 3; ++s) J[r][s] += xr * t[1 + s];
                }
              }
            } else {
              const double *sz = geo + (((L - X0 + 1) * EY + ey - Y0 + 1) * EZ + ez - Z0 + 1) * 3;
#pragma unroll
              for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) J[r][s] = r == s ? sz[r] : 0.;
            }
            invert<3>(J, Ji, det);
            if (k.nograd)
#pragma unroll
              for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) Ji[r][s] = 0.;
            wdl[qq * EL + e] = wq[q] * fabs(det);
            double *out = slot + (size_t)(qq * EL + e) * 8 * S;
            const double *R = tab + q * 32;
#pragma unroll
            for (int mm = 0; mm < 8; ++mm) {
              if (S == 4) out[mm * S] = R[mm * 4];
#pragma unroll
              for (int b = 0; b < 3; ++b) out[mm * S + S - 3 + b] = R[mm * 4 + 1] * Ji[0][b] + R[mm * 4 + 2] * Ji[1][b] + R[mm * 4 + 3] * Ji[2][b];
            }
          }
          __syncthreads();
          if (gram_task) {
            for (int qq = 0; qq < qc; ++qq) {
              const double wd = wdl[qq * EL + te];
              const double *Dm = slot + (size_t)(qq * EL + te) * 8 * S + m * S, *Dn = slot + (size_t)(qq * EL + te) * 8 * S + n * S;
              double t[S], r[S];
#pragma unroll
              for (int a = 0; a < S; ++a) t[a] = wd * Dm[a], r[a] = Dn[a];
#pragma unroll
              for (int a = 0; a < S; ++a)
#pragma unroll
                for (int b = 0; b < S; ++b) G[a][b] += t[a] * r[b];
            }
          }
          __syncthreads();
        }
        if (gram_task) {
          double *g = gram + ((size_t)((L & 1) * EL + te) * NP + p) * S * S;
#pragma unroll
          for (int a = 0; a < S; ++a)
#pragma unroll
            for (int b = 0; b < S; ++b) g[a * S + b] = G[a][b];
        }
        __syncthreads();
      }
      if (L < X0) continue;
      // ---- node plane X = L is final: rows into the stage, laid out like the CSR ----
      const int X = L, l0 = k.a0.len(X), lo0 = k.a0.lo(X);
      const i64 span = k.a2.pre(Ze) - k.a2.pre(Z0);
      if (tid < HY * HZ * 27 * NC) {
        const int c = tid % NC, off = (tid / NC) % 27, nd = tid / (NC * 27);
        const int Y = Y0 + nd / HZ, Z = Z0 + nd % HZ;
        const int u = off / 9 - 1, v = (off / 3) % 3 - 1, w = off % 3 - 1;
        if (Y < k.a1.N && Z < k.a2.N && X + u >= 0 && X + u < k.a0.N && Y + v >= 0 && Y + v < k.a1.N && Z + w >= 0 && Z + w < k.a2.N) {
          double H[S][S];
#pragma unroll
          for (int a = 0; a < S; ++a)
#pragma unroll
            for (int b = 0; b < S; ++b) H[a][b] = 0.;
          // elements containing both nodes, ascending (layer, then axis 1, then axis 2)
          for (int ex = max(max(X - 1, X + u - 1), 0); ex <= min(min(X, X + u), n0 - 1); ++ex)
            for (int ey = max(max(Y - 1, Y + v - 1), 0); ey <= min(min(Y, Y + v), n1 - 1); ++ey)
              for (int ez = max(max(Z - 1, Z + w - 1), 0); ez <= min(min(Z, Z + w), n2 - 1); ++ez) {
                const int mi = (X - ex) * 4 + (Y - ey) * 2 + (Z - ez), ni = (X + u - ex) * 4 + (Y + v - ey) * 2 + (Z + w - ez);
                const int e = (ey - Y0 + 1) * EZ + (ez - Z0 + 1);
                const bool tr = mi > ni;
                const double *g = gram + ((size_t)((ex & 1) * EL + e) * NP + (tr ? pair_index(ni, mi) : pair_index(mi, ni))) * S * S;
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                  for (int b = 0; b < S; ++b) H[a][b] += tr ? g[b * S + a] : g[a * S + b];
              }
          const int l1 = k.a1.len(Y), l2 = k.a2.len(Z);
          const int col = ((X + u - lo0) * l1 + (Y + v - k.a1.lo(Y))) * l2 + (Z + w - k.a2.lo(Z));
          double *row = stage + (size_t)(Y - Y0) * Q::LINE + (size_t)NC * NC * l0 * l1 * (k.a2.pre(Z) - k.a2.pre(Z0)) + (size_t)c * NC * l0 * l1 * l2 + col * NC;
#pragma unroll
          for (int d = 0; d < NC; ++d) {
            double s = 0.;
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
              for (int b = 0; b < S; ++b) s += Cs[c][a][d][b] * H[a][b];
            row[d] = s;
          }
        }
      }
      __syncthreads();
      for (int yy = 0; yy < HY && Y0 + yy < k.a1.N; ++yy) {
        const int Y = Y0 + yy, l1 = k.a1.len(Y);
        const i64 base = (i64)NC * NC * (k.a0.pre(X) * T1 * T2 + l0 * (k.a1.pre(Y) * T2 + (i64)l1 * k.a2.pre(Z0)));
        const int cnt = NC * NC * l0 * l1 * (int)span;
        const double *src = stage + (size_t)yy * Q::LINE;
        for (int i = tid; i < cnt; i += NT) __builtin_nontemporal_store(src[i], nh_gw(k.values) + base + i);
      }
      __syncthreads();
    }
  }
}

template <int NC, int S>
hipError_t launch_hex1(const Hex1K &k, size_t *lds_out, hipStream_t s) {
  using Q = Hex1Cfg<S>;
  const size_t ldsb = Q::lds_bytes(k.nq);
  *lds_out = ldsb;
  if (ldsb > 160 * 1024) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)((i64)k.nty * k.ntz * k.nxc);  // one workgroup per column chunk
  auto kern = k_hex1<NC, S>;
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
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), ldsb, s, k);
  return hipGetLastError();
}

// ---- uniform cells: replicate the rows of the 2 x 2 x 2 mesh ----
// Per axis a node is first, interior or last; with uniform cells its rows depend only on that class per axis, and the small mesh of
// min(n, 2) elements per axis holds every class (when n <= 2 the small mesh is the mesh).
struct UAxis {
  Axis big, small;
  int H, PER, TL;  // H = N: identity
};

static UAxis uniform_axis(int n) {
  UAxis u;
  u.big = Axis{n + 1};
  if (n <= 2) {
    u.small = u.big;
    u.H = n + 1, u.PER = 1, u.TL = 0;
  } else {
    u.small = Axis{3};
    u.H = 1, u.PER = 1, u.TL = 1;
  }
  return u;
}

__device__ __forceinline__ int urep(const UAxis &u, int X) {
  const int N = u.big.N, Ns = u.small.N;
  if (X < u.H) return X;
  if (X >= N - u.TL) return X - N + Ns;
  return u.H + (X - u.H) % u.PER;
}

// one workgroup per node line (X, Y) (grid-stride): the line's values are head | repeated middle | tail of the small line
__global__ void __launch_bounds__(256) k_hex1_rows_uniform(UAxis u0, UAxis u1, UAxis u2, int nc, const double *__restrict__ small, double *__restrict__ values) {
  const int N0 = u0.big.N, N1 = u1.big.N, N2 = u2.big.N, N2s = u2.small.N;
  const i64 T1 = u1.big.pre(N1), T2 = u2.big.pre(N2), T1s = u1.small.pre(u1.small.N), T2s = u2.small.pre(N2s);
  const int nc2 = nc * nc;
  for (i64 line = blockIdx.x; line < (i64)N0 * N1; line += gridDim.x) {
    const int X = (int)(line / N1), Y = (int)(line % N1);
    const int Xs = urep(u0, X), Ys = urep(u1, Y), l0 = u0.big.len(X), l1 = u1.big.len(Y);
    const i64 dst = (i64)nc2 * (u0.big.pre(X) * T1 * T2 + l0 * u1.big.pre(Y) * T2);
    const i64 src = (i64)nc2 * (u0.small.pre(Xs) * T1s * T2s + l0 * u1.small.pre(Ys) * T2s);
    const i64 w = (i64)nc2 * l0 * l1;  // values per unit of pre() along axis 2
    const i64 n = w * T2, ns = w * T2s;
    const i64 head = w * u2.big.pre(min(u2.H, N2));
    const i64 tail = w * (T2 - u2.big.pre(N2 - u2.TL));
    const i64 per = w * (u2.small.pre(u2.H + u2.PER) - u2.small.pre(u2.H));
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

int nh_hex1_nnz(const int *shape, int ncomp, int64_t *nnz) {
  NH_REQUIRE(shape && nnz, "nh_hex1_nnz: NULL argument");
  NH_REQUIRE(shape[0] >= 1 && shape[1] >= 1 && shape[2] >= 1 && ncomp >= 1 && ncomp <= 3, "nh_hex1_nnz: shape / ncomp");
  *nnz = (int64_t)ncomp * ncomp * Axis{shape[0] + 1}.pre(shape[0] + 1) * Axis{shape[1] + 1}.pre(shape[1] + 1) * Axis{shape[2] + 1}.pre(shape[2] + 1);
  return NH_OK;
}

int nh_hex1_pattern(const int *shape, int ncomp, int64_t *rowptr_dev, int64_t *colidx_dev, void *stream) {
  NH_REQUIRE(shape && rowptr_dev && colidx_dev, "nh_hex1_pattern: NULL argument");
  int64_t nnz;
  int rc = nh_hex1_nnz(shape, ncomp, &nnz);
  if (rc) return rc;
  const Axis a0{shape[0] + 1}, a1{shape[1] + 1}, a2{shape[2] + 1};
  const i64 nrows = (i64)a0.N * a1.N * a2.N * ncomp;
  const unsigned grid = (unsigned)std::min<i64>((nrows + 256) / 256, 256 * 64);
  hipLaunchKernelGGL(k_hex1_pattern, dim3(grid), dim3(256), 0, nh_stream(stream), a0, a1, a2, ncomp, (i64 *)rowptr_dev, (i64 *)colidx_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

int nh_hex1_matrix(const nh_hex1_args *a, void *stream) {
  NH_REQUIRE(a, "nh_hex1_matrix: NULL args");
  NH_REQUIRE(a->shape[0] >= 1 && a->shape[1] >= 1 && a->shape[2] >= 1, "nh_hex1_matrix: shape");
  NH_REQUIRE(a->ncomp >= 1 && a->ncomp <= 3, "nh_hex1_matrix: ncomp %d", a->ncomp);
  NH_REQUIRE(a->nq >= 1 && a->weights_dev && a->T_dev && a->values_dev && a->C_host, "nh_hex1_matrix: NULL argument");
  NH_REQUIRE((a->geom.kind == NH_GEOM_ISO && a->geom.verts_dev) || (a->geom.kind == NH_GEOM_BOX && a->geom.size_dev),
             "nh_hex1_matrix: geometry must be ISO (vertices) or BOX");
  NH_REQUIRE(a->geom.bnd_axis < 0, "nh_hex1_matrix: volume samples only");
  Hex1K k{};
  k.a0 = Axis{a->shape[0] + 1};
  k.a1 = Axis{a->shape[1] + 1};
  k.a2 = Axis{a->shape[2] + 1};
  k.nq = a->nq;
  k.w = a->weights_dev;
  k.gkind = a->geom.kind;
  k.verts = a->geom.verts_dev;
  k.size = a->geom.size_dev;
  k.T = a->T_dev;
  const int nc = a->ncomp;
  bool value_slot = false;
  for (int c = 0; c < nc; ++c)
    for (int s = 0; s < 4; ++s)
      for (int d = 0; d < nc; ++d)
        for (int t = 0; t < 4; ++t) {
          const double v = a->C_host[((c * 4 + s) * nc + d) * 4 + t];
          k.C[c][s][d][t] = v;
          if ((s == 0 || t == 0) && v != 0.) value_slot = true;
        }
  k.nograd = !uses_gradients(a->C_host, nc, 4, nc);
  k.values = a->values_dev;
  k.nty = (k.a1.N + HY - 1) / HY;
  k.ntz = (k.a2.N + HZ - 1) / HZ;
  k.nxc = (k.a0.N + HX - 1) / HX;
  hipStream_t s = nh_stream(stream);
  size_t ldsb = 0;
  hipError_t e;
  if (value_slot) e = nc == 1 ? launch_hex1<1, 4>(k, &ldsb, s) : nc == 2 ? launch_hex1<2, 4>(k, &ldsb, s) : launch_hex1<3, 4>(k, &ldsb, s);
  else e = nc == 1 ? launch_hex1<1, 3>(k, &ldsb, s) : nc == 2 ? launch_hex1<2, 3>(k, &ldsb, s) : launch_hex1<3, 3>(k, &ldsb, s);
  if (ldsb > 160 * 1024) {
    nh_set_error("nh_hex1_matrix: %d quadrature points need %zu bytes of LDS per workgroup (limit 160 KiB)", a->nq, ldsb);
    return NH_ELIMIT;
  }
  NH_CHECK_HIP(e);
  return NH_OK;
}

int nh_hex1_rows_uniform(const int *shape, int ncomp, const double *small_values_dev, double *values_dev, void *stream) {
  NH_REQUIRE(shape && small_values_dev && values_dev, "nh_hex1_rows_uniform: NULL argument");
  NH_REQUIRE(shape[0] >= 1 && shape[1] >= 1 && shape[2] >= 1 && ncomp >= 1 && ncomp <= 3, "nh_hex1_rows_uniform: shape / ncomp");
  const UAxis u0 = uniform_axis(shape[0]), u1 = uniform_axis(shape[1]), u2 = uniform_axis(shape[2]);
  const unsigned grid = (unsigned)std::min<i64>((i64)u0.big.N * u1.big.N, 256 * 16);
  hipLaunchKernelGGL(k_hex1_rows_uniform, dim3(grid), dim3(256), 0, nh_stream(stream), u0, u1, u2, ncomp, small_values_dev, values_dev);
  NH_LAUNCH_CHECK();
  return NH_OK;
}

}  // extern "C"
