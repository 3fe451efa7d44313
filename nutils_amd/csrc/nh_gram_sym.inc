// Symmetric scalar and two-component blocks with a constant form, local matrices to the gather scratch (NH_MATRIX_GATHER): the element kernel of the ragged rational workloads
// (BASELINE.json configs[4]: p = 3 hierarchical NURBS, 16-24 functions per element, plane elasticity).  Included by nh_assemble_generic.hip (anonymous namespace).
//
// What the reference computes per element is `einsum` of the weighted gradient tables with the form (evaluable.py:1885-1886) followed by the scatter of
// numeric.py:434-460.  Here, per element:  G_mn[a][b] = sum_q w_q |J_q| D[q][m][a] D[q][n][b]  (Gram sums over the points, independent of the components) and
// K_mn[c][d] = sum_ab C[c][a][d][b] G_mn[a][b], for the node pairs m >= n only; K_nm = K_mn^T is written beside it.
//
// k_matrix_generic's branch for this case spends ~5 900 wave instructions per element (profiles/r06_c5_gram.md): 2 850 in the point loop -- 14 LDS reads + 6 multiplies + 18
// multiply-adds per point for TWO node pairs of a lane, the second round of an element's 150 lane items 17 % full -- and ~3 000 around it (run-time divisions, a
// double-precision square root per item, the form tensor read from LDS per use, run-time component loops).  This kernel:
//   * a lane owns a 2 x 2 BLOCK of node pairs (nodes 2I, 2I+1 against 2J, 2J+1, I >= J).  The table is kept slot-major, D[q][a][m]: the two nodes of a lane are ONE 16-byte
//     LDS read per slot, consecutive lanes read consecutive 16-byte words (no bank conflicts; the node-major layout of the first version lost 58 % of its LDS cycles to them):
//     6 reads feed 36 multiply-adds per point;
//   * E elements share a workgroup of W waves and their blocks are dealt to the lanes TOGETHER (36-78 blocks per element: one element fills 56-61 % of a wave or two,
//     three elements of 24 functions fill 91 % of four waves);
//   * NC, S and the form tensor are compile-time / scalar-register operands; the block index is decoded once per lane with single-precision arithmetic;
//   * an element's table T[nb][nq][S] is one contiguous array: loaded with consecutive lanes on consecutive addresses, one batch AHEAD into registers (the tables in LDS
//     limit a CU to two waves per SIMD, so memory latency is covered inside the wave);
//   * the blocks of a batch are STORED after the next batch's table has gone to LDS: vector-memory operations retire in order, so a wave that waits for its table loads also
//     waits for every store before them -- deferred, the stores drain under the next batch's point loop instead of in front of it.
//   * gradient-only forms (USE0 = false) never form the value slot: 16 instead of 36 multiply-adds per block and point, table rows of two slots;
//   * TRI (MatK::sym == 3, the default where the whole assembly qualifies): the nodes of an element are taken in the order of their dofs and only the pairs m' >= n' are
//     written, packed -- the lower triangle of the symmetric global matrix is gathered from them, the upper one mirrored (nh_gather.hip: k_gather_values_2x2_tri, k_mirror_2x2).
// Sums run over the points in ascending order per entry, like the generic branch.  With the full scratch the results are bit-identical to it (the blocking changes which lane
// forms a sum, not the sum); with the triangular scratch a pair whose dof order differs from its local order is formed with test and trial roles swapped (products associate
// differently in the last bit) and the matrix comes out symmetric entry by entry (but for the two off-diagonal entries of a diagonal node block, which are formed apart) -- deterministic either way, parity 1e-13 against the reference's fixtures.
#ifndef NH_GS_UNROLL
#define NH_GS_UNROLL 5
#endif
#ifndef NH_GS_QPAD
#define NH_GS_QPAD 2  // doubles between the table rows of consecutive points (0: rounds 6's first layout)
#endif
#ifndef NH_GS_WPE
#define NH_GS_WPE 2  // waves per SIMD the register allocation of the gradient-only variant aims at (3: <= 168 registers)
#endif
template <int ND, int NC, int E, int W, bool USE0, bool TRI>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(USE0 ? 2 : NH_GS_WPE, 4))) void k_gram_sym(MatK p, FormK form) {
  constexpr int S = 1 + ND, JW = ND * ND + 1, A0 = USE0 ? 0 : 1;  // A0: first operator slot the form uses (pure gradient forms -- elasticity, Laplace -- never touch the value slot)
  static_assert((NC == 1 || NC == 2) && E <= W, "one or two components; a wave stages one element");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;  // (the wave index in a scalar register: what hangs off it -- element, offsets, table address -- follows)
  const int nq = p.nq, mp = (p.maxnbt + 1) & ~1;      // nodes padded to pairs
  constexpr int SS = S - A0;                          // slots kept in LDS
  // (stride of a point in the table: SS mp doubles + NH_GS_QPAD -- with SS mp = 48 the lanes of the staging phase, consecutive points of a function, met in TWO banks:
  // SQ_LDS_BANK_CONFLICT was 52 M cycles per launch beside 60 M of LDS activity, profiles/r06_c5_gram.md; + 2 keeps the 16-byte alignment of the node pairs)
  const int qs = SS * mp + NH_GS_QPAD, dsz = nq * qs, jsz = (nq * JW + 1) & ~1;
  double *Dall = lds;                                 // [E][nq][SS][mp]
  double *Jall = lds + E * dsz;                       // [E][nq][JW]
  int *meta = reinterpret_cast<int *>(Jall + E * jsz);  // [E]: nb
  int *rkl = meta + E + (E & 1);                        // TRI: [E][64] position of a node among the dofs of its element
  i64 *kbl = reinterpret_cast<i64 *>(rkl + 64 * E);     // [E] first scratch position of the element
  const float rnq = 1.f / (float)nq;
  const i64 nbatch = (p.nelems + E - 1) / E;
  constexpr int R = 10;  // 64 R >= nb nq (checked by the launcher)
  double tt[R][S], gJ[ND][ND], gw = 0.;
  int rk = 0;
  i64 e = 0, ie = 0;
  int nb = 0;
  bool live = false;
  // Element ids and table offsets are fetched AHEAD of the batch that needs them (elist -> off -> table address is a chain of dependent loads, each a memory latency
  // that two waves per SIMD cannot hide: 140 of the kernel's 410 us before this pipeline, profiles/r06_c5_gram.md): ids three batches ahead, offsets two.
  i64 eA = 0, eB = 0;        // ids of the batches issue() will take next (eA) and after that (eB)
  i64 oA0 = 0, oA1 = 0;      // off[eA], off[eA + 1]
  i64 kb = 0;                // first scratch position of the element in the registers
  auto elem_id = [&](i64 ib) -> i64 {
    const i64 j = ib * E + wave;
    return (wave < E && ib < nbatch && j < p.nelems) ? (p.elist ? p.elist[j] : j) : 0;
  };
  auto elem_off = [&](i64 ee, i64 &o0, i64 &o1) {
    if (p.test.off) o0 = p.test.off[ee], o1 = p.test.off[ee + 1];
    else o0 = ee * (i64)p.test.nb, o1 = o0 + p.test.nb;
  };
  auto issue = [&](i64 ib) {  // wave w < E loads element w of batch ib: its table (R rounds of 64 lanes x S doubles) and its geometry at the points, into registers
    ie = ib * E + wave;
    live = wave < E && ib < nbatch && ie < p.nelems;
    e = live ? eA : 0;
    nb = live ? (int)(oA1 - oA0) : 0;
    const i64 fn0 = p.test.off ? oA0 : (p.test.tab ? (i64)p.test.tab[e] * p.test.nb : 0), t0 = oA0;
    // advance the pipeline: the offsets of the batch after this one, the id of the one after that
    eA = eB;
    elem_off(eA, oA0, oA1);
    eB = elem_id(ib + 2 * (i64)gridDim.x);
    const double *T = p.test.T + fn0 * (i64)nq * S;  // [m][q][S], contiguous for the element
    const int n = nb * nq;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int t = lane + 64 * r;
#pragma unroll
      for (int i = A0; i < S; ++i) tt[r][i] = t < n ? T[(i64)t * S + i] : 0.;
    }
    if (live && lane < nq) {
      double det;
      geometry_at<ND>(p.geom, e, lane, nq, nullptr, gJ, det, nullptr);
      gw = p.weights[lane] * fabs(det) * (p.scale ? p.scale[(p.emap_by_elem ? e : ie) * nq + lane] : 1.);
    }
    if (TRI) rk = lane < nb ? p.trirank[t0 + lane] : 0;
    kb = TRI ? p.tribase[e] : p.eoff ? p.eoff[e] : (p.emap_by_elem ? e : ie) * (i64)nb * nb;
  };
  auto stage = [&]() {  // registers -> LDS: inverse Jacobians and weights, then the table turned into physical gradients, slot-major
    if (wave >= E) return;
    double *D = Dall + wave * dsz, *Jw = Jall + wave * jsz;
    if (live && lane < nq) {
#pragma unroll
      for (int j = 0; j < ND; ++j)
#pragma unroll
        for (int i = 0; i < ND; ++i) Jw[lane * JW + j * ND + i] = gJ[j][i];
      Jw[lane * JW + ND * ND] = gw;
    }
    if (lane == 0) meta[wave] = nb, kbl[wave] = kb;
    if (TRI) rkl[wave * 64 + lane] = rk;
    __builtin_amdgcn_wave_barrier();  // (a wave reads only the Jw rows / ranks it wrote itself: LDS operations of one wave execute in order)
    const int n = nb * nq;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int t = lane + 64 * r;
      if (t < n) {
        int m = (int)(((float)t + .5f) * rnq);
        int q = t - m * nq;
        if (q < 0) --m, q += nq;       // (the reciprocal may be off by one ulp at a multiple of nq)
        if (q >= nq) ++m, q -= nq;
        if (TRI) m = rkl[wave * 64 + m];  // the table in the order of the element's dofs
        const double *Ji = Jw + q * JW;
        double *dst = D + q * qs + m;
        if (USE0) dst[0] = tt[r][0];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
          double sm = 0;
#pragma unroll
          for (int j = 0; j < ND; ++j) sm += tt[r][1 + j] * Ji[j * ND + i];
          dst[(1 + i - A0) * mp] = sm;
        }
      }
    }
    if ((nb & 1) && lane < nq) {  // (odd nb: the partner of the last node is read, never written out: zero, not whatever the slot held)
#pragma unroll
      for (int a = A0; a < S; ++a) D[lane * qs + (a - A0) * mp + nb] = 0.;
    }
  };
  // results of a lane's block, kept until the next batch's table is in LDS
  double K[2][2][2][2];  // ([NC][NC] used)
  i64 kbase = 0;
  int km0 = 0, kn0 = 0, knb = -1, kflags = 0;  // knb < 0: nothing to store
  auto flush = [&]() {
    if (knb < 0) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!((kflags >> (2 * i + j)) & 1)) continue;
        const int m = km0 + i, n = kn0 + j;
        if constexpr (NC == 1) {  // scalar blocks: one value per node pair
          if (TRI) {
            p.local[kbase + m * (m + 1) / 2 + n] = K[i][j][0][0];
          } else {
            p.local[kbase + (i64)m * knb + n] = K[i][j][0][0];
            if (m != n) p.local[kbase + (i64)n * knb + m] = K[i][j][0][0];
          }
          continue;
        } else
        if (TRI) {  // packed lower triangle of the dof-sorted nodes: the pair itself, nothing mirrored
          double *dt = p.local + (kbase + m * (m + 1) / 2 + n) * (NC * NC);
          *reinterpret_cast<double2 *>(dt) = double2{K[i][j][0][0], K[i][j][0][1]};
          *reinterpret_cast<double2 *>(dt + 2) = double2{K[i][j][1][0], K[i][j][1][1]};
          continue;
        }
        double *dst = p.local + (kbase + (i64)m * knb + n) * (NC * NC);
        double *dst2 = p.local + (kbase + (i64)n * knb + m) * (NC * NC);
        if (form.mask[0][0] && form.mask[0][1] && form.mask[1][0] && form.mask[1][1]) {  // (all component blocks present: 16-byte stores)
          *reinterpret_cast<double2 *>(dst) = double2{K[i][j][0][0], K[i][j][0][1]};
          *reinterpret_cast<double2 *>(dst + 2) = double2{K[i][j][1][0], K[i][j][1][1]};
          if (m != n) {
            *reinterpret_cast<double2 *>(dst2) = double2{K[i][j][0][0], K[i][j][1][0]};
            *reinterpret_cast<double2 *>(dst2 + 2) = double2{K[i][j][0][1], K[i][j][1][1]};
          }
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int d = 0; d < NC; ++d) {
              if (!form.mask[c][d]) continue;
              dst[c * NC + d] = K[i][j][c][d];
              if (m != n) dst2[d * NC + c] = K[i][j][c][d];
            }
        }
      }
    knb = -1;
  };
  eA = elem_id(blockIdx.x);
  elem_off(eA, oA0, oA1);
  eB = elem_id(blockIdx.x + gridDim.x);
  issue(blockIdx.x);
  stage();
  __syncthreads();
  issue(blockIdx.x + gridDim.x);
  for (i64 ib = blockIdx.x; ib < nbatch; ib += gridDim.x) {
    // ---- the 2 x 2 blocks of the E elements in LDS, dealt to the lanes (one block per lane: the launcher checks that they fit) ----
    int cnt[E + 1];
    cnt[0] = 0;
#pragma unroll
    for (int s = 0; s < E; ++s) {
      const int P = (meta[s] + 1) >> 1;
      cnt[s + 1] = cnt[s] + P * (P + 1) / 2;
    }
    const int k = tid;
    if (k < cnt[E]) {
      int s = 0, base = 0;
#pragma unroll
      for (int j = 1; j < E; ++j) {
        const bool past = k >= cnt[j];
        s += past;
        base = past ? cnt[j] : base;
      }
      const int kl = k - base;
      int I = (int)((__builtin_sqrtf(8.f * (float)kl + 1.f) - 1.f) * .5f);  // kl = I (I + 1) / 2 + J, 0 <= J <= I
      I += (I + 1) * (I + 2) / 2 <= kl;
      I -= I * (I + 1) / 2 > kl;
      const int J = kl - I * (I + 1) / 2;
      const int nbs = meta[s];
      const int m0 = 2 * I, n0 = 2 * J;
      const bool hm = m0 + 1 < nbs, hn = n0 + 1 < nbs;  // (odd nb: the last node has no partner)
      const double *Ds = Dall + s * dsz, *Js = Jall + s * jsz;
      double G[2][2][S][S];  // (slots below A0 are never formed: their coefficients are zero)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int a = A0; a < S; ++a)
#pragma unroll
            for (int b = A0; b < S; ++b) G[i][j][a][b] = 0.;
      for (int q = 0; q < nq; ++q) {
        const double *Dq = Ds + q * qs;
        const double wq = Js[q * JW + ND * ND];
        double2 rm[S], rn[S];
#pragma unroll
        for (int a = A0; a < S; ++a) rm[a] = *reinterpret_cast<const double2 *>(Dq + (a - A0) * mp + m0), rn[a] = *reinterpret_cast<const double2 *>(Dq + (a - A0) * mp + n0);
#pragma unroll
        for (int a = A0; a < S; ++a) {
          const double w0 = wq * rm[a].x, w1 = wq * rm[a].y;
#pragma unroll
          for (int b = A0; b < S; ++b) {
            G[0][0][a][b] += w0 * rn[b].x;
            G[0][1][a][b] += w0 * rn[b].y;
            G[1][0][a][b] += w1 * rn[b].x;
            G[1][1][a][b] += w1 * rn[b].y;
          }
        }
      }
      // form tensor once per node pair; the blocks wait in registers (flush)
      kbase = kbl[s];
      km0 = m0, kn0 = n0, knb = nbs, kflags = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bool valid = !((i && !hm) || (j && !hn) || m0 + i < n0 + j);  // (diagonal blocks: the pair (m0, n1) is the mirror of (m1, n0))
          kflags |= (int)valid << (2 * i + j);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int d = 0; d < NC; ++d) {
              double acc = 0;  // (the skipped slots would add +-0: the sum is the generic branch's, bit for bit)
#pragma unroll
              for (int a = A0; a < S; ++a)
#pragma unroll
                for (int b = A0; b < S; ++b) acc += form.C[((c * S + a) * NC + d) * S + b] * G[i][j][a][b];
              K[i][j][c][d] = acc;
            }
        }
    }
    __syncthreads();  // every lane is done with the tables of this batch
    stage();          // the next batch's table (loaded during the point loop) to LDS
    issue(ib + 2 * gridDim.x);  // (loads BEFORE the stores: memory operations retire in order, loads queued behind 38 kB of stores would wait for their drain)
    flush();          // this batch's blocks to the scratch: they drain during the next point loop
    __syncthreads();
  }
}

// Does k_gram_sym take a launch with these maxima?  -> (elements, waves) per workgroup, or E = 0.  Conditions: NH_MATRIX_GATHER scratch, symmetric block (test == trial tables
// and dofs, symmetric form), constant form, two dimensions, 2 components, all points of an element in LDS, one 2 x 2 block per lane.
struct GramShape {
  int E, W;
  bool use0;
  size_t lds;
};
static GramShape nh_gram_sym_shape(const MatK &q, const FormK &form, int ndims) {
  GramShape g{0, 0, false, 0};
  const int off = getenv("NUTILS_AMD_NO_GRAM_SYM") ? atoi(getenv("NUTILS_AMD_NO_GRAM_SYM")) : 0;  // (read per call: tests switch it)
  if (off || !q.local || !q.sym || q.cq || ndims != 2 || form.nct != form.ncr || form.nct > 2 || q.maxnbt != q.maxnbr || q.maxnbt < 2 || q.maxnbt > 64) return g;
  const int NCf = form.nct;
  const int JW = ndims * ndims + 1, S = 1 + ndims, mp = (q.maxnbt + 1) & ~1, P = mp / 2, B = P * (P + 1) / 2;  // B: blocks of the largest element of this launch
  if (q.nq > 64 || q.nq * q.maxnbt > 640 || B > 256) return g;  // (large tables: the generic kernel chunks the points)
  // (elements, waves) per workgroup: the fullest lanes among the instantiated shapes
  static const int shapes[][2] = {{4, 4}, {3, 4}, {2, 4}, {1, 4}};
#ifdef NH_ABLATION
  static const int force = getenv("NUTILS_AMD_GRAM_SYM_SHAPE") ? atoi(getenv("NUTILS_AMD_GRAM_SYM_SHAPE")) : 0;  // e.g. 34: three elements on four waves
#else
  constexpr int force = 0;
#endif
  double best = 0;
  for (auto &sh : shapes) {
    if (sh[0] * B > 64 * sh[1] || (force && force != sh[0] * 10 + sh[1])) continue;
    const double fill = (double)sh[0] * B / (64. * sh[1]);
    if (fill > best + 1e-9) best = fill, g.E = sh[0], g.W = sh[1];
  }
  if (!g.E) return g;
  for (int c = 0; c < NCf; ++c)  // does the form touch the value slot of either side?
    for (int d = 0; d < NCf; ++d)
      for (int a = 0; a < S; ++a) g.use0 = g.use0 || form.C[((c * S + 0) * NCf + d) * S + a] != 0. || form.C[((c * S + a) * NCf + d) * S + 0] != 0.;
  g.lds = sizeof(double) * (size_t)g.E * ((size_t)q.nq * ((g.use0 ? S : S - 1) * mp + NH_GS_QPAD) + (((size_t)q.nq * JW + 1) & ~(size_t)1)) + sizeof(int) * (size_t)(g.E + (g.E & 1) + 64 * g.E) + sizeof(i64) * (size_t)g.E;
  if (g.lds > 64 * 1024) g.E = 0;
  return g;
}
static bool nh_gram_sym_applies(const MatK &q, const FormK &form, int ndims) { return nh_gram_sym_shape(q, form, ndims).E > 0; }

// -> *done: the launch was taken by k_gram_sym (q.sym == 3: triangular scratch -- the caller has checked that EVERY launch of the assembly is taken)
static int nh_gram_sym_launch(const MatK &q, const FormK &form, int ndims, bool *done, hipStream_t s) {
  *done = false;
  const GramShape g = nh_gram_sym_shape(q, form, ndims);
  if (!g.E) {
    NH_REQUIRE(q.sym != 3, "k_gram_sym: a launch of a triangular-scratch assembly does not fit the kernel");
    return NH_OK;
  }
  const int E = g.E, W = g.W;
  const size_t lds = g.lds;
  const i64 nbatch = (q.nelems + E - 1) / E;
  dim3 grid((unsigned)std::min<i64>(nbatch, 256 * 8)), block(64 * W);
#define LAUNCHG2(NCC, EE, WW, U0, TR)                                                                                                              \
  do {                                                                                                                                             \
    NH_CHECK_HIP(hipFuncSetAttribute((const void *)k_gram_sym<2, NCC, EE, WW, U0, TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));     \
    hipLaunchKernelGGL((k_gram_sym<2, NCC, EE, WW, U0, TR>), grid, block, lds, s, q, form);                                                        \
  } while (0)
#define LAUNCHG1(EE, WW, U0, TR)               \
  do {                                         \
    if (form.nct == 1) LAUNCHG2(1, EE, WW, U0, TR); \
    else LAUNCHG2(2, EE, WW, U0, TR);          \
  } while (0)
#define LAUNCHG(EE, WW)                                   \
  do {                                                    \
    if (g.use0 && q.sym == 3) LAUNCHG1(EE, WW, true, true);   \
    else if (g.use0) LAUNCHG1(EE, WW, true, false);       \
    else if (q.sym == 3) LAUNCHG1(EE, WW, false, true);   \
    else LAUNCHG1(EE, WW, false, false);                  \
  } while (0)
  switch (E * 10 + W) {
    case 44: LAUNCHG(4, 4); break;
    case 34: LAUNCHG(3, 4); break;
    case 24: LAUNCHG(2, 4); break;
    case 14: LAUNCHG(1, 4); break;
    default: return NH_OK;
  }
#undef LAUNCHG
#undef LAUNCHG1
#undef LAUNCHG2
  record_launch(GFAM_GRAM_SYM, GREC_GRAM_SYM, {E, W, form.nct, (int)g.use0, (int)(q.sym == 3)});
  NH_LAUNCH_CHECK();
  *done = true;
  return NH_OK;
}
