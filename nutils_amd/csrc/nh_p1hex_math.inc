// Element math of the P1-hex Laplace fast path, textually included into each kernel that needs it (a function taking the kernel
// argument struct by reference makes hipcc 7.2 copy it to private memory and costs 36 VGPRs + scratch in the main kernel).  Straight-line
// code without hooks or switches: nh_p1hex_element.inc, k_p1hex_unit_matrix, nh_gather.hip and tools/ubench/p1hex_math.hip include it as it is.
// In scope at the include site: P1Args p; macros NH_P1HEX_QS(q), NH_P1HEX_QM(q) (diffusion / mass coefficient at Gauss point q, or 1.);
// bool hasm (uniform: mass term requested) and output double Mm[3][3][3] (mass term by pair classes); double X[2][2][2][3]; outputs double R0[3][3], R1[3][3], R2[3][3] (diagonal j == k
// terms, indexed by the pair classes p_d = a_d + b_d) and W01[2][2][3], W02[2][2][3], W12[2][2][3] (off-diagonal terms).
// Computes: Jacobian columns, metric tensors at the 8 Gauss points, axis-by-axis contractions (DESIGN.md, "P1-hex local matrix
// by sum factorisation").
// REQUIRES a 2-point rule that is symmetric about 1/2, g0 + g1 = 1 (points.gauss1(2), the only rule the callers pass): the contractions read
// n[0][0], c[0][0], c[0][1], c[1][0] and take the other table values from the symmetry.  The host guards it: fill_p1args refuses any other rule,
// fused_p1hex_tables leaves it to the general kernel.  (The mass block and the Jacobian columns hold for any 2-point rule.)
{
  // uniform tables (SGPR resident): n[a][q] = N_a(g_q), c[p][q] = n[x][q] n[y][q] with p = x + y, wk = kappa w w w
  const double (&n)[2][2] = p.n;
  const double (&c)[3][2] = p.c;
  // ---- Jacobian columns (sum-factorised: column j is independent of xi_j) --------------
  double J0[2][2][3], J1[2][2][3], J2[2][2][3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double e0[2][2], e1[2][2], e2[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        e0[x][y] = X[1][x][y][d] - X[0][x][y][d];
        e1[x][y] = X[x][1][y][d] - X[x][0][y][d];
        e2[x][y] = X[x][y][1][d] - X[x][y][0][d];
      }
    // n[0][q] + n[1][q] = 1 (linear shape functions): n0 u + n1 v = u + n1 (v - u) -- one difference and one fma per Gauss point instead of a
    // multiplication and an fma (3 instead of 4 instructions per interpolated pair, 108 instead of 144 for the twelve column vectors)
    double t0[2][2], t1[2][2], t2[2][2];  // [q1][y]
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const double d0 = e0[1][y] - e0[0][y], d1 = e1[1][y] - e1[0][y], d2 = e2[1][y] - e2[0][y];
#pragma unroll
      for (int q1 = 0; q1 < 2; ++q1) {
        t0[q1][y] = fma(n[1][q1], d0, e0[0][y]);
        t1[q1][y] = fma(n[1][q1], d1, e1[0][y]);
        t2[q1][y] = fma(n[1][q1], d2, e2[0][y]);
      }
    }
#pragma unroll
    for (int q1 = 0; q1 < 2; ++q1) {
      const double d0 = t0[q1][1] - t0[q1][0], d1 = t1[q1][1] - t1[q1][0], d2 = t2[q1][1] - t2[q1][0];
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2) {
        J0[q1][q2][d] = fma(n[1][q2], d0, t0[q1][0]);  // (beta, gamma)
        J1[q1][q2][d] = fma(n[1][q2], d1, t1[q1][0]);  // (alpha, gamma)
        J2[q1][q2][d] = fma(n[1][q2], d2, t2[q1][0]);  // (alpha, beta)
      }
    }
  }
  // ---- metric tensors M_q = kappa w_q / |det J_q| adj(J_q) adj(J_q)^T at the 8 Gauss points --------
  // K[a][b] = sum_q sum_jk T_q[a][j] T_q[b][k] M_q[j][k]; the reference gradients T factor per axis
  // (T_q[a][j] = prod_d (d == j ? sigma(a_d) : n[a_d][q_d])), so the q-sum is contracted axis by axis
  // (sum factorisation) instead of forming the 8 x 3 physical gradients per point.
  double D0[2][2], D1[2][2], D2[2][2], M01[2][2][2], M02[2][2][2], M12[2][2][2], Dm[2][2][2];
#pragma unroll
  for (int qa = 0; qa < 2; ++qa)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int qc = 0; qc < 2; ++qc) {
        const double *c0 = J0[qb][qc], *c1 = J1[qa][qc], *c2 = J2[qa][qb];
        double A[3][3];  // rows of adj(J): A[j] = c_{j+1} x c_{j+2}
        A[0][0] = c1[1] * c2[2] - c1[2] * c2[1];
        A[0][1] = c1[2] * c2[0] - c1[0] * c2[2];
        A[0][2] = c1[0] * c2[1] - c1[1] * c2[0];
        A[1][0] = c2[1] * c0[2] - c2[2] * c0[1];
        A[1][1] = c2[2] * c0[0] - c2[0] * c0[2];
        A[1][2] = c2[0] * c0[1] - c2[1] * c0[0];
        A[2][0] = c0[1] * c1[2] - c0[2] * c1[1];
        A[2][1] = c0[2] * c1[0] - c0[0] * c1[2];
        A[2][2] = c0[0] * c1[1] - c0[1] * c1[0];
        const double det = c0[0] * A[0][0] + c0[1] * A[0][1] + c0[2] * A[0][2];
        const double sc = p.wk[qa][qb][qc] * NH_P1HEX_QS(qa * 4 + qb * 2 + qc) * fast_rcp(fabs(det));
        const double m00 = sc * (A[0][0] * A[0][0] + A[0][1] * A[0][1] + A[0][2] * A[0][2]);
        const double m11 = sc * (A[1][0] * A[1][0] + A[1][1] * A[1][1] + A[1][2] * A[1][2]);
        const double m22 = sc * (A[2][0] * A[2][0] + A[2][1] * A[2][1] + A[2][2] * A[2][2]);
        M01[qa][qb][qc] = sc * (A[0][0] * A[1][0] + A[0][1] * A[1][1] + A[0][2] * A[1][2]);
        M02[qa][qb][qc] = sc * (A[0][0] * A[2][0] + A[0][1] * A[2][1] + A[0][2] * A[2][2]);
        M12[qa][qb][qc] = sc * (A[1][0] * A[2][0] + A[1][1] * A[2][1] + A[1][2] * A[2][2]);
        D0[qb][qc] = qa ? D0[qb][qc] + m00 : m00;
        D1[qa][qc] = qb ? D1[qa][qc] + m11 : m11;
        D2[qa][qb] = qc ? D2[qa][qb] + m22 : m22;
        if (hasm) Dm[qa][qb][qc] = p.wm[qa][qb][qc] * NH_P1HEX_QM(qa * 4 + qb * 2 + qc) * fabs(det);
      }
  // ---- axis-by-axis contractions -------------------------------------------------------------------
  // The rule is symmetric about 1/2 (g0 + g1 = 1), so with al = n[0][0]: n[1][1] = al, n[0][1] = n[1][0] = 1 - al, and c[1][0] = c[1][1],
  // c[2][0] = c[0][1], c[2][1] = c[0][0].  A 2 -> 2 interpolation stage is then a difference and two fma (3 instead of 4 instructions):
  //   n[0][0] u0 + n[0][1] u1 = u1 + al (u0 - u1),   n[1][0] u0 + n[1][1] u1 = u0 - al (u0 - u1)
  // and a 2 -> 3 pair-class stage takes 5 instead of 6: the middle class has one coefficient, the last is the first with x and y swapped:
  //   out0 = c00 x + c01 y,   out1 = c10 (x + y),   out2 = c01 x + c00 y = (c00 + c01) (x + y) - out0
  const double al = n[0][0], nal = -al, c00 = c[0][0], c01 = c[0][1], c10 = c[1][0], cs = c00 + c01;
#define NH_P1HEX_LERP(o0, o1, u0, u1) \
  {                                   \
    const double d_ = (u0) - (u1);    \
    o0 = fma(al, d_, u1);             \
    o1 = fma(nal, d_, u0);            \
  }
#define NH_P1HEX_PAIR(o0, o1, o2, x, y) \
  {                                     \
    const double s_ = (x) + (y);        \
    o0 = fma(c00, x, c01 * (y));        \
    o1 = c10 * s_;                      \
    o2 = fma(cs, s_, -(o0));            \
  }
  {
    double U[2][3];
#pragma unroll
    for (int x = 0; x < 2; ++x) NH_P1HEX_PAIR(U[x][0], U[x][1], U[x][2], D0[x][0], D0[x][1])
#pragma unroll
    for (int p2 = 0; p2 < 3; ++p2) NH_P1HEX_PAIR(R0[0][p2], R0[1][p2], R0[2][p2], U[0][p2], U[1][p2])
#pragma unroll
    for (int x = 0; x < 2; ++x) NH_P1HEX_PAIR(U[x][0], U[x][1], U[x][2], D1[x][0], D1[x][1])
#pragma unroll
    for (int p2 = 0; p2 < 3; ++p2) NH_P1HEX_PAIR(R1[0][p2], R1[1][p2], R1[2][p2], U[0][p2], U[1][p2])
#pragma unroll
    for (int x = 0; x < 2; ++x) NH_P1HEX_PAIR(U[x][0], U[x][1], U[x][2], D2[x][0], D2[x][1])
#pragma unroll
    for (int p1 = 0; p1 < 3; ++p1) NH_P1HEX_PAIR(R2[0][p1], R2[1][p1], R2[2][p1], U[0][p1], U[1][p1])
  }
  {
    // W01[b0][a1][p2] = sum_ga c[p2][ga] sum_be n[a1][be] sum_al n[b0][al] M01[al][be][ga]   (two-term axes first: 12+12+20 ops)
    double V[2][2][2], V2[2][2][2];
#pragma unroll
    for (int be = 0; be < 2; ++be)
#pragma unroll
      for (int ga = 0; ga < 2; ++ga) NH_P1HEX_LERP(V[0][be][ga], V[1][be][ga], M01[0][be][ga], M01[1][be][ga])
#pragma unroll
    for (int b0 = 0; b0 < 2; ++b0)
#pragma unroll
      for (int ga = 0; ga < 2; ++ga) NH_P1HEX_LERP(V2[b0][0][ga], V2[b0][1][ga], V[b0][0][ga], V[b0][1][ga])
#pragma unroll
    for (int b0 = 0; b0 < 2; ++b0)
#pragma unroll
      for (int a1 = 0; a1 < 2; ++a1) NH_P1HEX_PAIR(W01[b0][a1][0], W01[b0][a1][1], W01[b0][a1][2], V2[b0][a1][0], V2[b0][a1][1])
    // W02[b0][a2][p1] = sum_be c[p1][be] sum_ga n[a2][ga] sum_al n[b0][al] M02[al][be][ga]
#pragma unroll
    for (int be = 0; be < 2; ++be)
#pragma unroll
      for (int ga = 0; ga < 2; ++ga) NH_P1HEX_LERP(V[0][be][ga], V[1][be][ga], M02[0][be][ga], M02[1][be][ga])
#pragma unroll
    for (int b0 = 0; b0 < 2; ++b0)
#pragma unroll
      for (int be = 0; be < 2; ++be) NH_P1HEX_LERP(V2[b0][0][be], V2[b0][1][be], V[b0][be][0], V[b0][be][1])
#pragma unroll
    for (int b0 = 0; b0 < 2; ++b0)
#pragma unroll
      for (int a2 = 0; a2 < 2; ++a2) NH_P1HEX_PAIR(W02[b0][a2][0], W02[b0][a2][1], W02[b0][a2][2], V2[b0][a2][0], V2[b0][a2][1])
    // W12[b1][a2][p0] = sum_al c[p0][al] sum_ga n[a2][ga] sum_be n[b1][be] M12[al][be][ga]
#pragma unroll
    for (int al_ = 0; al_ < 2; ++al_)
#pragma unroll
      for (int ga = 0; ga < 2; ++ga) NH_P1HEX_LERP(V[0][al_][ga], V[1][al_][ga], M12[al_][0][ga], M12[al_][1][ga])
#pragma unroll
    for (int b1 = 0; b1 < 2; ++b1)
#pragma unroll
      for (int al_ = 0; al_ < 2; ++al_) NH_P1HEX_LERP(V2[b1][0][al_], V2[b1][1][al_], V[b1][al_][0], V[b1][al_][1])
#pragma unroll
    for (int b1 = 0; b1 < 2; ++b1)
#pragma unroll
      for (int a2 = 0; a2 < 2; ++a2) NH_P1HEX_PAIR(W12[b1][a2][0], W12[b1][a2][1], W12[b1][a2][2], V2[b1][a2][0], V2[b1][a2][1])
  }
#undef NH_P1HEX_LERP
#undef NH_P1HEX_PAIR
  if (hasm) {
    // mass term: M[a][b] = sum_q w_q |det J_q| N_a N_b = Mm[a0+b0][a1+b1][a2+b2], contracted axis by axis with c[p][q] = n[x][q] n[y][q]
    double t1[2][2][3], t2[2][3][3];
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int p2 = 0; p2 < 3; ++p2) t1[qa][qb][p2] = c[p2][0] * Dm[qa][qb][0] + c[p2][1] * Dm[qa][qb][1];
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
      for (int p1 = 0; p1 < 3; ++p1)
#pragma unroll
        for (int p2 = 0; p2 < 3; ++p2) t2[qa][p1][p2] = c[p1][0] * t1[qa][0][p2] + c[p1][1] * t1[qa][1][p2];
#pragma unroll
    for (int p0 = 0; p0 < 3; ++p0)
#pragma unroll
      for (int p1 = 0; p1 < 3; ++p1)
#pragma unroll
        for (int p2 = 0; p2 < 3; ++p2) Mm[p0][p1][p2] = c[p0][0] * t2[0][p1][p2] + c[p0][1] * t2[1][p1][p2];
  }
}
