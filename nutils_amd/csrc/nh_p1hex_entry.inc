// The 36 entries a <= b of the P1-hex local matrix from the tables of nh_p1hex_math.inc, textually included after it (nh_p1hex_element.inc,
// k_fused_p1hex).  In scope: R0, R1, R2, W01, W02, W12, Mm and bool hasm.  Declares the lambda entry(a, bb).
// Nine signed table values each (+ the mass term), summed as (kd + t01) + (t02 + t12): the three diagonal terms, then one pair per off-diagonal
// table.  The two operands of a pair stand in the order of their table index, so entries that need the same pair with the same signs spell
// the same expression and the compiler keeps one of them (without fast-math it cannot reassociate a left-to-right sum to find them).
        auto entry = [&](int a, int bb) {
          const int a0 = a >> 2, a1 = (a >> 1) & 1, a2 = a & 1;
          const int b0 = bb >> 2, b1 = (bb >> 1) & 1, b2 = bb & 1;
          const int p0 = a0 + b0, p1 = a1 + b1, p2 = a2 + b2;
          const double s00 = (a0 == b0) ? 1. : -1., s11 = (a1 == b1) ? 1. : -1., s22 = (a2 == b2) ? 1. : -1.;
          const double s01 = (a0 == b1) ? 1. : -1., s10 = (b0 == a1) ? 1. : -1.;
          const double s02 = (a0 == b2) ? 1. : -1., s20 = (b0 == a2) ? 1. : -1.;
          const double s12 = (a1 == b2) ? 1. : -1., s21 = (b1 == a2) ? 1. : -1.;
          // s * W[x][y][pp] + t * W[u][v][pp], the operand with the smaller index 2 x + y first
          auto pair = [&](const double (&W)[2][2][3], double s, int x, int y, double t, int u, int v, int pp) {
            return 2 * x + y <= 2 * u + v ? s * W[x][y][pp] + t * W[u][v][pp] : t * W[u][v][pp] + s * W[x][y][pp];
          };
          const double kd = (s00 * R0[p1][p2] + s11 * R1[p0][p2]) + s22 * R2[p0][p1];
          const double t01 = pair(W01, s01, b0, a1, s10, a0, b1, p2);
          const double t02 = pair(W02, s02, b0, a2, s20, a0, b2, p1);
          const double t12 = pair(W12, s12, b1, a2, s21, a1, b2, p0);
          double k = (kd + t01) + (t02 + t12);
          if (hasm) k += Mm[p0][p1][p2];
          return k;
        };
