// Element phase of the marching kernels, textually included (one thread = one element): vertex coordinates from the staged tile,
// the element routine, and the reduction of the 36 upper-triangle entries (VEC: of the 8 values of K_e u_e) into the LDS rows of
// the element's 8 vertices.  In scope: P1Args p; acc, slot_of; element (gi, gj, gk), its position (ej, ek) in the tile; constants VK,
// NS, VW, VEC, MASS, COEF; macro NH_P1HEX_VERT(a, bb, c) = pointer to the staged data of local vertex (a, bb, c).
// Declares X (vertex coordinates) and the macros NH_P1HEX_ELEM (global element index) and NH_P1HEX_SLOT (LDS address of an entry), the macros
// for its own use only: both kernels that include it (k_p1hex_march, k_p1hex_skew) run it unchanged.
        double X[2][2][2][3];
        double un[8];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const double *src = NH_P1HEX_VERT(a, bb, c);
              X[a][bb][c][0] = src[0];
              X[a][bb][c][1] = src[1];
              X[a][bb][c][2] = src[2];
              un[a * 4 + bb * 2 + c] = VEC ? src[VW - 1] : 0.;
            }
#define NH_P1HEX_ELEM (((i64)gi * p.n1 + gj) * p.n2 + gk)
        double qs[8];  // coefficient at the Gauss points (1 without a coefficient array)
#pragma unroll
        for (int q = 0; q < 8; ++q) qs[q] = 1.;
        // (COEF is a separate instantiation: a conditional global load here makes the compiler wait for ALL outstanding vector memory
        // operations -- the vertex prefetch just issued, the stores of the last flush -- at the first use, also when it is not taken)
        if (COEF && p.qscale) {
          const double *src = p.qscale + NH_P1HEX_ELEM * 8;
#pragma unroll
          for (int q = 0; q < 8; ++q) qs[q] = src[q];
        }
        constexpr bool hasm = MASS;  // separate instantiation: the mass tables would cost the stiffness-only kernel 70 VGPRs (spills)
        double qm[8];  // mass coefficient at the Gauss points
#pragma unroll
        for (int q = 0; q < 8; ++q) qm[q] = 1.;
        if (MASS && COEF && p.qmass) {
          const double *src = p.qmass + NH_P1HEX_ELEM * 8;
#pragma unroll
          for (int q = 0; q < 8; ++q) qm[q] = src[q];
        }
        double *const pl[2] = {acc + slot_of(gi) + (ej * VK + ek) * NS, acc + slot_of(gi + 1) + (ej * VK + ek) * NS};
#define NH_P1HEX_SLOT(a0, a1, a2, b0, b1, b2) (pl[a0] + ((a1) * VK + (a2)) * NS + ((b0) - (a0)) * 9 + ((b1) - (a1)) * 3 + ((b2) - (a2)))
        if constexpr (VEC) {
          double r[8];
#define NH_P1HEX_QS(q) qs[q]
#define NH_P1HEX_QM(q) qm[q]
#include "nh_p1hex_apply.inc"
#undef NH_P1HEX_QS
#undef NH_P1HEX_QM
#pragma unroll
          for (int a = 0; a < 8; ++a) atomicAdd(NH_P1HEX_SLOT(a >> 2, (a >> 1) & 1, a & 1, a >> 2, (a >> 1) & 1, a & 1), r[a]);
        } else {
        double R0[3][3], R1[3][3], R2[3][3], W01[2][2][3], W02[2][2][3], W12[2][2][3], Mm[3][3][3];
#define NH_P1HEX_QS(q) qs[q]
#define NH_P1HEX_QM(q) qm[q]
#include "nh_p1hex_math.inc"
#undef NH_P1HEX_QS
#undef NH_P1HEX_QM
        // the 36 entries a <= b of the local matrix: entry(a, bb)
#include "nh_p1hex_entry.inc"
        {  // reduce: the accumulated rows of a plane are the vertices of the tile, so every local vertex has a row (no masking)
          // every entry goes to LDS as soon as it is formed: the ds_add_f64 stream overlaps the remaining arithmetic of the same wave
          // (issued in one burst at the end, the 36 atomics of all waves pile up in front of the barrier)
#pragma unroll
          for (int a = 0; a < 8; ++a) {
            const int a0 = a >> 2, a1 = (a >> 1) & 1, a2 = a & 1;
#pragma unroll
            for (int bb = a; bb < 8; ++bb) {
              const int b0 = bb >> 2, b1 = (bb >> 1) & 1, b2 = bb & 1;
              const double k = entry(a, bb);
              double *const dst = NH_P1HEX_SLOT(a0, a1, a2, b0, b1, b2);
              if (!(DEBUG(p) & 1)) atomicAdd(dst, k);
              else if (k == 1.2345e300) dst[0] = 1.;
            }
          }
        }
        }  // !VEC
#undef NH_P1HEX_ELEM
#undef NH_P1HEX_SLOT
