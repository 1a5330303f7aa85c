// bessx_k_coxzph.hip -- the proportional-hazards score test (Grambsch and Therneau) of ONE Cox model on a caller's DEVICE
// matrix (include/bessx.h section 2t).  Positions, r(k), e, wd, S0, W and the risk-set means U are those of
// bessx_k_coxinfo.hip, formed by the launchers of that unit, of bessx_k_coxeval.hip and bessx_k_coxsurv.hip as they are.
// With g_k the caller's time transform at position k (an exact 0 where status is 0) and q = 0, 1, 2:
//     c^q_k = wd_k g_k^q                       (c^0 = wd, c^1 = wd * g, c^2 = (wd * g) * g: one rounding per product)
//     h^q_k = c^q_k / S0(r(k)),   H^q_l = sum_{k <= l} h^q_k   (read at the last position of l's tie group under "breslow")
//     v^q_l = e_l H^q_l,          a^q_l = c^q_l - v^q_l       (formed as fma(-e_l, H^q_l, c^q_l), as k_cxi_vg's g is)
//     G1^q = sum_l v^q_l z_l z_l^T,   s^q = sum_l a^q_l z_l,   G2^q = sum_{events j} c^q_j u_j u_j^T,   I_q = G1^q - G2^q
// (z = (1, x): the sweeps carry an intercept entry that the finish drops).  q = 0 is section 2h: the same operations in
// the same order, so I_0, s^0 are its info and score bit for bit, and with g = 1 at every event so are I_1, I_2, s^1.
//   k_cxz_hazard   h^0, h^1, h^2 per position in one launch; h^0 is k_cxs_hazard's quotient.  Their forward scans are
//                  launch_cox_prefix_scan (the k_cxs_scan_* kernels), one per q: additions only, one fixed order.
//   k_cxz_vg       v^q and a^q in ROW order, the three-weight form of k_cxi_vg.
//   k_cxz_gram     k_info_gram with NW = 3 row-weight pairs (v^q, a^q) carried through ONE sweep: the A operand z and the
//                  loaded elements of X are shared, the B operand is scaled per weight, every weight has accumulators of
//                  its own (NW * IG_JC tiles of four doubles: 96 registers).  Tasks, slabs, the k order inside a slab,
//                  the three access shapes and the masking are k_info_gram's (bessx_k_infogram.hpp), so each weight's
//                  partials are bit for bit what k_info_gram writes with that weight alone.  The same kernel runs the G2
//                  sweeps over U (J x m, dense) with the weights c^q_j.
//   k_cxz_sum      k_info_finish per weight (blockIdx.z): the slabs' partials in the same fixed order.
//   k_cxz_finish   I_q = G1^q - G2^q without the intercept entry and s^0, s^1: the three-matrix form of k_cxi_finish.
// No floating-point atomics: the same call gives the same bits.  Block and slab counts depend on (n, m, J) alone.  Index
// arithmetic is in 64 bits.
#include "bessx_k_infogram.hpp"

namespace bessx {

namespace {

constexpr int CXZ_T = 256;
constexpr int CXZ_NW = 3;  // row-weight pairs of one sweep

}  // namespace

// gp: g in position order, an exact 0 where wd is not read for an event
__global__ void __launch_bounds__(CXZ_T) k_cxz_hazard(const double *__restrict__ wd, const double *__restrict__ gp,
                                                      const double *__restrict__ S, const int *__restrict__ first,
                                                      long long n, double *__restrict__ h0, double *__restrict__ h1,
                                                      double *__restrict__ h2) {
  const long long k = (long long)blockIdx.x * CXZ_T + threadIdx.x;
  if (k >= n) return;
  const double s = S[first[k]], c0 = wd[k], c1 = __dmul_rn(c0, gp[k]), c2 = __dmul_rn(c1, gp[k]);
  h0[k] = c0 / s;
  h1[k] = c1 / s;
  h2[k] = c2 / s;
}

// H: three arrays of n (stride hs); v, a: three arrays in row order (stride vs)
__global__ void __launch_bounds__(CXZ_T) k_cxz_vg(const double *__restrict__ e, const double *__restrict__ H, long long hs,
                                                  const int *__restrict__ lastk, const double *__restrict__ wd,
                                                  const double *__restrict__ gp, const int *__restrict__ pos, long long n,
                                                  double *__restrict__ v, double *__restrict__ a, long long vs) {
  const long long i = (long long)blockIdx.x * CXZ_T + threadIdx.x;
  if (i >= n) return;
  const int k = pos[i];
  const long long kl = lastk ? lastk[k] : k;
  const double ek = e[k], g = gp[k];
  double c = wd[k];
#pragma unroll
  for (int q = 0; q < CXZ_NW; q++) {
    const double vi = ek * H[q * hs + kl];
    v[q * vs + i] = vi;
    // c - e H with the product unrounded: the fused multiply-add that the compiler's contraction makes of k_cxi_vg's
    // g = wd - e H, written out so that every q gets it (left to contraction, q > 0 fuses c's own product instead)
    a[q * vs + i] = fma(-ek, H[q * hs + kl], c);
    c = c * g;
  }
}

// k_info_gram with CXZ_NW weight pairs: vw + w * ws, gw + w * ws are the n-vectors of weight w, part + w * ps its partials
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) k_cxz_gram(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                  const int *__restrict__ cols, int M, const double *__restrict__ vw,
                                                  const double *__restrict__ gw, long long ws, long long rps, int slabs,
                                                  int T_tiles, double *__restrict__ part, long long ps) {
  constexpr int E = VEC ? PrVec<T>::N : 4;
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int s = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
  if (s >= slabs) return;  // (wave-uniform; the kernel has no barrier)
  int It = 0, run = (int)blockIdx.x;
  while (run >= (It + 2 + IG_JC - 1) / IG_JC) {
    run -= (It + 2 + IG_JC - 1) / IG_JC;
    It++;
  }
  const int slot0 = run * IG_JC, nJ = min(IG_JC, It + 2 - slot0);
  const T *pa;
  const int ka = ig_entry(src, cs, cols, M, 16 * It + c, &pa);
  const T *pb[IG_JC];
  int kb[IG_JC];
  bool need_g = false;
#pragma unroll
  for (int jj = 0; jj < IG_JC; jj++) {
    const int slot = slot0 + jj;
    pb[jj] = src;
    kb[jj] = IG_ZERO;
    if (jj < nJ) {
      if (slot <= It) {
        kb[jj] = ig_entry(src, cs, cols, M, 16 * slot + c, &pb[jj]);
      } else {
        kb[jj] = c == 0 ? IG_G : IG_ZERO;
        need_g = true;
      }
    }
  }
  d4 acc[CXZ_NW][IG_JC];
#pragma unroll
  for (int w = 0; w < CXZ_NW; w++)
#pragma unroll
    for (int jj = 0; jj < IG_JC; jj++) acc[w][jj] = d4{0.0, 0.0, 0.0, 0.0};
  const long long r_end = min(n, ((long long)s + 1) * rps);
  for (long long rb = (long long)s * rps; rb < r_end; rb += 4 * E) {
    const long long i0 = rb + (long long)q * E;
    double vv[CXZ_NW][E], gg[CXZ_NW][E], xa[E];
#pragma unroll
    for (int w = 0; w < CXZ_NW; w++)
#pragma unroll
      for (int e = 0; e < E; e++) {
        const bool in = i0 + e < n;
        vv[w][e] = in ? vw[w * ws + i0 + e] : 0.0;
        gg[w][e] = (in && need_g) ? gw[w * ws + i0 + e] : 0.0;
      }
    ig_rows<T, VEC, E>(ka, pa, rs, i0, n, xa);
#pragma unroll
    for (int jj = 0; jj < IG_JC; jj++) {
      if (jj < nJ) {  // (wave-uniform)
        double xb[E];
        if (slot0 + jj == It) {
#pragma unroll
          for (int e = 0; e < E; e++) xb[e] = xa[e];  // the diagonal tile: B's entry is A's
        } else {
          ig_rows<T, VEC, E>(kb[jj], pb[jj], rs, i0, n, xb);
        }
#pragma unroll
        for (int w = 0; w < CXZ_NW; w++)
#pragma unroll
          for (int e = 0; e < E; e++) {
            // (an entry past M, and the score slot's columns 1 .. 15, are exact zeros whatever the weight is)
            const double b = kb[jj] == IG_G ? gg[w][e] : (kb[jj] == IG_ZERO ? 0.0 : xb[e] * vv[w][e]);
            acc[w][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[e], b, acc[w][jj], 0, 0, 0);
          }
      }
    }
  }
  const long long t0 = (long long)It * (It + 3) / 2 + slot0;
#pragma unroll
  for (int w = 0; w < CXZ_NW; w++)
#pragma unroll
    for (int jj = 0; jj < IG_JC; jj++) {
      if (jj < nJ) {
        double *o = part + w * ps + ((long long)s * T_tiles + t0 + jj) * 256 + lane;
        o[0] = acc[w][jj].x;
        o[64] = acc[w][jj].y;
        o[128] = acc[w][jj].z;
        o[192] = acc[w][jj].w;
      }
    }
}

// k_info_finish for weight w = blockIdx.z: partials part + w * ps, results G + w * gs (M x M, leading dimension M) and
// G + w * gs + M * M (M values)
__global__ void __launch_bounds__(256) k_cxz_sum(const double *__restrict__ part, long long ps, int slabs, int T_tiles,
                                                 int M, double *__restrict__ G, long long gs) {
  const int tile = (int)blockIdx.x, lg = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int e0 = (int)blockIdx.y * 64 + grp * 4;
  const double *pw = part + (long long)blockIdx.z * ps;
  double *info = G + (long long)blockIdx.z * gs, *score = info + (long long)M * M;
  const long long ld = M;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = lg; s < slabs; s += 16) {
    const double *p = pw + ((long long)s * T_tiles + tile) * 256 + e0;
    const d2 lo = *reinterpret_cast<const d2 *>(p), hi = *reinterpret_cast<const d2 *>(p + 2);
    sum[0] += lo.x;
    sum[1] += lo.y;
    sum[2] += hi.x;
    sum[3] += hi.y;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) sum[j] = pr_group_sum<16>(sum[j]);
  if (lg != 0) return;
  int It = 0;
  while ((It + 1) * (It + 4) / 2 <= tile) It++;
  const int slot = tile - It * (It + 3) / 2;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int e = e0 + j, reg = e >> 6, ln = e & 63;
    const int a = 16 * It + (ln >> 4) + 4 * reg, bl = ln & 15;
    if (a >= M) continue;
    if (slot > It) {
      if (bl == 0) score[a] = sum[j];
    } else {
      const int b = 16 * slot + bl;
      if (b <= a) {  // (b <= a < M) the lower triangle names the value, the upper one is its mirror
        info[a * ld + b] = sum[j];
        info[b * ld + a] = sum[j];
      }
    }
  }
}

// G1, G2: per weight q at + q * gs an (m + 1) x (m + 1) matrix followed by m + 1 values (k_cxz_sum's results); G2 null:
// no event, nothing is taken off.  info: three m x m matrices, score: two m-vectors.
__global__ void __launch_bounds__(CXZ_T) k_cxz_finish(const double *__restrict__ G1, const double *__restrict__ G2,
                                                      long long gs, int m, double *__restrict__ info0,
                                                      double *__restrict__ info1, double *__restrict__ info2, long long ld,
                                                      double *__restrict__ score0, double *__restrict__ score1) {
  const long long t = (long long)blockIdx.x * CXZ_T + threadIdx.x, M = (long long)m + 1;
  if (t >= (long long)m * m) return;
  const long long a = t / m, b = t % m, o = (a + 1) * M + b + 1;
  double *const info[CXZ_NW] = {info0, info1, info2};
#pragma unroll
  for (int q = 0; q < CXZ_NW; q++) info[q][a * ld + b] = G2 ? G1[q * gs + o] - G2[q * gs + o] : G1[q * gs + o];
  if (b == 0) {
    score0[a] = G1[M * M + a + 1];
    score1[a] = G1[gs + M * M + a + 1];
  }
}

// h0, h1, h2 (n doubles each) from wd, gp and S0 (position order); first = r(k)
hipError_t launch_cox_zph_hazard(const double *wd, const double *gp, const double *S, const int *first, long long n,
                                 double *h0, double *h1, double *h2, hipStream_t st) {
  if (!wd || !gp || !S || !first || !h0 || !h1 || !h2 || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxz_hazard, dim3((unsigned)((n + CXZ_T - 1) / CXZ_T)), dim3(CXZ_T), 0, st, wd, gp, S, first, n, h0,
                     h1, h2);
  LAUNCH_CHECK();
  return hipSuccess;
}

// v^q, a^q (q = 0, 1, 2 at v + q * vs, a + q * vs, ROW order) from e, H^q (at H + q * hs), wd, gp (position order);
// lastk null: ties "order"
hipError_t launch_cox_zph_vg(const double *e, const double *H, long long hs, const int *lastk, const double *wd,
                             const double *gp, const int *pos, long long n, double *v, double *a, long long vs,
                             hipStream_t st) {
  if (!e || !H || !wd || !gp || !pos || !v || !a || n < 1 || n > 0x7fffffffLL || hs < n || vs < n)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxz_vg, dim3((unsigned)((n + CXZ_T - 1) / CXZ_T)), dim3(CXZ_T), 0, st, e, H, hs, lastk, wd, gp, pos,
                     n, v, a, vs);
  LAUNCH_CHECK();
  return hipSuccess;
}

template <typename T>
static hipError_t cxz_launch_gram(const T *src, long long rs, long long cs, long long n, const int *cols, int M,
                                  const double *vw, const double *gw, long long ws, const InfoSplit &sp, double *part,
                                  long long ps, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const dim3 grid((unsigned)sp.tasks, (unsigned)((sp.slabs + 3) / 4));
  if (vec)
    hipLaunchKernelGGL((k_cxz_gram<T, true>), grid, dim3(256), 0, st, src, rs, cs, n, cols, M, vw, gw, ws, sp.rps,
                       sp.slabs, sp.T, part, ps);
  else
    hipLaunchKernelGGL((k_cxz_gram<T, false>), grid, dim3(256), 0, st, src, rs, cs, n, cols, M, vw, gw, ws, sp.rps,
                       sp.slabs, sp.T, part, ps);
  LAUNCH_CHECK();
  return hipSuccess;
}

// doubles of the three weights' partials (each weight's share is even: 16-byte loads in k_cxz_sum)
long long cox_zph_gram_workspace(long long n, int m) { return CXZ_NW * info_gram_workspace(n, m); }

// launch_info_gram for three weight pairs in one sweep: vw, gw hold the n-vectors of weight q at + q * ws; part:
// cox_zph_gram_workspace(n, m) doubles; G receives per weight q, at + q * gs, the (m + 1) x (m + 1) matrix (leading
// dimension m + 1) followed by the m + 1 score values: gs >= (m + 1) * (m + 2).  Device memory.
hipError_t launch_cox_zph_gram(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *vw, const double *gw, long long ws, double *part, double *G, long long gs,
                               hipStream_t st) {
  if (!src || !vw || !gw || !part || !G || n < 1 || n > 0x7fffffffLL || m < 0 || m + 1 > INFO_M_MAX ||
      (m > 0 && !cols) || rs < 0 || cs < 0 || ws < n || gs < ((long long)m + 1) * (m + 2))
    return hipErrorInvalidValue;
  const int M = m + 1;
  const InfoSplit sp = ig_split(n, M);
  const long long ps = (long long)sp.slabs * sp.T * 256;
  hipError_t e = f32 ? cxz_launch_gram(static_cast<const float *>(src), rs, cs, n, cols, M, vw, gw, ws, sp, part, ps, st)
                     : cxz_launch_gram(static_cast<const double *>(src), rs, cs, n, cols, M, vw, gw, ws, sp, part, ps, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cxz_sum, dim3((unsigned)sp.T, 4, CXZ_NW), dim3(256), 0, st, part, ps, sp.slabs, sp.T, M, G, gs);
  LAUNCH_CHECK();
  return hipSuccess;
}

// info0, info1, info2 (m x m, leading dimension ld) and score0, score1 (m) from the two sweeps' results (G2 null: no event)
hipError_t launch_cox_zph_finish(const double *G1, const double *G2, long long gs, int m, double *info0, double *info1,
                                 double *info2, long long ld, double *score0, double *score1, hipStream_t st) {
  if (!G1 || !info0 || !info1 || !info2 || !score0 || !score1 || m < 1 || ld < m || gs < ((long long)m + 1) * (m + 2))
    return hipErrorInvalidValue;
  const long long cnt = (long long)m * m;
  hipLaunchKernelGGL(k_cxz_finish, dim3((unsigned)((cnt + CXZ_T - 1) / CXZ_T)), dim3(CXZ_T), 0, st, G1, G2, gs, m, info0,
                     info1, info2, ld, score0, score1);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
