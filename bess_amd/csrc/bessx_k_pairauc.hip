// bessx_k_pairauc.hip -- weighted counts of ordered pairs of rows for R models on a caller's DEVICE matrix: the kernels
// behind bessx_cox_auc_device (cumulative/dynamic AUC(t) and Uno's C) and bessx_auc_device (logistic ROC AUC).  The
// weighted, segment-aware successor of k_cxe_pairs (bessx_k_coxeval.hip).
// Positions: k = 0 .. n - 1 is the rank of a row in the host's order (Cox: the stable ascending order of the times;
// logistic: cases first); the host uploads pos[row].  The T cuts s_1 <= .. <= s_T (s_j = rows with time <= t_j) split the
// positions into S = T + 1 segments, and the host cuts every segment into TILES of at most 1024 consecutive positions
// (tstart[0 .. NT], tseg[tile], tnext[tile] = the first tile of a later segment): no tile straddles a cut, so a
// (k-tile, l-tile) pair lies in ONE cell (case segment c, control segment b).
//   predictor pass   the loops of bessx_k_xb.hpp with a store epilogue of its own: eta(i, r) goes to position pos[i] of an
//                    R x n position-major array (launch_cox_eval_eta would also write exp(eta), which nothing here reads).
//   k_pa_pairs       grid (k-tiles, models).  A workgroup keeps the eta and the case weight of its 1024 positions in
//                    registers (4 per thread), streams the l-tiles -- eta, the control weight and, for Uno's C, the
//                    tie-group index first[l] -- through LDS (every read of the inner loop is a broadcast) and adds
//                    w_l * 1(eta_k > eta_l) and w_l * 1(eta_k = eta_l) to two fp64 accumulators per owned position.
//                    AUC mode walks the l-tiles of later segments only; UNO mode walks the l-tiles from its own on and
//                    a pair counts when first[l] > kg[k] (kg = first for an event, INT_MAX otherwise: the pair set of
//                    k_cxe_pairs).  Whenever the l-segment b changes, sum_k cw_k * acc_k is reduced over the block -- a
//                    thread's four positions in order, the lanes by the DPP tree of pr_group_sum, the waves in wave
//                    order -- and stored to the workgroup's own slot part[r][k-tile][b]: one writer per slot, no atomics.
//   k_pa_colscan     part[r][kt][b] becomes the running sum over the k-tiles 0 .. kt, in tile order, in place.
//   k_pa_cut         out[q][r] = sum over b >= from[q], ascending, of part[r][last[q]][b]: with last[j] the last tile of a
//                    segment <= j and from[j] = j + 1 this is greater[j] = sum_{c <= j < b} M[c][b] -- two nested running
//                    sums, T^2 additions per model, not T^3.  Uno's C is the one entry (last tile, from 0).
// fp64, every sum in one fixed order, the grids depend on (n, the cuts, R) alone: the same call gives the same bits.
// Half credit for ties is the host's.  Index arithmetic is in 64 bits.  Nothing is n x T or n x n.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int PA_T = 256, PA_E = 4, PA_B = PA_T * PA_E;  // threads, positions per thread, positions per tile
static_assert(PA_B == PAIRAUC_TILE, "the host cuts the tiles");

struct PaStore {
  static constexpr bool REDUCE = false, SKIPZ = true;
  const int *__restrict__ pos;
  long long n;
  double *__restrict__ eta;
  __device__ __forceinline__ void store(double v, long long i, int r) const { eta[(long long)r * n + pos[i]] = v; }
};

}  // namespace

// part[((r * NT + kt) * S + b) * 2 + {0, 1}] = sum over the positions k of tile kt and l of segment b of
// cw[k] lw[l] 1(eta_k > eta_l) / 1(eta_k = eta_l) (UNO: and first[l] > kg[k]).  Slots it does not write stay as the
// launcher zeroed them.
template <bool UNO>
__global__ void __launch_bounds__(PA_T) k_pa_pairs(const double *__restrict__ eta, const double *__restrict__ cw,
                                                   const double *__restrict__ lw, const int *__restrict__ kg,
                                                   const int *__restrict__ first, const int *__restrict__ tstart,
                                                   const int *__restrict__ tseg, const int *__restrict__ tnext,
                                                   long long n, int NT, int S, double *__restrict__ part) {
  const int kt = blockIdx.x, r = blockIdx.y, t = threadIdx.x;
  int lt = UNO ? kt : tnext[kt];
  if (lt >= NT) return;  // (uniform: the last segment's tiles have no controls)
  __shared__ double le[PA_B], ls[PA_B];
  __shared__ int lg[PA_B];
  __shared__ double red[2][4];
  const double *er = eta + (long long)r * n;
  const int k0 = tstart[kt], k1 = tstart[kt + 1];
  double ek[PA_E], ck[PA_E], ag[PA_E], ae[PA_E];
  int gk[PA_E];
#pragma unroll
  for (int q = 0; q < PA_E; q++) {
    const int k = k0 + q * PA_T + t;
    const bool ok = k < k1;
    ek[q] = ok ? er[k] : 0.0;
    ck[q] = ok ? cw[k] : 0.0;  // (a position past the tile's end carries no weight)
    gk[q] = UNO ? (ok ? kg[k] : 0x7fffffff) : 0;
    ag[q] = ae[q] = 0.0;
  }
  double *out = part + ((long long)r * NT + kt) * S * 2;
  // sum_k ck * acc over the block in a fixed order, to the slot of segment b; the accumulators start again
  auto flush = [&](int b) {
    double sg = 0.0, se = 0.0;
#pragma unroll
    for (int q = 0; q < PA_E; q++) {
      sg += ck[q] * ag[q];
      se += ck[q] * ae[q];
      ag[q] = ae[q] = 0.0;
    }
    sg = pr_group_sum<64>(sg);
    se = pr_group_sum<64>(se);
    if ((t & 63) == 0) {
      red[0][t >> 6] = sg;
      red[1][t >> 6] = se;
    }
    __syncthreads();
    if (t < 2) out[2 * (long long)b + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
  };
  int b = tseg[lt];
  for (; lt < NT; lt++) {
    const int bn = tseg[lt];
    if (bn != b) {  // (uniform)
      flush(b);
      b = bn;
    }
    __syncthreads();  // (the tile before is read, and so is red)
    const int l0 = tstart[lt], ln = tstart[lt + 1] - l0;
#pragma unroll
    for (int q = 0; q < PA_E; q++) {
      const int j = q * PA_T + t;
      if (j < ln) {
        le[j] = er[l0 + j];
        ls[j] = lw[l0 + j];
        if (UNO) lg[j] = first[l0 + j];
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < ln; j++) {
      const double el = le[j], wl = ls[j];  // (every lane reads the same word: a broadcast)
      const int gl = UNO ? lg[j] : 0;
#pragma unroll
      for (int q = 0; q < PA_E; q++) {
        const bool c = !UNO || gl > gk[q];
        ag[q] += (c && ek[q] > el) ? wl : 0.0;
        ae[q] += (c && ek[q] == el) ? wl : 0.0;
      }
    }
  }
  flush(b);
}

// column col = 2 * b + {0, 1} of model r = blockIdx.y: the running sum over the k-tiles, in place
__global__ void __launch_bounds__(PA_T) k_pa_colscan(double *__restrict__ part, int NT, int S2) {
  const int col = blockIdx.x * PA_T + threadIdx.x;
  if (col >= S2) return;
  double *p = part + (long long)blockIdx.y * NT * S2 + col;
  double s = 0.0;
  for (int kt = 0; kt < NT; kt++) {
    s += p[(long long)kt * S2];
    p[(long long)kt * S2] = s;
  }
}

// og[q * R + r], oe[q * R + r] = sum_{b >= from[q]} of the scanned part[r][last[q]][b] (0 where last[q] < 0)
__global__ void __launch_bounds__(PA_T) k_pa_cut(const double *__restrict__ part, const int *__restrict__ last,
                                                 const int *__restrict__ from, int Q, int R, int NT, int S,
                                                 double *__restrict__ og, double *__restrict__ oe) {
  const long long id = (long long)blockIdx.x * PA_T + threadIdx.x;
  if (id >= (long long)Q * R) return;
  const int q = (int)(id / R), r = (int)(id - (long long)q * R);
  double sg = 0.0, se = 0.0;
  const int lk = last[q];
  if (lk >= 0) {
    const double *p = part + ((long long)r * NT + lk) * S * 2;
    for (int b = from[q]; b < S; b++) {
      sg += p[2 * (long long)b];
      se += p[2 * (long long)b + 1];
    }
  }
  og[id] = sg;
  oe[id] = se;
}

// an upper bound of the tiles the host cuts n positions with T cuts into
long long pairauc_tiles_max(long long n, int T) { return (n + PA_B - 1) / PA_B + T; }

// doubles of device memory a bessx_cox_auc_device call holds at most: eta (R n), the three weight vectors (3 n), the
// partials (2 R tiles (T + 1)), the results (2 R (T + 1)); the int vectors pos, kg, first (3 n) and the tile and cut
// tables (3 tiles + 2 T + 4) as half a double each.  Nothing n x T.
long long pairauc_workspace(long long n, int T, int R) {
  const long long nt = pairauc_tiles_max(n, T);
  return (long long)R * n + 3 * n + 2LL * R * nt * (T + 1) + 2LL * R * (T + 1) + (3 * n + 3 * nt + 2LL * T + 4 + 1) / 2;
}

// eta[r * n + pos[i]] = eta(i, r); src, cols, B (m x R) as in launch_predict; zero: R device doubles of 0.0
hipError_t launch_pairauc_eta(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                              const double *B, const double *zero, int R, const int *pos, double *eta, hipStream_t st) {
  if (!src || !zero || !pos || !eta || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || R < 1 ||
      R > 65535 || rs < 0 || cs < 0)
    return hipErrorInvalidValue;
  const PaStore epi{pos, n, eta};
  if (f32) return xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, zero, R, epi, st);
  return xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, zero, R, epi, st);
}

// og, oe (Q x R): the Q sums of k_pa_cut over the pair counts of eta (R x n, position-major) with the case weights cw and
// the control weights lw (n each); uno: the pair set of Uno's C (kg, first: n ints each; null otherwise).  tstart (NT + 1),
// tseg, tnext (NT each): the tiles, every one of 1 .. 1024 positions, tstart[NT] = n; S: segments (tseg < S); last, from
// (Q each): what k_pa_cut adds.  part: 2 R NT S doubles.  only = 1 / 2 launches the pair kernel / the two finish kernels
// alone.  All device memory.
hipError_t launch_pairauc(const double *eta, const double *cw, const double *lw, const int *kg, const int *first,
                          const int *tstart, const int *tseg, const int *tnext, long long n, int NT, int S, int R, int uno,
                          const int *last, const int *from, int Q, double *part, double *og, double *oe, int only,
                          hipStream_t st) {
  if (!eta || !cw || !lw || (uno && (!kg || !first)) || !tstart || !tseg || !tnext || !last || !from || !part || !og ||
      !oe || n < 1 || n > 0x7fffffffLL || NT < 1 || NT > n || S < 1 || S > PAIRAUC_T_MAX + 1 || R < 1 || R > 65535 || Q < 1 ||
      Q > S)
    return hipErrorInvalidValue;
  if (only != 2) {
    hipError_t e = hipMemsetAsync(part, 0, 2 * (size_t)R * (size_t)NT * (size_t)S * sizeof(double), st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)NT, (unsigned)R);
    if (uno)
      hipLaunchKernelGGL(k_pa_pairs<true>, grid, dim3(PA_T), 0, st, eta, cw, lw, kg, first, tstart, tseg, tnext, n, NT, S,
                         part);
    else
      hipLaunchKernelGGL(k_pa_pairs<false>, grid, dim3(PA_T), 0, st, eta, cw, lw, kg, first, tstart, tseg, tnext, n, NT, S,
                         part);
    LAUNCH_CHECK();
  }
  if (only != 1) {
    hipLaunchKernelGGL(k_pa_colscan, dim3((unsigned)((2 * S + PA_T - 1) / PA_T), (unsigned)R), dim3(PA_T), 0, st, part, NT,
                       2 * S);
    LAUNCH_CHECK();
    const long long QR = (long long)Q * R;
    hipLaunchKernelGGL(k_pa_cut, dim3((unsigned)((QR + PA_T - 1) / PA_T)), dim3(PA_T), 0, st, part, last, from, Q, R, NT, S,
                       og, oe);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

}  // namespace bessx
