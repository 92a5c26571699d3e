// Nonparametric bootstrap of the held-out calibration and decision-curve statistics: Brier score,
// Σp (for O:E), the reliability bins, TP/FP at a grid of treat thresholds and the weighted
// two-parameter logistic recalibration fit (Cox: logit P(y=1) = a + b·logit p), one workgroup per
// replicate, on the resample bootstrap.hip draws for the same seed, mode and replicate: both draw
// through resample.h, where the law is stated.
//
// Per replicate: zero the counts → n integer atomicAdds → block-wide inclusive scan of the
// (positive, negative) multiplicities, thread t owning rows [t·chunk, (t+1)·chunk); the same walk
// folds Σc·(p−y)² and Σc·p and finds the first and last drawn row of each class → bin and threshold
// counts are differences of the cumulative arrays → the status is decided in integers and float
// comparisons → Newton from the null model, one pass over the drawn rows per evaluation.
// The multiplicity of row i is read back as (cp[i] + cn[i]) − (cp[i−1] + cn[i−1]), so the kernel
// keeps the two u32 arrays of bootstrap.hip and no third one.
// Every f64 sum is folded chunk (rows ascending, undrawn rows skipped) → wave (xor tree) → waves in
// order; a bin's Σc·p is folded by wave (bin mod 16), lanes striding its rows, then the xor tree.
// Both orders depend on n and the bin ranges alone: nothing depends on the grid, on which
// workgroup ran the replicate, or on where the two arrays live:
//   LDS     while 8 B/row fit: kCalLdsRows = 20,000 rows = 160,000 B of the CU's 160 KiB
//           (163,840 B), leaving room for the 2,176 B of static scratch below;
//   global  above that, workgroup w owns slice w of the caller's workspace (2n u32 per slice).
// The Newton state lives in every thread: all of them fold the 16 wave partials in the same order
// and take the same branches.  No float atomics; results are written with ordinary vector stores.
#include "resample.h"

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does this file

namespace hfens {

constexpr int kCalLdsRows = 20000;
constexpr int kCalStatic = 2176;             // sc_pn 128 + sc_ix 256 + sc_bs 256 + sc_nt 1536
constexpr int kCalMaxIter = 50;
constexpr int kCalMaxHalve = 40;
constexpr double kCalStepTol = 1e-10;
constexpr double kCalRise = 1e-12;

struct CalArgs {
  const unsigned char* y;   // [n] labels in score order
  const int* map;           // [n] drawn row → position in score order
  const double* p;          // [n] scores in [0, 1], descending
  const double* l;          // [n] logit of the clamped score
  const int* bin_end;       // [K] rows before the end of bin k = rows scoring ≥ k/K (bin_end[0] = n)
  const int* thr;           // [T] rows scoring ≥ t_g
  int n, p0, K, T;          // p0: draws j < p0 take stratum [0, p0), the rest [p0, n)  (plain: p0 = n)
  unsigned long long seed;
  long long b0;
  int nb;
  unsigned* ws;             // global path: [slices][2n]
  long long* pn;            // [nb][2]
  double* brier;            // [nb]
  double* sum_p;            // [nb]
  long long* bin_n;         // [nb][K]
  long long* bin_pos;       // [nb][K]
  double* bin_sum_p;        // [nb][K]
  long long* dc;            // [nb][T][2]  TP FP
  long long* status;        // [nb]
  double* coef;             // [nb][2]  intercept, slope
  long long* iters;         // [nb]
};

struct CalSums { double dev, g0, g1, h00, h01, h11; };

// One evaluation at (a, b): deviance, gradient and Hessian of the weighted log-likelihood, every
// thread returning the same six sums.  `buf` alternates between calls, so one barrier per call is
// enough: a thread can write buffer k again only after every thread has passed the barrier of the
// call in between, which it reaches after reading buffer k.
__device__ __forceinline__ CalSums cal_pass(const CalArgs& A, const unsigned* cp, const unsigned* cn, int r0, int r1,
                                            double a, double b, double (*sc)[6], int lane, int wave) {
  double dev = 0.0, g0 = 0.0, g1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0;
  unsigned prev = r0 > 0 && r0 < r1 ? cp[r0 - 1] + cn[r0 - 1] : 0u;
  for (int i = r0; i < r1; ++i) {
    const unsigned cur = cp[i] + cn[i];
    const unsigned c = cur - prev;
    prev = cur;
    if (c == 0u) continue;
    const double w = (double)c, li = A.l[i];
    const bool pos = A.y[i] != 0;
    const double e = a + b * li;
    const double z = exp(-fabs(e));
    const double q = 1.0 / (1.0 + z);
    const double mu = e >= 0.0 ? q : z * q;
    const double v = (z * q) * q;                       // μ(1 − μ)
    const double r = (pos ? 1.0 : 0.0) - mu;
    dev += w * (log1p(z) + fmax(e, 0.0) - (pos ? e : 0.0));
    const double wr = w * r, wv = w * v, wvl = wv * li;
    g0 += wr;
    g1 += wr * li;
    h00 += wv;
    h01 += wvl;
    h11 += wvl * li;
  }
  dev = wave_sum(dev);
  g0 = wave_sum(g0);
  g1 = wave_sum(g1);
  h00 = wave_sum(h00);
  h01 = wave_sum(h01);
  h11 = wave_sum(h11);
  if (lane == 0) {
    sc[wave][0] = dev; sc[wave][1] = g0; sc[wave][2] = g1;
    sc[wave][3] = h00; sc[wave][4] = h01; sc[wave][5] = h11;
  }
  __syncthreads();
  CalSums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 2   // unrolled 16 times it holds 96 doubles in flight and spills
  for (int w = 0; w < kBootWaves; ++w) {
    s.dev += sc[w][0]; s.g0 += sc[w][1]; s.g1 += sc[w][2];
    s.h00 += sc[w][3]; s.h01 += sc[w][4]; s.h11 += sc[w][5];
  }
  return s;
}

template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void calibration_kernel(CalArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned cal_lds[];
  __shared__ unsigned sc_pn[kBootWaves][2];
  __shared__ int sc_ix[kBootWaves][4];        // first/last drawn positive, first/last drawn negative
  __shared__ double sc_bs[kBootWaves][2];     // Σc(p−y)², Σc·p
  __shared__ double sc_nt[2][kBootWaves][6];
  const int n = A.n, K = A.K, T = A.T;
  unsigned* cp;   // counts, then cumulative positive multiplicity
  if constexpr (kLds) cp = cal_lds;
  else cp = A.ws + (size_t)blockIdx.x * 2 * (size_t)n;
  unsigned* cn = cp + n;   // cumulative negative multiplicity
  const BootThread t = boot_thread(n);
  const int tid = t.tid, lane = t.lane, wave = t.wave, r0 = t.r0, r1 = t.r1;
  const double kNan = boot_nan();

  for (int bb = blockIdx.x; bb < A.nb; bb += gridDim.x) {
    boot_draw(cp, A.map, n, A.p0, A.seed, (unsigned long long)(A.b0 + bb));
    // the scan's second walk also folds the Brier and Σp partials and finds the first and last drawn
    // row of each class
    double sb = 0.0, sq = 0.0;
    int fpos = n, lpos = -1, fneg = n, lneg = -1;
    boot_scan(cp, cn, A.y, t, sc_pn, [&](int i, unsigned c, bool pos) {
      if (c == 0u) return;
      const double w = (double)c, pi = A.p[i];
      const double d = pi - (pos ? 1.0 : 0.0);
      sb += w * (d * d);
      sq += w * pi;
      if (pos) { fpos = min(fpos, i); lpos = i; } else { fneg = min(fneg, i); lneg = i; }
    });
    sb = wave_sum(sb);
    sq = wave_sum(sq);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      fpos = min(fpos, __shfl_xor(fpos, o, kWave));
      fneg = min(fneg, __shfl_xor(fneg, o, kWave));
      lpos = max(lpos, __shfl_xor(lpos, o, kWave));
      lneg = max(lneg, __shfl_xor(lneg, o, kWave));
    }
    if (lane == 0) {
      sc_bs[wave][0] = sb; sc_bs[wave][1] = sq;
      sc_ix[wave][0] = fpos; sc_ix[wave][1] = lpos; sc_ix[wave][2] = fneg; sc_ix[wave][3] = lneg;
    }
    __syncthreads();

    const unsigned Pb = cp[n - 1], Nb = cn[n - 1];
    for (int w = 0; w < kBootWaves; ++w) {
      fpos = min(fpos, sc_ix[w][0]); lpos = max(lpos, sc_ix[w][1]);
      fneg = min(fneg, sc_ix[w][2]); lneg = max(lneg, sc_ix[w][3]);
    }
    // l is non-increasing over rows: a class's largest l is at its first drawn row, its smallest at the last
    int status = 0;
    if (Pb == 0u || Nb == 0u) status = 1;
    else if (!(A.l[lpos] < A.l[fneg] && A.l[lneg] < A.l[fpos])) status = 2;
    if (tid == 0) {
      double B2 = 0.0, SP = 0.0;
      for (int w = 0; w < kBootWaves; ++w) { B2 += sc_bs[w][0]; SP += sc_bs[w][1]; }
      A.pn[2 * (size_t)bb] = Pb;
      A.pn[2 * (size_t)bb + 1] = Nb;
      A.brier[bb] = B2 / (double)n;
      A.sum_p[bb] = SP;
    }

    // reliability bins: bin k holds rows [bin_end[k+1], bin_end[k]) of the descending order
    for (int k = tid; k < K; k += kBootThreads) {
      const int s = k + 1 < K ? A.bin_end[k + 1] : 0, e = A.bin_end[k];
      const unsigned tp1 = e > 0 ? cp[e - 1] : 0u, fp1 = e > 0 ? cn[e - 1] : 0u;
      const unsigned tp0 = s > 0 ? cp[s - 1] : 0u, fp0 = s > 0 ? cn[s - 1] : 0u;
      A.bin_pos[(size_t)bb * K + k] = tp1 - tp0;
      A.bin_n[(size_t)bb * K + k] = (tp1 - tp0) + (fp1 - fp0);
    }
    for (int k = wave; k < K; k += kBootWaves) {
      const int s = k + 1 < K ? A.bin_end[k + 1] : 0, e = A.bin_end[k];
      double acc = 0.0;
      for (int i = s + lane; i < e; i += kWave) {
        const unsigned c = (cp[i] + cn[i]) - (i > 0 ? cp[i - 1] + cn[i - 1] : 0u);
        if (c != 0u) acc += (double)c * A.p[i];
      }
      acc = wave_sum(acc);
      if (lane == 0) A.bin_sum_p[(size_t)bb * K + k] = acc;
    }
    // decision curve: rows [0, thr[g]) are treated at t_g
    for (int g = tid; g < T; g += kBootThreads) {
      const int k = A.thr[g];
      long long* d = A.dc + 2 * ((size_t)bb * T + g);
      d[0] = k > 0 ? cp[k - 1] : 0u;
      d[1] = k > 0 ? cn[k - 1] : 0u;
    }

    // Cox recalibration: Newton from the null model, all threads in step
    double a = kNan, s = kNan;
    int it = 0;
    if (status == 0) {
      // (a, s) is the accepted point with deviance dcur, (a1, s1) the candidate a + t·(da, db) after h
      // halvings.  One call site for the pass: the first evaluation is a candidate accepted unseen.
      a = log((double)Pb / (double)Nb);
      s = 0.0;
      double a1 = a, s1 = s, da = 0.0, db = 0.0, t = 1.0, dcur = 0.0;
      int h = kCalMaxHalve, buf = 0;
      status = 3;
      for (;;) {
        const CalSums nx = cal_pass(A, cp, cn, r0, r1, a1, s1, sc_nt[buf], lane, wave);
        buf ^= 1;
        if (h < kCalMaxHalve && nx.dev - dcur > kCalRise * fabs(dcur)) {
          ++h;
          t *= 0.5;
          a1 = a + t * da;
          s1 = s + t * db;
          continue;
        }
        a = a1;
        s = s1;
        dcur = nx.dev;
        if (it == kCalMaxIter) break;
        ++it;
        const double det = nx.h00 * nx.h11 - nx.h01 * nx.h01;
        da = (nx.h11 * nx.g0 - nx.h01 * nx.g1) / det;
        db = (nx.h00 * nx.g1 - nx.h01 * nx.g0) / det;
        if (fabs(da) <= kCalStepTol && fabs(db) <= kCalStepTol) {   // the undamped step; NaN never passes
          a = a + da;
          s = s + db;
          status = 0;
          break;
        }
        t = 1.0;
        h = 0;
        a1 = a + t * da;
        s1 = s + t * db;
      }
      if (status != 0) { a = kNan; s = kNan; }
    }
    if (tid == 0) {
      A.status[bb] = status;
      A.coef[2 * (size_t)bb] = a;
      A.coef[2 * (size_t)bb + 1] = s;
      A.iters[bb] = it;
    }
    __syncthreads();   // the arrays are zeroed for the next replicate
  }
}

void calibration_lds_rows(uintptr_t out) { *reinterpret_cast<long long*>(out) = kCalLdsRows; }

// use_lds, ws, ws_slices and grid: see boot_launch (2 u32 arrays per row)
void bootstrap_calibration(uintptr_t y, uintptr_t map, uintptr_t p, uintptr_t l, uintptr_t bin_end, uintptr_t thr,
                           long long n, long long p0, int K, int T, long long seed, long long b0, long long nb,
                           int use_lds, uintptr_t ws, long long ws_slices, uintptr_t pn, uintptr_t brier,
                           uintptr_t sum_p, uintptr_t bin_n, uintptr_t bin_pos, uintptr_t bin_sum_p, uintptr_t dc,
                           uintptr_t status, uintptr_t coef, uintptr_t iters, int grid, uintptr_t stream) {
  HFENS_REQUIRE(K >= 1 && K <= 64, "bootstrap_calibration: 1 <= bins <= 64");
  HFENS_REQUIRE(T >= 1 && T <= 4096, "bootstrap_calibration: 1 <= thresholds <= 4096");
  CalArgs A{(const unsigned char*)y, (const int*)map, (const double*)p, (const double*)l, (const int*)bin_end,
            (const int*)thr, (int)n, (int)p0, K, T, (unsigned long long)seed, b0, (int)nb, (unsigned*)ws,
            (long long*)pn, (double*)brier, (double*)sum_p, (long long*)bin_n, (long long*)bin_pos,
            (double*)bin_sum_p, (long long*)dc, (long long*)status, (double*)coef, (long long*)iters};
  boot_launch("bootstrap_calibration", calibration_kernel<true>, calibration_kernel<false>, A, 2, kCalLdsRows,
              kCalStatic, n, p0, b0, nb, use_lds, ws, ws_slices, grid, stream);
}

}  // namespace hfens
