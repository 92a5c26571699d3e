// Paired bootstrap comparison of up to 8 score columns on the same held-out rows: column 0 is the
// reference model, columns 1..M−1 its comparators.  One workgroup per replicate draws the rows ONCE,
// by the law of resample.h as bootstrap.hip does, and every column is then scored on those same
// counts.  plain: no map, row r is counted.  stratified: j < P draws rowmap[r] (the r-th positive),
// j ≥ P rowmap[P + r].
//
// Per replicate: zero the counts → n integer atomicAdds into cnt[original row] → the paired
// statistics in original row order, thread t owning rows [t·chunk, (t+1)·chunk): per comparator the
// reclassification counts (integers) and per column Σc·p over the drawn positives, over the drawn
// negatives and Σc·(p−y)² (f64) → then per column, one after another: gather the counts through
// the column's descending score order (cp[pos] = cnt[order[pos]]: `order` is read coalesced, the
// LDS read is the random one, the write is linear) and run what bootstrap.hip runs on them, the
// scan and the rank statistics of resample.h: a column's a2, ap and conf are bit for bit those of
// bootstrap.hip on that column.
// Every f64 sum is folded chunk (rows ascending) → wave (xor tree) → waves in order, which depends
// on n alone; nothing depends on the grid, on which workgroup ran the replicate, or on where the
// three arrays live:
//   LDS     while 12 B/row fit: kCmpLdsRows = 13,000 rows = 156,000 B of the CU's 160 KiB
//           (163,840 B), leaving room for the 1,664 B of static reduction scratch below;
//   global  above that, workgroup w owns slice w of the caller's workspace (3n u32 per slice).
// No float atomics; results are written with ordinary vector stores.
#include "resample.h"

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does this file

namespace hfens {

constexpr int kCmpLdsRows = 13000;
constexpr int kCmpMaxModels = 8;
constexpr int kCmpStatic = 1664;            // sc_pn 128 + sc_a2 128 + sc_ap 128 + sc_rc 512 + sc_sm 768

struct CmpArgs {
  const unsigned char* y;    // [n] labels by original row
  const int* rowmap;         // stratified: [n] the positives' rows, then the negatives'; plain: null
  const int* order;          // [M][n] position in the column's descending score order → row
  const unsigned char* ys;   // [M][n] labels in that order
  const int* gfirst;         // [M][n] first position of the position's tie group
  const int* glast;          // [M][n] last position of it
  const int* k0;             // [M] rows scoring > threshold
  const unsigned char* hi;   // [M][n] by original row: score > threshold
  const double* p;           // [M][n] by original row: the score
  int n, p0, M;              // p0: draws j < p0 take stratum [0, p0), the rest [p0, n)  (plain: p0 = n)
  unsigned long long seed;
  long long b0;
  int nb;
  unsigned* ws;              // global path: [slices][3n]
  double* auroc;             // [nb][M]
  double* ap;                // [nb][M]
  long long* a2;             // [nb][M]
  long long* pn;             // [nb][2]
  long long* conf;           // [nb][M][4]  TP FP FN TN
  long long* reclass;        // [nb][M][4]  eu ed nu nd (column 0: zeros)
  double* sums;              // [nb][M][3]  Σc·p positives, Σc·p negatives, Σc·(p−y)²
};

template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void compare_kernel(CmpArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned cmp_lds[];
  __shared__ unsigned sc_pn[kBootWaves][2];
  __shared__ unsigned long long sc_a2[kBootWaves];
  __shared__ double sc_ap[kBootWaves];
  __shared__ unsigned sc_rc[2][kBootWaves][4];
  __shared__ double sc_sm[2][kBootWaves][3];
  const int n = A.n, M = A.M;
  unsigned* cnt;   // multiplicity of every original row
  if constexpr (kLds) cnt = cmp_lds;
  else cnt = A.ws + (size_t)blockIdx.x * 3 * (size_t)n;
  unsigned* cp = cnt + n;   // a column's gathered counts, then its cumulative positive multiplicity
  unsigned* cn = cp + n;    // its cumulative negative multiplicity
  const BootThread t = boot_thread(n);
  const int tid = t.tid, lane = t.lane, wave = t.wave, r0 = t.r0, r1 = t.r1;

  for (int bb = blockIdx.x; bb < A.nb; bb += gridDim.x) {
    boot_draw(cnt, A.rowmap, n, A.p0, A.seed, (unsigned long long)(A.b0 + bb));

    // paired statistics in original row order.  Buffer m & 1 of the scratch is written again at
    // column m + 2 only, after the barrier of column m + 1, which thread 0 reaches after reading it.
    for (int m = 0; m < M; ++m) {
      const unsigned char* him = A.hi + (size_t)m * n;
      const double* pm = A.p + (size_t)m * n;
      unsigned eu = 0, ed = 0, nu = 0, nd = 0;
      double spos = 0.0, sneg = 0.0, ssq = 0.0;
      for (int i = r0; i < r1; ++i) {
        const unsigned c = cnt[i];
        if (c == 0u) continue;
        const bool pos = A.y[i] != 0;
        const bool h0 = A.hi[i] != 0, hm = him[i] != 0;
        if (h0 && !hm) { if (pos) eu += c; else nu += c; }
        if (!h0 && hm) { if (pos) ed += c; else nd += c; }
        const double w = (double)c, pi = pm[i];
        const double d = pi - (pos ? 1.0 : 0.0);
        if (pos) spos += w * pi; else sneg += w * pi;
        ssq += w * (d * d);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        eu += __shfl_xor(eu, o, kWave);
        ed += __shfl_xor(ed, o, kWave);
        nu += __shfl_xor(nu, o, kWave);
        nd += __shfl_xor(nd, o, kWave);
      }
      spos = wave_sum(spos);
      sneg = wave_sum(sneg);
      ssq = wave_sum(ssq);
      const int k = m & 1;
      if (lane == 0) {
        sc_rc[k][wave][0] = eu; sc_rc[k][wave][1] = ed; sc_rc[k][wave][2] = nu; sc_rc[k][wave][3] = nd;
        sc_sm[k][wave][0] = spos; sc_sm[k][wave][1] = sneg; sc_sm[k][wave][2] = ssq;
      }
      __syncthreads();
      if (tid == 0) {
        unsigned long long rc[4] = {0, 0, 0, 0};
        double sm[3] = {0.0, 0.0, 0.0};
        for (int w = 0; w < kBootWaves; ++w) {
          for (int q = 0; q < 4; ++q) rc[q] += sc_rc[k][w][q];
          for (int q = 0; q < 3; ++q) sm[q] += sc_sm[k][w][q];
        }
        long long* ro = A.reclass + 4 * ((size_t)bb * M + m);
        double* so = A.sums + 3 * ((size_t)bb * M + m);
        for (int q = 0; q < 4; ++q) ro[q] = (long long)rc[q];
        for (int q = 0; q < 3; ++q) so[q] = sm[q];
      }
    }

    for (int m = 0; m < M; ++m) {
      const int* ord = A.order + (size_t)m * n;
      for (int i = tid; i < n; i += kBootThreads) cp[i] = cnt[ord[i]];
      __syncthreads();
      boot_scan(cp, cn, A.ys + (size_t)m * n, t, sc_pn, [](int, unsigned, bool) {});
      __syncthreads();
      const size_t at = (size_t)bb * M + m;
      boot_rank_stats(cp, cn, A.gfirst + (size_t)m * n, A.glast + (size_t)m * n, t, cp[n - 1], cn[n - 1], A.k0[m],
                      sc_a2, sc_ap, A.a2 + at, m == 0 ? A.pn + 2 * (size_t)bb : nullptr, A.auroc + at, A.ap + at,
                      A.conf + 4 * at);
      __syncthreads();   // cp and cn are gathered anew for the next column, cnt zeroed for the next replicate
    }
  }
}

void compare_lds_rows(uintptr_t out) { *reinterpret_cast<long long*>(out) = kCmpLdsRows; }

// use_lds, ws, ws_slices and grid: see boot_launch (3 u32 arrays per row)
void bootstrap_compare(uintptr_t y, uintptr_t rowmap, uintptr_t order, uintptr_t ys, uintptr_t gfirst, uintptr_t glast,
                       uintptr_t k0, uintptr_t hi, uintptr_t p, long long n, long long p0, int M, long long seed,
                       long long b0, long long nb, int use_lds, uintptr_t ws, long long ws_slices, uintptr_t auroc,
                       uintptr_t ap, uintptr_t a2, uintptr_t pn, uintptr_t conf, uintptr_t reclass, uintptr_t sums,
                       int grid, uintptr_t stream) {
  HFENS_REQUIRE(M >= 1 && M <= kCmpMaxModels, "bootstrap_compare: 1 <= M <= 8");
  HFENS_REQUIRE(p0 == n || rowmap != 0, "bootstrap_compare: two strata need a row map");
  CmpArgs A{(const unsigned char*)y, (const int*)rowmap, (const int*)order, (const unsigned char*)ys,
            (const int*)gfirst, (const int*)glast, (const int*)k0, (const unsigned char*)hi, (const double*)p,
            (int)n, (int)p0, M, (unsigned long long)seed, b0, (int)nb, (unsigned*)ws, (double*)auroc, (double*)ap,
            (long long*)a2, (long long*)pn, (long long*)conf, (long long*)reclass, (double*)sums};
  boot_launch("bootstrap_compare", compare_kernel<true>, compare_kernel<false>, A, 3, kCmpLdsRows, kCmpStatic, n,
              p0, b0, nb, use_lds, ws, ws_slices, grid, stream);
}

}  // namespace hfens
