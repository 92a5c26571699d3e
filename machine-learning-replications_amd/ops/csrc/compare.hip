// Paired bootstrap comparison of up to 8 score columns on the same held-out rows: column 0 is the
// reference model, columns 1..M−1 its comparators.  One workgroup per replicate draws the rows ONCE,
// by the law of bootstrap.hip bit for bit, and every column is then scored on those same counts:
//
//   draw j of replicate b over a stratum of m rows:
//     u = splitmix64(seed ^ splitmix64((b << 40) ^ j)),  r = ((u >> 32)·m) >> 32   ∈ [0, m)
//   plain: row r.  stratified: j < P draws rowmap[r] (the r-th positive), j ≥ P rowmap[P + r].
//
// Per replicate: zero the counts → n integer atomicAdds into cnt[original row] → the paired
// statistics in original row order, thread t owning rows [t·chunk, (t+1)·chunk): per comparator the
// reclassification counts (integers) and per column Σc·p over the drawn positives, over the drawn
// negatives and Σc·(p−y)² (f64) → then per column, one after another: gather the counts through
// the column's descending score order (cp[pos] = cnt[order[pos]]: `order` is read coalesced, the
// LDS read is the random one, the write is linear) and run what bootstrap.hip runs on them: the
// block-wide scan of (positive, negative) multiplicities, the tie-group sums for the doubled AUROC
// numerator (u64, exact) and AP (f64), the confusion counts from the prefix of rows above the
// threshold.  A column's a2, ap and conf are bit for bit those of bootstrap.hip on that column.
// Every f64 sum is folded chunk (rows ascending) → wave (xor tree) → waves in order, which depends
// on n alone; nothing depends on the grid, on which workgroup ran the replicate, or on where the
// three arrays live:
//   LDS     while 12 B/row fit: kCmpLdsRows = 13,000 rows = 156,000 B of the CU's 160 KiB
//           (163,840 B), leaving room for the 1,664 B of static reduction scratch below;
//   global  above that, workgroup w owns slice w of the caller's workspace (3n u32 per slice).
// No float atomics; results are written with ordinary vector stores.
#include "common.h"

#include <algorithm>

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does this file

namespace hfens {

constexpr int kCmpThreads = 1024;
constexpr int kCmpWaves = kCmpThreads / kWave;
constexpr int kCmpLdsRows = 13000;
constexpr int kCmpMaxModels = 8;
constexpr long long kCmpMaxN = 1LL << 25;   // doubled AUROC numerator < 2^53
constexpr long long kCmpMaxB = 1LL << 24;   // replicate index shares the counter with the draw
constexpr int kCmpLdsPerCu = 160 * 1024;
constexpr int kCmpStatic = 1664;            // sc_pn 128 + sc_a2 128 + sc_ap 128 + sc_rc 512 + sc_sm 768

__device__ __forceinline__ unsigned long long cmp_splitmix64(unsigned long long x) {   // as bootstrap.hip
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

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
__global__ __launch_bounds__(kCmpThreads) void compare_kernel(CmpArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned cmp_lds[];
  __shared__ unsigned sc_pn[kCmpWaves][2];
  __shared__ unsigned long long sc_a2[kCmpWaves];
  __shared__ double sc_ap[kCmpWaves];
  __shared__ unsigned sc_rc[2][kCmpWaves][4];
  __shared__ double sc_sm[2][kCmpWaves][3];
  const int n = A.n, M = A.M;
  unsigned* cnt;   // multiplicity of every original row
  if constexpr (kLds) cnt = cmp_lds;
  else cnt = A.ws + (size_t)blockIdx.x * 3 * (size_t)n;
  unsigned* cp = cnt + n;   // a column's gathered counts, then its cumulative positive multiplicity
  unsigned* cn = cp + n;    // its cumulative negative multiplicity
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int chunk = (n + kCmpThreads - 1) / kCmpThreads;
  const int r0 = min(n, tid * chunk), r1 = min(n, r0 + chunk);
  const double kNan = __longlong_as_double(0x7ff8000000000000ll);

  for (int bb = blockIdx.x; bb < A.nb; bb += gridDim.x) {
    const unsigned long long b = (unsigned long long)(A.b0 + bb);
    for (int i = tid; i < n; i += kCmpThreads) cnt[i] = 0u;
    __syncthreads();
    for (int j = tid; j < n; j += kCmpThreads) {
      const unsigned long long u = cmp_splitmix64(A.seed ^ cmp_splitmix64((b << 40) ^ (unsigned long long)j));
      const bool head = j < A.p0;
      const unsigned long long m = head ? A.p0 : n - A.p0;
      const int r = (int)(((u >> 32) * m) >> 32);
      const int at = (head ? 0 : A.p0) + r;
      atomicAdd(&cnt[A.rowmap ? A.rowmap[at] : at], 1u);
    }
    __syncthreads();

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
        for (int w = 0; w < kCmpWaves; ++w) {
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
      const unsigned char* ys = A.ys + (size_t)m * n;
      const int* gfirst = A.gfirst + (size_t)m * n;
      const int* glast = A.glast + (size_t)m * n;
      for (int i = tid; i < n; i += kCmpThreads) cp[i] = cnt[ord[i]];
      __syncthreads();

      // block-wide inclusive scan of (positive, negative) multiplicities
      unsigned sp = 0, sn = 0;
      for (int i = r0; i < r1; ++i) {
        const unsigned c = cp[i];
        if (ys[i]) sp += c; else sn += c;
      }
      unsigned ip = sp, in = sn;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const unsigned tp = __shfl_up(ip, o, kWave), tn = __shfl_up(in, o, kWave);
        if (lane >= o) { ip += tp; in += tn; }
      }
      if (lane == kWave - 1) { sc_pn[wave][0] = ip; sc_pn[wave][1] = in; }
      __syncthreads();
      unsigned runp = ip - sp, runn = in - sn;
      for (int w = 0; w < wave; ++w) { runp += sc_pn[w][0]; runn += sc_pn[w][1]; }
      for (int i = r0; i < r1; ++i) {
        const unsigned c = cp[i];
        if (ys[i]) runp += c; else runn += c;
        cp[i] = runp;
        cn[i] = runn;
      }
      __syncthreads();

      // tie-group sums: group k ends at position e = glast[e], starts at f = gfirst[e]
      const unsigned Pb = cp[n - 1], Nb = cn[n - 1];
      unsigned long long a2 = 0;
      double apv = 0.0;
      for (int e = r0; e < r1; ++e) {
        if (glast[e] != e) continue;
        const int f = gfirst[e];
        const unsigned tp = cp[e], fp = cn[e];
        const unsigned tp0 = f > 0 ? cp[f - 1] : 0u, fp0 = f > 0 ? cn[f - 1] : 0u;
        a2 += (unsigned long long)(fp - fp0) * (unsigned long long)(tp + tp0);
        if (tp != tp0) apv += (double)((unsigned long long)(tp - tp0) * tp) / (double)(tp + fp);   // product < 2^50: exact
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a2 += __shfl_xor(a2, o, kWave);
      apv = wave_sum(apv);
      if (lane == 0) { sc_a2[wave] = a2; sc_ap[wave] = apv; }
      __syncthreads();
      if (tid == 0) {
        const bool degenerate = Pb == 0u || Nb == 0u;
        unsigned long long A2 = 0;
        double aps = 0.0;
        for (int w = 0; w < kCmpWaves; ++w) { A2 += sc_a2[w]; aps += sc_ap[w]; }
        const size_t at = (size_t)bb * M + m;
        A.a2[at] = (long long)A2;
        if (m == 0) {
          A.pn[2 * (size_t)bb] = Pb;
          A.pn[2 * (size_t)bb + 1] = Nb;
        }
        A.auroc[at] = degenerate ? kNan : (double)A2 / (double)(2ull * Pb * Nb);
        A.ap[at] = degenerate ? kNan : aps / (double)Pb;
        const int k0 = A.k0[m];
        const unsigned tp = k0 > 0 ? cp[k0 - 1] : 0u, fp = k0 > 0 ? cn[k0 - 1] : 0u;
        long long* cf = A.conf + 4 * at;
        cf[0] = tp;
        cf[1] = fp;
        cf[2] = Pb - tp;
        cf[3] = Nb - fp;
      }
      __syncthreads();   // cp and cn are gathered anew for the next column, cnt zeroed for the next replicate
    }
  }
}

void compare_lds_rows(uintptr_t out) { *reinterpret_cast<long long*>(out) = kCmpLdsRows; }

// use_lds: arrays in LDS (n ≤ kCmpLdsRows) or in `ws` = [ws_slices][3n] u32, one slice per workgroup.
// grid ≤ 0 picks one; the results do not depend on it.
void bootstrap_compare(uintptr_t y, uintptr_t rowmap, uintptr_t order, uintptr_t ys, uintptr_t gfirst, uintptr_t glast,
                       uintptr_t k0, uintptr_t hi, uintptr_t p, long long n, long long p0, int M, long long seed,
                       long long b0, long long nb, int use_lds, uintptr_t ws, long long ws_slices, uintptr_t auroc,
                       uintptr_t ap, uintptr_t a2, uintptr_t pn, uintptr_t conf, uintptr_t reclass, uintptr_t sums,
                       int grid, uintptr_t stream) {
  HFENS_REQUIRE(n >= 1 && n <= kCmpMaxN, "bootstrap_compare: 1 <= n <= 2^25");
  HFENS_REQUIRE(M >= 1 && M <= kCmpMaxModels, "bootstrap_compare: 1 <= M <= 8");
  HFENS_REQUIRE(p0 >= 1 && p0 <= n, "bootstrap_compare: first stratum must hold 1..n rows");
  HFENS_REQUIRE(p0 == n || rowmap != 0, "bootstrap_compare: two strata need a row map");
  HFENS_REQUIRE(b0 >= 0 && nb >= 0 && b0 + nb <= kCmpMaxB, "bootstrap_compare: replicates must lie in [0, 2^24]");
  HFENS_REQUIRE(use_lds ? n <= kCmpLdsRows : (ws != 0 && ws_slices >= 1),
                "bootstrap_compare: n exceeds the LDS path / no global workspace");
  if (nb == 0) return;
  int dev = 0, ncu = 256;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t lds = use_lds ? 12 * (size_t)n : 0;
  // at most two 1024-thread workgroups are resident on a CU
  long long cap = use_lds ? (long long)ncu * std::min(2, (int)(kCmpLdsPerCu / (lds + kCmpStatic)))
                          : std::min(2LL * ncu, ws_slices);
  if (grid > 0) cap = use_lds ? grid : std::min((long long)grid, ws_slices);
  grid = (int)std::min(nb, cap);
  CmpArgs A{(const unsigned char*)y, (const int*)rowmap, (const int*)order, (const unsigned char*)ys,
            (const int*)gfirst, (const int*)glast, (const int*)k0, (const unsigned char*)hi, (const double*)p,
            (int)n, (int)p0, M, (unsigned long long)seed, b0, (int)nb, (unsigned*)ws, (double*)auroc, (double*)ap,
            (long long*)a2, (long long*)pn, (long long*)conf, (long long*)reclass, (double*)sums};
  hipStream_t st = as_stream(stream);
  if (use_lds) {
    if (lds > 48 * 1024)
      HFENS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&compare_kernel<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(compare_kernel<true>, dim3(grid), dim3(kCmpThreads), lds, st, A);
  } else {
    hipLaunchKernelGGL(compare_kernel<false>, dim3(grid), dim3(kCmpThreads), 0, st, A);
  }
  launch_check();
}

}  // namespace hfens
