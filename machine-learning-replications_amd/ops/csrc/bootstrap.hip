// Nonparametric bootstrap of held-out AUROC, AP, the confusion counts at one threshold and the
// ROC curve on an FPR grid: one workgroup per replicate, every replicate statistic a scan over
// integer multiplicities of a score order that is sorted once on the host side of the op.
//
//   draw j of replicate b over a stratum of m rows (the law the host mirror and the oracle share):
//     u = splitmix64(seed ^ splitmix64((b << 40) ^ j)),  r = ((u >> 32)·m) >> 32   ∈ [0, m)
//   plain: j ∈ [0, n), m = n, row r.  stratified: j < P draws the r-th positive (m = P), j ≥ P the
//   r-th negative (m = N); `map` turns the drawn row into its position in the descending score
//   order (plain: the inverse sort permutation; stratified: positives' positions, then negatives').
//
// Per replicate: zero the counts → n integer atomicAdds → block-wide inclusive scan of the
// (positive, negative) multiplicities, thread t owning rows [t·chunk, (t+1)·chunk) → tie-group
// sums for the doubled AUROC numerator (u64, exact) and AP (f64) → confusion counts from the
// prefix of rows scoring above the threshold → one binary search per FPR grid point.
// The integer outputs do not depend on any order of summation; AP is folded chunk → wave
// (xor tree) → waves in order, which depends on n alone.  Nothing depends on the grid, on which
// workgroup ran the replicate, or on where the two arrays live:
//   LDS     while 8 B/row fit: kBootLdsRows = 20,000 rows = 160,000 B of the CU's 160 KiB
//           (163,840 B), leaving room for the 384 B of static reduction scratch below;
//   global  above that, workgroup w owns slice w of the caller's workspace (2n u32 per slice).
// No float atomics; results are written with ordinary vector stores.
#include "common.h"

#include <algorithm>

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does this file

namespace hfens {

constexpr int kBootThreads = 1024;
constexpr int kBootWaves = kBootThreads / kWave;
constexpr int kBootLdsRows = 20000;
constexpr long long kBootMaxN = 1LL << 25;   // doubled AUROC numerator < 2^53
constexpr long long kBootMaxB = 1LL << 24;   // replicate index shares the counter with the draw
constexpr int kBootLdsPerCu = 160 * 1024;
constexpr int kBootStatic = 384;             // sc_pn + sc_a2 + sc_ap

__device__ __forceinline__ unsigned long long boot_splitmix64(unsigned long long x) {   // as gbdt.hip
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct BootArgs {
  const unsigned char* y;   // [n] labels in score order
  const int* gfirst;        // [n] first row of the row's tie group
  const int* glast;         // [n] last row of it
  const int* map;           // [n] drawn row → position in score order
  int n, p0, k0, G;         // p0: draws j < p0 take stratum [0, p0), the rest [p0, n)  (plain: p0 = n)
  unsigned long long seed;
  long long b0;
  int nb;
  unsigned* ws;             // global path: [slices][2n]
  double* auroc;
  double* ap;
  long long* a2;
  long long* pn;            // [nb][2]
  long long* conf;          // [nb][4]  TP FP FN TN
  double* tpr;              // [nb][G]
};

template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void bootstrap_kernel(BootArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned boot_lds[];
  __shared__ unsigned sc_pn[kBootWaves][2];
  __shared__ unsigned long long sc_a2[kBootWaves];
  __shared__ double sc_ap[kBootWaves];
  const int n = A.n, G = A.G;
  unsigned* cp;   // counts, then cumulative positive multiplicity
  if constexpr (kLds) cp = boot_lds;
  else cp = A.ws + (size_t)blockIdx.x * 2 * (size_t)n;
  unsigned* cn = cp + n;   // cumulative negative multiplicity
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int chunk = (n + kBootThreads - 1) / kBootThreads;
  const int r0 = min(n, tid * chunk), r1 = min(n, r0 + chunk);
  const double kNan = __longlong_as_double(0x7ff8000000000000ll);

  for (int bb = blockIdx.x; bb < A.nb; bb += gridDim.x) {
    const unsigned long long b = (unsigned long long)(A.b0 + bb);
    for (int i = tid; i < n; i += kBootThreads) cp[i] = 0u;
    __syncthreads();
    for (int j = tid; j < n; j += kBootThreads) {
      const unsigned long long u = boot_splitmix64(A.seed ^ boot_splitmix64((b << 40) ^ (unsigned long long)j));
      const bool head = j < A.p0;
      const unsigned long long m = head ? A.p0 : n - A.p0;
      const int r = (int)(((u >> 32) * m) >> 32);
      atomicAdd(&cp[A.map[(head ? 0 : A.p0) + r]], 1u);
    }
    __syncthreads();

    // block-wide inclusive scan of (positive, negative) multiplicities
    unsigned sp = 0, sn = 0;
    for (int i = r0; i < r1; ++i) {
      const unsigned c = cp[i];
      if (A.y[i]) sp += c; else sn += c;
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
      if (A.y[i]) runp += c; else runn += c;
      cp[i] = runp;
      cn[i] = runn;
    }
    __syncthreads();

    // tie-group sums: group k ends at row e = glast[e], starts at f = gfirst[e]
    const unsigned Pb = cp[n - 1], Nb = cn[n - 1];
    unsigned long long a2 = 0;
    double apv = 0.0;
    for (int e = r0; e < r1; ++e) {
      if (A.glast[e] != e) continue;
      const int f = A.gfirst[e];
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
    const bool degenerate = Pb == 0u || Nb == 0u;
    if (tid == 0) {
      unsigned long long A2 = 0;
      double aps = 0.0;
      for (int w = 0; w < kBootWaves; ++w) { A2 += sc_a2[w]; aps += sc_ap[w]; }
      A.a2[bb] = (long long)A2;
      A.pn[2 * (size_t)bb] = Pb;
      A.pn[2 * (size_t)bb + 1] = Nb;
      A.auroc[bb] = degenerate ? kNan : (double)A2 / (double)(2ull * Pb * Nb);
      A.ap[bb] = degenerate ? kNan : aps / (double)Pb;
      const unsigned tp = A.k0 > 0 ? cp[A.k0 - 1] : 0u, fp = A.k0 > 0 ? cn[A.k0 - 1] : 0u;
      long long* cf = A.conf + 4 * (size_t)bb;
      cf[0] = tp;
      cf[1] = fp;
      cf[2] = Pb - tp;
      cf[3] = Nb - fp;
    }

    // TPR at FPR = g/(G−1): vertices are (0, 0) and the tie-group ends; cn is monotone over rows
    const unsigned long long G1 = (unsigned long long)(G - 1);
    for (int g = tid; g < G; g += kBootThreads) {
      double out = kNan;
      if (!degenerate) {
        const unsigned long long bound = (unsigned long long)g * Nb;
        int lo = -1, hi = n - 1;   // rows ≤ lo satisfy cn·(G−1) ≤ bound, rows > hi do not
        while (lo < hi) {
          const int mid = lo + (hi - lo + 1) / 2;
          if ((unsigned long long)cn[mid] * G1 <= bound) lo = mid; else hi = mid - 1;
        }
        int e = lo;
        if (e >= 0 && A.glast[e] != e) e = A.gfirst[e] - 1;   // its group's end fails: step back a vertex
        const unsigned tpk = e >= 0 ? cp[e] : 0u, fpk = e >= 0 ? cn[e] : 0u;
        if (e == n - 1 || (unsigned long long)fpk * G1 == bound) {
          out = (double)tpk / (double)Pb;
        } else {
          const int e1 = A.glast[e + 1];   // next vertex fails the test, so fp1 > fpk
          const unsigned tp1 = cp[e1], fp1 = cn[e1];
          const unsigned long long num = bound - (unsigned long long)fpk * G1;
          const unsigned long long den = G1 * (unsigned long long)(fp1 - fpk);
          const double frac = (double)num / (double)den;
          out = ((double)tpk + (double)(tp1 - tpk) * frac) / (double)Pb;
        }
      }
      A.tpr[(size_t)bb * G + g] = out;
    }
    __syncthreads();   // the arrays are zeroed for the next replicate
  }
}

void bootstrap_lds_rows(uintptr_t out) { *reinterpret_cast<long long*>(out) = kBootLdsRows; }

// use_lds: arrays in LDS (n ≤ kBootLdsRows) or in `ws` = [ws_slices][2n] u32, one slice per workgroup.
// grid ≤ 0 picks one; the results do not depend on it.
void bootstrap_metrics(uintptr_t y, uintptr_t gfirst, uintptr_t glast, uintptr_t map, long long n, long long p0,
                       long long k0, int G, long long seed, long long b0, long long nb, int use_lds, uintptr_t ws,
                       long long ws_slices, uintptr_t auroc, uintptr_t ap, uintptr_t a2, uintptr_t pn,
                       uintptr_t conf, uintptr_t tpr, int grid, uintptr_t stream) {
  HFENS_REQUIRE(n >= 1 && n <= kBootMaxN, "bootstrap_metrics: 1 <= n <= 2^25");
  HFENS_REQUIRE(p0 >= 1 && p0 <= n, "bootstrap_metrics: first stratum must hold 1..n rows");
  HFENS_REQUIRE(k0 >= 0 && k0 <= n, "bootstrap_metrics: threshold prefix out of range");
  HFENS_REQUIRE(G >= 2 && G <= 65536, "bootstrap_metrics: 2 <= grid_points <= 65536");
  HFENS_REQUIRE(b0 >= 0 && nb >= 0 && b0 + nb <= kBootMaxB, "bootstrap_metrics: replicates must lie in [0, 2^24]");
  HFENS_REQUIRE(use_lds ? n <= kBootLdsRows : (ws != 0 && ws_slices >= 1),
                "bootstrap_metrics: n exceeds the LDS path / no global workspace");
  if (nb == 0) return;
  int dev = 0, ncu = 256;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t lds = use_lds ? 8 * (size_t)n : 0;
  // at most two 1024-thread workgroups are resident on a CU
  long long cap = use_lds ? (long long)ncu * std::min(2, (int)(kBootLdsPerCu / (lds + kBootStatic)))
                          : std::min(2LL * ncu, ws_slices);
  if (grid > 0) cap = use_lds ? grid : std::min((long long)grid, ws_slices);
  grid = (int)std::min(nb, cap);
  BootArgs A{(const unsigned char*)y, (const int*)gfirst, (const int*)glast, (const int*)map, (int)n, (int)p0,
             (int)k0, G, (unsigned long long)seed, b0, (int)nb, (unsigned*)ws, (double*)auroc, (double*)ap,
             (long long*)a2, (long long*)pn, (long long*)conf, (double*)tpr};
  hipStream_t st = as_stream(stream);
  if (use_lds) {
    if (lds > 48 * 1024)
      HFENS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&bootstrap_kernel<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bootstrap_kernel<true>, dim3(grid), dim3(kBootThreads), lds, st, A);
  } else {
    hipLaunchKernelGGL(bootstrap_kernel<false>, dim3(grid), dim3(kBootThreads), 0, st, A);
  }
  launch_check();
}

}  // namespace hfens
