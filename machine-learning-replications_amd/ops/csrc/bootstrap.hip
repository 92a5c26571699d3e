// Nonparametric bootstrap of held-out AUROC, AP, the confusion counts at one threshold and the
// ROC curve on an FPR grid: one workgroup per replicate, every replicate statistic a scan over
// integer multiplicities of a score order that is sorted once on the host side of the op.
//
// The resampling law is that of resample.h; `map` turns the drawn row into its position in the
// descending score order (plain: the inverse sort permutation; stratified: positives' positions,
// then negatives').
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
#include "resample.h"

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does this file

namespace hfens {

constexpr int kBootLdsRows = 20000;
constexpr int kBootStatic = 384;             // sc_pn + sc_a2 + sc_ap

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
  const BootThread t = boot_thread(n);

  for (int bb = blockIdx.x; bb < A.nb; bb += gridDim.x) {
    boot_draw(cp, A.map, n, A.p0, A.seed, (unsigned long long)(A.b0 + bb));
    boot_scan(cp, cn, A.y, t, sc_pn, [](int, unsigned, bool) {});
    __syncthreads();
    const unsigned Pb = cp[n - 1], Nb = cn[n - 1];
    boot_rank_stats(cp, cn, A.gfirst, A.glast, t, Pb, Nb, A.k0, sc_a2, sc_ap, A.a2 + bb, A.pn + 2 * (size_t)bb,
                    A.auroc + bb, A.ap + bb, A.conf + 4 * (size_t)bb);

    // TPR at FPR = g/(G−1): vertices are (0, 0) and the tie-group ends; cn is monotone over rows
    const bool degenerate = Pb == 0u || Nb == 0u;
    const unsigned long long G1 = (unsigned long long)(G - 1);
    for (int g = t.tid; g < G; g += kBootThreads) {
      double out = boot_nan();
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

// use_lds, ws, ws_slices and grid: see boot_launch (2 u32 arrays per row)
void bootstrap_metrics(uintptr_t y, uintptr_t gfirst, uintptr_t glast, uintptr_t map, long long n, long long p0,
                       long long k0, int G, long long seed, long long b0, long long nb, int use_lds, uintptr_t ws,
                       long long ws_slices, uintptr_t auroc, uintptr_t ap, uintptr_t a2, uintptr_t pn,
                       uintptr_t conf, uintptr_t tpr, int grid, uintptr_t stream) {
  HFENS_REQUIRE(k0 >= 0 && k0 <= n, "bootstrap_metrics: threshold prefix out of range");
  HFENS_REQUIRE(G >= 2 && G <= 65536, "bootstrap_metrics: 2 <= grid_points <= 65536");
  BootArgs A{(const unsigned char*)y, (const int*)gfirst, (const int*)glast, (const int*)map, (int)n, (int)p0,
             (int)k0, G, (unsigned long long)seed, b0, (int)nb, (unsigned*)ws, (double*)auroc, (double*)ap,
             (long long*)a2, (long long*)pn, (long long*)conf, (double*)tpr};
  boot_launch("bootstrap_metrics", bootstrap_kernel<true>, bootstrap_kernel<false>, A, 2, kBootLdsRows,
              kBootStatic, n, p0, b0, nb, use_lds, ws, ws_slices, grid, stream);
}

}  // namespace hfens
