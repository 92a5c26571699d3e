// Permutation importance of the fused HF stack on held-out rows: two kernels.
//
//   score row j = (kf, r):  k = feat[kf]  (−1: no substitution — the baseline row)
//   h(j, i)  = X[i] with column k replaced by X[src[r][i]][k]          (src[r]: a permutation of the rows)
//   S[j][i]  = P(h(j, i))                                              (f32)
//
// stack_permute evaluates the whole stack on hybrid rows that never exist in HBM; it calls the shared
// tile body of stack_model.h.  Every hybrid row is independent, so the kernel is lane ↔ hybrid row, as
// stack_infer is (and not lane ↔ cell, which left partial.hip with a handful of waves): tiles of 64
// consecutive flat indices j·n + i are dealt to workgroups round-robin, each lane copies X[i] into its
// row of the wave's LDS tile, overwrites column k with the gathered value (a 4-byte read from the
// column-major copy Xt, which stays in L2; src is read coalesced) and keeps its row's probability.
// No atomics and no cross-lane step: S is bit-identical for every grid.  The baseline comes from this
// kernel too (k = −1), so a column whose permutation changes no value has importance exactly 0 (the
// compiler contracts the meta-LR sum per kernel: see partial.hip).
//
// rank_rows ranks every score row against the labels: one 1024-thread workgroup per row,
//   a2    = Σ over tie groups (negatives in the group)·(positives above it + positives through it)   (int64, exact)
//   auroc = a2 / (2·P·N)                                                                             (one f64 division)
//   ap    = resample.h's formula and fold (chunk → wave → waves)
//   brier = (Σ_i ((double)S[j][i] − y_i)²) / n, in original row order, folded chunk → wave → waves
// with unit multiplicities through resample.h's scan and rank statistics; the tie groups are read off
// the sorted keys.  The row is sorted in the kernel while 13 B/row fit LDS (kRankLdsRows): a bitonic
// network over a monotone u32 image of the score (descending; −0 = +0) with the label carried along,
// all comparators pointing the same way (merge size k: first i ↔ its mirror in the block, then i ↔ i + j
// for j = k/4 … 1), so that the padding to a power of two is virtual: a comparator whose upper end
// is ≥ n is skipped.  Consecutive threads take consecutive i within a run of j, so the strides that
// alias banks are j = 1 and 2 only (2-way).  Above the limit the caller sorts (scores and labels in
// score order, in global memory) and the same kernel skips the sort and keeps its two u32 arrays in
// the caller's workspace, one slice per workgroup.  AUROC and AP depend on the tie-group sums and the
// group ends only, not on the order inside a tie, so the paths agree.
#include "stack_model.h"   // ahead of resample.h: the tile body keeps the contraction it has in the other stack ops
#include "resample.h"

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does this file

namespace hfens {

constexpr int kPermuteMaxF = 64;   // stack_infer's limit

template <int KS, int W, bool X3>
__global__ __launch_bounds__(64 * W) void stack_permute_kernel(const float* __restrict__ X,
                                                                         const float* __restrict__ Xt, int n,
                                                                         const int* __restrict__ src, int R,
                                                                         const int* __restrict__ feat,
                                                                         long long total, StackModel M, int CH,
                                                                         int nodes_in_lds, float* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  StackLds L = stack_lds_view<KS, W, X3>(lds, M, CH, nodes_in_lds);
  stack_stage_model<KS, X3>(M, L);
  int staged = 0;   // SV chunk resident in LDS (block-uniform)
  __syncthreads();
  const int F = M.F, ldx = F | 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xw = L.xs + wave * 64 * ldx;
  float* xl = xw + lane * ldx;                    // this lane's hybrid row
  const long long ntile = (total + 63) / 64;
  const long long stride = (long long)gridDim.x * W;

  // block-uniform tile loop (all waves take part in the restaging barriers when the SVs exceed LDS)
  for (long long base = 0; base < ntile; base += stride) {
    const long long tile = base + (long long)wave * gridDim.x + blockIdx.x;
    const bool valid = tile < ntile;
    if (L.nch == 1 && !valid) continue;              // no barrier below: a wave without a tile sits out
    const long long flat = valid ? tile * 64 + lane : 0;
    const bool live = valid && flat < total;      // waves without a tile and lanes beyond the end compute row 0 and discard
    int i = 0, k = -1, s = 0;
    if (live) {
      const unsigned fl = (unsigned)flat;         // total < 2^31 (host check)
      const unsigned j = fl / (unsigned)n;
      i = (int)(fl - j * (unsigned)n);
      const unsigned kf = j / (unsigned)R, r = j - kf * (unsigned)R;
      const int kk = feat[kf];
      if (kk >= 0 && kk < F) {
        k = kk;
        s = src[(size_t)r * n + i];
      }
    }
    const float* xr0 = X + (size_t)i * F;
#pragma unroll
    for (int c = 0; c < 2 * KS; ++c)
      if (c < F) xl[c] = xr0[c];
    if (k >= 0 && (unsigned)s < (unsigned)n) xl[k] = Xt[(size_t)k * n + s];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float p = stack_score_tile<KS, X3>(M, L, xw, staged, live);   // lane ↔ its hybrid row
    if (live) S[flat] = p;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // xw is rewritten by the next tile
  }
}

struct PermuteArgs {
  const float* X;
  const float* Xt;
  int n;
  const int* src;
  int R;
  const int* feat;
  long long total;
  float* S;
  int grid;
  hipStream_t st;
};

template <int KS, int W, bool X3>
static void permute_go(const PermuteArgs& a, const StackModel& M, const StackPlan& p) {
  const int grid = stack_grid(a.grid, (a.total + 63) / 64, p);   // one tile per workgroup until every CU is taken
  hipLaunchKernelGGL((stack_permute_kernel<KS, W, X3>), dim3(grid), dim3(64 * W), p.lds, a.st, a.X, a.Xt, a.n,
                     a.src, a.R, a.feat, a.total, M, p.CH, p.in_lds, a.S);
  launch_check();
}

// 8 waves per workgroup; the bf16x3 products (X3) for the narrow shapes while every SV stays
// resident in LDS, else the f32 MFMA path with chunked restaging — stack_infer's defaults.
template <int KS>
static void permute_pick(const PermuteArgs& a, const StackModel& M) {
  if constexpr (KS <= 9) {
    const StackPlan q = stack_plan<KS, 8, true>(M, stack_permute_kernel<KS, 8, true>);
    if (q.CH >= M.mp && q.blocks_per_cu > 0) return permute_go<KS, 8, true>(a, M, q);
  }
  const StackPlan p = stack_plan<KS, 8, false>(M, stack_permute_kernel<KS, 8, false>);
  HFENS_REQUIRE(p.CH >= 32 && p.blocks_per_cu > 0, "stack_permute: feature tile does not fit LDS");
  permute_go<KS, 8, false>(a, M, p);
}

// X [n][F] and its column-major copy Xt [F][n] (f32), src [R][n] (int32, values in [0, n)),
// feat [K] (int32, −1 or a column), S [K][R][n] (f32)
void stack_permute(uintptr_t X, uintptr_t Xt, long long n, uintptr_t src, long long R, uintptr_t feat, long long K,
                   int F, int mp, int T, int Kn, double ngl2e, double svc_b, double probA, double probB,
                   double gb_init, double gb_lr, double lr_b, double mw0, double mw1, double mw2, double mb,
                   uintptr_t mean, uintptr_t inv_scale, uintptr_t svt, uintptr_t sn, uintptr_t coef,
                   uintptr_t nodes, uintptr_t values, uintptr_t lr_w, uintptr_t st_off, uintptr_t st_pairs,
                   double st_base, uintptr_t S, int grid, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= kPermuteMaxF, "stack_permute: 1 <= F <= 64");
  HFENS_REQUIRE(n >= 1 && R >= 1 && K >= 1, "stack_permute: at least one row, one repeat and one column");
  HFENS_REQUIRE(n <= 0x7fffffffLL && R <= 0x7fffffffLL && K <= 0x7fffffffLL &&
                    (double)n * (double)R * (double)K <= 2147483647.0,
                "stack_permute: K*R*n must stay below 2^31 (chunk the score rows)");
  const StackModel M = stack_model("stack_permute", F, mp, T, Kn, ngl2e, svc_b, probA, probB, gb_init, gb_lr, lr_b,
                                   mw0, mw1, mw2, mb, mean, inv_scale, svt, sn, coef, nodes, values, lr_w,
                                   st_off, st_pairs, st_base);
  const PermuteArgs a{(const float*)X, (const float*)Xt, (int)n, (const int*)src, (int)R, (const int*)feat,
                      n * R * K, (float*)S, grid, as_stream(stream)};
  switch (stack_ks(F)) {
    case 4: permute_pick<4>(a, M); break;
    case 9: permute_pick<9>(a, M); break;
    case 12: permute_pick<12>(a, M); break;
    case 16: permute_pick<16>(a, M); break;
    default: permute_pick<32>(a, M); break;
  }
}

// ---- rank_rows ------------------------------------------------------------------------------------
// LDS per row: key 4 B + cumulative positives 4 B + cumulative negatives 4 B + label 1 B = 13 B;
// 12,500 rows = 162,500 B of the CU's 160 KiB (163,840 B) beside the 544 B of static scratch below.
constexpr int kRankLdsRows = 12500;
constexpr int kRankStatic = 544;   // sc_pn + sc_a2 + sc_ap + sc_br + sc_conf

struct RankArgs {
  const float* S;             // [M][n] scores in original row order
  const unsigned char* y;     // [n] labels in original row order
  const float* ss;            // global path: [M][n] scores sorted descending
  const unsigned char* ys;    // global path: [M][n] labels in that order
  unsigned* ws;               // global path: [slices][2n]
  int n, M;
  long long* a2;
  double* auroc;
  double* ap;
  double* brier;
};

// u32 image of a finite f32 that ascends as the score descends; −0 and +0 share one image
__device__ __forceinline__ unsigned rank_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void rank_rows_kernel(RankArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned rank_lds[];
  __shared__ unsigned sc_pn[kBootWaves][2];
  __shared__ unsigned long long sc_a2[kBootWaves];
  __shared__ double sc_ap[kBootWaves];
  __shared__ double sc_br[kBootWaves];
  __shared__ long long sc_conf[4];
  const int n = A.n;
  unsigned* key = rank_lds;   // LDS path only
  unsigned* cp;               // cumulative positives
  if constexpr (kLds) cp = rank_lds + n;
  else cp = A.ws + (size_t)blockIdx.x * 2 * (size_t)n;
  unsigned* cn = cp + n;      // cumulative negatives
  unsigned char* yl = reinterpret_cast<unsigned char*>(rank_lds + 3 * (size_t)n);   // LDS path only
  const BootThread t = boot_thread(n);
  int npow = 1;
  while (npow < n) npow <<= 1;

  for (int j = blockIdx.x; j < A.M; j += gridDim.x) {
    const float* s = A.S + (size_t)j * n;
    double br = 0.0;
    for (int i = t.r0; i < t.r1; ++i) {
      const double d = (double)s[i] - (double)A.y[i];
      br += d * d;
    }
    br = wave_sum(br);
    if (t.lane == 0) sc_br[t.wave] = br;

    const float* ss = nullptr;
    const unsigned char* yo;
    if constexpr (kLds) {
      for (int i = t.tid; i < n; i += kBootThreads) {
        key[i] = rank_key(s[i]);
        yl[i] = A.y[i];
      }
      __syncthreads();
      auto cmpx = [&](int i, int p) {   // i < p: the smaller key to i; p beyond n is the virtual padding
        if (p < n) {
          const unsigned a = key[i], b = key[p];
          if (a > b) {
            key[i] = b;
            key[p] = a;
            const unsigned char ya = yl[i];
            yl[i] = yl[p];
            yl[p] = ya;
          }
        }
      };
      for (int k = 2; k <= npow; k <<= 1) {
        const int hk = k >> 1;
        for (int q = t.tid; q < (npow >> 1); q += kBootThreads) {
          const int off = q & (hk - 1), b0 = (q - off) << 1;   // block start = (q / hk)·k
          cmpx(b0 + off, b0 + k - 1 - off);
        }
        __syncthreads();
        for (int jj = k >> 2; jj > 0; jj >>= 1) {
          for (int q = t.tid; q < (npow >> 1); q += kBootThreads) {
            const int off = q & (jj - 1), i = ((q - off) << 1) + off;
            cmpx(i, i + jj);
          }
          __syncthreads();
        }
      }
      yo = yl;
    } else {
      ss = A.ss + (size_t)j * n;
      yo = A.ys + (size_t)j * n;
    }
    auto keyat = [&](int e) -> unsigned {
      if constexpr (kLds) return key[e];
      else return rank_key(ss[e]);
    };

    for (int i = t.r0; i < t.r1; ++i) cp[i] = 1u;   // unit multiplicities; the scan reads the thread's own rows
    boot_scan(cp, cn, yo, t, sc_pn, [](int, unsigned, bool) {});
    __syncthreads();
    const unsigned Pb = cp[n - 1], Nb = cn[n - 1];

    // the tie groups off the sorted keys: the first row of the group that is open at the thread's
    // first row by bisection, every later one as the walk meets it
    int f = t.r0;
    if (t.r0 < t.r1 && t.r0 > 0) {
      const unsigned k0 = keyat(t.r0);
      if (keyat(t.r0 - 1) == k0) {
        int lo = 0, hi = t.r0 - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (keyat(mid) < k0) lo = mid + 1; else hi = mid;
        }
        f = lo;
      }
    }
    const int r0 = t.r0;
    boot_rank_stats(cp, cn, [&](int e, int& fo) {
      const unsigned ke = keyat(e);
      if (e > r0 && keyat(e - 1) != ke) f = e;
      fo = f;
      return e == n - 1 || keyat(e + 1) != ke;
    }, t, Pb, Nb, 0, sc_a2, sc_ap, A.a2 + j, nullptr, A.auroc + j, A.ap + j, sc_conf);
    if (t.tid == 0) {   // after the barrier inside boot_rank_stats
      double b = 0.0;
      for (int w = 0; w < kBootWaves; ++w) b += sc_br[w];
      A.brier[j] = b / (double)n;
    }
    __syncthreads();   // the arrays and the scratch are reused by the next row
  }
}

void rank_lds_rows(uintptr_t out) { *reinterpret_cast<long long*>(out) = kRankLdsRows; }

// use_lds: the row is sorted in LDS (n ≤ kRankLdsRows); else ss, ys hold the rows presorted and
// ws = [ws_slices][2n] u32, one slice per workgroup.  grid ≤ 0 picks one; the results do not depend on it.
void rank_rows(uintptr_t S, uintptr_t y, uintptr_t ss, uintptr_t ys, long long n, long long M, int use_lds,
               uintptr_t ws, long long ws_slices, uintptr_t a2, uintptr_t auroc, uintptr_t ap, uintptr_t brier,
               int grid, uintptr_t stream) {
  HFENS_REQUIRE(n >= 1 && n <= kBootMaxN, "rank_rows: 1 <= n <= 2^25");
  HFENS_REQUIRE(M >= 0 && M <= 0x7fffffffLL, "rank_rows: bad number of score rows");
  HFENS_REQUIRE(use_lds ? n <= kRankLdsRows : (ss != 0 && ys != 0 && ws != 0 && ws_slices >= 1),
                "rank_rows: n exceeds the LDS path / no presorted rows or global workspace");
  if (M == 0) return;
  int dev = 0, ncu = 256;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t lds = use_lds ? 12 * (size_t)n + (((size_t)n + 3) & ~(size_t)3) : 0;
  // at most two 1024-thread workgroups are resident on a CU
  long long cap = use_lds ? (long long)ncu * std::min(2, (int)(kBootLdsPerCu / (lds + kRankStatic)))
                          : std::min(2LL * ncu, ws_slices);
  if (grid > 0) cap = use_lds ? grid : std::min((long long)grid, ws_slices);
  grid = (int)std::min(M, cap);
  RankArgs A{(const float*)S, (const unsigned char*)y, (const float*)ss, (const unsigned char*)ys, (unsigned*)ws,
             (int)n, (int)M, (long long*)a2, (double*)auroc, (double*)ap, (double*)brier};
  hipStream_t st = as_stream(stream);
  if (use_lds) {
    if (lds > 48 * 1024)
      HFENS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(rank_rows_kernel<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(rank_rows_kernel<true>, dim3(grid), dim3(kBootThreads), lds, st, A);
  } else {
    hipLaunchKernelGGL(rank_rows_kernel<false>, dim3(grid), dim3(kBootThreads), 0, st, A);
  }
  launch_check();
}

}  // namespace hfens
