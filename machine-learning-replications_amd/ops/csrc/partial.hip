// Partial dependence and ICE curves of the fused HF stack.
//
//   cell c    = (k1, v1, k2, v2)                                    (k = −1: no substitution in that slot)
//   h(c,r)    = X[r] with column k1 set to v1 and column k2 set to v2
//   ice[r][c] = P(h(c,r))                                           (f32, optional)
//   pd[c]     = (Σ_{r = 0, 1, …, n−1, in that order} (double)ice[r][c]) / (double)n      (f64)
//
// stack_partial evaluates the whole stack on hybrid rows that never exist in HBM; it calls the
// shared tile body of stack_model.h, which stack_infer calls too: same source, and ice equal to
// stack_infer of the hybrid row to about 1 ulp of the f32 probability — not bit-equal, because the
// compiler contracts the meta-LR sum per kernel (three chained FMAs here, an FMA, a packed
// multiply and two adds in stack_infer_kernel).  The structure is that of shapley.hip's
// stack_coalition: one wave owns 64
// consecutive cells, lane ↔ cell c0 + lane.  For each cohort row r (read at a wave-uniform
// address) every lane copies X[r] into its row of the wave's LDS row tile and overwrites at most
// two columns, the wave calls the tile body on the 64 rows, and every lane adds its row's
// probability to its own f64 sum — no cross-lane step and no atomics, so pd is bit-identical from
// run to run and for every grid, and equal to the sequential f64 mean of the ice column.
//
// Tiles are dealt to workgroups round-robin (tile t → workgroup t mod grid), so a few hundred
// cells already spread over as many CUs; the tile loop is block-uniform, so that all waves meet
// the restaging barriers when the SVs exceed LDS.
#include "stack_model.h"

namespace hfens {

constexpr int kPartialMaxF = 64;   // stack_infer's limit

template <int KS, int W, bool X3>
__global__ __launch_bounds__(64 * W) void stack_partial_kernel(const float* __restrict__ X, int n,
                                                                         const int2* __restrict__ feat,
                                                                         const float2* __restrict__ value,
                                                                         long long C, StackModel M, int CH,
                                                                         int nodes_in_lds, double* __restrict__ pd,
                                                                         float* __restrict__ ice) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  StackLds L = stack_lds_view<KS, W, X3>(lds, M, CH, nodes_in_lds);
  stack_stage_model<KS, X3>(M, L);
  int staged = 0;   // SV chunk resident in LDS (block-uniform)
  __syncthreads();
  const int F = M.F, ldx = F | 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xw = L.xs + wave * 64 * ldx;
  float* xl = xw + lane * ldx;                    // this lane's hybrid row
  const long long ntile = (C + 63) / 64;
  const long long stride = (long long)gridDim.x * W;

  // block-uniform tile loop (all waves take part in the restaging barriers when the SVs exceed LDS)
  for (long long base = 0; base < ntile; base += stride) {
    const long long tile = base + (long long)wave * gridDim.x + blockIdx.x;
    const bool valid = tile < ntile;
    if (L.nch == 1 && !valid) continue;              // no barrier below: a wave without a tile sits out
    const long long cell = valid ? tile * 64 + lane : 0;
    const bool live = valid && cell < C;          // waves without a tile and lanes beyond C compute and discard
    int k1 = -1, k2 = -1;
    float v1 = 0.f, v2 = 0.f;
    if (live) {
      const int2 kk = feat[cell];
      const float2 vv = value[cell];
      if (kk.x >= 0 && kk.x < F) { k1 = kk.x; v1 = vv.x; }
      if (kk.y >= 0 && kk.y < F) { k2 = kk.y; v2 = vv.y; }
    }
    double acc = 0.0;
    for (int r = 0; r < n; ++r) {
      // hybrid row of (cell, r) into this lane's row of the wave's LDS tile
      const float* xr0 = X + (size_t)r * F;
#pragma unroll
      for (int k = 0; k < 2 * KS; ++k)
        if (k < F) xl[k] = xr0[k];
      if (k1 >= 0) xl[k1] = v1;
      if (k2 >= 0) xl[k2] = v2;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // SVs beyond LDS: every chunk is restaged for every (tile, cohort row), as in shapley.hip
      const float p = stack_score_tile<KS, X3>(M, L, xw, staged, live);   // lane ↔ hybrid row of its cell
      if (live) {
        if (ice != nullptr) ice[(size_t)r * C + cell] = p;
        acc += (double)p;   // the stored f32, widened
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // xw is rewritten for the next cohort row
    }
    if (live) pd[cell] = acc / (double)n;
  }
}

struct PartialArgs {
  const float* X;
  int n;
  const int2* feat;
  const float2* value;
  long long C;
  double* pd;
  float* ice;
  int grid;
  hipStream_t st;
};

template <int KS, int W, bool X3>
static void partial_go(const PartialArgs& a, const StackModel& M, const StackPlan& p) {
  const int grid = stack_grid(a.grid, (a.C + 63) / 64, p);   // one tile per workgroup until every CU is taken
  hipLaunchKernelGGL((stack_partial_kernel<KS, W, X3>), dim3(grid), dim3(64 * W), p.lds, a.st, a.X, a.n, a.feat,
                     a.value, a.C, M, p.CH, p.in_lds, a.pd, a.ice);
  launch_check();
}

// 8 waves per workgroup; the bf16x3 products (X3) for the narrow shapes while every SV stays
// resident in LDS, else the f32 MFMA path with chunked restaging — stack_infer's defaults.
template <int KS>
static void partial_pick(const PartialArgs& a, const StackModel& M) {
  if constexpr (KS <= 9) {
    const StackPlan q = stack_plan<KS, 8, true>(M, stack_partial_kernel<KS, 8, true>);
    if (q.CH >= M.mp && q.blocks_per_cu > 0) return partial_go<KS, 8, true>(a, M, q);
  }
  const StackPlan p = stack_plan<KS, 8, false>(M, stack_partial_kernel<KS, 8, false>);
  HFENS_REQUIRE(p.CH >= 32 && p.blocks_per_cu > 0, "stack_partial: feature tile does not fit LDS");
  partial_go<KS, 8, false>(a, M, p);
}

void stack_partial(uintptr_t X, long long n, uintptr_t feat, uintptr_t value, long long C, int F, int mp, int T,
                   int K, double ngl2e, double svc_b, double probA, double probB, double gb_init, double gb_lr,
                   double lr_b, double mw0, double mw1, double mw2, double mb, uintptr_t mean,
                   uintptr_t inv_scale, uintptr_t svt, uintptr_t sn, uintptr_t coef, uintptr_t nodes,
                   uintptr_t values, uintptr_t lr_w, uintptr_t st_off, uintptr_t st_pairs, double st_base,
                   uintptr_t pd, uintptr_t ice, int grid, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= kPartialMaxF, "stack_partial: 1 <= F <= 64");
  HFENS_REQUIRE(n >= 1 && n <= 0x7fffffffLL, "stack_partial: at least one cohort row");
  HFENS_REQUIRE(C >= 1, "stack_partial: at least one cell");
  const StackModel M = stack_model("stack_partial", F, mp, T, K, ngl2e, svc_b, probA, probB, gb_init, gb_lr, lr_b,
                                   mw0, mw1, mw2, mb, mean, inv_scale, svt, sn, coef, nodes, values, lr_w,
                                   st_off, st_pairs, st_base);
  const PartialArgs a{(const float*)X, (int)n, (const int2*)feat, (const float2*)value, C,
                      (double*)pd, (float*)ice, grid, as_stream(stream)};
  switch (stack_ks(F)) {
    case 4: partial_pick<4>(a, M); break;
    case 9: partial_pick<9>(a, M); break;
    case 12: partial_pick<12>(a, M); break;
    case 16: partial_pick<16>(a, M); break;
    default: partial_pick<32>(a, M); break;
  }
}

}  // namespace hfens
