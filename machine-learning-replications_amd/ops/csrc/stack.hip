// Fused inference of the whole HF stack (SURVEY.md §2.3 K11 stack_infer; reference
// predict_hf.py:36 → StackingClassifier.predict_proba, semantics SURVEY.md Appendix B) over rows in
// HBM.  The stages and their arithmetic are stack_model.h's; this kernel calls the shared tile
// body and owns only how the rows get there.
//
// One wave owns 64 rows.  Each input row is read from HBM exactly once — prefetched into registers
// one tile ahead, then parked in a per-wave LDS tile that the MFMA operands, the tree walk and
// the LR dot all read — and one f32 probability is written.  For the shipped model that is
// 72 B/row against ~15 kFLOP of MFMA work + 434 exp2/row, i.e. MFMA/transcendental-bound, not
// HBM-bound.  All support vectors (+‖sv‖², coefs) and the tree tables are staged in LDS once per
// workgroup (streamed in chunks when they exceed LDS); the grid is persistent (occupancy-sized).
#include "stack_model.h"

#include <cstdlib>

namespace hfens {

// KS = MFMA k-steps (2 features each); the row tile holds 64·F ≤ 64·2KS values, so each lane
// prefetches at most 2KS of them.
template <int KS, int W, typename TX, bool X3 = false>
__global__ __launch_bounds__(64 * W) void stack_infer_kernel(const TX* __restrict__ X,
                                                                       long long n, StackModel M,
                                                                       int CH, int nodes_in_lds,
                                                                       float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  StackLds L = stack_lds_view<KS, W, X3>(lds, M, CH, nodes_in_lds);
  stack_stage_model<KS, X3>(M, L);
  int staged = 0;   // SV chunk resident in LDS (block-uniform)
  __syncthreads();
  const int F = M.F, ldx = F | 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xw = L.xs + wave * 64 * ldx;
  const long long ntile = (n + 63) / 64;
  const long long stride = (long long)gridDim.x * W;
  const long long nel = n * F;

  // register prefetch of one 64-row tile: element e = lane + 64·i of the tile's flat block
  float pre[2 * KS];
  auto fetch = [&](long long tile) {
    const long long base = tile * 64 * F;
#pragma unroll
    for (int i = 0; i < 2 * KS; ++i) {
      const long long g = base + lane + 64 * i;
      pre[i] = (i < F && tile < ntile && g < nel) ? (float)X[g] : 0.f;
    }
  };
  // block-uniform tile loop (all waves take part in the chunk barriers when the SVs exceed LDS)
  for (long long base = (long long)blockIdx.x * W; base < ntile; base += stride) {
    const long long tile = base + wave;
    const bool valid = tile < ntile;
    const long long row0 = tile * 64;
    if (base == (long long)blockIdx.x * W) fetch(tile);
    // park the prefetched tile in LDS (flat index e ↔ row e/F, col e%F), fetch the next one
#pragma unroll
    for (int i = 0; i < 2 * KS; ++i) {
      if (i < F) {
        const int e = lane + 64 * i;
        const int r = e / F;
        xw[r * ldx + (e - r * F)] = pre[i];
      }
    }
    fetch(tile + stride);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float p = stack_score_tile<KS, X3>(M, L, xw, staged, valid);   // lane ↔ row row0 + lane
    if (valid) {
      if (row0 + lane < n) out[row0 + lane] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // xw is rewritten by the next tile
  }
}

template <int KS, int W, typename TX, bool X3 = false>
static StackPlan infer_plan(const StackModel& M) {
  return stack_plan<KS, W, X3>(M, stack_infer_kernel<KS, W, TX, X3>);
}

template <int KS, int W, typename TX, bool X3 = false>
static void stack_go(const TX* X, long long n, const StackModel& M, const StackPlan& p, int grid,
                     float* out, hipStream_t st) {
  const long long tiles = (n + 63) / 64;
  grid = stack_grid(grid, (tiles + W - 1) / W, p);
  hipLaunchKernelGGL((stack_infer_kernel<KS, W, TX, X3>), dim3(grid), dim3(64 * W), p.lds, st, X, n, M, p.CH,
                     p.in_lds, out);
  launch_check();
}

static int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}

// Pick the workgroup size that keeps the most waves resident per CU: one workgroup shares one
// LDS copy of the SVs, so wider workgroups trade LDS for occupancy.  Only shapes that compile
// without VGPR spills are candidates (KS ≤ 9: 8 or 12 waves; 12 waves fit 152 VGPRs at 3
// waves/SIMD — measured 4.9 G rows/s vs 4.7 for 8); HFENS_STACK_WAVES=8|12|16 forces a shape.
template <int KS, typename TX>
static void stack_pick(const TX* X, long long n, const StackModel& M, int grid, float* out,
                       hipStream_t st) {
  static const int forced = env_int("HFENS_STACK_WAVES", 0);
  constexpr bool narrow = KS <= 9;
  if constexpr (narrow) {
    // X3 (bf16x3 products on the bf16 matrix cores) when every SV stays resident in LDS;
    // HFENS_STACK_X3=0 keeps the f32 MFMA path
    if (env_int("HFENS_STACK_X3", 1) != 0) {
      const int xw = forced == 12 || forced == 8 ? forced : env_int("HFENS_STACK_X3_WAVES", 8);
      if (xw == 12) {
        const StackPlan q = infer_plan<KS, 12, TX, true>(M);
        if (q.CH >= M.mp && q.blocks_per_cu > 0) return stack_go<KS, 12, TX, true>(X, n, M, q, grid, out, st);
      } else {
        const StackPlan q = infer_plan<KS, 8, TX, true>(M);
        if (q.CH >= M.mp && q.blocks_per_cu > 0) return stack_go<KS, 8, TX, true>(X, n, M, q, grid, out, st);
      }
    }
  }
  const StackPlan p8 = infer_plan<KS, 8, TX>(M);
  StackPlan p12, p16;
  if constexpr (narrow) {
    p12 = infer_plan<KS, 12, TX>(M);
    p16 = infer_plan<KS, 16, TX>(M);
  }
  // fewer SV chunks first (restaging costs L2 traffic + barriers), then more resident waves
  auto score = [&](const StackPlan& p, int w) {
    return p.CH ? (long long)(p.CH >= M.mp) * 1000 + w * p.blocks_per_cu : -1LL;
  };
  const long long s8 = score(p8, 8), s12 = narrow ? score(p12, 12) : -1;
  if constexpr (narrow) {
    if (forced == 16 && p16.CH) return stack_go<KS, 16, TX>(X, n, M, p16, grid, out, st);
    if (forced == 12 && p12.CH) return stack_go<KS, 12, TX>(X, n, M, p12, grid, out, st);
  }
  HFENS_REQUIRE(s8 > 0 || s12 > 0, "stack_infer: feature tile does not fit LDS");
  if constexpr (narrow) {
    if (forced != 8 && s12 > s8) return stack_go<KS, 12, TX>(X, n, M, p12, grid, out, st);
  }
  stack_go<KS, 8, TX>(X, n, M, p8, grid, out, st);
}

template <typename TX>
static void stack_launch(const TX* X, long long n, const StackModel& M, int grid, float* out,
                         hipStream_t st) {
  switch (stack_ks(M.F)) {
    case 4: stack_pick<4, TX>(X, n, M, grid, out, st); break;
    case 9: stack_pick<9, TX>(X, n, M, grid, out, st); break;
    case 12: stack_pick<12, TX>(X, n, M, grid, out, st); break;
    case 16: stack_pick<16, TX>(X, n, M, grid, out, st); break;
    default: stack_pick<32, TX>(X, n, M, grid, out, st); break;
  }
}

// Largest SV chunk over the workgroup shapes (== mp ⇔ every SV stays resident in LDS).
long long stack_infer_lds(int F, int mp, int nodes_total) {
  (void)nodes_total;
  return stack_chunk(8, F, mp, stack_ks(F), 0);
}

void stack_infer(uintptr_t X, int x_f64, long long n, int F, int mp, int T, int K, double ngl2e,
                 double svc_b, double probA, double probB, double gb_init, double gb_lr, double lr_b,
                 double mw0, double mw1, double mw2, double mb, uintptr_t mean, uintptr_t inv_scale,
                 uintptr_t svt, uintptr_t sn, uintptr_t coef, uintptr_t nodes, uintptr_t values,
                 uintptr_t lr_w, uintptr_t st_off, uintptr_t st_pairs, double st_base, uintptr_t out,
                 int grid, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= 64, "stack_infer: 1 <= F <= 64");
  const StackModel M = stack_model("stack_infer", F, mp, T, K, ngl2e, svc_b, probA, probB, gb_init, gb_lr, lr_b,
                                   mw0, mw1, mw2, mb, mean, inv_scale, svt, sn, coef, nodes, values, lr_w,
                                   st_off, st_pairs, st_base);
  if (n == 0) return;
  hipStream_t st = as_stream(stream);
  if (x_f64) stack_launch((const double*)X, n, M, grid, (float*)out, st);
  else stack_launch((const float*)X, n, M, grid, (float*)out, st);
}

}  // namespace hfens
