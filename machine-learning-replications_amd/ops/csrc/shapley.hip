// Exact interventional Shapley values of the fused HF stack.
//
//   h(S,b)[k] = x[k] if bit k of S is set, else bg[b][k]          (hybrid row of coalition S)
//   v[p][S]   = (1/B)·Σ_b P(h(S,b))                                (stack_coalition, f64)
//   φ[p][k]   = Σ_S c_k(S)·v[p][S],  c_k(S) = w(|S|−1) if k ∈ S else −w(|S|)   (shapley_reduce, f64)
//   Φ[p][i][j] = Σ_S c_ij(S)·v[p][S]                                (shapley_interactions, f64; below)
//
// stack_coalition evaluates the whole stack on hybrid rows that never exist in HBM; it calls the
// shared tile body of stack_model.h, which stack_infer calls too, so P is the same function of a
// row in both.  One wave owns 64 consecutive coalitions of one patient: lane ↔ coalition
// S0 + lane.  For each background row b it builds its 64 hybrid rows in its LDS row tile by bit
// select from the patient row (held in registers) and bg[b], calls the tile body on them, and
// every lane adds its row's probability to an f64 sum — b = 0, 1, …, B−1 in that order,
// no cross-lane step and no atomics, so v is bit-identical from run to run and for every grid.
// The 2^F·B·F hybrid matrix is neither written nor read; one f64 per coalition is stored.
#include "stack_model.h"

namespace hfens {

constexpr int kShapMaxF = 20;   // v is 8 MB per patient at F = 20

template <int KS, int W, bool X3>
__global__ __launch_bounds__(64 * W) void stack_coalition_kernel(const float* __restrict__ X, long long n,
                                                                           const float* __restrict__ BG, int B,
                                                                           StackModel M, int CH, int nodes_in_lds,
                                                                           double* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  StackLds L = stack_lds_view<KS, W, X3>(lds, M, CH, nodes_in_lds);
  stack_stage_model<KS, X3>(M, L);
  int staged = 0;   // SV chunk resident in LDS (block-uniform)
  __syncthreads();
  const int F = M.F, ldx = F | 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xw = L.xs + wave * 64 * ldx;
  const long long nS = 1LL << F;
  const long long tps = (nS + 63) / 64;           // 64-coalition tiles per patient
  const long long nitem = n * tps;
  const long long stride = (long long)gridDim.x * W;

  // block-uniform item loop (all waves take part in the restaging barriers when the SVs exceed LDS)
  for (long long base = (long long)blockIdx.x * W; base < nitem; base += stride) {
    const long long item = base + wave;
    const bool valid = item < nitem;
    const long long p = valid ? item / tps : 0;
    const long long S = valid ? (item - p * tps) * 64 + lane : 0;   // this lane's coalition
    const unsigned bits = (unsigned)S;
    float xp[2 * KS];                              // the patient's row
#pragma unroll
    for (int k = 0; k < 2 * KS; ++k) xp[k] = k < F ? X[p * F + k] : 0.f;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
      // hybrid row of (S, b) into this lane's row of the wave's LDS tile
      const float* bg = BG + (size_t)b * F;
#pragma unroll
      for (int k = 0; k < 2 * KS; ++k)
        if (k < F) xw[lane * ldx + k] = (bits >> k) & 1u ? xp[k] : bg[k];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // SVs beyond LDS: every chunk is restaged for every (item, background row) — B times
      // stack_infer's restaging traffic per tile.  Correct but slow; a chunk loop outside the
      // background loop would need the B partial decision sums of a tile kept per lane.
      const float ph = stack_score_tile<KS, X3>(M, L, xw, staged, valid);   // lane ↔ hybrid row of S
      if (valid) acc += (double)ph;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // xw is rewritten for the next background row
    }
    if (valid && S < nS) v[p * nS + S] = acc / (double)B;
  }
}

template <int KS, int W, bool X3>
static void coalition_go(const float* X, long long n, const float* BG, int B, const StackModel& M,
                         const StackPlan& p, int grid, double* v, hipStream_t st) {
  const long long items = n * (((1LL << M.F) + 63) / 64);
  grid = stack_grid(grid, (items + W - 1) / W, p);
  hipLaunchKernelGGL((stack_coalition_kernel<KS, W, X3>), dim3(grid), dim3(64 * W), p.lds, st, X, n, BG, B, M,
                     p.CH, p.in_lds, v);
  launch_check();
}

// 8 waves per workgroup; the bf16x3 products (X3) for the narrow shapes while every SV stays
// resident in LDS, else the f32 MFMA path with chunked restaging — stack_infer's defaults.
template <int KS>
static void coalition_pick(const float* X, long long n, const float* BG, int B, const StackModel& M, int grid,
                           double* v, hipStream_t st) {
  if constexpr (KS <= 9) {
    const StackPlan q = stack_plan<KS, 8, true>(M, stack_coalition_kernel<KS, 8, true>);
    if (q.CH >= M.mp && q.blocks_per_cu > 0) return coalition_go<KS, 8, true>(X, n, BG, B, M, q, grid, v, st);
  }
  const StackPlan p = stack_plan<KS, 8, false>(M, stack_coalition_kernel<KS, 8, false>);
  HFENS_REQUIRE(p.CH >= 32 && p.blocks_per_cu > 0, "stack_coalition: feature tile does not fit LDS");
  coalition_go<KS, 8, false>(X, n, BG, B, M, p, grid, v, st);
}

void stack_coalition(uintptr_t X, long long n, uintptr_t BG, long long B, int F, int mp, int T, int K,
                     double ngl2e, double svc_b, double probA, double probB, double gb_init, double gb_lr,
                     double lr_b, double mw0, double mw1, double mw2, double mb, uintptr_t mean,
                     uintptr_t inv_scale, uintptr_t svt, uintptr_t sn, uintptr_t coef, uintptr_t nodes,
                     uintptr_t values, uintptr_t lr_w, uintptr_t st_off, uintptr_t st_pairs, double st_base,
                     uintptr_t v, int grid, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= kShapMaxF, "stack_coalition: 1 <= F <= 20");
  HFENS_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "stack_coalition: at least one background row");
  const StackModel M = stack_model("stack_coalition", F, mp, T, K, ngl2e, svc_b, probA, probB, gb_init, gb_lr,
                                   lr_b, mw0, mw1, mw2, mb, mean, inv_scale, svt, sn, coef, nodes, values, lr_w,
                                   st_off, st_pairs, st_base);
  if (n == 0) return;
  hipStream_t st = as_stream(stream);
  const float* x = (const float*)X;
  const float* bg = (const float*)BG;
  switch (stack_ks(F)) {
    case 4: coalition_pick<4>(x, n, bg, (int)B, M, grid, (double*)v, st); break;
    case 9: coalition_pick<9>(x, n, bg, (int)B, M, grid, (double*)v, st); break;
    default: coalition_pick<12>(x, n, bg, (int)B, M, grid, (double*)v, st); break;   // F ≤ 20 ⇒ KS ≤ 12
  }
}

// φ[p][k] = Σ_S c_k(S)·v[p][S] in f64, one workgroup per patient: thread t sums coalitions t,
// t + 256, … in that order, then thread k folds the 256 partials of feature k in thread order —
// fixed order throughout, so φ is bit-identical from run to run.  w[s] = s!(F−s−1)!/F!, s < F.
__global__ __launch_bounds__(256) void shapley_reduce_kernel(const double* __restrict__ v, int F,
                                                             const double* __restrict__ w,
                                                             double* __restrict__ phi) {
  __shared__ double sh[256][kShapMaxF + 1];
  __shared__ double wl[kShapMaxF + 1];
  const int t = threadIdx.x;
  const long long nS = 1LL << F;
  const double* vp = v + (size_t)blockIdx.x * nS;
  if (t <= F) wl[t] = t < F ? w[t] : 0.0;
  __syncthreads();
  double acc[kShapMaxF];
#pragma unroll
  for (int k = 0; k < kShapMaxF; ++k) acc[k] = 0.0;
  for (long long S = t; S < nS; S += 256) {
    const unsigned bits = (unsigned)S;
    const int s = __popc(bits);
    const double vS = vp[S];
    const double in = s > 0 ? wl[s - 1] * vS : 0.0;   // k ∈ S:  w(|S|−1)·v(S)
    const double out = -(wl[s] * vS);                 // k ∉ S: −w(|S|)·v(S)   (wl[F] = 0)
#pragma unroll
    for (int k = 0; k < kShapMaxF; ++k)
      if (k < F) acc[k] += (bits >> k) & 1u ? in : out;
  }
#pragma unroll
  for (int k = 0; k < kShapMaxF; ++k)
    if (k < F) sh[t][k] = acc[k];
  __syncthreads();
  if (t < F) {
    double s = 0.0;
    for (int tt = 0; tt < 256; ++tt) s += sh[tt][t];
    phi[(size_t)blockIdx.x * F + t] = s;
  }
}

void shapley_reduce(uintptr_t v, long long n, int F, uintptr_t w, uintptr_t phi, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= kShapMaxF, "shapley_reduce: 1 <= F <= 20");
  if (n == 0) return;
  hipLaunchKernelGGL(shapley_reduce_kernel, dim3((unsigned)n), dim3(256), 0, as_stream(stream),
                     (const double*)v, F, (const double*)w, (double*)phi);
  launch_check();
}

// Shapley interaction values from the same table: for i < j
//   Φ[p][i][j] = Φ[p][j][i] = Σ_T c_ij(T)·v[p][T],
//   c_ij(T) = u(|T|−2) if both i, j ∈ T, −u(|T|−1) if exactly one is, u(|T|) if neither,
//   u(s) = s!(F−s−2)!/(2(F−1)!), s ≤ F−2,
// and Φ[p][i][i] = φ[p][i] − Σ_{j≠i} Φ[p][i][j] (the sum over j ascending, from 0, then one
// subtraction).  The F(F−1)/2 pairs are numbered row by row — (0,1), (0,2), …, (F−2,F−1) — and
// split into groups of kPairGroup, the coalitions into slabs of kPairSlab: one workgroup per
// (patient, group, slab) keeps kPairGroup f64 accumulators per thread, thread t taking
// coalitions slab·kPairSlab + t, + 256, … in that order.  Per coalition: one popcount, the three
// products, and per pair popc(bits & pair mask) ∈ {0, 1, 2} selects one of them.  The 256
// per-thread partials of a pair are folded as 16 runs of 16 consecutive threads, each in thread
// order, then the 16 runs in run order; shapley_pair_finish folds the slab partials of a pair in
// slab order, stores both halves and forms the diagonal.  Every order is fixed by the constants
// alone and there are no atomics, so Φ is bit-identical from run to run.
constexpr int kPairGroup = 16;      // ops/api.py: SHAPLEY_PAIR_GROUP
constexpr int kPairSlab = 4096;     // ops/api.py: SHAPLEY_PAIR_SLAB
constexpr int kPairMax = kShapMaxF * (kShapMaxF - 1) / 2;   // 190 ≤ 256 threads

// pair number q < F(F−1)/2 → (i, j), i < j
__device__ inline void pair_of(int q, int F, int& i, int& j) {
  i = 0;
  for (int len = F - 1; q >= len; --len) {
    q -= len;
    ++i;
  }
  j = i + 1 + q;
}

__global__ __launch_bounds__(256) void shapley_pair_partial_kernel(const double* __restrict__ v, int F,
                                                                   const double* __restrict__ u, int npairs,
                                                                   int ngroups, int nslab,
                                                                   double* __restrict__ part) {
  __shared__ double sh[256][kPairGroup + 1];
  __shared__ double run[16][kPairGroup + 1];
  __shared__ double ue[kShapMaxF + 3];   // ue[x] = u(x − 2), 0 outside 0 ≤ x − 2 ≤ F − 2
  __shared__ unsigned pm[kPairGroup];
  const int t = threadIdx.x;
  long long b = blockIdx.x;
  const int slab = (int)(b % nslab);
  b /= nslab;
  const int g = (int)(b % ngroups);
  const long long p = b / ngroups;
  const long long nS = 1LL << F;
  const double* vp = v + (size_t)p * nS;
  if (t < kShapMaxF + 3) ue[t] = t >= 2 && t <= F ? u[t - 2] : 0.0;
  if (t < kPairGroup) {
    const int q = g * kPairGroup + t;
    unsigned m = 0u;   // a pair past the last one selects u(|T|)·v every time and is never stored
    if (q < npairs) {
      int i, j;
      pair_of(q, F, i, j);
      m = (1u << i) | (1u << j);
    }
    pm[t] = m;
  }
  __syncthreads();
  unsigned mask[kPairGroup];
#pragma unroll
  for (int a = 0; a < kPairGroup; ++a) mask[a] = __builtin_amdgcn_readfirstlane(pm[a]);
  double acc[kPairGroup];
#pragma unroll
  for (int a = 0; a < kPairGroup; ++a) acc[a] = 0.0;
  const long long S0 = (long long)slab * kPairSlab;
  const long long S1 = S0 + kPairSlab < nS ? S0 + kPairSlab : nS;
  for (long long S = S0 + t; S < S1; S += 256) {
    const unsigned bits = (unsigned)S;
    const int s = __popc(bits);
    const double vS = vp[S];
    const double both = ue[s] * vS;          // i, j ∈ T:      u(|T|−2)·v(T)
    const double one = -(ue[s + 1] * vS);    // one of them:  −u(|T|−1)·v(T)
    const double none = ue[s + 2] * vS;      // neither:       u(|T|)·v(T)
#pragma unroll
    for (int a = 0; a < kPairGroup; ++a) {
      const int c = __popc(bits & mask[a]);
      acc[a] += c == 2 ? both : c == 1 ? one : none;
    }
  }
#pragma unroll
  for (int a = 0; a < kPairGroup; ++a) sh[t][a] = acc[a];
  __syncthreads();
  {
    const int a = t & (kPairGroup - 1), r = t >> 4;   // 256 threads = 16 runs × kPairGroup pairs
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += sh[r * 16 + k][a];
    run[r][a] = s;
  }
  __syncthreads();
  if (t < kPairGroup && g * kPairGroup + t < npairs) {
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += run[r][t];
    part[((size_t)p * nslab + slab) * ((size_t)ngroups * kPairGroup) + g * kPairGroup + t] = s;
  }
}

// One workgroup per patient: thread q folds pair q's slab partials in slab order and stores both
// halves; then thread i forms the diagonal of row i from the matrix kept in LDS.
__global__ __launch_bounds__(256) void shapley_pair_finish_kernel(const double* __restrict__ part, int F,
                                                                  int npairs, int ngroups, int nslab,
                                                                  const double* __restrict__ phi,
                                                                  double* __restrict__ Phi) {
  __shared__ double P[kShapMaxF][kShapMaxF + 1];
  const int t = threadIdx.x;
  const size_t p = blockIdx.x;
  const size_t ld = (size_t)ngroups * kPairGroup;
  double* out = Phi + p * F * F;
  if (t < npairs) {
    int i, j;
    pair_of(t, F, i, j);
    const double* q = part + p * nslab * ld + t;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += q[(size_t)k * ld];
    P[i][j] = s;
    P[j][i] = s;
    out[i * F + j] = s;
    out[j * F + i] = s;
  }
  __syncthreads();
  if (t < F) {
    double s = 0.0;
    for (int j = 0; j < F; ++j)
      if (j != t) s += P[t][j];
    out[t * F + t] = phi[p * F + t] - s;
  }
}

void shapley_interactions(uintptr_t v, long long n, int F, uintptr_t u, uintptr_t phi, uintptr_t part,
                          long long part_len, uintptr_t Phi, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= kShapMaxF, "shapley_interactions: 1 <= F <= 20");
  static_assert(kPairMax <= 256 && (kPairGroup & (kPairGroup - 1)) == 0 && 256 / kPairGroup == 16,
                "one finishing thread per pair; 16 runs of 16 threads in the fold");
  const int npairs = F * (F - 1) / 2;
  const int ngroups = (npairs + kPairGroup - 1) / kPairGroup;
  const long long nS = 1LL << F;
  const int nslab = (int)((nS + kPairSlab - 1) / kPairSlab);
  HFENS_REQUIRE(n >= 0 && part_len == n * nslab * ngroups * kPairGroup,
                "shapley_interactions: the partial workspace holds n * slabs * groups * 16 values");
  if (n == 0) return;
  const long long blocks = n * ngroups * nslab;
  HFENS_REQUIRE(blocks <= 0x7fffffffLL && n <= 0x7fffffffLL, "shapley_interactions: too many patients for one call");
  hipStream_t st = as_stream(stream);
  if (npairs > 0) {
    hipLaunchKernelGGL(shapley_pair_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)v, F,
                       (const double*)u, npairs, ngroups, nslab, (double*)part);
    launch_check();
  }
  hipLaunchKernelGGL(shapley_pair_finish_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)part, F,
                     npairs, ngroups, nslab, (const double*)phi, (double*)Phi);
  launch_check();
}

}  // namespace hfens
