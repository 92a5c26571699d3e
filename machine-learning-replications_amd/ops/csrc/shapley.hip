// Exact interventional Shapley values of the fused HF stack.
//
//   h(S,b)[k] = x[k] if bit k of S is set, else bg[b][k]          (hybrid row of coalition S)
//   v[p][S]   = (1/B)·Σ_b P(h(S,b))                                (stack_coalition, f64)
//   φ[p][k]   = Σ_S c_k(S)·v[p][S],  c_k(S) = w(|S|−1) if k ∈ S else −w(|S|)   (shapley_reduce, f64)
//
// stack_coalition evaluates the whole stack (the stages and arithmetic of stack.hip) on hybrid
// rows that never exist in HBM.  One wave owns 64 consecutive coalitions of one patient: lane ↔
// coalition S0 + lane.  For each background row b it builds its 64 hybrid rows in its LDS row tile
// by bit select from the patient row (held in registers) and bg[b], runs stack.hip's tile body on
// them, and every lane adds its row's probability to an f64 sum — b = 0, 1, …, B−1 in that order,
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
  const int F = M.F, mp = M.mp;
  const int ldx = F | 1;
  const int nch = (mp + CH - 1) / CH;
  constexpr int NB3 = x3_blocks<KS>();
  float* sv_l = lds;                              // [2KS][CH] f32, or X3: [NB3][CH][16] bf16
  unsigned short* sv3 = reinterpret_cast<unsigned short*>(lds);
  float* sn_l = sv_l + (X3 ? NB3 * CH * 8 : 2 * KS * CH);   // [CH]
  float* cf_l = sn_l + CH;                        // [CH]
  float* mu_l = cf_l + CH;                        // [2KS] mean, then [2KS] 1/scale
  float* is_l = mu_l + 2 * KS;
  float* xs = is_l + 2 * KS;                      // [waves][64][ldx]
  const int xs_n = W * 64 * ldx;
  int4* nd_l = reinterpret_cast<int4*>(xs + ((xs_n + 3) & ~3));
  float* nv_l = reinterpret_cast<float*>(nd_l + (nodes_in_lds ? M.T * M.K : 0));
  auto stage = [&](int c) {  // SV chunk c → LDS (block-wide; caller synchronises), as stack.hip
    const int c0 = c * CH, cl = min(CH, mp - c0);
    if constexpr (X3) {
      for (int i = threadIdx.x; i < NB3 * CH * 16; i += blockDim.x) {
        const int m = i / (CH * 16), rem = i - m * CH * 16, j = rem >> 4, he = rem & 15;
        const int h = he >> 3, q = 8 * m + (he & 7);
        unsigned val = 0;
        if (j < cl && q < 3 * 2 * KS) {
          const int pl = q / (2 * KS), f = q - pl * (2 * KS);
          if (f < F) {
            unsigned b[3];
            x3_split(M.svt[(size_t)f * mp + c0 + j], b);
            const int js = x3_sv_piece(h, pl);
            val = js == 0 ? b[0] : (js == 1 ? b[1] : b[2]);
          }
        }
        sv3[i] = (unsigned short)val;
      }
      for (int i = threadIdx.x; i < 2 * CH; i += blockDim.x) {
        const int k = i / CH, j = i - k * CH;
        sn_l[i] = j < cl ? (k == 0 ? M.ngl2e * M.sn[c0 + j] : M.coef[c0 + j]) : 0.f;
      }
      return;
    }
    for (int i = threadIdx.x; i < (2 * KS + 2) * CH; i += blockDim.x) {
      const int k = i / CH, j = i - k * CH;
      float val = 0.f;
      if (j < cl) {
        if (k < 2 * KS) val = k < F ? M.svt[(size_t)k * mp + c0 + j] : 0.f;
        else if (k == 2 * KS) val = M.ngl2e * M.sn[c0 + j];
        else val = M.coef[c0 + j];
      }
      lds[i] = val;
    }
  };
  stage(0);
  int staged = 0;   // SV chunk resident in LDS (block-uniform)
  for (int i = threadIdx.x; i < 2 * KS; i += blockDim.x) {
    mu_l[i] = i < F ? M.mean[i] : 0.f;
    is_l[i] = i < F ? M.inv_scale[i] : 0.f;
  }
  if (nodes_in_lds) {
    for (int i = threadIdx.x; i < M.T * M.K; i += blockDim.x) {
      nd_l[i] = M.nodes[i];
      nv_l[i] = M.values[i];
    }
  }
  __syncthreads();
  const int4* nodes = nodes_in_lds ? nd_l : M.nodes;
  const float* nvals = nodes_in_lds ? nv_l : M.values;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, hi = lane >> 5;
  float* xw = xs + wave * 64 * ldx;
  const long long nS = 1LL << F;
  const long long tps = (nS + 63) / 64;           // 64-coalition tiles per patient
  const long long nitem = n * tps;
  const long long stride = (long long)gridDim.x * W;

  // block-uniform item loop (all waves take part in the chunk barriers when nch > 1)
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
      float za[KS], zb[KS];
      float zna = 0.f, znb = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = 2 * s + hi;
        float a = 0.f, bb = 0.f;
        if (k < F) {
          const float mu = mu_l[k], is = is_l[k];
          a = (xw[r32 * ldx + k] - mu) * is;
          bb = (xw[(32 + r32) * ldx + k] - mu) * is;
        }
        za[s] = a;
        zb[s] = bb;
        zna = fmaf(a, a, zna);
        znb = fmaf(bb, bb, znb);
      }
      zna += __shfl_xor(zna, 32, kWave);
      znb += __shfl_xor(znb, 32, kWave);
      // X3: this lane's row pieces for its lane half's item list (rows r32 and 32 + r32)
      bf16x8_t z3a[X3 ? NB3 : 1], z3b[X3 ? NB3 : 1];
      if constexpr (X3) {
        unsigned pa3[2 * KS][3], pb3[2 * KS][3];
#pragma unroll
        for (int f = 0; f < 2 * KS; ++f) {
          float a = 0.f, bb = 0.f;
          if (f < F) {
            const float mu = mu_l[f], is = is_l[f];
            a = (xw[r32 * ldx + f] - mu) * is;
            bb = (xw[(32 + r32) * ldx + f] - mu) * is;
          }
          x3_split(a, pa3[f]);
          x3_split(bb, pb3[f]);
        }
#pragma unroll
        for (int m = 0; m < NB3; ++m) {
          unsigned wa[4], wb[4];
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) {
            unsigned lo_a = 0, hi_a = 0, lo_b = 0, hi_b = 0;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
              const int q = 8 * m + 2 * e2 + d;
              unsigned va = 0, vb = 0;
              if (q < 3 * 2 * KS) {
                const int pl = q / (2 * KS), f = q - pl * (2 * KS);
                const int i0 = x3_z_piece(0, pl), i1 = x3_z_piece(1, pl);
                va = hi ? pa3[f][i1] : pa3[f][i0];
                vb = hi ? pb3[f][i1] : pb3[f][i0];
              }
              if (d == 0) { lo_a = va; lo_b = vb; } else { hi_a = va; hi_b = vb; }
            }
            wa[e2] = lo_a | (hi_a << 16);
            wb[e2] = lo_b | (hi_b << 16);
          }
          z3a[m] = __builtin_bit_cast(bf16x8_t, (u32x4_t){wa[0], wa[1], wa[2], wa[3]});
          z3b[m] = __builtin_bit_cast(bf16x8_t, (u32x4_t){wb[0], wb[1], wb[2], wb[3]});
        }
      }
      // exponent of exp(−γ‖sv−z‖²) in base 2, exactly as stack.hip forms it
      const float zsa = M.ngl2e * zna, zsb = M.ngl2e * znb, k2 = -2.f * M.ngl2e;
      float pa = 0.f, pb = 0.f;
      auto mma = [&](int t, f32x16& A, f32x16& Bm) {
        A = f32x16{0.f};
        Bm = f32x16{0.f};
        if constexpr (X3) {
#pragma unroll
          for (int m = 0; m < NB3; ++m) {
            const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(&sv3[((size_t)m * CH + t + r32) * 16 + 8 * hi]);
            const bf16x8_t sv = __builtin_bit_cast(bf16x8_t, raw);
            A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sv, z3a[m], A, 0, 0, 0);
            Bm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sv, z3b[m], Bm, 0, 0, 0);
          }
          return;
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float sv = sv_l[(2 * s + hi) * CH + t + r32];
          A = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, za[s], A, 0, 0, 0);
          Bm = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, zb[s], Bm, 0, 0, 0);
        }
      };
      // accumulator reg r ↔ SV t + (r&3) + 8(r>>2) + 4·hi ; column (lane&31) ↔ hybrid row
      auto epi = [&](int t, const f32x16& A, const f32x16& Bm) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int b0 = t + 8 * g + 4 * hi;
          const f32x4 snv = *reinterpret_cast<const f32x4*>(&sn_l[b0]);
          const f32x4 cfv = *reinterpret_cast<const f32x4*>(&cf_l[b0]);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            pa = fmaf(cfv[q], __builtin_amdgcn_exp2f(fmaf(k2, A[4 * g + q], snv[q] + zsa)), pa);
            pb = fmaf(cfv[q], __builtin_amdgcn_exp2f(fmaf(k2, Bm[4 * g + q], snv[q] + zsb)), pb);
          }
        }
      };
      for (int c = 0; c < nch; ++c) {
        // SVs beyond LDS: every chunk is restaged for every (item, background row) — B times
        // stack_infer's restaging traffic per tile.  Correct but slow; a chunk loop outside the
        // background loop would need the B partial decision sums of a tile kept per lane.
        if (nch > 1 && staged != c) {  // block-uniform: restage chunk c
          __syncthreads();
          stage(c);
          __syncthreads();
          staged = c;
        }
        const int cl = min(CH, mp - c * CH);
        for (int t = 0; t < cl; t += 32) {
          f32x16 A, Bm;
          mma(t, A, Bm);
          epi(t, A, Bm);
        }
      }
      pa += __shfl_xor(pa, 32, kWave);
      pb += __shfl_xor(pb, 32, kWave);
      if (valid) {
        // ---- scalar tail: lane ↔ hybrid row of coalition S
        const float dec = (lane < 32 ? pa : pb) + M.svc_b;
        const double p_svc = couple_p1((double)dec, M.probA, M.probB);
        const float* xr = xw + lane * ldx;
        float p_gbc, lin = M.lr_b;
        if (M.st_off != nullptr) {
          float raw = M.st_base;
          for (int k = 0; k < F; ++k) {
            const float xv = xr[k];
            lin = fmaf(xv, M.lr_w[k], lin);
            const int j1 = M.st_off[k + 1];
            for (int j = M.st_off[k]; j < j1; ++j) {
              const float2 pr = M.st_pairs[j];
              raw += xv > pr.x ? pr.y : 0.f;
            }
          }
          p_gbc = sigmoidf_(raw);
        } else {
          float raw = 0.f;
          for (int tr = 0; tr < M.T; ++tr) {
            const int4* tn = nodes + tr * M.K;
            int node = 0;
            int4 ndv = tn[0];
            while (ndv.x >= 0) {
              node = (xr[ndv.x] <= __int_as_float(ndv.w)) ? ndv.y : ndv.z;
              ndv = tn[node];
            }
            raw += nvals[tr * M.K + node];
          }
          p_gbc = sigmoidf_(M.gb_init + M.gb_lr * raw);
          for (int k = 0; k < F; ++k) lin = fmaf(xr[k], M.lr_w[k], lin);
        }
        const float p_lg = sigmoidf_(lin);
        const float m = M.meta_b + M.meta_w0 * (float)p_svc + M.meta_w1 * p_gbc + M.meta_w2 * p_lg;
        acc += (double)sigmoidf_(m);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // xw is rewritten for the next background row
    }
    if (valid && S < nS) v[p * nS + S] = acc / (double)B;
  }
}

// stack.hip's LDS plan (SVs resident if at all possible, trees only when they fit too) for this
// kernel's register count
template <int KS, int W, bool X3>
static StackPlan coalition_plan(const StackModel& M) {
  StackPlan p;
  const size_t node_bytes = M.st_off ? 0 : (size_t)M.T * M.K * 20;
  bool in_lds = node_bytes > 0 && node_bytes <= 24 * 1024;
  int CH = stack_chunk(W, M.F, M.mp, KS, in_lds ? node_bytes : 0, X3);
  if (in_lds && CH < M.mp) {
    const int ch2 = stack_chunk(W, M.F, M.mp, KS, 0, X3);
    if (ch2 > CH) { in_lds = false; CH = ch2; }
  }
  if (CH < 32) return p;
  p.CH = CH;
  p.in_lds = in_lds;
  p.lds = stack_lds_bytes(W, M.F, CH, KS, in_lds ? node_bytes : 0, X3);
  HFENS_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p.blocks_per_cu, stack_coalition_kernel<KS, W, X3>,
                                                           64 * W, p.lds));
  return p;
}

template <int KS, int W, bool X3>
static void coalition_go(const float* X, long long n, const float* BG, int B, const StackModel& M,
                         const StackPlan& p, int grid, double* v, hipStream_t st) {
  if (grid <= 0) {
    int dev = 0, ncu = 256;
    HFENS_CHECK(hipGetDevice(&dev));
    HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const long long items = n * (((1LL << M.F) + 63) / 64);
    const long long need = (items + W - 1) / W;
    const long long cap = (long long)(p.blocks_per_cu > 0 ? p.blocks_per_cu : 1) * ncu;
    grid = (int)(need < cap ? need : cap);
  }
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
    const StackPlan q = coalition_plan<KS, 8, true>(M);
    if (q.CH >= M.mp && q.blocks_per_cu > 0) return coalition_go<KS, 8, true>(X, n, BG, B, M, q, grid, v, st);
  }
  const StackPlan p = coalition_plan<KS, 8, false>(M);
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
  HFENS_REQUIRE(mp % 32 == 0 && mp > 0, "stack_coalition: padded SV count must be a positive multiple of 32");
  HFENS_REQUIRE(T >= 0 && K >= 1, "stack_coalition: bad tree table shape");
  if (n == 0) return;
  StackModel M{F, mp, T, K, (float)ngl2e, (float)svc_b, probA, probB, (float)gb_init, (float)gb_lr,
               (float)lr_b, (float)mw0, (float)mw1, (float)mw2, (float)mb, (const float*)mean,
               (const float*)inv_scale, (const float*)svt, (const float*)sn, (const float*)coef,
               (const int4*)nodes, (const float*)values, (const float*)lr_w, (const int*)st_off,
               (const float2*)st_pairs, (float)st_base};
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

}  // namespace hfens
