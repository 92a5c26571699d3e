// Partial dependence and ICE curves of the fused HF stack.
//
//   cell c    = (k1, v1, k2, v2)                                    (k = −1: no substitution in that slot)
//   h(c,r)    = X[r] with column k1 set to v1 and column k2 set to v2
//   ice[r][c] = P(h(c,r))                                           (f32, optional)
//   pd[c]     = (Σ_{r = 0, 1, …, n−1, in that order} (double)ice[r][c]) / (double)n      (f64)
//
// stack_partial evaluates the whole stack (the stages and arithmetic of stack.hip) on hybrid rows
// that never exist in HBM, with the structure of shapley.hip's stack_coalition: one wave owns 64
// consecutive cells, lane ↔ cell c0 + lane.  For each cohort row r (read at a wave-uniform
// address) every lane copies X[r] into its row of the wave's LDS row tile and overwrites at most
// two columns, the wave runs stack.hip's tile body on the 64 rows, and every lane adds its row's
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
  float* xl = xw + lane * ldx;                    // this lane's hybrid row
  const long long ntile = (C + 63) / 64;
  const long long stride = (long long)gridDim.x * W;

  // block-uniform tile loop (all waves take part in the chunk barriers when nch > 1)
  for (long long base = 0; base < ntile; base += stride) {
    const long long tile = base + (long long)wave * gridDim.x + blockIdx.x;
    const bool valid = tile < ntile;
    if (nch == 1 && !valid) continue;              // no barrier below: a wave without a tile sits out
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
      const float zsa = M.ngl2e * zna, zsb = M.ngl2e * znb, k2e = -2.f * M.ngl2e;
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
            pa = fmaf(cfv[q], __builtin_amdgcn_exp2f(fmaf(k2e, A[4 * g + q], snv[q] + zsa)), pa);
            pb = fmaf(cfv[q], __builtin_amdgcn_exp2f(fmaf(k2e, Bm[4 * g + q], snv[q] + zsb)), pb);
          }
        }
      };
      for (int c = 0; c < nch; ++c) {
        // SVs beyond LDS: every chunk is restaged for every (tile, cohort row), as in shapley.hip
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
      if (live) {
        // ---- scalar tail: lane ↔ hybrid row of its cell
        const float dec = (lane < 32 ? pa : pb) + M.svc_b;
        const double p_svc = couple_p1((double)dec, M.probA, M.probB);
        float p_gbc, lin = M.lr_b;
        if (M.st_off != nullptr) {
          float raw = M.st_base;
          for (int k = 0; k < F; ++k) {
            const float xv = xl[k];
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
              node = (xl[ndv.x] <= __int_as_float(ndv.w)) ? ndv.y : ndv.z;
              ndv = tn[node];
            }
            raw += nvals[tr * M.K + node];
          }
          p_gbc = sigmoidf_(M.gb_init + M.gb_lr * raw);
          for (int k = 0; k < F; ++k) lin = fmaf(xl[k], M.lr_w[k], lin);
        }
        const float p_lg = sigmoidf_(lin);
        const float m = M.meta_b + M.meta_w0 * (float)p_svc + M.meta_w1 * p_gbc + M.meta_w2 * p_lg;
        const float p = sigmoidf_(m);
        if (ice != nullptr) ice[(size_t)r * C + cell] = p;
        acc += (double)p;   // the stored f32, widened
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // xw is rewritten for the next cohort row
    }
    if (live) pd[cell] = acc / (double)n;
  }
}

// stack.hip's LDS plan (SVs resident if at all possible, trees only when they fit too) for this
// kernel's register count
template <int KS, int W, bool X3>
static StackPlan partial_plan(const StackModel& M) {
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
  HFENS_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p.blocks_per_cu, stack_partial_kernel<KS, W, X3>,
                                                           64 * W, p.lds));
  return p;
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
  int grid = a.grid;
  if (grid <= 0) {
    int dev = 0, ncu = 256;
    HFENS_CHECK(hipGetDevice(&dev));
    HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const long long need = (a.C + 63) / 64;       // one tile per workgroup until every CU is taken
    const long long cap = (long long)(p.blocks_per_cu > 0 ? p.blocks_per_cu : 1) * ncu;
    grid = (int)(need < cap ? need : cap);
  }
  hipLaunchKernelGGL((stack_partial_kernel<KS, W, X3>), dim3(grid), dim3(64 * W), p.lds, a.st, a.X, a.n, a.feat,
                     a.value, a.C, M, p.CH, p.in_lds, a.pd, a.ice);
  launch_check();
}

// 8 waves per workgroup; the bf16x3 products (X3) for the narrow shapes while every SV stays
// resident in LDS, else the f32 MFMA path with chunked restaging — stack_infer's defaults.
template <int KS>
static void partial_pick(const PartialArgs& a, const StackModel& M) {
  if constexpr (KS <= 9) {
    const StackPlan q = partial_plan<KS, 8, true>(M);
    if (q.CH >= M.mp && q.blocks_per_cu > 0) return partial_go<KS, 8, true>(a, M, q);
  }
  const StackPlan p = partial_plan<KS, 8, false>(M);
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
  HFENS_REQUIRE(mp % 32 == 0 && mp > 0, "stack_partial: padded SV count must be a positive multiple of 32");
  HFENS_REQUIRE(T >= 0 && K >= 1, "stack_partial: bad tree table shape");
  StackModel M{F, mp, T, K, (float)ngl2e, (float)svc_b, probA, probB, (float)gb_init, (float)gb_lr,
               (float)lr_b, (float)mw0, (float)mw1, (float)mw2, (float)mb, (const float*)mean,
               (const float*)inv_scale, (const float*)svt, (const float*)sn, (const float*)coef,
               (const int4*)nodes, (const float*)values, (const float*)lr_w, (const int*)st_off,
               (const float2*)st_pairs, (float)st_base};
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
