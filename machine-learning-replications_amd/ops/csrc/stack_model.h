// The fused stack evaluation, once, for the three kernels that run it: stack.hip (stack_infer over
// rows in HBM), shapley.hip (stack_coalition over coalition hybrid rows built on chip) and
// partial.hip (stack_partial over substituted cohort rows built on chip).
//
//   z      = (x − mean)·(1/scale)                                  (StandardScaler)
//   dec    = Σ_i c_i·exp(−γ‖sv_i − z‖²) + b_svc                    (RBF SVC on the MFMA: f32, or X3)
//   p_svc  = libsvm Platt sigmoid + iterative 2-class coupling      (f64, couple_p1)
//   p_gbc  = σ(init + lr·Σ_t value_t[leaf_t(x)])                    (folded stumps, or the tree walk)
//   p_lg   = σ(w·x + b)                                             (L1-LR on raw inputs)
//   P      = σ(w_m·[p_svc, p_gbc, p_lg] + b_m)                      (meta LR)
//
// Device side: the LDS view (StackLds), the staging of the model into it (stack_stage_svs,
// stack_stage_model) and stack_score_tile, which takes one wave's 64 rows from its LDS row tile to
// each lane's probability.  A kernel keeps only how its rows come to be in the tile and where the
// probabilities go.  Host side: the model struct and its argument checks (stack_model), the LDS
// plan with the occupancy of the kernel it is made for (stack_plan) and the persistent grid
// (stack_grid).
#pragma once
#include "common.h"

#include <cstdlib>
#include <string>

namespace hfens {

struct StackModel {
  int F;
  int mp;           // padded SV count (multiple of 32) — all SVs staged in LDS at once
  int T, K;         // trees × nodes per tree
  float ngl2e;      // −γ·log2(e)
  float svc_b;      // libsvm intercept (−rho)
  double probA, probB;
  float gb_init, gb_lr;
  float lr_b;
  float meta_w0, meta_w1, meta_w2, meta_b;
  const float* mean;       // [F]
  const float* inv_scale;  // [F]
  const float* svt;        // [F'][mp] k-major
  const float* sn;         // [mp]
  const float* coef;       // [mp]
  const int4* nodes;       // [T*K] {feature, left, right, bits(thr32)}
  const float* values;     // [T*K]
  const float* lr_w;       // [F]
  const int* st_off;       // [F+1] stump-table offsets (nullptr ⇒ generic tree walk)
  const float2* st_pairs;  // [P] {thr32, lr·(v_right − v_left)}
  float st_base;           // init + lr·Σ v_left
};

// The model from an op's scalar and pointer arguments, with the checks every op shares.
static StackModel stack_model(const char* op, int F, int mp, int T, int K, double ngl2e, double svc_b,
                              double probA, double probB, double gb_init, double gb_lr, double lr_b, double mw0,
                              double mw1, double mw2, double mb, uintptr_t mean, uintptr_t inv_scale,
                              uintptr_t svt, uintptr_t sn, uintptr_t coef, uintptr_t nodes, uintptr_t values,
                              uintptr_t lr_w, uintptr_t st_off, uintptr_t st_pairs, double st_base) {
  HFENS_REQUIRE(mp % 32 == 0 && mp > 0, std::string(op) + ": padded SV count must be a positive multiple of 32");
  HFENS_REQUIRE(T >= 0 && K >= 1, std::string(op) + ": bad tree table shape");
  return StackModel{F, mp, T, K, (float)ngl2e, (float)svc_b, probA, probB, (float)gb_init, (float)gb_lr,
                    (float)lr_b, (float)mw0, (float)mw1, (float)mw2, (float)mb, (const float*)mean,
                    (const float*)inv_scale, (const float*)svt, (const float*)sn, (const float*)coef,
                    (const int4*)nodes, (const float*)values, (const float*)lr_w, (const int*)st_off,
                    (const float2*)st_pairs, (float)st_base};
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }

// X3: the sv·z products on the bf16 matrix cores, exactly split.  Every f32 operand v is cut into
// three bf16 pieces v = v0 + v1 + v2 (truncation: 8 + 8 + 8 significant bits, no rounding), and
// sv·z = Σ_f Σ_{i+j ≤ 2} sv_f,i · z_f,j (the 6 largest piece products; the dropped ones are
// ≤ 3·2⁻²⁴ of |sv_f||z_f|, f32-level).  The 6·2KS (product, feature) items are packed along K in two
// lane-half lists — half 0: (0,0), (0,1), (1,0); half 1: (0,2), (1,1), (2,0) as (sv piece, z
// piece) — so one v_mfma_f32_32x32x16_bf16 takes 16 items: ⌈3KS/4⌉ MFMAs per 32 × 32 tile against
// KS of v_mfma_f32_32x32x2f32 (7 vs 9 for the 17-feature model, at 16× the rate per instruction).
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

template <int KS>
constexpr int x3_blocks() { return (3 * 2 * KS + 7) / 8; }   // MFMA k-blocks of 8 items per half

__device__ __forceinline__ void x3_split(float v, unsigned (&b)[3]) {   // bf16 bits of the 3 pieces
  const unsigned u0 = __float_as_uint(v) & 0xFFFF0000u;
  const float r1 = v - __uint_as_float(u0);
  const unsigned u1 = __float_as_uint(r1) & 0xFFFF0000u;
  const float r2 = r1 - __uint_as_float(u1);
  b[0] = u0 >> 16;
  b[1] = u1 >> 16;
  b[2] = __float_as_uint(r2) >> 16;   // r2 has ≤ 8 significant bits: exact in bf16
}

// piece of the SV (js) and of the row (iz) for item-list position p (0..2) of lane half h
__host__ __device__ constexpr int x3_sv_piece(int h, int p) { return h ? 2 - p : (p == 1 ? 1 : 0); }
__host__ __device__ constexpr int x3_z_piece(int h, int p) { return h ? p : (p == 2 ? 1 : 0); }

// ---- LDS view -------------------------------------------------------------------------------
// KS = MFMA k-steps (2 features each), W = waves per workgroup, CH = SVs per staged chunk.
struct StackLds {
  int CH, nch;      // SVs per staged chunk, chunks (1: every SV resident).  nch is here and not
                    // in the tile body: a division there is redone for every tile
  float* sv;        // [2KS][CH] f32, or X3: [NB3][CH][16] bf16
  float* sn;        // [CH] γ'·‖sv‖²
  float* cf;        // [CH] coefs
  float* mu;        // [2KS] mean
  float* is;        // [2KS] 1/scale
  float* xs;        // [W][64][F|1] row tiles, one per wave
  int4* nd;         // [T·K] tree nodes and values, when nodes_in_lds
  float* nv;
  int nodes_in_lds;
  const int4* nodes;    // the tree tables the tail walks: nd, nv or the model's own in HBM
  const float* nvals;   // (set by stack_stage_model)
};

template <int KS, int W, bool X3>
__device__ __forceinline__ StackLds stack_lds_view(float* lds, const StackModel& M, int CH, int nodes_in_lds) {
  StackLds L;
  L.CH = CH;
  L.nch = (M.mp + CH - 1) / CH;
  L.sv = lds;
  L.sn = lds + (X3 ? x3_blocks<KS>() * CH * 8 : 2 * KS * CH);
  L.cf = L.sn + CH;
  L.mu = L.cf + CH;
  L.is = L.mu + 2 * KS;
  L.xs = L.is + 2 * KS;
  const int xs_n = W * 64 * (M.F | 1);
  L.nd = reinterpret_cast<int4*>(L.xs + ((xs_n + 3) & ~3));
  L.nv = reinterpret_cast<float*>(L.nd + (nodes_in_lds ? M.T * M.K : 0));
  L.nodes_in_lds = nodes_in_lds;
  L.nodes = nullptr;
  L.nvals = nullptr;
  return L;
}

// SV chunk c → LDS (block-wide; the caller synchronises)
template <int KS, bool X3>
__device__ __forceinline__ void stack_stage_svs(const StackModel& M, const StackLds& L, int c) {
  const int F = M.F, mp = M.mp, CH = L.CH;
  const int c0 = c * CH, cl = min(CH, mp - c0);
  if constexpr (X3) {
    constexpr int NB3 = x3_blocks<KS>();
    unsigned short* sv3 = reinterpret_cast<unsigned short*>(L.sv);
    // item (m, j, 8h + e): list position q = 8m + e of half h → (piece, feature) of SV j
    for (int i = threadIdx.x; i < NB3 * CH * 16; i += blockDim.x) {
      const int m = i / (CH * 16), rem = i - m * CH * 16, j = rem >> 4, he = rem & 15;
      const int h = he >> 3, q = 8 * m + (he & 7);
      unsigned v = 0;
      if (j < cl && q < 3 * 2 * KS) {
        const int pl = q / (2 * KS), f = q - pl * (2 * KS);
        if (f < F) {
          unsigned b[3];
          x3_split(M.svt[(size_t)f * mp + c0 + j], b);
          const int js = x3_sv_piece(h, pl);
          v = js == 0 ? b[0] : (js == 1 ? b[1] : b[2]);
        }
      }
      sv3[i] = (unsigned short)v;
    }
    for (int i = threadIdx.x; i < 2 * CH; i += blockDim.x) {
      const int k = i / CH, j = i - k * CH;
      L.sn[i] = j < cl ? (k == 0 ? M.ngl2e * M.sn[c0 + j] : M.coef[c0 + j]) : 0.f;
    }
    return;
  }
  for (int i = threadIdx.x; i < (2 * KS + 2) * CH; i += blockDim.x) {   // sv, sn, cf are contiguous
    const int k = i / CH, j = i - k * CH;
    float v = 0.f;
    if (j < cl) {
      if (k < 2 * KS) v = k < F ? M.svt[(size_t)k * mp + c0 + j] : 0.f;
      else if (k == 2 * KS) v = M.ngl2e * M.sn[c0 + j];
      else v = M.coef[c0 + j];
    }
    L.sv[i] = v;
  }
}

// Once per workgroup: SV chunk 0, the scaler and, when they fit, the tree tables (block-wide; the
// caller synchronises).  The tree-table pointers are chosen here, on the branch that copies them,
// so that the tail's loads know their address space (chosen ahead of the copy, the kernels spill
// 24 to 40 B/lane more at the shapes that spill).
template <int KS, bool X3>
__device__ __forceinline__ void stack_stage_model(const StackModel& M, StackLds& L) {
  stack_stage_svs<KS, X3>(M, L, 0);
  for (int i = threadIdx.x; i < 2 * KS; i += blockDim.x) {
    L.mu[i] = i < M.F ? M.mean[i] : 0.f;
    L.is[i] = i < M.F ? M.inv_scale[i] : 0.f;
  }
  if (L.nodes_in_lds) {
    for (int i = threadIdx.x; i < M.T * M.K; i += blockDim.x) {
      L.nd[i] = M.nodes[i];
      L.nv[i] = M.values[i];
    }
  }
  L.nodes = L.nodes_in_lds ? L.nd : M.nodes;
  L.nvals = L.nodes_in_lds ? L.nv : M.values;
}

// ---- the tile body ----------------------------------------------------------------------------
// One wave owns 64 rows in its LDS row tile xw ([64][F|1], written and wavefront-fenced by the
// caller): two 32-row MFMA tiles (data rows are the B operand/columns, SVs the A operand, so Σ over
// SVs = register sum + one cross-half shuffle), then lane l finishes row l's scalar tail and gets
// its probability (0 when !live: the tail is skipped, but every lane takes part in the MFMA part
// and, when the SVs exceed LDS, every wave of the workgroup in the restaging barriers).  `staged`
// is the SV chunk resident in LDS, block-uniform and carried from tile to tile (0 after
// stack_stage_model).  A row's result does not depend on its lane, its tile or CH.
template <int KS, bool X3>
__device__ __forceinline__ float stack_score_tile(const StackModel& M, const StackLds& L, const float* xw,
                                                  int& staged, bool live) {
  const int F = M.F, mp = M.mp, CH = L.CH, nch = L.nch;
  const int ldx = F | 1;
  constexpr int NB3 = x3_blocks<KS>();
  const unsigned short* sv3 = reinterpret_cast<const unsigned short*>(L.sv);
  const int lane = threadIdx.x & 63;
  const int r32 = lane & 31, hi = lane >> 5;
  float za[KS], zb[KS];
  float zna = 0.f, znb = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 2 * s + hi;
    float a = 0.f, b = 0.f;
    if (k < F) {
      const float mu = L.mu[k], is = L.is[k];
      a = (xw[r32 * ldx + k] - mu) * is;
      b = (xw[(32 + r32) * ldx + k] - mu) * is;
    }
    za[s] = a;
    zb[s] = b;
    zna = fmaf(a, a, zna);
    znb = fmaf(b, b, znb);
  }
  zna += __shfl_xor(zna, 32, kWave);
  znb += __shfl_xor(znb, 32, kWave);
  // X3: this lane's row pieces for its lane half's item list (rows r32 and 32 + r32)
  bf16x8_t z3a[X3 ? NB3 : 1], z3b[X3 ? NB3 : 1];
  if constexpr (X3) {
    unsigned pa3[2 * KS][3], pb3[2 * KS][3];
#pragma unroll
    for (int f = 0; f < 2 * KS; ++f) {
      float a = 0.f, b = 0.f;
      if (f < F) {
        const float mu = L.mu[f], is = L.is[f];
        a = (xw[r32 * ldx + f] - mu) * is;
        b = (xw[(32 + r32) * ldx + f] - mu) * is;
      }
      x3_split(a, pa3[f]);
      x3_split(b, pb3[f]);
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
  // exponent of exp(−γ‖sv−z‖²) in base 2: (γ'·‖sv‖²) + (γ'·‖z‖²) + (−2γ')·(sv·z), γ' = −γ·log2 e;
  // ‖sv‖² is staged pre-scaled.  No clamp at 0: a rounding-negative distance only turns
  // exp2 into 1+ε, exactly like the double-precision kernel evaluation it mirrors.
  const float zsa = M.ngl2e * zna, zsb = M.ngl2e * znb, k2 = -2.f * M.ngl2e;
  float pa = 0.f, pb = 0.f;
  auto mma = [&](int t, f32x16& A, f32x16& B) {
    A = f32x16{0.f};
    B = f32x16{0.f};
    if constexpr (X3) {
#pragma unroll
      for (int m = 0; m < NB3; ++m) {
        const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(&sv3[((size_t)m * CH + t + r32) * 16 + 8 * hi]);
        const bf16x8_t sv = __builtin_bit_cast(bf16x8_t, raw);
        A = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sv, z3a[m], A, 0, 0, 0);
        B = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sv, z3b[m], B, 0, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float sv = L.sv[(2 * s + hi) * CH + t + r32];
      A = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, za[s], A, 0, 0, 0);
      B = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, zb[s], B, 0, 0, 0);
    }
  };
  // accumulator reg r ↔ SV t + (r&3) + 8(r>>2) + 4·hi ; column (lane&31) ↔ data row
  auto epi = [&](int t, const f32x16& A, const f32x16& B) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int b0 = t + 8 * g + 4 * hi;
      const f32x4 snv = *reinterpret_cast<const f32x4*>(&L.sn[b0]);
      const f32x4 cfv = *reinterpret_cast<const f32x4*>(&L.cf[b0]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pa = fmaf(cfv[q], __builtin_amdgcn_exp2f(fmaf(k2, A[4 * g + q], snv[q] + zsa)), pa);
        pb = fmaf(cfv[q], __builtin_amdgcn_exp2f(fmaf(k2, B[4 * g + q], snv[q] + zsb)), pb);
      }
    }
  };
  for (int c = 0; c < nch; ++c) {
    // SVs beyond LDS: every chunk is restaged for every tile (L2 traffic + two barriers each)
    if (nch > 1 && staged != c) {  // block-uniform
      __syncthreads();
      stack_stage_svs<KS, X3>(M, L, c);
      __syncthreads();
      staged = c;
    }
    const int cl = min(CH, mp - c * CH);
    // (a software-pipelined variant — MFMAs of tile t+32 issued before the epilogue of t —
    // measured 9 % slower: +49 VGPRs cost a wave/SIMD of occupancy)
    for (int t = 0; t < cl; t += 32) {
      f32x16 A, B;
      mma(t, A, B);
      epi(t, A, B);
    }
  }
  pa += __shfl_xor(pa, 32, kWave);
  pb += __shfl_xor(pb, 32, kWave);
  if (!live) return 0.f;
  // ---- scalar tail: lane ↔ row `lane` of the tile
  const float dec = (lane < 32 ? pa : pb) + M.svc_b;
  const double p_svc = couple_p1((double)dec, M.probA, M.probB);
  const float* xr = xw + lane * ldx;
  float p_gbc, lin = M.lr_b;
  if (M.st_off != nullptr) {
    // folded stumps: one LDS read per feature feeds both the LR dot and the stump pairs;
    // the tables are wave-uniform (scalar loads)
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
      const int4* tn = L.nodes + tr * M.K;
      int node = 0;
      int4 ndv = tn[0];
      while (ndv.x >= 0) {
        node = (xr[ndv.x] <= __int_as_float(ndv.w)) ? ndv.y : ndv.z;
        ndv = tn[node];
      }
      raw += L.nvals[tr * M.K + node];
    }
    p_gbc = sigmoidf_(M.gb_init + M.gb_lr * raw);
    for (int k = 0; k < F; ++k) lin = fmaf(xr[k], M.lr_w[k], lin);
  }
  const float p_lg = sigmoidf_(lin);
  const float m = M.meta_b + M.meta_w0 * (float)p_svc + M.meta_w1 * p_gbc + M.meta_w2 * p_lg;
  return sigmoidf_(m);
}

// ---- LDS plan and launch grid (host) ------------------------------------------------------------
// floats of LDS per staged SV: f32 k-major features, or X3's bf16 item blocks; + ‖sv‖², coef
static int stack_sv_floats(int ks, bool x3) { return x3 ? ((3 * 2 * ks + 7) / 8) * 8 + 2 : 2 * ks + 2; }

static size_t stack_lds_bytes(int W, int F, int CH, int ks, size_t node_bytes, bool x3 = false) {
  size_t xs = (size_t)W * 64 * (F | 1);
  xs = (xs + 3) & ~(size_t)3;
  return ((size_t)stack_sv_floats(ks, x3) * CH + 4 * ks + xs) * 4 + node_bytes;
}

constexpr size_t kStackLdsCap = 160 * 1024;

// SV chunk (multiple of 32): all SVs resident when they fit, else the largest chunk that does.
static int stack_chunk(int W, int F, int mp, int ks, size_t node_bytes, bool x3 = false) {
  const size_t fixed = stack_lds_bytes(W, F, 0, ks, node_bytes, x3);
  if (fixed >= kStackLdsCap) return 0;
  long long ch = (long long)((kStackLdsCap - fixed) / ((size_t)stack_sv_floats(ks, x3) * 4)) / 32 * 32;
  if (ch > mp) ch = mp;
  return (int)ch;
}

static int stack_ks(int F) {
  const int ks = (F + 1) / 2;
  return ks <= 4 ? 4 : ks <= 9 ? 9 : ks <= 12 ? 12 : ks <= 16 ? 16 : 32;
}

struct StackPlan {
  int CH = 0, in_lds = 0, blocks_per_cu = 0;
  size_t lds = 0;
};

// LDS plan for W waves/workgroup: SVs resident if at all possible (trees only when they fit too);
// occupancy from the runtime for the real register count of `kernel`, the <KS, W, X3> instance it
// will launch.
template <int KS, int W, bool X3, typename Kernel>
static StackPlan stack_plan(const StackModel& M, Kernel kernel) {
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
  HFENS_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p.blocks_per_cu, kernel, 64 * W, p.lds));
  return p;
}

// Persistent grid: the `need`ed workgroups, at most as many as the device keeps resident;
// `grid` > 0 forces a size.
static int stack_grid(int grid, long long need, const StackPlan& p) {
  if (grid > 0) return grid;
  int dev = 0, ncu = 256;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const long long cap = (long long)(p.blocks_per_cu > 0 ? p.blocks_per_cu : 1) * ncu;
  return (int)(need < cap ? need : cap);
}

}  // namespace hfens
