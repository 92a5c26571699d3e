// Model struct, scalar helpers, X3 operand split and LDS plan shared by the fused stack kernels
// (stack.hip: stack_infer over rows in HBM; shapley.hip: stack_coalition over hybrid rows built
// on chip).
#pragma once
#include "common.h"

#include <cstdlib>

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

__device__ __forceinline__ double couple_p1(double dec, double A, double B) {
  const double fApB = dec * A + B;
  double r01 = fApB >= 0 ? exp(-fApB) / (1.0 + exp(-fApB)) : 1.0 / (1.0 + exp(fApB));
  r01 = fmin(fmax(r01, 1e-7), 1 - 1e-7);
  const double r10 = 1.0 - r01;
  const double q00 = r10 * r10, q11 = r01 * r01, q01 = -r10 * r01;
  double p0 = 0.5, p1 = 0.5;
  for (int it = 0; it < 100; ++it) {
    double qp0 = q00 * p0 + q01 * p1;
    double qp1 = q01 * p0 + q11 * p1;
    double pqp = p0 * qp0 + p1 * qp1;
    if (fmax(fabs(qp0 - pqp), fabs(qp1 - pqp)) < 0.0025) break;
    double d = (-qp0 + pqp) / q00;
    p0 += d;
    pqp = (pqp + d * (d * q00 + 2 * qp0)) / (1 + d) / (1 + d);
    qp0 = (qp0 + d * q00) / (1 + d);
    qp1 = (qp1 + d * q01) / (1 + d);
    p0 /= (1 + d);
    p1 /= (1 + d);
    d = (-qp1 + pqp) / q11;
    p1 += d;
    p0 /= (1 + d);
    p1 /= (1 + d);
  }
  return p1;
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

}  // namespace hfens
