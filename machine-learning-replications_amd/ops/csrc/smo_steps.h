// The steps of libsvm's Solver::Solve for C-SVC that the three exact-SMO kernels share:
// smo_kernel (svm.hip: one workgroup per problem), smo_coop_kernel and smo_coop_otf_kernel
// (svm_coop.hip: W workgroups per problem, stored and recomputed Gram).  All three promise libsvm's
// pair sequence bit for bit, so the candidate rank, the pair update with its clipping, the bound
// masks, calculate_rho and the exact block arg-reduction exist here once.
//
// libsvm's arithmetic is x86-64 without FMA: every helper that does f64 arithmetic switches
// contraction off inside its own body (the build contracts everywhere else), so it stays off when
// the helper is inlined and nothing leaks into the including file.
// Licence: the pair rule, tie rules, clipping and calculate_rho follow LIBSVM (BSD-3-Clause, Chang &
// Lin; notice in THIRD_PARTY_NOTICES.md at the repository root).
#pragma once
#include "common.h"

namespace hfens {

constexpr double kSmoTau = 1e-12;
constexpr double kSmoInf = 1.0e300;

// Value of register slot k of a per-thread array, and a store to it, as selects over the unrolled
// slots (a dynamic index would put the array in scratch).
template <int KM>
__device__ __forceinline__ double smo_pick(const double* arr, int kk) {
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k == kk) v = arr[k];
  return v;
}
template <int KM>
__device__ __forceinline__ float smo_pick(const float* arr, int kk) {
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k == kk) v = arr[k];
  return v;
}
template <int KM>
__device__ __forceinline__ void smo_put(double* arr, int kk, double v) {
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if (k == kk) arr[k] = v;
}

// Per-thread bound state, one bit per register slot.
struct SmoMasks {
  unsigned long long ypos = 0ull;    // y_t = +1
  unsigned long long upm = 0ull;     // t ∈ I_up   (y=+1: α<C ; y=−1: α>0)
  unsigned long long lowm = 0ull;    // t ∈ I_low  (y=+1: α>0 ; y=−1: α<C)
  unsigned long long freem = 0ull;   // 0 < α < C
  unsigned long long upperm = 0ull;  // α = C
};

// a point enters with α = 0: at the lower bound.  (Selects, not branches: the branchy form of
// this helper cost smo_kernel<4..8> 8 to 56 B/lane of scratch, profiles/smo_steps.md.)
__device__ __forceinline__ void smo_masks_init(SmoMasks& m, unsigned long long bit, bool pos) {
  m.ypos |= pos ? bit : 0ull;
  m.upm |= pos ? bit : 0ull;
  m.lowm |= pos ? 0ull : bit;
}

// the owner's refresh after α of the point behind `bit` became a
__device__ __forceinline__ void smo_masks_set(SmoMasks& m, unsigned long long bit, double a, double C) {
  const bool pos = (m.ypos & bit) != 0ull;
  const bool atU = a >= C, atL = a <= 0;
  m.freem = (!atU && !atL) ? (m.freem | bit) : (m.freem & ~bit);
  m.upperm = atU ? (m.upperm | bit) : (m.upperm & ~bit);
  const bool up = pos ? !atU : !atL;
  const bool low = pos ? !atL : !atU;
  m.upm = up ? (m.upm | bit) : (m.upm & ~bit);
  m.lowm = low ? (m.lowm | bit) : (m.lowm & ~bit);
}

// arg-max step with libsvm's tie rule (the later index wins)
__device__ __forceinline__ void smo_arg_take(double& b, int& idx, double v, int t) {
  if (v > b || (v == b && t > idx)) { b = v; idx = t; }
}

// Second-order WSS rank of a candidate of I_low (gd = Gmax + y·G > 0, tested by the caller) with
// Gram entry q = K_it: the quotient num/quad itself (libsvm's obj_diff, negated exactly), so the
// choice never depends on how points are grouped over threads or workgroups.  The tie rule stays
// with the caller.  (The candidate test stays outside: a helper that returns "candidate?" along
// with the key cost smo_kernel<8> 8 B/lane of scratch in every shape tried.)
__device__ __forceinline__ double smo_wss2_key(double gd, float q) {
#pragma clang fp contract(off)
  double quad = 2.0 - 2.0 * (double)q;
  if (quad <= 0) quad = kSmoTau;
  return (gd * gd) / quad;
}

// libsvm's update of the pair (i, j) with its four-way box clipping; G_i = −y_i·Gmax exactly.
// ci, cj are the coefficients y·Δα of Gram rows i and j in the gradient update.
struct SmoPair {
  double ai, aj, ci, cj;
};

__device__ __forceinline__ SmoPair smo_pair_update(int yi, int yj, double Ci, double Cj, double Kij, double Gmax,
                                                   double Gj, double ai_old, double aj_old) {
#pragma clang fp contract(off)
  const double Qij = (double)(yi * yj) * Kij;
  const double Gi = -(double)yi * Gmax;
  double ai = ai_old, aj = aj_old;
  if (yi != yj) {
    double quad = 2.0 + 2.0 * Qij;
    if (quad <= 0) quad = kSmoTau;
    const double delta = (-Gi - Gj) / quad;
    const double diff = ai - aj;
    ai += delta;
    aj += delta;
    if (diff > 0) {
      if (aj < 0) { aj = 0; ai = diff; }
    } else {
      if (ai < 0) { ai = 0; aj = -diff; }
    }
    if (diff > Ci - Cj) {
      if (ai > Ci) { ai = Ci; aj = Ci - diff; }
    } else {
      if (aj > Cj) { aj = Cj; ai = Cj + diff; }
    }
  } else {
    double quad = 2.0 - 2.0 * Qij;
    if (quad <= 0) quad = kSmoTau;
    const double delta = (Gi - Gj) / quad;
    const double sum = ai + aj;
    ai -= delta;
    aj += delta;
    if (sum > Ci) {
      if (ai > Ci) { ai = Ci; aj = sum - Ci; }
    } else {
      if (aj < 0) { aj = 0; ai = sum; }
    }
    if (sum > Cj) {
      if (aj > Cj) { aj = Cj; ai = sum - Cj; }
    } else {
      if (ai < 0) { ai = 0; aj = sum; }
    }
  }
  return SmoPair{ai, aj, (double)yi * (ai - ai_old), (double)yj * (aj - aj_old)};
}

// Per-wave partial of a block reduction: order-preserving u64 keys (exact for f64).
struct SmoRedPart {
  unsigned long long ka, kb;
  int idx, pad;
};

// Block reduction of (a, b, idx): a → max; (b, idx) → arg-max with ties to the larger idx.  Wave
// stage on DPP/permlane (u32 max of the key halves, then of the index among the lanes holding the
// arg-max — no LDS round trips), one barrier, then every thread folds the NWaves partials and
// receives the result as keys.  Callers alternate two partial buffers so consecutive reductions
// need no second barrier.
// WantA = false: the caller passes a uniform `a` and ignores the max (WSS step 1), so its two
// wave-max chains are skipped (the result's ka is then f64_okey(a)).
template <int NWaves, bool WantA = true>
__device__ __forceinline__ SmoRedPart smo_block_red(double a, double b, int idx, SmoRedPart* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long ka = f64_okey(a), kb = f64_okey(b);
  unsigned ah = (unsigned)(ka >> 32), al = (unsigned)ka;
  if constexpr (WantA) {
    ah = wave_max_u32((unsigned)(ka >> 32));
    al = wave_max_u32((unsigned)(ka >> 32) == ah ? (unsigned)ka : 0u);
  }
  const unsigned bh = wave_max_u32((unsigned)(kb >> 32));
  const unsigned bl = wave_max_u32((unsigned)(kb >> 32) == bh ? (unsigned)kb : 0u);
  const bool top = (unsigned)(kb >> 32) == bh && (unsigned)kb == bl;
  const unsigned bi = wave_max_u32(top ? (unsigned)(idx + 1) : 0u);
  if (lane == 0)
    sh[wave] = SmoRedPart{((unsigned long long)ah << 32) | al, ((unsigned long long)bh << 32) | bl, (int)bi - 1, 0};
  __syncthreads();
  SmoRedPart r = sh[0];
#pragma unroll
  for (int w = 1; w < NWaves; ++w) {
    const SmoRedPart p = sh[w];
    r.ka = p.ka > r.ka ? p.ka : r.ka;
    if (p.kb > r.kb || (p.kb == r.kb && p.idx > r.idx)) { r.kb = p.kb; r.idx = p.idx; }
  }
  return r;
}

// calculate_rho, one point: α = C bounds ρ from one side by its label, a free point joins the mean,
// α = 0 bounds from the other side.  ru = max(−ub), rl = max(lb).
__device__ __forceinline__ void smo_rho_classify(bool pos, bool upper, bool free, double yG, double& ru, double& rl,
                                                 double& sum_free, int& nfree) {
#pragma clang fp contract(off)
  if (upper) {
    if (!pos) ru = fmax(ru, -yG); else rl = fmax(rl, yG);
  } else if (free) {
    ++nfree;
    sum_free += yG;
  } else {
    if (pos) ru = fmax(ru, -yG); else rl = fmax(rl, yG);
  }
}

// calculate_rho over a workgroup: the keys of max(−ub) and max(lb), and the free points' sum and
// count added in wave order.  Every thread receives the result.  `sh` may still be read by the
// reduction before: one barrier first.
struct SmoRhoPart {
  unsigned long long kru, krl;
  double S, n;
};

template <int NWaves>
__device__ __forceinline__ SmoRhoPart smo_rho_block(double ru, double rl, double sum_free, int nfree, SmoRedPart* sh,
                                                    double (*ssum)[NWaves]) {
#pragma clang fp contract(off)
  __syncthreads();
  const SmoRedPart rr = smo_block_red<NWaves>(ru, rl, -1, sh);
  const double s = wave_sum(sum_free), c = wave_sum((double)nfree);
  if ((threadIdx.x & 63) == 0) { ssum[0][threadIdx.x >> 6] = s; ssum[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  double S = 0.0, n = 0.0;
  for (int w = 0; w < NWaves; ++w) { S += ssum[0][w]; n += ssum[1][w]; }
  return SmoRhoPart{rr.ka, rr.kb, S, n};
}

__device__ __forceinline__ double smo_rho_value(double ub, double lb, double S, double n) {
#pragma clang fp contract(off)
  return n > 0 ? S / n : (ub + lb) / 2;
}

}  // namespace hfens
