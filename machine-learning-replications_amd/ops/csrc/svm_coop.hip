// Cooperative exact SMO: one libsvm C-SVC problem spread over W workgroups.
//
// The single-workgroup solver (svm.hip smo_kernel) is VALU-bound on ONE CU: every pair (i, j)
// costs ~50 f64/bitmask instructions per point in the two WSS passes and the gradient update,
// so at l = 8-10k points one CU spends most of its ~10 µs per pair issuing them.  Here each
// problem's points are cut into W contiguous slices, one per workgroup ("member"), and the two
// block arg-reductions of every iteration become two in-launch exchanges between the members:
// every member publishes its partial (arg-max key, index and the owner's payload: α_i; α_j,
// G_j, K_ij) as data-tagged 8-byte granules {epoch, value} written by agent-scope relaxed
// atomic stores (write-through: no fence, no flag), and one wave per member sweeps all W
// partials until every tag equals the exchange's epoch.  Every member then folds the same W
// partials in the same order and performs the same pair update, so all members agree on
// (i, j, α_i, α_j) with no further communication; each member updates only its own slice of G
// with its own slices of Gram rows i and j (1/W of each row read).
//
// Exactness: the reductions are exact max / arg-max (ties → larger index) — independent of
// how the points are partitioned — and the per-point arithmetic is smo_kernel's (the steps of
// smo_steps.h: libsvm order, no FMA contraction), so the pair sequence, α and ρ match smo_kernel's.
//
// Liveness: every spin is bounded; a member that times out sets *err and leaves, its peers
// then time out too and the launch drains (the host raises on err).  The launcher admits at
// most one member per CU, so every member is resident at once; the members of one problem are
// placed on one XCD (blocks b and b+8 share an XCD under round-robin dispatch — speed only,
// never correctness).
#include <cstdlib>

#include "common.h"
#include "smo_steps.h"

namespace hfens {

typedef __attribute__((address_space(1))) unsigned long long gu64_t;

struct SmoCoopProb {
  long long koff;   // K_p offset (floats)
  long long aoff;   // alpha offset (doubles)
  long long moff;   // Mapped: offset of this problem's column map in `maps` (see smo_coop_kernel)
  int l;            // problem size
  int ld;           // K_p leading dimension
  int npos;         // indices [0, npos) have y = +1, the rest y = −1
  int S;            // points per member (multiple of 4): member w owns columns [w·S, min(lphys, (w+1)·S))
  int lphys;        // columns of K_p's rows (= l unless Mapped)
  int pad;
  double Cp, Cn;
};

struct SmoCoopOut {
  double* rho;      // [P]
  int* iters;       // [P]
  double* gap;      // [P]
  unsigned* err;    // [1] set on a spin timeout
  long long* prof;  // [P][7] s_memtime phase totals of member 0 (nullptr = off): step2, red2,
                    // xchg2, pair, update, red1, xchg1
  int prefetch;     // 1: pull the member's candidate Gram row into L2 while the exchange runs
  int pad_;
  long long wait_ticks;    // one exchange waits at most this long (100 MHz real-time counter), then
                           // flags err: a member that is not resident costs a bounded delay, and the
                           // host re-solves with the one-workgroup kernel (models/smo.py)
  long long inject_ticks;  // test hook: member 1 of problem 0 starts this late (0 = off)
};

constexpr int kCoopThreads = 512;
constexpr int kCoopWaves = kCoopThreads / 64;
constexpr int kGran = 10;             // granules per member slot
constexpr int kPkBits = 15;           // Mapped: point key = libsvm index << 15 | column
constexpr int kPkMask = (1 << kPkBits) - 1;
constexpr int kMaxMembers = 16;
constexpr long long kWaitMsDefault = 20;   // HFENS_SMO_WAIT_MS: per-exchange deadline

// 100 MHz constant-rate counter (independent of the shader clock)
__device__ __forceinline__ long long rt_now() { return (long long)__builtin_amdgcn_s_memrealtime(); }

// the test hook of SmoCoopOut::inject_ticks: one member arrives late (never in production runs)
__device__ __forceinline__ void coop_inject_delay(long long ticks, int p, int w) {
  if (ticks <= 0 || p != 0 || w != 1) return;
  const long long until = rt_now() + ticks;
  while (rt_now() < until) __builtin_amdgcn_s_sleep(127);
}

__device__ __forceinline__ void put_granule(unsigned long long* g, unsigned epoch, unsigned v) {
  __hip_atomic_store((gu64_t*)g, ((unsigned long long)epoch << 32) | v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void put_u64(unsigned long long* g, unsigned epoch, unsigned long long x) {
  put_granule(g, epoch, (unsigned)x);
  put_granule(g + 1, epoch, (unsigned)(x >> 32));
}
__device__ __forceinline__ unsigned long long u64_of(const unsigned* v) {
  return (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
}
__device__ __forceinline__ double f64_of(const unsigned* v) {
  return __longlong_as_double((long long)u64_of(v));
}
__device__ __forceinline__ unsigned long long bits_of(double x) {
  return (unsigned long long)__double_as_longlong(x);
}

// Wave 0 sweeps the first `ng` granules of every member's slot (GS granules per slot) until all
// of them carry `epoch` and leaves the values in vals[member][granule] (LDS); one barrier.
// false = timed out.
template <int GS>
__device__ __forceinline__ bool coop_gather_t(unsigned long long* slot, int W, int ng, unsigned epoch,
                                              unsigned (*vals)[GS], const SmoCoopOut& out, int* sh_fail) {
  constexpr int R = (kMaxMembers * GS + 63) / 64;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int tot = W * ng;
    unsigned v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = 0u;
    const long long deadline = rt_now() + out.wait_ticks;
    unsigned spins = 0;
    bool fail = false;
    for (;;) {
      bool ok = true;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int gi = lane + 64 * r;
        if (gi < tot) {
          const int m = gi / ng, k = gi - m * ng;
          const unsigned long long x =
              __hip_atomic_load((gu64_t*)(slot + m * GS + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          v[r] = (unsigned)x;
          ok = ok && (unsigned)(x >> 32) == epoch;
        }
      }
      if (__all(ok)) break;
      // the real-time counter is read every 64th poll only (a scalar memory read of its own)
      // every 64th poll: the deadline (real-time counter) and the error flag — once any member
      // of the launch has given up, the others leave at their next check instead of waiting out
      // their own deadlines
      if ((++spins & 63u) == 0 &&
          (rt_now() > deadline || __hip_atomic_load(out.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
        fail = true;
        if (lane == 0) atomicOr(out.err, 1u);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int gi = lane + 64 * r;
      if (gi < tot) {
        const int m = gi / ng, k = gi - m * ng;
        vals[m][k] = v[r];
      }
    }
    if (lane == 0) *sh_fail = fail ? 1 : 0;
  }
  __syncthreads();
  return *sh_fail == 0;
}

// A member's LDS: the alternating reduction partials, the gathered granules of the last two
// exchanges (GS granules per member slot), the gather's verdict and the ρ sums.
template <int GS>
struct CoopLds {
  SmoRedPart shA[kCoopWaves], shB[kCoopWaves];
  unsigned vals[2][kMaxMembers][GS];
  int fail;
  double ssum[2][kCoopWaves];
};

// The exchanges of both cooperative kernels (GS = kGran: stored Gram; GS = kOtfGran: the Gram
// recomputed, whose slots carry the candidate's row behind the common granules).  Slots alternate
// with the epoch's parity.
template <int GS>
__device__ __forceinline__ unsigned long long* coop_slot(unsigned long long* slot0, unsigned epoch) {
  return slot0 + (size_t)(epoch & 1) * kMaxMembers * GS;
}

// exchange 1: a member's step-1 partial (kb, idx, α_idx) in granules 0..4
__device__ __forceinline__ void coop_put1(unsigned long long* mine, unsigned epoch, const SmoRedPart& loc, double a) {
  put_u64(mine, epoch, loc.kb);
  put_granule(mine + 2, epoch, (unsigned)loc.idx);
  put_u64(mine + 3, epoch, bits_of(a));
}

struct CoopWin1 {
  unsigned long long kb;   // Gmax key
  int idx;                 // i
  double a;                // α_i
  int m;                   // the member that proposed it
};

template <int GS>
__device__ __forceinline__ CoopWin1 coop_fold1(const unsigned (*v)[GS], int W) {
  CoopWin1 r{u64_of(&v[0][0]), (int)v[0][2], f64_of(&v[0][3]), 0};
  for (int m = 1; m < W; ++m) {
    const unsigned long long k2 = u64_of(&v[m][0]);
    const int i2 = (int)v[m][2];
    if (k2 > r.kb || (k2 == r.kb && i2 > r.idx)) { r.kb = k2; r.idx = i2; r.a = f64_of(&v[m][3]); r.m = m; }
  }
  return r;
}

// exchange 2: (max yG over I_low, best objective key, j, α_j, G_j, K_ij) in granules 0..9
__device__ __forceinline__ void coop_put2(unsigned long long* mine, unsigned epoch, const SmoRedPart& loc, double aj,
                                          double gj, float kij) {
  put_u64(mine, epoch, loc.ka);
  put_u64(mine + 2, epoch, loc.kb);
  put_granule(mine + 4, epoch, (unsigned)loc.idx);
  put_u64(mine + 5, epoch, bits_of(aj));
  put_u64(mine + 7, epoch, bits_of(gj));
  put_granule(mine + 9, epoch, __float_as_uint(kij));
}

struct CoopWin2 {
  unsigned long long ka, kb;   // keys of max yG over I_low and of the best objective
  int j;
  double aj, Gj, Kij;
  int m;                       // the member that proposed j
};

template <int GS>
__device__ __forceinline__ CoopWin2 coop_fold2(const unsigned (*v)[GS], int W) {
  CoopWin2 r{u64_of(&v[0][0]), u64_of(&v[0][2]), (int)v[0][4], f64_of(&v[0][5]), f64_of(&v[0][7]),
             (double)__uint_as_float(v[0][9]), 0};
  for (int m = 1; m < W; ++m) {
    const unsigned long long a2 = u64_of(&v[m][0]);
    r.ka = a2 > r.ka ? a2 : r.ka;
    const unsigned long long k2 = u64_of(&v[m][2]);
    const int j2 = (int)v[m][4];
    if (k2 > r.kb || (k2 == r.kb && j2 > r.j)) {
      r.kb = k2;
      r.j = j2;
      r.aj = f64_of(&v[m][5]);
      r.Gj = f64_of(&v[m][7]);
      r.Kij = (double)__uint_as_float(v[m][9]);
      r.m = m;
    }
  }
  return r;
}

// calculate_rho over all members: every member's keys of max(−ub) and max(lb) and its free
// points' sum and count in granules 0..7, folded in member order by member 0, which also writes
// the iteration count and the gap.
template <int GS>
__device__ __forceinline__ void coop_rho_finish(double ru, double rl, double sum_free, int nfree,
                                                unsigned long long* slot0, unsigned epoch, int p, int w, int W,
                                                long long iter, double last_gap, CoopLds<GS>& sh,
                                                const SmoCoopOut& out) {
#pragma clang fp contract(off)
  const SmoRhoPart rp = smo_rho_block<kCoopWaves>(ru, rl, sum_free, nfree, sh.shA, sh.ssum);
  ++epoch;
  unsigned long long* s3 = coop_slot<GS>(slot0, epoch);
  if (threadIdx.x == 0) {
    unsigned long long* mine = s3 + w * GS;
    put_u64(mine, epoch, rp.kru);       // max(−yG) over the upper-bound candidates
    put_u64(mine + 2, epoch, rp.krl);   // max(yG) over the lower-bound candidates
    put_u64(mine + 4, epoch, bits_of(rp.S));
    put_u64(mine + 6, epoch, bits_of(rp.n));
  }
  if (!coop_gather_t<GS>(s3, W, 8, epoch, sh.vals[epoch & 1], out, &sh.fail)) return;
  if (w == 0 && threadIdx.x == 0) {
    const unsigned(*v)[GS] = sh.vals[epoch & 1];
    unsigned long long kru = u64_of(&v[0][0]), krl = u64_of(&v[0][2]);
    double St = 0.0, Ct = 0.0;
    for (int m = 0; m < W; ++m) {
      const unsigned long long a2 = u64_of(&v[m][0]), b2 = u64_of(&v[m][2]);
      kru = a2 > kru ? a2 : kru;
      krl = b2 > krl ? b2 : krl;
      St += f64_of(&v[m][4]);
      Ct += f64_of(&v[m][6]);
    }
    out.rho[p] = smo_rho_value(-f64_from_okey(kru), f64_from_okey(krl), St, Ct);
    out.iters[p] = (int)iter;
    out.gap[p] = last_gap;
  }
}

// Point ownership inside member w: thread tid, group g < K4, lane-of-vector e < 4 owns column
// c = w·S + 4·(tid + g·kCoopThreads) + e  (valid while c < min(lphys, (w+1)·S)).
//
// Mapped = false: column c of the stored Gram K_p is point c of the problem.
// Mapped = true: the problem is a Platt-CV sub-problem whose Gram is a principal submatrix of its
// parent's (the fit's final problem: same scaled rows, same γ, so the same f32 entries) — no Gram
// of its own is computed or stored.  K_p is the parent's; maps[moff + c] is the sub-problem's
// (libsvm-order) index of parent column c, or −1 when that row is in the held-out fold.  Members
// own contiguous PARENT columns, so row slices stay one float4 load; every point carries the key
// pk = index << 15 | column through the reductions and exchanges: comparing keys compares libsvm
// indices (ties → larger index, as unmapped), and the column locates its Gram row and its owner.
template <int K4, bool Mapped>
__global__ __launch_bounds__(kCoopThreads) void smo_coop_kernel(const SmoCoopProb* __restrict__ probs, int P,
                                                                int W, const float* __restrict__ K,
                                                                const int* __restrict__ maps,
                                                                double* __restrict__ alpha_all,
                                                                unsigned long long* __restrict__ xchg,
                                                                double eps, long long max_iter, SmoCoopOut out) {
  // libsvm's arithmetic (x86-64, no FMA): a*b + c*d stays un-contracted, as in smo_kernel
#pragma clang fp contract(off)
  constexpr int KM = 4 * K4;
  static_assert(KM <= 64, "per-thread point masks are 64-bit");
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int p = xcd + 8 * (q / W), w = q % W;
  if (p >= P) return;
  coop_inject_delay(out.inject_ticks, p, w);
  const SmoCoopProb Pr = probs[p];
  const float* Kp = K + Pr.koff;
  const int tid = threadIdx.x;
  if (Mapped && (Pr.lphys > kPkMask + 1 || Pr.l > kPkMask + 1)) {   // keys would overflow: every member leaves
    if (threadIdx.x == 0) atomicOr(out.err, 2u);
    return;
  }
  const int base = w * Pr.S;
  const int send = min(Pr.lphys, base + Pr.S);   // may be ≤ base: an empty member still exchanges
  unsigned long long* slot0 = xchg + (size_t)p * 2 * kMaxMembers * kGran;
  __shared__ CoopLds<kGran> sh;
  unsigned epoch = 0;

  double G[KM], A[KM];
  float Qi[KM];
  int PK[Mapped ? KM : 1];   // Mapped: key of the point in each slot
  SmoMasks M;
  unsigned long long validm = 0ull;
#pragma unroll
  for (int g = 0; g < K4; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * g + e;
      const int c = base + 4 * (tid + g * kCoopThreads) + e;
      G[k] = -1.0;   // p_i = −1 for C-SVC, α = 0
      A[k] = 0.0;
      Qi[k] = 0.f;
      int t = c;
      if constexpr (Mapped) {
        t = c >= send ? -1 : Pr.moff >= 0 ? maps[Pr.moff + c] : c;   // moff < 0: the problem's own Gram
        PK[k] = t >= 0 ? (t << kPkBits) | c : -1;
      }
      if (c < send && t >= 0) {
        validm |= 1ull << k;
        smo_masks_init(M, 1ull << k, t < Pr.npos);
      }
    }
  // key of slot k (unmapped: its column), and the column and libsvm index of a key
  auto key_of = [&](int k) {
    if constexpr (Mapped) return PK[k];
    else return base + 4 * (tid + (k >> 2) * kCoopThreads) + (k & 3);
  };
  auto col_of = [&](int t) { return Mapped ? (t & kPkMask) : t; };
  auto idx_of = [&](int t) { return Mapped ? (t >> kPkBits) : t; };
  // (thread, register slot) of the point with key t of this member
  auto owner_thr = [&](int t) { return ((col_of(t) - base) >> 2) % kCoopThreads; };
  auto owner_k = [&](int t) { return 4 * (((col_of(t) - base) >> 2) / kCoopThreads) + ((col_of(t) - base) & 3); };
  // While wave 0 polls an exchange, waves 1.. touch one dword per 128-byte line of the FULL Gram
  // row of this member's own candidate: the winning candidate's row — whichever member proposed
  // it — is then in this XCD's L2 (members of a problem share an XCD) when every member reads its
  // slice after the exchange, so the two dependent row reads of a pair cost an L2 hit instead of
  // an HBM round trip.  Issued after the owner's granule stores (a stalled owner would delay the
  // exchange itself) and consumed only after the exchange (the barrier waits on LDS traffic only,
  // so nothing waits for these loads until the data is long there).  Rows of ≤ 4·448·32 points
  // are covered entirely; longer rows only partly (a hint, never a correctness matter).
  struct Pf { float v[4]; };
  auto prefetch_issue = [&](int r) {
    Pf pf{{0.f, 0.f, 0.f, 0.f}};
    if (out.prefetch && r >= 0 && tid >= 64) {
      const float* row = Kp + (size_t)col_of(r) * Pr.ld;
      const int lines = (Pr.lphys + 31) >> 5;
      constexpr int kPf = kCoopThreads - 64;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = tid - 64 + u * kPf;
        if (c < lines) pf.v[u] = row[(size_t)c << 5];
      }
    }
    return pf;
  };
  auto prefetch_retire = [&](const Pf& pf) { asm volatile("" ::"v"(pf.v[0]), "v"(pf.v[1]), "v"(pf.v[2]), "v"(pf.v[3])); };
  // exchange 1: every member's step-1 partial (kb, idx, α_idx) → (Gmax key, i, α_i)
  auto exchange1 = [&](const SmoRedPart& loc, unsigned long long& kb, int& idx, double& a_i) -> bool {
    ++epoch;
    unsigned long long* s = coop_slot<kGran>(slot0, epoch);
    const bool has = loc.idx >= 0;
    if (has ? tid == owner_thr(loc.idx) : tid == 0)
      coop_put1(s + w * kGran, epoch, loc, has ? smo_pick<KM>(A, owner_k(loc.idx)) : 0.0);
    const Pf pf = prefetch_issue(loc.idx);
    if (!coop_gather_t<kGran>(s, W, 5, epoch, sh.vals[epoch & 1], out, &sh.fail)) return false;
    prefetch_retire(pf);
    const CoopWin1 r = coop_fold1<kGran>(sh.vals[epoch & 1], W);
    kb = r.kb;
    idx = r.idx;
    a_i = r.a;
    return true;
  };

  // ---- WSS step 1 for the first iteration
  SmoRedPart loc;
  {
    double bb = -kSmoInf;
    int bi = -1;
#pragma unroll
    for (int k = 0; k < KM; ++k)
      if ((M.upm >> k) & 1ull) {
        const int t = key_of(k);
        const double v = ((M.ypos >> k) & 1ull) ? -G[k] : G[k];
        smo_arg_take(bb, bi, v, t);
      }
    loc = smo_block_red<kCoopWaves, false>(-kSmoInf, bb, bi, sh.shA);
  }
  unsigned long long r1kb = 0ull;
  int i = -1;
  double ai_old = 0.0;
  if (!exchange1(loc, r1kb, i, ai_old)) return;
  long long iter = 0;
  double last_gap = 0.0;
  long long ph[7] = {0, 0, 0, 0, 0, 0, 0};
  const bool prof = out.prof != nullptr && w == 0 && tid == 0;
  long long tc = prof ? __builtin_amdgcn_s_memtime() : 0;
  auto tick = [&](int k) {
    if (prof) {
      const long long now = __builtin_amdgcn_s_memtime();
      ph[k] += now - tc;
      tc = now;
    }
  };
  for (; iter < max_iter; ++iter) {
    if (i < 0) break;
    const double Gmax = f64_from_okey(r1kb);
    const int yi = idx_of(i) < Pr.npos ? 1 : -1;
    // ---- WSS step 2 over this member's slice of row i
    const float4* Ki4 = reinterpret_cast<const float4*>(Kp + (size_t)col_of(i) * Pr.ld + base);
    double gmax2 = -kSmoInf, bkey = -kSmoInf;
    int bj = -1;
    float4 qv[K4];
#pragma unroll
    for (int g = 0; g < K4; ++g)
      qv[g] = base + 4 * (tid + g * kCoopThreads) < send ? Ki4[tid + g * kCoopThreads] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int g = 0; g < K4; ++g) {
      const int t0 = base + 4 * (tid + g * kCoopThreads);
      const float4 qq = qv[g];
      Qi[4 * g] = qq.x; Qi[4 * g + 1] = qq.y; Qi[4 * g + 2] = qq.z; Qi[4 * g + 3] = qq.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 4 * g + e;
        if ((M.lowm >> k) & 1ull) {
          const double yG = ((M.ypos >> k) & 1ull) ? G[k] : -G[k];
          gmax2 = fmax(gmax2, yG);
          const double gd = Gmax + yG;
          if (gd > 0) {
            const double key = smo_wss2_key(gd, Qi[k]);
            if constexpr (Mapped) {   // slots are in column order, not index order
              if (bj < 0 || key > bkey || (key == bkey && key_of(k) > bj)) { bkey = key; bj = key_of(k); }
            } else if (bj < 0 || key >= bkey) { bkey = key; bj = t0 + e; }
          }
        }
      }
    }
    tick(0);
    loc = smo_block_red<kCoopWaves>(gmax2, bj >= 0 ? bkey : -kSmoInf, bj, sh.shB);
    tick(1);
    // ---- exchange 2: (max yG over I_low, best objective key, j, α_j, G_j, K_ij)
    ++epoch;
    unsigned long long* s2 = coop_slot<kGran>(slot0, epoch);
    {
      const bool has = loc.idx >= 0;
      if (has ? tid == owner_thr(loc.idx) : tid == 0) {
        const int kk = has ? owner_k(loc.idx) : 0;
        coop_put2(s2 + w * kGran, epoch, loc, has ? smo_pick<KM>(A, kk) : 0.0, has ? smo_pick<KM>(G, kk) : 0.0,
                  has ? smo_pick<KM>(Qi, kk) : 0.f);
      }
    }
    const Pf pf2 = prefetch_issue(loc.idx);
    if (!coop_gather_t<kGran>(s2, W, 10, epoch, sh.vals[epoch & 1], out, &sh.fail)) return;
    prefetch_retire(pf2);
    tick(2);
    const CoopWin2 r2 = coop_fold2<kGran>(sh.vals[epoch & 1], W);
    const int j = r2.j;
    const double gmax2_all = f64_from_okey(r2.ka);
    last_gap = Gmax + gmax2_all;
    if (Gmax + gmax2_all < eps || j < 0) break;
    // ---- pair update (identical in every member)
    const int yj = idx_of(j) < Pr.npos ? 1 : -1;
    const double Ci = yi > 0 ? Pr.Cp : Pr.Cn, Cj = yj > 0 ? Pr.Cp : Pr.Cn;
    const SmoPair pr = smo_pair_update(yi, yj, Ci, Cj, r2.Kij, Gmax, r2.Gj, ai_old, r2.aj);
    const double ci = pr.ci, cj = pr.cj;
    tick(3);
    // owners in this member: α and the bound masks of i and j
#pragma unroll
    for (int wv = 0; wv < 2; ++wv) {
      const int t = wv == 0 ? i : j;
      if (col_of(t) < base || col_of(t) >= send || tid != owner_thr(t)) continue;
      const int kk = owner_k(t);
      const double a = wv == 0 ? pr.ai : pr.aj;
      smo_put<KM>(A, kk, a);
      smo_masks_set(M, 1ull << kk, a, wv == 0 ? Ci : Cj);
    }
    // ---- gradient update of this member's slice (row i in registers, row j loaded now), fused
    // with the next step-1 candidates
    const float4* Kj4 = reinterpret_cast<const float4*>(Kp + (size_t)col_of(j) * Pr.ld + base);
    float4 qjv[K4];
#pragma unroll
    for (int g = 0; g < K4; ++g)
      qjv[g] = base + 4 * (tid + g * kCoopThreads) < send ? Kj4[tid + g * kCoopThreads] : make_float4(0.f, 0.f, 0.f, 0.f);
    double bb = -kSmoInf;
    int bi = -1;
#pragma unroll
    for (int g = 0; g < K4; ++g) {
      const int t0 = base + 4 * (tid + g * kCoopThreads);
      const float4 qq = qjv[g];
      const float qj[4] = {qq.x, qq.y, qq.z, qq.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 4 * g + e;
        const bool pos = (M.ypos >> k) & 1ull;
        const double upd = (double)Qi[k] * ci + (double)qj[e] * cj;
        G[k] += pos ? upd : -upd;
        if ((M.upm >> k) & 1ull) {
          const double v = pos ? -G[k] : G[k];
          const int tk = Mapped ? key_of(k) : t0 + e;
          smo_arg_take(bb, bi, v, tk);
        }
      }
    }
    tick(4);
    loc = smo_block_red<kCoopWaves, false>(-kSmoInf, bb, bi, sh.shA);
    tick(5);
    if (!exchange1(loc, r1kb, i, ai_old)) return;
    tick(6);
  }
  if (prof)
    for (int k = 0; k < 7; ++k) out.prof[(size_t)p * 7 + k] = ph[k];
  // ---- α out (owners) and calculate_rho over all members
#pragma unroll
  for (int k = 0; k < KM; ++k)
    if ((validm >> k) & 1ull) alpha_all[Pr.aoff + idx_of(key_of(k))] = A[k];
  double ru = -kSmoInf, rl = -kSmoInf, sum_free = 0.0;
  int nfree = 0;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (!((validm >> k) & 1ull)) continue;
    const bool pos = (M.ypos >> k) & 1ull;
    smo_rho_classify(pos, (M.upperm >> k) & 1ull, (M.freem >> k) & 1ull, pos ? G[k] : -G[k], ru, rl, sum_free, nfree);
  }
  coop_rho_finish<kGran>(ru, rl, sum_free, nfree, slot0, epoch, p, w, W, iter, last_gap, sh, out);
}

// Exchange deadline and the late-member test hook, from the environment (read per launch).
static void coop_timing(SmoCoopOut& o) {
  const char* w = std::getenv("HFENS_SMO_WAIT_MS");
  const char* d = std::getenv("HFENS_SMO_INJECT_DELAY_MS");
  const double wait_ms = (w && w[0]) ? std::atof(w) : (double)kWaitMsDefault;
  o.wait_ticks = (long long)(wait_ms * 1e5);               // 100 MHz counter
  o.inject_ticks = (d && d[0]) ? (long long)(std::atof(d) * 1e5) : 0;
}

// What both cooperative launchers do ahead of the launch: the member and problem counts, the CU
// bound, the exchange deadline, and the zeroed exchange buffer (`gran` granules per member slot).
// Returns the block count.
static unsigned coop_prepare(const char* op, int P, int W, uintptr_t xchg, int gran, SmoCoopOut& o, hipStream_t st) {
  const std::string name(op);
  HFENS_REQUIRE(W >= 1 && W <= kMaxMembers, name + ": 1 <= W <= 16 members per problem");
  HFENS_REQUIRE(P >= 1, name + ": no problems");
  int dev = 0, ncu = 256;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  // members spin on each other, so all of them must be resident at once: at most one member per
  // CU (a 512-thread block always fits beside anything else's finished work); the padding
  // blocks of an incomplete group of 8 problems exit at once
  HFENS_REQUIRE((long long)P * W <= ncu, name + ": P·W exceeds the CU count (choose a smaller W)");
  coop_timing(o);
  // every polled granule starts at epoch 0 (epochs count from 1 within the call)
  HFENS_CHECK(hipMemsetAsync((void*)xchg, 0, (size_t)P * 2 * kMaxMembers * gran * sizeof(unsigned long long), st));
  return (unsigned)(8LL * ((P + 7) / 8) * W);
}

// Members of one problem spin on each other, so all of them must be resident together: the
// launchers bound P·W by the CU count (one member per CU), and the Python side subtracts the CUs
// it leaves to concurrent kernels.  This returns what the hardware would co-schedule of the
// kernel on an idle device (occupancy per CU × CUs): the upper bound models/smo.py clamps W with.
void coop_resident_blocks(uintptr_t out) {
  int dev = 0, ncu = 256, per_cu = 0;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  HFENS_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, smo_coop_kernel<8, true>, kCoopThreads, 0));
  ((long long*)out)[0] = (long long)per_cu * ncu;
  ((long long*)out)[1] = ncu;
}

void smo_coop_batch(uintptr_t probs, int P, int W, int max_S, uintptr_t K, uintptr_t maps, uintptr_t alpha,
                    uintptr_t xchg, double eps, long long max_iter, uintptr_t rho, uintptr_t iters, uintptr_t gap,
                    uintptr_t err, uintptr_t prof, uintptr_t stream) {
  HFENS_REQUIRE(max_S >= 4 && max_S % 4 == 0, "smo_coop_batch: slice must be a positive multiple of 4");
  const char* pfe = std::getenv("HFENS_SMO_PREFETCH");
  SmoCoopOut o{(double*)rho, (int*)iters, (double*)gap, (unsigned*)err, (long long*)prof,
               (pfe && pfe[0] == '0') ? 0 : 1};
  hipStream_t st = as_stream(stream);
  const unsigned blocks = coop_prepare("smo_coop_batch", P, W, xchg, kGran, o, st);
  auto pp = (const SmoCoopProb*)probs;
  auto kp = (const float*)K;
  auto ap = (double*)alpha;
  auto xp = (unsigned long long*)xchg;
  auto mp = (const int*)maps;
  // maps != 0: Platt sub-problems index their parents' Grams (columns < 2^15: checked per problem
  // in the kernel, which flags err and leaves — the host then re-solves unmapped)
#define COOP_CASE(K4)                                                                                           \
  if (max_S <= 4 * K4 * kCoopThreads) {                                                                         \
    if (mp != nullptr)                                                                                          \
      hipLaunchKernelGGL((smo_coop_kernel<K4, true>), dim3(blocks), dim3(kCoopThreads), 0, st, pp, P, \
                         W, kp, mp, ap, xp, eps, max_iter, o);                                                  \
    else                                                                                                        \
      hipLaunchKernelGGL((smo_coop_kernel<K4, false>), dim3(blocks), dim3(kCoopThreads), 0, st, pp,   \
                         P, W, kp, mp, ap, xp, eps, max_iter, o);                                               \
    launch_check();                                                                                             \
    return;                                                                                                     \
  }
  COOP_CASE(1) COOP_CASE(2) COOP_CASE(4) COOP_CASE(8)
#undef COOP_CASE
  throw std::invalid_argument("smo_coop_batch: slice larger than 16384 points");
}

// ------------------------------------------------------------------------------------------
// smo_coop_otf: the same cooperative solver with NO stored Gram.  Each thread keeps its points'
// rows z_t and norms ‖z_t‖² in registers and re-evaluates its entries of Gram rows i and j per
// pair with gram_rbf_kernel's exact expression — its f32-input MFMA dot product is bit-for-bit a
// k-ordered fmaf chain, then the same norm sum, clamp and exp2 — so the values, and hence the
// pair sequence, equal the stored-Gram solvers'.  z_i and z_j travel inside the two exchanges
// (the candidate's owner publishes its row as F + 1 more granules), so a pair reads nothing from
// HBM: two in-launch exchanges plus register arithmetic.  Memory is O(l·F) instead of O(l²) (the
// bench's 36 problems: 7 GB of Gram neither written nor re-read) and the Gram launch goes away.
// Points are strided over threads (t = base + tid + 512·m): no vector-load layout to keep.
// Measured: at ≤ 2 points per thread it runs with the stored-Gram kernel; at 4 points per thread
// (256 VGPRs + spills) it is slower, so the host picks it only for slices of ≤ 1024 points.
struct SmoOtfProb {
  long long zoff;   // first row of this problem in zcat ([rows][F] f32, problem order)
  long long aoff;   // alpha offset (doubles)
  int l;            // problem size
  int npos;         // indices [0, npos) have y = +1, the rest y = −1
  int S;            // points per member: member w owns [w·S, min(l, (w+1)·S))
  float ngl2e;      // −γ·log2(e)
  double Cp, Cn;
};

constexpr int kOtfGran = 32;   // granules per member slot: exchange 2 carries 11 + F
constexpr int kOtfMaxF = 20;

__device__ __forceinline__ float rbf_entry(float dot, float nr, float nc, float ngl2e) {
  float d2 = fmaf(-2.f, dot, nr + nc);   // gram_rbf_kernel's epilogue, operand for operand
  d2 = fmaxf(d2, 0.f);
  return __builtin_amdgcn_exp2f(ngl2e * d2);
}

template <int KM, int FP>
__global__ __launch_bounds__(kCoopThreads) void smo_coop_otf_kernel(const SmoOtfProb* __restrict__ probs, int P,
                                                                    int W, int F, const float* __restrict__ zcat,
                                                                    double* __restrict__ alpha_all,
                                                                    unsigned long long* __restrict__ xchg,
                                                                    double eps, long long max_iter, SmoCoopOut out) {
#pragma clang fp contract(off)
  static_assert(KM <= 64 && FP <= kOtfMaxF, "register tile");
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int p = xcd + 8 * (q / W), w = q % W;
  if (p >= P) return;
  coop_inject_delay(out.inject_ticks, p, w);
  const SmoOtfProb Pr = probs[p];
  const int tid = threadIdx.x;
  const int base = w * Pr.S;
  const int send = min(Pr.l, base + Pr.S);   // may be ≤ base: an empty member still exchanges
  unsigned long long* slot0 = xchg + (size_t)p * 2 * kMaxMembers * kOtfGran;
  __shared__ CoopLds<kOtfGran> sh;
  unsigned epoch = 0;

  float zr[KM][FP], nz[KM];   // this thread's points: rows and squared norms
  double G[KM], A[KM];
  float Qi[KM], Qj[KM];
  SmoMasks M;
  unsigned long long validm = 0ull;
#pragma unroll
  for (int m = 0; m < KM; ++m) {
    const int t = base + tid + kCoopThreads * m;
    const bool ok = t < send;
    const float* zt = zcat + (size_t)(Pr.zoff + (ok ? t : 0)) * F;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < FP; ++k) {
      zr[m][k] = (ok && k < F) ? zt[k] : 0.f;
      if (k < F) sq = fmaf(zr[m][k], zr[m][k], sq);
    }
    nz[m] = sq;
    G[m] = -1.0;   // p_i = −1 for C-SVC, α = 0
    A[m] = 0.0;
    Qi[m] = 0.f;
    Qj[m] = 0.f;
    if (ok) {
      validm |= 1ull << m;
      smo_masks_init(M, 1ull << m, t < Pr.npos);
    }
  }
  auto owner_thr = [&](int t) { return (t - base) % kCoopThreads; };
  auto owner_m = [&](int t) { return (t - base) / kCoopThreads; };
  // this thread's entries of Gram row r; the row's features and norm come from an exchange (LDS)
  auto gram_row = [&](int r, const unsigned* zb, float nzr, float* Qo) {
    float zrow[FP];
#pragma unroll
    for (int k = 0; k < FP; ++k) zrow[k] = k < F ? __uint_as_float(zb[k]) : 0.f;
#pragma unroll
    for (int m = 0; m < KM; ++m) {
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < FP; ++k)
        if (k < F) dot = fmaf(zrow[k], zr[m][k], dot);
      Qo[m] = base + tid + kCoopThreads * m == r ? 1.f : rbf_entry(dot, nzr, nz[m], Pr.ngl2e);
    }
  };
  // owner of point t: granule 0 = ‖z_t‖², granules 1..F = z_t
  auto publish_row = [&](unsigned long long* dst, int t) {
    const int mm = owner_m(t);
    float nn = 0.f, zz[FP];
#pragma unroll
    for (int k = 0; k < FP; ++k) zz[k] = 0.f;
#pragma unroll
    for (int m = 0; m < KM; ++m)
      if (m == mm) {
        nn = nz[m];
#pragma unroll
        for (int k = 0; k < FP; ++k) zz[k] = zr[m][k];
      }
    put_granule(dst, epoch, __float_as_uint(nn));
#pragma unroll
    for (int k = 0; k < FP; ++k)
      if (k < F) put_granule(dst + 1 + k, epoch, __float_as_uint(zz[k]));
  };
  auto publish_zero_row = [&](unsigned long long* dst) {
    for (int k = 0; k <= F; ++k) put_granule(dst + k, epoch, 0u);
  };
  // exchange 1: (kb, idx, α_idx, ‖z_idx‖², z_idx) → (Gmax key, i, α_i, member holding z_i)
  auto exchange1 = [&](const SmoRedPart& loc, unsigned long long& kb, int& idx, double& a_i, int& ms) -> bool {
    ++epoch;
    unsigned long long* s = coop_slot<kOtfGran>(slot0, epoch);
    const bool has = loc.idx >= 0;
    if (has ? tid == owner_thr(loc.idx) : tid == 0) {
      unsigned long long* mine = s + w * kOtfGran;
      coop_put1(mine, epoch, loc, has ? smo_pick<KM>(A, owner_m(loc.idx)) : 0.0);
      if (has) publish_row(mine + 5, loc.idx);
      else publish_zero_row(mine + 5);
    }
    if (!coop_gather_t<kOtfGran>(s, W, 6 + F, epoch, sh.vals[epoch & 1], out, &sh.fail)) return false;
    const CoopWin1 r = coop_fold1<kOtfGran>(sh.vals[epoch & 1], W);
    kb = r.kb;
    idx = r.idx;
    a_i = r.a;
    ms = r.m;
    return true;
  };

  // ---- WSS step 1 for the first iteration
  SmoRedPart loc;
  {
    double bb = -kSmoInf;
    int bi = -1;
#pragma unroll
    for (int m = 0; m < KM; ++m)
      if ((M.upm >> m) & 1ull) {
        const int t = base + tid + kCoopThreads * m;
        const double v = ((M.ypos >> m) & 1ull) ? -G[m] : G[m];
        smo_arg_take(bb, bi, v, t);
      }
    loc = smo_block_red<kCoopWaves, false>(-kSmoInf, bb, bi, sh.shA);
  }
  unsigned long long r1kb = 0ull;
  int i = -1, mi = 0;
  double ai_old = 0.0;
  if (!exchange1(loc, r1kb, i, ai_old, mi)) return;
  long long iter = 0;
  double last_gap = 0.0;
  for (; iter < max_iter; ++iter) {
    if (i < 0) break;
    const double Gmax = f64_from_okey(r1kb);
    const int yi = i < Pr.npos ? 1 : -1;
    {
      const unsigned* zb = &sh.vals[epoch & 1][mi][6];
      gram_row(i, zb, __uint_as_float(sh.vals[epoch & 1][mi][5]), Qi);
    }
    // ---- WSS step 2 over this member's entries of row i
    double gmax2 = -kSmoInf, bkey = -kSmoInf;
    int bj = -1;
#pragma unroll
    for (int m = 0; m < KM; ++m) {
      if ((M.lowm >> m) & 1ull) {
        const double yG = ((M.ypos >> m) & 1ull) ? G[m] : -G[m];
        gmax2 = fmax(gmax2, yG);
        const double gd = Gmax + yG;
        if (gd > 0) {
          const double key = smo_wss2_key(gd, Qi[m]);
          if (bj < 0 || key >= bkey) { bkey = key; bj = base + tid + kCoopThreads * m; }
        }
      }
    }
    loc = smo_block_red<kCoopWaves>(gmax2, bj >= 0 ? bkey : -kSmoInf, bj, sh.shB);
    // ---- exchange 2: (max yG over I_low, best key, j, α_j, G_j, K_ij, ‖z_j‖², z_j)
    ++epoch;
    unsigned long long* s2 = coop_slot<kOtfGran>(slot0, epoch);
    {
      const bool has = loc.idx >= 0;
      if (has ? tid == owner_thr(loc.idx) : tid == 0) {
        unsigned long long* mine = s2 + w * kOtfGran;
        const int mm = has ? owner_m(loc.idx) : 0;
        coop_put2(mine, epoch, loc, has ? smo_pick<KM>(A, mm) : 0.0, has ? smo_pick<KM>(G, mm) : 0.0,
                  has ? smo_pick<KM>(Qi, mm) : 0.f);
        if (has) publish_row(mine + 10, loc.idx);
        else publish_zero_row(mine + 10);
      }
    }
    if (!coop_gather_t<kOtfGran>(s2, W, 11 + F, epoch, sh.vals[epoch & 1], out, &sh.fail)) return;
    const CoopWin2 r2 = coop_fold2<kOtfGran>(sh.vals[epoch & 1], W);
    const int j = r2.j, mj = r2.m;
    const double gmax2_all = f64_from_okey(r2.ka);
    last_gap = Gmax + gmax2_all;
    if (Gmax + gmax2_all < eps || j < 0) break;
    // ---- pair update (identical in every member; libsvm's clipping)
    const int yj = j < Pr.npos ? 1 : -1;
    const double Ci = yi > 0 ? Pr.Cp : Pr.Cn, Cj = yj > 0 ? Pr.Cp : Pr.Cn;
    const SmoPair pr = smo_pair_update(yi, yj, Ci, Cj, r2.Kij, Gmax, r2.Gj, ai_old, r2.aj);
    const double ci = pr.ci, cj = pr.cj;
#pragma unroll
    for (int wv = 0; wv < 2; ++wv) {
      const int t = wv == 0 ? i : j;
      if (t < base || t >= send || tid != owner_thr(t)) continue;
      const int mm = owner_m(t);
      const double a = wv == 0 ? pr.ai : pr.aj;
      smo_put<KM>(A, mm, a);
      smo_masks_set(M, 1ull << mm, a, wv == 0 ? Ci : Cj);
    }
    // ---- gradient update with rows i (registers) and j (recomputed now), fused with the next
    // step-1 candidates
    gram_row(j, &sh.vals[epoch & 1][mj][11], __uint_as_float(sh.vals[epoch & 1][mj][10]), Qj);
    double bb = -kSmoInf;
    int bi = -1;
#pragma unroll
    for (int m = 0; m < KM; ++m) {
      const bool pos = (M.ypos >> m) & 1ull;
      const double upd = (double)Qi[m] * ci + (double)Qj[m] * cj;
      G[m] += pos ? upd : -upd;
      if ((M.upm >> m) & 1ull) {
        const int t = base + tid + kCoopThreads * m;
        const double v = pos ? -G[m] : G[m];
        smo_arg_take(bb, bi, v, t);
      }
    }
    loc = smo_block_red<kCoopWaves, false>(-kSmoInf, bb, bi, sh.shA);
    if (!exchange1(loc, r1kb, i, ai_old, mi)) return;
  }
  // ---- α out (owners) and calculate_rho over all members
#pragma unroll
  for (int m = 0; m < KM; ++m)
    if ((validm >> m) & 1ull) alpha_all[Pr.aoff + base + tid + kCoopThreads * m] = A[m];
  double ru = -kSmoInf, rl = -kSmoInf, sum_free = 0.0;
  int nfree = 0;
#pragma unroll
  for (int m = 0; m < KM; ++m) {
    if (!((validm >> m) & 1ull)) continue;
    const bool pos = (M.ypos >> m) & 1ull;
    smo_rho_classify(pos, (M.upperm >> m) & 1ull, (M.freem >> m) & 1ull, pos ? G[m] : -G[m], ru, rl, sum_free, nfree);
  }
  coop_rho_finish<kOtfGran>(ru, rl, sum_free, nfree, slot0, epoch, p, w, W, iter, last_gap, sh, out);
}

void smo_coop_otf_batch(uintptr_t probs, int P, int W, int F, int max_S, uintptr_t zcat, uintptr_t alpha,
                        uintptr_t xchg, double eps, long long max_iter, uintptr_t rho, uintptr_t iters,
                        uintptr_t gap, uintptr_t err, uintptr_t stream) {
  HFENS_REQUIRE(F >= 1 && F <= kOtfMaxF, "smo_coop_otf_batch: 1 <= F <= 20 (rows held in registers)");
  HFENS_REQUIRE(max_S >= 1 && max_S <= 4 * kCoopThreads, "smo_coop_otf_batch: at most 2048 points per member");
  SmoCoopOut o{(double*)rho, (int*)iters, (double*)gap, (unsigned*)err, nullptr};
  hipStream_t st = as_stream(stream);
  const unsigned blocks = coop_prepare("smo_coop_otf_batch", P, W, xchg, kOtfGran, o, st);
  auto pp = (const SmoOtfProb*)probs;
  auto zp = (const float*)zcat;
  auto ap = (double*)alpha;
  auto xp = (unsigned long long*)xchg;
  const int KM = (max_S + kCoopThreads - 1) / kCoopThreads;
#define OTF_CASE(KM_, FP_)                                                                                   \
  if (KM <= KM_ && F <= FP_) {                                                                               \
    hipLaunchKernelGGL((smo_coop_otf_kernel<KM_, FP_>), dim3(blocks), dim3(kCoopThreads), 0, st, pp, \
                       P, W, F, zp, ap, xp, eps, max_iter, o);                                              \
    launch_check();                                                                                          \
    return;                                                                                                  \
  }
  OTF_CASE(1, 8) OTF_CASE(1, 20) OTF_CASE(2, 8) OTF_CASE(2, 20) OTF_CASE(4, 8) OTF_CASE(4, 20)
#undef OTF_CASE
  throw std::invalid_argument("smo_coop_otf_batch: unsupported tile");
}

}  // namespace hfens
