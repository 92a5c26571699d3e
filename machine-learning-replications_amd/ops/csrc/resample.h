// What the bootstrap ops (bootstrap.hip, calibration.hip, compare.hip) share: the resampling law,
// the block-wide scan of the drawn multiplicities, the rank statistics and the launch path.  One
// 1024-thread workgroup handles a replicate; thread t owns rows [t·chunk, (t+1)·chunk).
//
// The law (the host mirror and the oracles in ops/reference.py follow it; the ops score the same
// resamples bit for bit because they all draw through boot_draw below):
//   draw j of replicate b over a stratum of m rows:
//     u = splitmix64(seed ^ splitmix64((b << 40) ^ j)),  r = ((u >> 32)·m) >> 32   ∈ [0, m)
//   plain: j ∈ [0, n), m = n, row r.  stratified: j < P draws the r-th positive (m = P), j ≥ P the
//   r-th negative (m = N).  `map`, if given, turns the drawn row (p0 + r in the second stratum) into
//   the index that is counted; no map counts the drawn row itself.
#pragma once
#include "common.h"

#include <algorithm>
#include <string>

#pragma clang fp contract(off)   // the mirror rounds a + b·c twice; so does everything below

namespace hfens {

constexpr int kBootThreads = 1024;
constexpr int kBootWaves = kBootThreads / kWave;
constexpr long long kBootMaxN = 1LL << 25;   // doubled AUROC numerator < 2^53
constexpr long long kBootMaxB = 1LL << 24;   // replicate index shares the counter with the draw
constexpr int kBootLdsPerCu = 160 * 1024;

__device__ __forceinline__ double boot_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

struct BootThread { int tid, lane, wave, r0, r1; };   // r0:r1 = the thread's rows

__device__ __forceinline__ BootThread boot_thread(int n) {
  const int tid = threadIdx.x, chunk = (n + kBootThreads - 1) / kBootThreads;
  const int r0 = min(n, tid * chunk);
  return {tid, tid & (kWave - 1), tid / kWave, r0, min(n, r0 + chunk)};
}

// Zero cnt[0, n), count replicate b's n draws into it with integer atomics, and end on the barrier.
__device__ __forceinline__ void boot_draw(unsigned* cnt, const int* map, int n, int p0, unsigned long long seed,
                                          unsigned long long b) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += kBootThreads) cnt[i] = 0u;
  __syncthreads();
  for (int j = tid; j < n; j += kBootThreads) {
    const unsigned long long u = splitmix64(seed ^ splitmix64((b << 40) ^ (unsigned long long)j));
    const bool head = j < p0;
    const unsigned long long m = head ? p0 : n - p0;
    const int r = (int)(((u >> 32) * m) >> 32);
    const int at = (head ? 0 : p0) + r;
    atomicAdd(&cnt[map ? map[at] : at], 1u);
  }
  __syncthreads();
}

// Block-wide inclusive scan of the (positive, negative) multiplicities: cp holds the counts on entry
// and the cumulative positives on return, cn the cumulative negatives; y is the label of every row.
// The second walk calls row(i, c, pos) on every row of the thread with its count, in row order.  The
// caller's next barrier publishes cp and cn.
template <class Row>
__device__ __forceinline__ void boot_scan(unsigned* cp, unsigned* cn, const unsigned char* y, const BootThread& t,
                                          unsigned (*sc_pn)[2], Row row) {
  unsigned sp = 0, sn = 0;
  for (int i = t.r0; i < t.r1; ++i) {
    const unsigned c = cp[i];
    if (y[i]) sp += c; else sn += c;
  }
  unsigned ip = sp, in = sn;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned tp = __shfl_up(ip, o, kWave), tn = __shfl_up(in, o, kWave);
    if (t.lane >= o) { ip += tp; in += tn; }
  }
  if (t.lane == kWave - 1) { sc_pn[t.wave][0] = ip; sc_pn[t.wave][1] = in; }
  __syncthreads();
  unsigned runp = ip - sp, runn = in - sn;
  for (int w = 0; w < t.wave; ++w) { runp += sc_pn[w][0]; runn += sc_pn[w][1]; }
  for (int i = t.r0; i < t.r1; ++i) {
    const unsigned c = cp[i];
    const bool pos = y[i] != 0;
    // negatives first, as selects: on the global path hipcc then issues the two stores back to back, as
    // the kernels did before they shared this function.  With an address increment scheduled between
    // them (what `if (pos) runp += c; else runn += c;` gives here) bootstrap_metrics at n = 10^6 is 3 % slower.
    runn += pos ? 0u : c;
    runp += pos ? c : 0u;
    cp[i] = runp;
    cn[i] = runn;
    row(i, c, pos);
  }
}

// Rank statistics of one scanned score order: the tie-group sums for the doubled AUROC numerator
// (u64, exact) and AP (f64: chunk → wave xor tree → waves in order, which depends on n alone), then
// thread 0 writes a2, pn (unless null), auroc, ap and the confusion counts of the first k0 rows.
// The tie groups come from the caller: group(e, f), called on the thread's rows in row order, says
// whether row e ends its group and, if it does, sets f to the group's first row.
// Pb, Nb = cp[n−1], cn[n−1].
template <class Group>
__device__ __forceinline__ void boot_rank_stats(const unsigned* cp, const unsigned* cn, Group group,
                                                const BootThread& t, unsigned Pb, unsigned Nb,
                                                int k0, unsigned long long* sc_a2, double* sc_ap, long long* a2_out,
                                                long long* pn, double* auroc, double* ap, long long* conf) {
  unsigned long long a2 = 0;
  double apv = 0.0;
  for (int e = t.r0; e < t.r1; ++e) {
    int f;
    if (!group(e, f)) continue;
    const unsigned tp = cp[e], fp = cn[e];
    const unsigned tp0 = f > 0 ? cp[f - 1] : 0u, fp0 = f > 0 ? cn[f - 1] : 0u;
    a2 += (unsigned long long)(fp - fp0) * (unsigned long long)(tp + tp0);
    if (tp != tp0) apv += (double)((unsigned long long)(tp - tp0) * tp) / (double)(tp + fp);   // product < 2^50: exact
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a2 += __shfl_xor(a2, o, kWave);
  apv = wave_sum(apv);
  if (t.lane == 0) { sc_a2[t.wave] = a2; sc_ap[t.wave] = apv; }
  __syncthreads();
  if (t.tid == 0) {
    const bool degenerate = Pb == 0u || Nb == 0u;
    unsigned long long A2 = 0;
    double aps = 0.0;
    for (int w = 0; w < kBootWaves; ++w) { A2 += sc_a2[w]; aps += sc_ap[w]; }
    *a2_out = (long long)A2;
    if (pn) { pn[0] = Pb; pn[1] = Nb; }
    *auroc = degenerate ? boot_nan() : (double)A2 / (double)(2ull * Pb * Nb);
    *ap = degenerate ? boot_nan() : aps / (double)Pb;
    const unsigned tp = k0 > 0 ? cp[k0 - 1] : 0u, fp = k0 > 0 ? cn[k0 - 1] : 0u;
    conf[0] = tp;
    conf[1] = fp;
    conf[2] = Pb - tp;
    conf[3] = Nb - fp;
  }
}

// The same with the tie groups precomputed: group k ends at row e = glast[e] and starts at f = gfirst[e].
__device__ __forceinline__ void boot_rank_stats(const unsigned* cp, const unsigned* cn, const int* gfirst,
                                                const int* glast, const BootThread& t, unsigned Pb, unsigned Nb,
                                                int k0, unsigned long long* sc_a2, double* sc_ap, long long* a2_out,
                                                long long* pn, double* auroc, double* ap, long long* conf) {
  boot_rank_stats(cp, cn, [gfirst, glast](int e, int& f) {
    if (glast[e] != e) return false;
    f = gfirst[e];
    return true;
  }, t, Pb, Nb, k0, sc_a2, sc_ap, a2_out, pn, auroc, ap, conf);
}

// The launch path of the three ops: the requirements they share, the grid, the LDS-or-global launch.
// use_lds: `words` u32 arrays of n rows in LDS (n ≤ lds_rows) beside the kernel's static_lds bytes, or
// in `ws` = [ws_slices][words·n] u32, one slice per workgroup.  grid ≤ 0 picks one; the results do
// not depend on it.  A.nb == 0 launches nothing.
template <class Args>
void boot_launch(const std::string& op, void (*lds_kernel)(Args), void (*global_kernel)(Args), const Args& A,
                 int words, int lds_rows, int static_lds, long long n, long long p0, long long b0, long long nb,
                 int use_lds, uintptr_t ws, long long ws_slices, int grid, uintptr_t stream) {
  HFENS_REQUIRE(n >= 1 && n <= kBootMaxN, op + ": 1 <= n <= 2^25");
  HFENS_REQUIRE(p0 >= 1 && p0 <= n, op + ": first stratum must hold 1..n rows");
  HFENS_REQUIRE(b0 >= 0 && nb >= 0 && b0 + nb <= kBootMaxB, op + ": replicates must lie in [0, 2^24]");
  HFENS_REQUIRE(use_lds ? n <= lds_rows : (ws != 0 && ws_slices >= 1),
                op + ": n exceeds the LDS path / no global workspace");
  if (nb == 0) return;
  int dev = 0, ncu = 256;
  HFENS_CHECK(hipGetDevice(&dev));
  HFENS_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t lds = use_lds ? 4 * (size_t)words * (size_t)n : 0;
  // at most two 1024-thread workgroups are resident on a CU
  long long cap = use_lds ? (long long)ncu * std::min(2, (int)(kBootLdsPerCu / (lds + static_lds)))
                          : std::min(2LL * ncu, ws_slices);
  if (grid > 0) cap = use_lds ? grid : std::min((long long)grid, ws_slices);
  grid = (int)std::min(nb, cap);
  hipStream_t st = as_stream(stream);
  if (use_lds) {
    if (lds > 48 * 1024)
      HFENS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lds_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(lds_kernel, dim3(grid), dim3(kBootThreads), lds, st, A);
  } else {
    hipLaunchKernelGGL(global_kernel, dim3(grid), dim3(kBootThreads), 0, st, A);
  }
  launch_check();
}

}  // namespace hfens
