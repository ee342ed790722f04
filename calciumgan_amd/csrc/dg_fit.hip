// Latent correlations of the dichotomised-Gaussian model (DESIGN.md 20;
// data/dg_fit.py gauss_correlation is the numpy statement): for every neuron
// pair i > j the root in lambda of
//
//   f(lambda) = Phi_2(gamma_i, gamma_j; lambda) - fl32(r_i r_j) - cov[i][j]
//
// by the reference's bisection on [-0.99999, 0.99999], with its early returns.
// Phi_2 is Plackett's integral over 64 uniform panels of a 16-point
// Gauss-Legendre rule in theta = asin(lambda) u, u in (0, 1):
//
//   Phi_2 = Phi(h) Phi(k) + asin(lambda) / (2 pi) *
//           sum_n w_n exp((h k sin(theta_n) - (h^2 + k^2) / 2) / cos^2(theta_n))
//
// dg_pairs_kernel  one 16-lane DPP row per pair, four pairs per wave, one wave
//                  per workgroup; a grid of at most CG_DG_FIT_MAX_BLOCKS
//                  workgroups walks the pairs.  Lane c of a row takes the 64
//                  nodes of panels 4 c .. 4 c + 3 and adds their terms one
//                  after the other; the sixteen partial sums meet in a DPP
//                  tree over neighbours (quad swaps, half-row mirror, row
//                  mirror), after which every lane of the row holds the same
//                  bits.  Each lane then carries the row's bisection state
//                  itself: nothing is broadcast, nothing goes through LDS.
//                  A row walks its own pairs (slot, slot + slots, ...): each
//                  trip of the wave's loop is one evaluation of Phi_2 per row,
//                  for whatever pair and step the row is at, so a row whose
//                  pair returns early goes on to its next pair while the other
//                  rows bisect.  A row out of pairs evaluates lambda = 0 and
//                  discards it: every DPP move is executed by all 64 lanes.
//
// Every operation outside exp, sincos, asin and erfc is rounded to float64 on
// its own, in the statement's order (no contraction into fused multiply-adds in
// this file).  No atomics, no workspace, nothing zeroed beforehand: the same
// bits every call.  The diagonal (1 / 0 / 0) is written by the same launch.
#include "cg_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kDgThreads = 64;
constexpr int kDgRows = CG_DG_FIT_BLOCK_PAIRS;
static_assert(kDgRows * 16 == kDgThreads, "one 16-lane row per pair");
constexpr int kDgMaxC = 4096;
constexpr double kDgBracket = 0.99999;
constexpr double kDgCovSkip = 1e-10;
constexpr double kDgInv2Pi = 0.15915494309189535;

// 16-point Gauss-Legendre on (0, 1), (x + 1) / 2, and the weights of (-1, 1):
// the literals of data/dg_fit.py
__constant__ double kDgX[16] = {
    0.005299532504175031, 0.0277124884633837,  0.06718439880608412,
    0.1222977958224985,   0.19106187779867811, 0.2709916111713863,
    0.35919822461037054,  0.4524937450811813,  0.5475062549188188,
    0.6408017753896295,   0.7290083888286136,  0.8089381222013219,
    0.8777022041775016,   0.9328156011939159,  0.9722875115366163,
    0.994700467495825};
__constant__ double kDgW[16] = {
    0.027152459411754037, 0.062253523938647706, 0.09515851168249259,
    0.12462897125553403,  0.14959598881657676,  0.16915651939500262,
    0.1826034150449236,   0.18945061045506859,  0.18945061045506859,
    0.1826034150449236,   0.16915651939500262,  0.14959598881657676,
    0.12462897125553403,  0.09515851168249259,  0.062253523938647706,
    0.027152459411754037};

template <int CTRL>
__device__ __forceinline__ double dg_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// sum over a 16-lane row, neighbours first; every lane receives the same bits
// (each step adds the two halves of a group, and a + b == b + a)
__device__ __forceinline__ double dg_row_sum(double v) {
  v = v + dg_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v = v + dg_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v = v + dg_dpp<0x141>(v);  // row_half_mirror
  v = v + dg_dpp<0x140>(v);  // row_mirror
  return v;
}

__device__ __forceinline__ double dg_normal_cdf(double x) {
  return 0.5 * erfc(-x * 0.7071067811865476);
}

// Phi_2 with pp = Phi(h) Phi(k), hk = h k, hs = (h h + k k) / 2; c is the lane
// within the row.  Called by all 64 lanes.
__device__ __forceinline__ double dg_phi2(double pp, double hk, double hs, double lam,
                                          int c) {
  const double a = asin(lam);
  double acc = 0.0;
  for (int pn = 0; pn < 4; ++pn) {
    const double panel = (double)(4 * c + pn);
#pragma unroll 2
    for (int q = 0; q < 16; ++q) {
      const double u = (panel + kDgX[q]) * (1.0 / 64);
      const double w = kDgW[q] * (1.0 / 128);
      const double th = a * u;
      double s, co;
      sincos(th, &s, &co);
      const double e = exp((hk * s - hs) / (co * co));
      acc = acc + w * e;
    }
  }
  acc = dg_row_sum(acc);
  return pp + (a * acc) * kDgInv2Pi;
}

__global__ __launch_bounds__(kDgThreads) void dg_pairs_kernel(
    const double* __restrict__ rates, const double* __restrict__ gamma,
    const double* __restrict__ cov, long long s0, long long s1, int C, long long npairs,
    double tol, int maxiters, double* __restrict__ corr, int* __restrict__ status,
    int* __restrict__ iterations) {
  const int c = threadIdx.x & 15;
  const int row = threadIdx.x >> 4;
  const long long nslots = (long long)gridDim.x * kDgRows;

  for (long long d = (long long)blockIdx.x * kDgThreads + threadIdx.x; d < C;
       d += (long long)gridDim.x * kDgThreads) {
    corr[d * C + d] = 1.0;
    status[d * C + d] = 0;
    iterations[d * C + d] = 0;
  }

  // Every row walks its own pairs (slot, slot + nslots, ...) through a small
  // state machine, and every trip of the loop is one evaluation of Phi_2 for
  // each row of the wave, whatever pair and state the row is in: a row that
  // returns early (most pairs of two rare neurons do) takes its next pair while
  // its neighbours go on bisecting.  The loop is uniform over the wave; a row
  // out of pairs evaluates lambda = 0 and discards it.
  enum { kF0, kF1, kBisect, kIdle };
  long long p = (long long)blockIdx.x * kDgRows + row;
  int state = kIdle, i = 1, j = 0, n = 0;
  double cv = 0.0, prod = 0.0, pp = 0.0, hk = 0.0, hs = 0.0, f0 = 0.0;
  double lo = -kDgBracket, hi = kDgBracket;

  auto store = [&](double lam, int st, int it) {
    if (c == 0) {
      const long long o_ij = (long long)i * C + j, o_ji = (long long)j * C + i;
      corr[o_ij] = lam;
      corr[o_ji] = lam;
      status[o_ij] = st;
      status[o_ji] = st;
      iterations[o_ij] = it;
      iterations[o_ji] = it;
    }
    p += nslots;
    state = kIdle;
  };

  for (;;) {
    // (row-uniform, no cross-lane moves inside)
    while (state == kIdle && p < npairs) {
      // p -> (i, j), i > j, row by row: row i starts at i (i - 1) / 2
      i = (int)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
      i = min(max(i, 1), C - 1);
      while (i < C - 1 && (long long)(i + 1) * i / 2 <= p) ++i;
      while (i > 1 && (long long)i * (i - 1) / 2 > p) --i;
      j = (int)(p - (long long)i * (i - 1) / 2);
      j = min(max(j, 0), i - 1);
      cv = cov[i * s0 + j * s1];
      if (fabs(cv) <= kDgCovSkip) {
        store(0.0, 1, 0);
        continue;
      }
      const double h = gamma[i], k = gamma[j];
      prod = (double)((float)rates[i] * (float)rates[j]);
      pp = dg_normal_cdf(h) * dg_normal_cdf(k);
      hk = h * k;
      hs = (h * h + k * k) * 0.5;
      state = kF0;
    }
    if (__ballot(state != kIdle) == 0ull) break;

    const double mid = (lo + hi) / 2;
    const double lam = state == kF0 ? -kDgBracket
                     : state == kF1 ? kDgBracket
                     : state == kBisect ? mid : 0.0;
    const double f = (dg_phi2(pp, hk, hs, lam, c) - prod) - cv;  // all 64 lanes

    if (state == kF0) {
      // (the reference evaluates f1 before it looks at f0; the outcome of
      // |f0| < tol does not depend on it)
      if (fabs(f) < tol) {
        store(-kDgBracket, 2, 0);
      } else {
        f0 = f;
        state = kF1;
      }
    } else if (state == kF1) {
      if (fabs(f) < tol) {
        store(kDgBracket, 3, 0);
      } else if (f0 * f > tol) {
        store(0.0, 4, 0);
      } else {
        lo = -kDgBracket;
        hi = kDgBracket;
        n = 0;
        state = kBisect;
      }
    } else if (state == kBisect) {
      // the midpoint has met an end of the bracket: every further iteration
      // would repeat this one
      const bool stuck = mid == lo || mid == hi;
      if (f > 0) hi = mid;
      else if (f < 0) lo = mid;
      ++n;
      if (!(fabs(f) > tol)) {
        store(mid, fabs(f) <= tol ? 0 : 5, n);
      } else if (stuck || n >= maxiters) {
        store(mid, 5, maxiters);
      }
    }
  }
}

}  // namespace

extern "C" int cg_dg_correlation(const double* rates, const double* gamma,
                                 const double* cov, long long cov_s0, long long cov_s1,
                                 int C, double tol, int maxiters, double* corr,
                                 int* status, int* iterations, void* stream) {
  if (!rates || !gamma || !cov || !corr || !status || !iterations || C < 2 ||
      C > kDgMaxC || !(tol > 0.0) || maxiters < 1)
    return CG_EINVAL;
  const long long npairs = (long long)C * (C - 1) / 2;
  long long groups = (npairs + kDgRows - 1) / kDgRows;
  if (groups > CG_DG_FIT_MAX_BLOCKS) groups = CG_DG_FIT_MAX_BLOCKS;
  hipLaunchKernelGGL(dg_pairs_kernel, dim3((unsigned)groups), dim3(kDgThreads), 0,
                     cg_stream(stream), rates, gamma, cov, cov_s0, cov_s1, C, npairs, tol,
                     maxiters, corr, status, iterations);
  CG_LAUNCH_CHECK();
}
