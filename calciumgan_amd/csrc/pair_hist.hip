// Histogram counts behind the KL figures of the recorded-data report (DESIGN.md
// 14; spike_metrics.pair_histograms is the numpy statement).  For pair p the two
// samples are the non-NaN elements a[p][i][j] and b[p][i][j] with i < j; their
// pooled values are cut into num_bins equal-width, right-closed bins exactly as
// pandas.cut(pooled, bins=num_bins) cuts them:
//
//   mn, mx the pooled minimum and maximum (a zero maximum is taken as +0)
//   mn == mx:  mn -= (mn != 0 ? 0.001 |mn| : 0.001), mx += (mx != 0 ? 0.001 |mx| : 0.001)
//   otherwise: adj = (mx - mn) 0.001
//   step = (mx - mn) / num_bins
//   e[k] = fl(fl(k step) + mn)   (step == 0: fl(fl(fl(k / num_bins) (mx - mn)) + mn))
//   e[num_bins] = mx;  mn != mx: e[0] -= adj
//   id(x) = number of edges < x;  x counts in bin id - 1 when 1 <= id <= num_bins
//
// every operation rounded to float64 on its own.  The bin comes from comparing x
// with the edges (a binary search over the edges in LDS), never from
// (x - mn) / step: the quotient disagrees with pandas for values within a
// rounding of an edge.
//
// One workgroup per pair, two sweeps over both upper triangles straight from
// global memory (a wave per row, lanes along j; at C = 102 a pair is 83 KB and
// the second sweep finds it in L2):
//   sweep 1  minimum, maximum, the two set sizes and an infinity flag: wave
//            reduction, then one LDS slot per wave
//   edges    thread k forms e[k] into LDS; adjacent edges are compared
//   sweep 2  each wave adds into its own LDS histogram (integer LDS adds: any
//            order gives the same counts), the waves' histograms are summed
// status: 1 a side is empty, 2 a pooled value is infinite, 4 two edges coincide
// (looked for only when there is a value and none is infinite).  With status
// != 0 counts and edges are written as zeros.  Every output element is written
// by the launch; no global atomics, no workspace.
#include "cg_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPhThreads = 512;
constexpr int kPhWaves = kPhThreads / 64;
constexpr int kPhMaxBins = 256;
constexpr int kPhMaxC = 4096;

__global__ __launch_bounds__(kPhThreads) void pair_hist_kernel(
    const double* __restrict__ a, long long a_sp, long long a_si, long long a_sj,
    const double* __restrict__ b, long long b_sp, long long b_si, long long b_sj,
    int C, int N, int* __restrict__ counts, int* __restrict__ valid,
    double* __restrict__ edges, int* __restrict__ status) {
  __shared__ double sm_mn[kPhWaves], sm_mx[kPhWaves];
  __shared__ int sm_cnt[kPhWaves][2], sm_inf[kPhWaves];
  __shared__ double sm_e[kPhMaxBins + 1];
  __shared__ int sm_hist[kPhWaves][2][kPhMaxBins];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p = blockIdx.x;
  const double* side[2] = {a + p * a_sp, b + p * b_sp};
  const long long s_i[2] = {a_si, b_si}, s_j[2] = {a_sj, b_sj};

  // sweep 1
  double mn = INFINITY, mx = -INFINITY;
  int cnt[2] = {0, 0}, inf = 0;
#pragma unroll
  for (int s = 0; s < 2; ++s)
    for (int i = wave; i < C - 1; i += kPhWaves) {
      const double* row = side[s] + i * s_i[s];
      for (int j = i + 1 + lane; j < C; j += 64) {
        const double x = row[j * s_j[s]];
        if (x == x) {
          mn = fmin(mn, x);
          mx = fmax(mx, x);
          cnt[s] += 1;
          inf |= (int)isinf(x);
        }
      }
    }
  // (the block fold in its two steps: the histograms are zeroed under the same
  // barrier)
  block_fold_put<FoldMin>(mn, sm_mn);
  block_fold_put<FoldMax>(mx, sm_mx);
  block_fold_put<2>(cnt, sm_cnt[wave], 1);
  inf = __any(inf);
  if (lane == 0) sm_inf[wave] = inf;
  for (int k = lane; k < 2 * N; k += 64) sm_hist[wave][k / N][k % N] = 0;
  __syncthreads();
  // (every thread folds the waves' slots: the values are uniform from here on)
  mn = block_fold_get<kPhWaves, FoldMin>(sm_mn);
  mx = block_fold_get<kPhWaves, FoldMax>(sm_mx);
  const int n_a = block_fold_get<kPhWaves>(&sm_cnt[0][0], 2);
  const int n_b = block_fold_get<kPhWaves>(&sm_cnt[0][1], 2);
  inf = 0;
#pragma unroll
  for (int w = 0; w < kPhWaves; ++w) inf |= sm_inf[w];
  int st = ((n_a == 0 || n_b == 0) ? 1 : 0) | (inf ? 2 : 0);
  const bool have_edges = n_a + n_b > 0 && !inf;  // uniform
  if (have_edges) {
    mx = mx + 0.0;  // -0 -> +0, every other value unchanged
    const bool flat = mn == mx;
    double adj = 0.0;
    if (flat) {
      mn -= (mn != 0.0 ? 0.001 * fabs(mn) : 0.001);
      mx += (mx != 0.0 ? 0.001 * fabs(mx) : 0.001);
    } else {
      adj = (mx - mn) * 0.001;
    }
    if (tid <= N) {
      const double delta = mx - mn;
      const double step = delta / (double)N;
      double e;
      if (step == 0.0) {
        e = (double)tid / (double)N;
        e = e * delta;
      } else {
        e = (double)tid * step;
      }
      e = e + mn;
      if (tid == N) e = mx;
      if (tid == 0 && !flat) e = e - adj;
      sm_e[tid] = e;
    }
    __syncthreads();
    if (__syncthreads_or(tid < N && sm_e[tid] == sm_e[tid + 1])) st |= 4;
  }

  if (tid == 0) {
    valid[p * 2] = n_a;
    valid[p * 2 + 1] = n_b;
    status[p] = st;
  }
  if (edges && tid <= N) edges[p * (N + 1) + tid] = st ? 0.0 : sm_e[tid];
  if (st) {
    for (int k = tid; k < 2 * N; k += kPhThreads) counts[p * 2 * N + k] = 0;
    return;
  }

  // sweep 2
#pragma unroll
  for (int s = 0; s < 2; ++s)
    for (int i = wave; i < C - 1; i += kPhWaves) {
      const double* row = side[s] + i * s_i[s];
      for (int j = i + 1 + lane; j < C; j += 64) {
        const double x = row[j * s_j[s]];
        if (x == x) {
          // lower bound over e[0 .. N]: the number of edges < x
          int lo = 0, n = N + 1;
          while (n > 0) {
            const int half = n >> 1;
            if (sm_e[lo + half] < x) {
              lo += half + 1;
              n -= half + 1;
            } else {
              n = half;
            }
          }
          if (lo >= 1 && lo <= N) atomicAdd(&sm_hist[wave][s][lo - 1], 1);
        }
      }
    }
  __syncthreads();
  for (int k = tid; k < 2 * N; k += kPhThreads) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kPhWaves; ++w) sum += sm_hist[w][k / N][k % N];
    counts[p * 2 * N + k] = sum;
  }
}

}  // namespace

extern "C" int cg_pair_histogram(const double* a, long long a_sp, long long a_si,
                                 long long a_sj, const double* b, long long b_sp,
                                 long long b_si, long long b_sj, int P, int C,
                                 int num_bins, int* counts, int* valid,
                                 double* edges, int* status, void* stream) {
  if (!a || !b || !counts || !valid || !status || P < 1 || C < 2 || C > kPhMaxC ||
      num_bins < 1 || num_bins > kPhMaxBins)
    return CG_EINVAL;
  hipLaunchKernelGGL(pair_hist_kernel, dim3((unsigned)P), dim3(kPhThreads), 0,
                     cg_stream(stream), a, a_sp, a_si, a_sj, b, b_sp, b_si, b_sj, C,
                     num_bins, counts, valid, edges, status);
  CG_LAUNCH_CHECK();
}
