// Spike statistics of a batch of calcium traces on the device (validation-time
// counterparts of spike_helper.deconvolve_signals, spike_metrics.mean_firing_rate
// / covariance and compute_dg_metrics.report):
//   cg_oasis_ar1_batched  OASIS AR(1) with s_min, one trace per lane, float64,
//                         bit-identical to csrc/oasis_ar1.c
//   cg_spike_stats        per sample: firing rate per neuron and the upper
//                         triangle of the covariance of the 500-ms bin counts
//   cg_spike_stats_error  sums of |d| and d^2 between two such sets, ordered
//   cg_spike_corrcoef     per sample: Pearson correlation of the same bin counts,
//                         float64 (compute_metrics.py --device gpu)
// None of these is a throughput kernel: the deconvolution is a chain of
// dependent float64 divisions per trace (13 056 traces = 204 waves at B = 128),
// the statistics are integer sums over a few MB.
#include "cg_common.h"
#include "oasis_flat.h"

namespace {

constexpr int kOasisThreads = 64;  // one wave per workgroup: 204 waves spread over the CUs
// bytes of one stack entry: v, w (f64) and l (i32), struct of arrays
constexpr long long kPoolBytes = 2 * sizeof(double) + sizeof(int);
// the full-depth stack of this many bytes at most is asked for; larger batches
// are deconvolved in groups of traces, one launch after the other
constexpr long long kOasisWsCap = 1ll << 30;
constexpr int kOasisMaxT = 1 << 24;

inline long long round_up64(long long n) { return (n + 63) / 64 * 64; }

struct OasisArgs {
  const float* x;
  long long sx_outer, sx_t, sx_inner;
  float* spikes;
  long long so_outer, so_t, so_inner;
  double* c;  // [traces][T] or null
  double* s;
  const double* gpow;
  double* sv;
  double* sw;
  int* sl;
  long long group;   // traces the stack is laid out for (its row length)
  long long trace0;  // first trace of this launch
  long long ntraces; // traces of the whole call
  int n_inner, T, affine;
  float scale, offset;
  double g, s_min, threshold;
};

__global__ __launch_bounds__(kOasisThreads) void oasis_ar1_kernel(OasisArgs a) {
  const long long slot = (long long)blockIdx.x * kOasisThreads + threadIdx.x;
  const long long trace = a.trace0 + slot;
  if (slot >= a.group || trace >= a.ntraces) return;
  const long long outer = trace / a.n_inner, inner = trace % a.n_inner;
  cg_oasis_flat(a.x + outer * a.sx_outer + inner * a.sx_inner, a.sx_t, a.affine,
                a.scale, a.offset, a.T, a.g, a.s_min, a.threshold, a.gpow,
                a.sv + slot, a.sw + slot, a.sl + slot, a.group,
                a.spikes + outer * a.so_outer + inner * a.so_inner, a.so_t,
                a.c ? a.c + trace * a.T : nullptr,
                a.s ? a.s + trace * a.T : nullptr);
}

// ---------------------------------------------------------------------------
// Per-sample statistics.  A workgroup forms the sample's bin counts (integers
// <= 12) in LDS, then its share of the C (C + 1) / 2 pairs: S_ij = sum_bin n_i
// n_j and S_i = sum_bin n_i are exact integers, and
//   cov_ij = (nb S_ij - S_i S_j) / (nb (nb - 1))
// rounds once in float64 and once to float32.  gridDim.y workgroups share a
// sample's pairs (each forms the counts for itself: the spikes come from L2).
// ---------------------------------------------------------------------------
constexpr int kStatsThreads = 256;
constexpr int kBinFrames = 12;  // 500 ms at 24 Hz
constexpr int kStatsMaxLds = 60 * 1024;

// the sample's 500-ms bin counts, cnt[bin][c] (the caller synchronises)
__device__ __forceinline__ void stage_bin_counts(const float* sp, long long s_t,
                                                 long long s_c, int C, int nb,
                                                 unsigned char* cnt) {
  for (int idx = threadIdx.x; idx < nb * C; idx += kStatsThreads) {
    const int bin = idx / C, c = idx - bin * C;
    const float* p = sp + (long long)bin * kBinFrames * s_t + (long long)c * s_c;
    int n = 0;
#pragma unroll
    for (int f = 0; f < kBinFrames; ++f) n += p[f * s_t] != 0.f ? 1 : 0;
    cnt[idx] = (unsigned char)n;
  }
}

__global__ __launch_bounds__(kStatsThreads) void spike_stats_kernel(
    const float* __restrict__ spikes, long long s_b, long long s_t, long long s_c,
    int T, int C, int nb, float duration, float* __restrict__ rates,
    float* __restrict__ cov) {
  extern __shared__ unsigned char lds[];
  int* sums = reinterpret_cast<int*>(lds);       // [C]
  unsigned char* cnt = lds + (size_t)C * 4;      // [nb][C]
  const int b = blockIdx.x;
  const float* sp = spikes + (long long)b * s_b;
  stage_bin_counts(sp, s_t, s_c, C, nb, cnt);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kStatsThreads) {
    int n = 0;
    for (int bin = 0; bin < nb; ++bin) n += cnt[bin * C + c];
    sums[c] = n;
    if (blockIdx.y == 0) {
      // the rate counts every frame, the trailing partial bin too
      int all = n;
      for (int t = nb * kBinFrames; t < T; ++t)
        all += sp[(long long)t * s_t + (long long)c * s_c] != 0.f ? 1 : 0;
      rates[(long long)b * C + c] = __fdiv_rn((float)all, duration);
    }
  }
  __syncthreads();
  const int P = C * (C + 1) / 2;
  const double denom = (double)nb * (double)(nb - 1);
  for (int p = blockIdx.y * kStatsThreads + threadIdx.x; p < P;
       p += gridDim.y * kStatsThreads) {
    // np.triu_indices order: row i holds j = i .. C - 1
    int i = 0, rem = p;
    while (rem >= C - i) { rem -= C - i; ++i; }
    const int j = i + rem;
    int sij = 0;
    for (int bin = 0; bin < nb; ++bin)
      sij += (int)cnt[bin * C + i] * (int)cnt[bin * C + j];
    const long long num = (long long)nb * sij - (long long)sums[i] * sums[j];
    cov[(long long)b * P + p] = (float)((double)num / denom);
  }
}

// Pearson correlation of the same bin counts (spike_metrics.
// correlation_coefficients_exact): num = nb S_ij - S_i S_j and v_i = nb S_ii -
// S_i^2 are exact 64-bit integers, converted to float64 exactly (< 2^53), then
//   r_ij = num / sqrt(v_i v_j)
// -- NaN (0 / 0) where a train's counts do not vary, as np.corrcoef gives.  The
// full matrix is written; (j, i) is the value of (i, j).
__global__ __launch_bounds__(kStatsThreads) void spike_corrcoef_kernel(
    const float* __restrict__ spikes, long long s_b, long long s_t, long long s_c,
    int C, int nb, double* __restrict__ corr) {
  extern __shared__ unsigned char lds[];
  int* sums = reinterpret_cast<int*>(lds);       // [C]
  unsigned char* cnt = lds + (size_t)C * 4;      // [nb][C]
  const int b = blockIdx.x;
  stage_bin_counts(spikes + (long long)b * s_b, s_t, s_c, C, nb, cnt);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kStatsThreads) {
    int n = 0;
    for (int bin = 0; bin < nb; ++bin) n += cnt[bin * C + c];
    sums[c] = n;
  }
  __syncthreads();
  const int P = C * (C + 1) / 2;
  double* out = corr + (long long)b * C * C;
  for (int p = blockIdx.y * kStatsThreads + threadIdx.x; p < P;
       p += gridDim.y * kStatsThreads) {
    int i = 0, rem = p;
    while (rem >= C - i) { rem -= C - i; ++i; }
    const int j = i + rem;
    int sij = 0, sii = 0, sjj = 0;
    for (int bin = 0; bin < nb; ++bin) {
      const int ni = cnt[bin * C + i], nj = cnt[bin * C + j];
      sij += ni * nj;
      sii += ni * ni;
      sjj += nj * nj;
    }
    const long long num = (long long)nb * sij - (long long)sums[i] * sums[j];
    const long long vi = (long long)nb * sii - (long long)sums[i] * sums[i];
    const long long vj = (long long)nb * sjj - (long long)sums[j] * sums[j];
    const double r = (double)num / sqrt((double)vi * (double)vj);
    out[(long long)i * C + j] = r;
    out[(long long)j * C + i] = r;
  }
}

// ---------------------------------------------------------------------------
// Error sums between two sets of statistics, ordered: block k leaves its four
// partial sums in ws[4 k ..], one wave adds the rows in order.  The grid depends
// on the element counts only, so two runs (or two processes) agree to the bit.
// ---------------------------------------------------------------------------
constexpr int kErrThreads = 256;
constexpr int kErrMaxParts = 1024;

__global__ __launch_bounds__(kErrThreads) void stats_error_kernel(
    const float* __restrict__ fr_a, const float* __restrict__ fr_b, long long n_fr,
    const float* __restrict__ cov_a, const float* __restrict__ cov_b,
    long long n_cov, float* __restrict__ ws) {
  __shared__ float sm[kErrThreads / 64][4];
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const long long stride = (long long)gridDim.x * kErrThreads;
  const long long first = (long long)blockIdx.x * kErrThreads + threadIdx.x;
  for (long long e = first; e < n_fr; e += stride) {
    const float d = fr_a[e] - fr_b[e];
    v[0] += fabsf(d);
    v[1] += d * d;
  }
  for (long long e = first; e < n_cov; e += stride) {
    const float d = cov_a[e] - cov_b[e];
    v[2] += fabsf(d);
    v[3] += d * d;
  }
  block_fold_put<4>(v, sm[threadIdx.x >> 6], 1);
  __syncthreads();
  if (threadIdx.x < 4)
    ws[(long long)blockIdx.x * 4 + threadIdx.x] =
        block_fold_get<kErrThreads / 64>(&sm[0][threadIdx.x], 4);
}

__global__ __launch_bounds__(64) void stats_error_finish_kernel(
    const float* __restrict__ ws, int nparts, float* __restrict__ out) {
  // lane q < 4 adds column q of the partial rows in row order
  if (threadIdx.x < 4) {
    float t = 0.f;
    for (int k = 0; k < nparts; ++k) t += ws[(long long)k * 4 + threadIdx.x];
    out[threadIdx.x] = t;
  }
}

inline int err_parts(long long n) {
  long long parts = (n + kErrThreads * 8 - 1) / (kErrThreads * 8);
  if (parts < 1) parts = 1;
  if (parts > kErrMaxParts) parts = kErrMaxParts;
  return (int)parts;
}

}  // namespace

// Bytes of the stack workspace cg_oasis_ar1_batched wants for `traces` traces of
// T frames: the full-depth stack (T entries of 20 bytes per trace, traces
// rounded up to whole waves), at most 1 GiB -- beyond that the call walks the
// batch in groups of traces.  < 0: invalid.
extern "C" long long cg_oasis_ws_bytes(long long traces, int T) {
  if (traces < 1 || T < 1 || T > kOasisMaxT) return -1;
  const long long per_trace = kPoolBytes * T;
  long long group = round_up64(traces);
  if (group * per_trace > kOasisWsCap) {
    group = kOasisWsCap / per_trace / 64 * 64;
    if (group < 64) group = 64;
  }
  return group * per_trace;
}

extern "C" int cg_oasis_ar1_batched(
    const float* x, int n_outer, int n_inner, int T, long long sx_outer,
    long long sx_t, long long sx_inner, float scale, float offset, double g,
    double s_min, double threshold, const double* gpow, float* spikes,
    long long so_outer, long long so_t, long long so_inner, double* c, double* s,
    void* ws, long long ws_bytes, void* stream) {
  if (!x || !gpow || !spikes || !ws || n_outer < 1 || n_inner < 1 || T < 1 ||
      T > kOasisMaxT)
    return CG_EINVAL;
  const long long traces = (long long)n_outer * n_inner;
  const long long per_trace = kPoolBytes * T;
  // whole waves of traces the caller's workspace holds at full depth
  long long group = ws_bytes / per_trace / 64 * 64;
  if (group > round_up64(traces)) group = round_up64(traces);
  if (group < 64 || ((uintptr_t)ws & 7)) return CG_EINVAL;
  OasisArgs a;
  a.x = x; a.sx_outer = sx_outer; a.sx_t = sx_t; a.sx_inner = sx_inner;
  a.spikes = spikes; a.so_outer = so_outer; a.so_t = so_t; a.so_inner = so_inner;
  a.c = c; a.s = s; a.gpow = gpow;
  a.sv = reinterpret_cast<double*>(ws);
  a.sw = a.sv + group * T;
  a.sl = reinterpret_cast<int*>(a.sw + group * T);
  a.group = group; a.ntraces = traces;
  a.n_inner = n_inner; a.T = T;
  a.affine = !(scale == 1.f && offset == 0.f);
  a.scale = scale; a.offset = offset;
  a.g = g; a.s_min = s_min; a.threshold = threshold;
  // (launches of one stream run one after the other: the groups share the stack)
  for (long long t0 = 0; t0 < traces; t0 += group) {
    a.trace0 = t0;
    const long long n = traces - t0 < group ? traces - t0 : group;
    hipLaunchKernelGGL(oasis_ar1_kernel,
                       dim3((unsigned)((n + kOasisThreads - 1) / kOasisThreads)),
                       dim3(kOasisThreads), 0, cg_stream(stream), a);
  }
  CG_LAUNCH_CHECK();
}

extern "C" int cg_spike_stats(const float* spikes, int B, int T, int C,
                              long long s_b, long long s_t, long long s_c,
                              float* rates, float* cov, void* stream) {
  if (!spikes || !rates || !cov || B < 1 || C < 1 || T < 1) return CG_EINVAL;
  const int nb = T / kBinFrames;
  if (nb < 2) return CG_EINVAL;
  const long long lds = (long long)C * 4 + (long long)nb * C;
  if (lds > kStatsMaxLds || C > 4096) return CG_EINVAL;
  const int P = C * (C + 1) / 2;
  int split = (P + kStatsThreads * 4 - 1) / (kStatsThreads * 4);
  if (split < 1) split = 1;
  if (split > 8) split = 8;
  const float duration = (float)((double)T / 24.0);
  hipLaunchKernelGGL(spike_stats_kernel, dim3(B, split), dim3(kStatsThreads),
                     (size_t)lds, cg_stream(stream), spikes, s_b, s_t, s_c, T, C, nb,
                     duration, rates, cov);
  CG_LAUNCH_CHECK();
}

extern "C" int cg_spike_corrcoef(const float* spikes, int B, int T, int C,
                                 long long s_b, long long s_t, long long s_c,
                                 double* corr, void* stream) {
  if (!spikes || !corr || B < 1 || C < 1 || T < 1) return CG_EINVAL;
  const int nb = T / kBinFrames;
  if (nb < 2) return CG_EINVAL;
  const long long lds = (long long)C * 4 + (long long)nb * C;
  if (lds > kStatsMaxLds || C > 4096) return CG_EINVAL;
  const int P = C * (C + 1) / 2;
  int split = (P + kStatsThreads * 4 - 1) / (kStatsThreads * 4);
  if (split < 1) split = 1;
  if (split > 8) split = 8;
  hipLaunchKernelGGL(spike_corrcoef_kernel, dim3(B, split), dim3(kStatsThreads),
                     (size_t)lds, cg_stream(stream), spikes, s_b, s_t, s_c, C, nb, corr);
  CG_LAUNCH_CHECK();
}

// floats of `ws` cg_spike_stats_error needs for these element counts
extern "C" long long cg_spike_stats_error_ws_elems(long long n_fr, long long n_cov) {
  if (n_fr < 0 || n_cov < 0) return -1;
  return 4ll * err_parts(n_fr > n_cov ? n_fr : n_cov);
}

extern "C" int cg_spike_stats_error(const float* fr_a, const float* fr_b,
                                    long long n_fr, const float* cov_a,
                                    const float* cov_b, long long n_cov,
                                    float* out, float* ws, void* stream) {
  if (!out || !ws || n_fr < 0 || n_cov < 0 || (n_fr && (!fr_a || !fr_b)) ||
      (n_cov && (!cov_a || !cov_b)))
    return CG_EINVAL;
  const int parts = err_parts(n_fr > n_cov ? n_fr : n_cov);
  hipLaunchKernelGGL(stats_error_kernel, dim3(parts), dim3(kErrThreads), 0,
                     cg_stream(stream), fr_a, fr_b, n_fr, cov_a, cov_b, n_cov, ws);
  hipLaunchKernelGGL(stats_error_finish_kernel, dim3(1), dim3(64), 0, cg_stream(stream),
                     ws, parts, out);
  CG_LAUNCH_CHECK();
}
