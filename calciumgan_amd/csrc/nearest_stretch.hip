// Nearest stretch of a recording to every query trial (compute_metrics.py
// --novelty_metrics; signals_metrics.nearest_stretch is the numpy
// statement).  With R the (T_raw, C) float32 recording, Q the (N, L, C) queries
// and offsets s_j = j step, j < S = (T_raw - L) / step + 1:
//   d2[n][j] = sum_{t,c} (Q[n][t][c] - R[s_j + t][c])^2
//            = |q_n|^2 + W_j - 2 x[n][j],   x[n][j] = sum_k q[n][k] r[s_j C + k]
// every term float64 (products of float32 values are exact there), k = t C + c
// < K = L C.  x is a GEMM (N x K)(K x S) whose B operand is the recording itself
// read at a column stride of step C elements: no window is ever materialised.
//
//   prep     |q_n|^2 (one workgroup per query, ordered block fold) and the
//            squared norm of every recording row (one lane per row, in column
//            order); then W_j = the sum of the L rows of stretch j, four
//            interleaved chains joined in a fixed order -- not a difference of
//            running sums, which would lose the small stretches of a long
//            recording.
//   gemm     one workgroup of four waves per (128 queries, 64 offsets, K
//            split): wave w owns queries 32 w .. 32 w + 31, eight 16 x 16
//            float64 accumulators on v_mfma_f64_16x16x4_f64.  The recording's
//            span of a tile -- 63 step C + chunk consecutive elements of its
//            flat image -- is staged in LDS once per chunk of K and read by all
//            four waves; neighbouring offsets share all but step rows of it.
//            It is staged element by (row, column), so any strides of raw take
//            this path.  The queries come from global memory / L2 into
//            registers, sixteen k per lane group and step: lane group g holds
//            k = 16 s + 4 g .. + 3 of step s as one 16-byte load and feeds
//            element i to MFMA i; B follows the same order, so the permutation
//            of k inside a step cancels.  float32 -> float64 on the way in.
//            The next step's queries are loaded before this step's MFMAs.
//            A span that does not fit the LDS budget (step C > 292) reads B
//            from global memory, element by element: slower, not different.
//            Rows past N repeat query N - 1 and columns past S read zeros; both
//            are dropped.  The K tail is zero on both sides.
//   finish   x = the splits' partial sums in split order, d2 = (|q|^2 + W) - 2 x
//            clamped at 0, a non-finite one NaN; d2 is stored if asked for, and
//            the least admitted finite value of every segment of 1024 offsets
//            with its lowest index goes to the workspace.
//   pick     one lane per query folds the segments in order.
// Five launches, no atomics, nothing zeroed beforehand, every workspace element
// that is read was written by the call, the plan a function of the shape
// alone: the same bits every call.
#include "cg_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;
// four consecutive floats at any 4-byte alignment
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kNsThreads = 256;
constexpr int kNsWaves = kNsThreads / 64;
constexpr int kNsTileN = 128;            // queries of a workgroup: 32 per wave
constexpr int kNsWaveN = kNsTileN / kNsWaves;
constexpr int kNsTileS = 64;             // offsets of a workgroup
constexpr int kNsRowTiles = kNsWaveN / 16, kNsColTiles = kNsTileS / 16;
constexpr int kNsGroup = 16;             // k of one step: 4 MFMAs of 4
constexpr int kNsLdsFloats = 18432;      // 72 KiB: two workgroups a CU
constexpr int kNsMinChunk = 4;           // steps per chunk at least, staged
constexpr int kNsMaxChunk = 512;         // steps per chunk at most
constexpr int kNsMaxSplits = 16;
constexpr int kNsMinSplitSteps = 64;     // steps of a split at least
constexpr int kNsUnits = 256;            // compute units the plan balances over
constexpr int kNsSegment = 1024;         // offsets per finish workgroup
constexpr int kNsMaxN = 65535;              // a grid dimension
constexpr long long kNsMaxK = 1LL << 30;
constexpr long long kNsMaxRaw = 1LL << 40;  // T_raw C
constexpr int kNsMaxStep = 1 << 20;

struct NsPlan {
  long long S, S_pad, tilesS;
  int tilesN, splits, split_steps, chunk_steps, staged, steps, segments;
};

inline bool ns_shape_ok(int N, int L, int C, long long T_raw, int step) {
  return N >= 1 && L >= 1 && C >= 1 && step >= 1 && N <= kNsMaxN &&
         step <= kNsMaxStep && (long long)L <= T_raw &&
         (long long)L * C <= kNsMaxK && T_raw <= kNsMaxRaw / C &&
         T_raw < (1LL << 31) - kNsTileS;  // (S <= T_raw)
}

inline NsPlan ns_plan(int N, int L, int C, long long T_raw, int step) {
  NsPlan p;
  p.S = (T_raw - L) / step + 1;
  p.tilesS = (p.S - 1) / kNsTileS + 1;
  p.S_pad = p.tilesS * kNsTileS;
  p.tilesN = (N - 1) / kNsTileN + 1;
  p.segments = (int)((p.S - 1) / kNsSegment + 1);
  const long long K = (long long)L * C;
  p.steps = (int)((K - 1) / kNsGroup + 1);
  const long long span = (long long)(kNsTileS - 1) * step * C;
  p.staged = span + kNsMinChunk * kNsGroup <= kNsLdsFloats;
  p.chunk_steps = kNsMaxChunk;
  if (p.staged && (kNsLdsFloats - span) / kNsGroup < p.chunk_steps)
    p.chunk_steps = (int)((kNsLdsFloats - span) / kNsGroup);
  // the fewest splits within 3 % of the best balance over kNsUnits units:
  // rounds of workgroups a unit runs, in units of 1 / splits of K
  int most = (p.steps - 1) / kNsMinSplitSteps + 1;
  if (most > kNsMaxSplits) most = kNsMaxSplits;
  const long long tiles = p.tilesS * p.tilesN;
  double best = 0.0;
  for (int s = 1; s <= most; ++s) {
    const double cost = (double)((tiles * s - 1) / kNsUnits + 1) / s;
    if (s == 1 || cost < best) best = cost;
  }
  p.splits = 1;
  for (int s = 1; s <= most; ++s) {
    const double cost = (double)((tiles * s - 1) / kNsUnits + 1) / s;
    if (cost <= 1.03 * best) { p.splits = s; break; }
  }
  p.split_steps = (p.steps - 1) / p.splits + 1;
  p.splits = (p.steps - 1) / p.split_steps + 1;
  if (p.chunk_steps > p.split_steps) p.chunk_steps = p.split_steps;
  return p;
}

// workspace, in doubles: q2 [N], rowsq [T_raw], W [S], segment minima
// [N][segments], their indices (int32, two to a double) and the partial
// products [splits][N][S_pad]
struct NsLayout {
  long long q2, rowsq, w, segmin, segidx, part, total;
};

inline NsLayout ns_layout(const NsPlan& p, int N, long long T_raw) {
  NsLayout l;
  l.q2 = 0;
  l.rowsq = l.q2 + N;
  l.w = l.rowsq + T_raw;
  l.segmin = l.w + p.S;
  l.segidx = l.segmin + (long long)N * p.segments;
  l.part = l.segidx + ((long long)N * p.segments + 1) / 2;
  l.total = l.part + (long long)p.splits * N * p.S_pad;
  return l;
}

struct NsArgs {
  const float* q;
  long long q_sn, q_st, q_sc;
  const float* raw;
  long long T_raw, r_st, r_sc;
  const int* exclude;
  double *d2, *nearest;
  int* index;
  double *q2, *rowsq, *w, *segmin, *part;
  int* segidx;
  long long S, S_pad, jstride;  // jstride = step C
  int N, L, C, K, step, exclude_len;
  int splits, split_steps, chunk_steps, steps, segments;
};

// workgroups 0 .. N - 1: |q_n|^2; the rest: 256 recording rows each
__global__ __launch_bounds__(kNsThreads) void ns_prep_kernel(NsArgs a) {
  __shared__ double slots[kNsWaves];
  if ((int)blockIdx.x < a.N) {
    const float* qn = a.q + (long long)blockIdx.x * a.q_sn;
    double s = 0.0;
    for (int k = threadIdx.x; k < a.K; k += kNsThreads) {
      const int t = k / a.C, c = k - t * a.C;
      const double v = (double)qn[(long long)t * a.q_st + (long long)c * a.q_sc];
      s += v * v;
    }
    block_fold_put(s, slots);
    __syncthreads();
    if (threadIdx.x == 0) a.q2[blockIdx.x] = block_fold_get<kNsWaves>(slots);
    return;
  }
  const long long row =
      (long long)(blockIdx.x - a.N) * kNsThreads + threadIdx.x;
  if (row >= a.T_raw) return;
  const float* r = a.raw + row * a.r_st;
  double s = 0.0;
  for (int c = 0; c < a.C; ++c) {
    const double v = (double)r[(long long)c * a.r_sc];
    s += v * v;
  }
  a.rowsq[row] = s;
}

// W_j: rows s_j .. s_j + L - 1, four interleaved chains, ((0 + 1) + (2 + 3))
__global__ __launch_bounds__(kNsThreads) void ns_w_kernel(NsArgs a) {
  const long long j = (long long)blockIdx.x * kNsThreads + threadIdx.x;
  if (j >= a.S) return;
  const double* r = a.rowsq + j * a.step;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int t = 0;
  for (; t + 4 <= a.L; t += 4) {
    s0 += r[t]; s1 += r[t + 1]; s2 += r[t + 2]; s3 += r[t + 3];
  }
  if (t < a.L) s0 += r[t];
  if (t + 1 < a.L) s1 += r[t + 1];
  if (t + 2 < a.L) s2 += r[t + 2];
  a.w[j] = (s0 + s1) + (s2 + s3);
}

// elements k .. k + 3 of query row `row`, zeros from K on
template <bool QFLAT>
__device__ __forceinline__ f32x4 ns_load_q(const float* row, int k, const NsArgs& a) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (QFLAT) {
    if (k + 3 < a.K) {
      const f32x4u u = *reinterpret_cast<const f32x4u*>(row + k);
      v = f32x4{u[0], u[1], u[2], u[3]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k + i < a.K) v[i] = row[k + i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (k + i < a.K) {
        const int t = (k + i) / a.C, c = k + i - t * a.C;
        v[i] = row[(long long)t * a.q_st + (long long)c * a.q_sc];
      }
    }
  }
  return v;
}

// grid (offset tile, query tile, split)
template <bool QFLAT, bool STAGED>
__global__ __launch_bounds__(kNsThreads, 2) void ns_gemm_kernel(NsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ns_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, g = lane >> 4;
  const long long j0 = (long long)blockIdx.x * kNsTileS;
  const int n0 = blockIdx.y * kNsTileN + wave * kNsWaveN;
  const int step0 = blockIdx.z * a.split_steps;
  const int step1 = step0 + a.split_steps < a.steps ? step0 + a.split_steps : a.steps;
  const long long raw_elems = a.T_raw * a.C;
  // rows past the last query repeat it: their accumulator rows are dropped
  const float* qrow[kNsRowTiles];
#pragma unroll
  for (int r = 0; r < kNsRowTiles; ++r) {
    const int n = n0 + r * 16 + lr;
    qrow[r] = a.q + (long long)(n < a.N ? n : a.N - 1) * a.q_sn;
  }
  f64x4 acc[kNsRowTiles][kNsColTiles];
#pragma unroll
  for (int r = 0; r < kNsRowTiles; ++r)
#pragma unroll
    for (int c = 0; c < kNsColTiles; ++c) acc[r][c] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int c0 = step0; c0 < step1; c0 += a.chunk_steps) {
    const int c1 = c0 + a.chunk_steps < step1 ? c0 + a.chunk_steps : step1;
    if (STAGED) {
      // LDS element e is flat element j0 jstride + 16 c0 + e of the recording,
      // zero past its end; one division per lane, then (row, column) advance
      const int count = (kNsTileS - 1) * (int)a.jstride + (c1 - c0) * kNsGroup;
      __syncthreads();  // the previous chunk has been read
      long long f = j0 * a.jstride + (long long)c0 * kNsGroup + tid;
      long long row = f / a.C;
      int col = (int)(f - row * a.C);
      const int drow = kNsThreads / a.C, dcol = kNsThreads - drow * a.C;
      for (int e = tid; e < count; e += kNsThreads) {
        ns_lds[e] = f < raw_elems ? a.raw[row * a.r_st + (long long)col * a.r_sc] : 0.f;
        f += kNsThreads;
        row += drow;
        col += dcol;
        if (col >= a.C) { col -= a.C; ++row; }
      }
      __syncthreads();
    }
    if (n0 >= a.N) continue;  // (the wave still stages and meets the barriers)

    f32x4 qn[kNsRowTiles];
#pragma unroll
    for (int r = 0; r < kNsRowTiles; ++r)
      qn[r] = ns_load_q<QFLAT>(qrow[r], c0 * kNsGroup + 4 * g, a);
    for (int s = c0; s < c1; ++s) {
      const int k = s * kNsGroup + 4 * g;
      f32x4 qa[kNsRowTiles];
#pragma unroll
      for (int r = 0; r < kNsRowTiles; ++r) qa[r] = qn[r];
      if (s + 1 < c1) {
#pragma unroll
        for (int r = 0; r < kNsRowTiles; ++r)
          qn[r] = ns_load_q<QFLAT>(qrow[r], k + kNsGroup, a);
      }
      float b[kNsColTiles][4];
#pragma unroll
      for (int c = 0; c < kNsColTiles; ++c) {
        if (STAGED) {
          const float* bp =
              ns_lds + (c * 16 + lr) * (int)a.jstride + (s - c0) * kNsGroup + 4 * g;
#pragma unroll
          for (int i = 0; i < 4; ++i) b[c][i] = k + i < a.K ? bp[i] : 0.f;
        } else {
          const long long j = j0 + c * 16 + lr;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float v = 0.f;
            if (j < a.S && k + i < a.K) {
              const int t = (k + i) / a.C, cc = k + i - t * a.C;
              v = a.raw[(j * a.step + t) * a.r_st + (long long)cc * a.r_sc];
            }
            b[c][i] = v;
          }
        }
      }
      // A: row lane & 15, k = lane >> 4; B: k = lane >> 4, column lane & 15
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < kNsRowTiles; ++r) {
          if (r == 0 || n0 + r * 16 < a.N) {
            const double av = (double)qa[r][i];
#pragma unroll
            for (int c = 0; c < kNsColTiles; ++c)
              acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                  av, (double)b[c][i], acc[r][c], 0, 0, 0);
          }
        }
      }
    }
  }

  // C/D: column lane & 15, row (lane >> 4) + 4 reg
  double* part = a.part + (long long)blockIdx.z * a.N * a.S_pad;
#pragma unroll
  for (int r = 0; r < kNsRowTiles; ++r) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int n = n0 + r * 16 + g + 4 * reg;
      if (n < a.N) {
#pragma unroll
        for (int c = 0; c < kNsColTiles; ++c)
          part[(long long)n * a.S_pad + j0 + c * 16 + lr] = acc[r][c][reg];
      }
    }
  }
}

// grid (segment, query)
__global__ __launch_bounds__(kNsThreads) void ns_finish_kernel(NsArgs a) {
#pragma clang fp contract(off)
  __shared__ double vals[kNsWaves];
  __shared__ int idxs[kNsWaves];
  const int n = blockIdx.y;
  const double q2 = a.q2[n];
  const long long ex = a.exclude ? (long long)a.exclude[n] : -1;
  const double inf = __builtin_inf();
  double best = inf;
  int at = -1;
  const long long j1 = (long long)(blockIdx.x + 1) * kNsSegment;
  for (long long j = (long long)blockIdx.x * kNsSegment + threadIdx.x;
       j < j1 && j < a.S; j += kNsThreads) {
    const double* p = a.part + (long long)n * a.S_pad + j;
    double x = p[0];
    for (int s = 1; s < a.splits; ++s) x += p[(long long)s * a.N * a.S_pad];
    double d = q2 + a.w[j];
    d = d - 2.0 * x;
    if (d < 0.0) d = 0.0;
    if (!(d - d == 0.0)) d = __builtin_nan("");
    if (a.d2) a.d2[(long long)n * a.S + j] = d;
    long long gap = j * a.step - ex;
    if (gap < 0) gap = -gap;
    const bool admitted = ex < 0 || gap >= a.exclude_len;
    if (admitted && d < best) { best = d; at = (int)j; }  // (j ascends: lowest)
  }
  // the least value, the lowest index among equals; no offset: (inf, -1)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (oa >= 0 && (at < 0 || ov < best || (ov == best && oa < at))) {
      best = ov; at = oa;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    vals[threadIdx.x >> 6] = best;
    idxs[threadIdx.x >> 6] = at;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kNsWaves; ++w) {
      if (idxs[w] >= 0 && (at < 0 || vals[w] < best || (vals[w] == best && idxs[w] < at))) {
        best = vals[w]; at = idxs[w];
      }
    }
    a.segmin[(long long)n * a.segments + blockIdx.x] = best;
    a.segidx[(long long)n * a.segments + blockIdx.x] = at;
  }
}

__global__ __launch_bounds__(kNsThreads) void ns_pick_kernel(NsArgs a) {
  const int n = blockIdx.x * kNsThreads + threadIdx.x;
  if (n >= a.N) return;
  double best = 0.0;
  int at = -1;
  for (int s = 0; s < a.segments; ++s) {
    const double v = a.segmin[(long long)n * a.segments + s];
    const int i = a.segidx[(long long)n * a.segments + s];
    if (i >= 0 && (at < 0 || v < best)) { best = v; at = i; }
  }
  a.nearest[n] = at < 0 ? __builtin_nan("") : best;
  a.index[n] = at;
}

template <bool QFLAT, bool STAGED>
hipError_t ns_launch_gemm(const NsArgs& a, const NsPlan& p, hipStream_t stream) {
  size_t lds = 0;
  if (STAGED) {
    lds = ((size_t)(kNsTileS - 1) * a.jstride + (size_t)p.chunk_steps * kNsGroup) *
          sizeof(float);
    if (int e = cg_allow_dynamic_lds<&ns_gemm_kernel<QFLAT, STAGED>>(
            (int)(kNsLdsFloats * sizeof(float))))
      return (hipError_t)e;
  }
  hipLaunchKernelGGL((ns_gemm_kernel<QFLAT, STAGED>),
                     dim3((unsigned)p.tilesS, p.tilesN, p.splits), dim3(kNsThreads),
                     lds, stream, a);
  return hipGetLastError();
}

}  // namespace

extern "C" long long cg_nearest_stretch_ws_bytes(int N, int L, int C,
                                                 long long T_raw, int step) {
  if (!ns_shape_ok(N, L, C, T_raw, step)) return -1;
  return ns_layout(ns_plan(N, L, C, T_raw, step), N, T_raw).total *
         (long long)sizeof(double);
}

extern "C" int cg_nearest_stretch(const float* q, int N, int L, int C,
                                  long long q_sn, long long q_st, long long q_sc,
                                  const float* raw, long long T_raw,
                                  long long r_st, long long r_sc, int step,
                                  const int* exclude, int exclude_len,
                                  double* d2, double* nearest, int* index,
                                  void* ws, void* stream) {
  if (!q || !raw || !nearest || !index || !ws ||
      (reinterpret_cast<uintptr_t>(ws) & 7) || exclude_len < 0 ||
      !ns_shape_ok(N, L, C, T_raw, step))
    return CG_EINVAL;
  const NsPlan p = ns_plan(N, L, C, T_raw, step);
  const NsLayout l = ns_layout(p, N, T_raw);
  double* w = static_cast<double*>(ws);
  NsArgs a;
  a.q = q; a.q_sn = q_sn; a.q_st = q_st; a.q_sc = q_sc;
  a.raw = raw; a.T_raw = T_raw; a.r_st = r_st; a.r_sc = r_sc;
  a.exclude = exclude; a.d2 = d2; a.nearest = nearest; a.index = index;
  a.q2 = w + l.q2; a.rowsq = w + l.rowsq; a.w = w + l.w;
  a.segmin = w + l.segmin; a.part = w + l.part;
  a.segidx = reinterpret_cast<int*>(w + l.segidx);
  a.S = p.S; a.S_pad = p.S_pad; a.jstride = (long long)step * C;
  a.N = N; a.L = L; a.C = C; a.K = L * C; a.step = step;
  a.exclude_len = exclude_len;
  a.splits = p.splits; a.split_steps = p.split_steps;
  a.chunk_steps = p.chunk_steps; a.steps = p.steps; a.segments = p.segments;
  hipStream_t s = cg_stream(stream);
  hipError_t e;

  const long long row_blocks = (T_raw - 1) / kNsThreads + 1;
  hipLaunchKernelGGL(ns_prep_kernel, dim3((unsigned)(N + row_blocks)),
                     dim3(kNsThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ns_w_kernel, dim3((unsigned)((p.S - 1) / kNsThreads + 1)),
                     dim3(kNsThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  // a query's K elements consecutive in memory: 16-byte loads
  const bool qflat = q_sc == 1 && (q_st == C || L == 1);
  if (p.staged)
    e = qflat ? ns_launch_gemm<true, true>(a, p, s) : ns_launch_gemm<false, true>(a, p, s);
  else
    e = qflat ? ns_launch_gemm<true, false>(a, p, s) : ns_launch_gemm<false, false>(a, p, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ns_finish_kernel, dim3((unsigned)p.segments, N),
                     dim3(kNsThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ns_pick_kernel, dim3((unsigned)((N - 1) / kNsThreads + 1)),
                     dim3(kNsThreads), 0, s, a);
  CG_LAUNCH_CHECK();
}
