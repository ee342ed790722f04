// Statistics and histogram buckets of float32 device tensors (--plot_weights:
// the reference's Summary.plot_weights, gan/utils/summary_helper.py:523-557,
// writes mean / stddev / min / max and a tf.summary.histogram of every trainable
// variable once per epoch).  One call summarises any number of segments of one
// flat float32 buffer -- every variable of a model lives in nets.FlatParams.data.
// The numpy statements are summary_helper.variable_statistics and
// summary_helper.histogram_buckets (DESIGN.md "Weight summaries").
//
//   cg_tensor_summary  for segment s, the n = seg_len[s] values d = (double)x at
//                      data + seg_off[s], every operation rounded to float64 on
//                      its own (no fused multiply-add):
//     mn = min d, mx = max d (a zero maximum is taken as +0), sum, mean = sum / n
//     sq = sum (d - mean)^2, stddev = sqrt(sq / n), range = mx - mn
//     range == 0:  one bucket (mn - 0.5, mn + 0.5, n)
//     otherwise:   w = range / k, idx(d) = min((long)floor((d - mn) / w), k - 1),
//                  e[j] = mn + fl(j w) for j < k, e[k] = mx,
//                  bucket j = (e[j], e[j + 1], #{d : idx(d) = j})
//
// A segment is cut into chunks of kTsChunk = 4096 elements, a "tile" each, so a
// variable of 2 M elements is 512 tiles spread over the chip and a bias of 64 is
// one.  The tiles of all segments are numbered in segment order; a workgroup
// finds the segment of its tile by bisection of the tile_start table.  Five
// launches whatever the number of segments:
//   plan     one workgroup: tile_start[s] = sum of ceil(seg_len / 4096) before s
//   pass 1   a workgroup per tile (grid-stride over 2048): minimum, maximum, sum
//            and the number of NaN / Inf of its chunk -> one partial row per tile
//   finish 1 a workgroup per segment: folds the segment's partial rows in a fixed
//            order, writes n, mn, mx, sum, mean, nonfinite; zeroes the segment's
//            counts (a kernel of the call, not a memset node)
//   pass 2   a workgroup per tile: sum of (d - mean)^2 of its chunk -> one partial
//            per tile; bucket indices by a float64 DIVISION (the correctly
//            rounded quotient: a reciprocal multiply or float32 arithmetic puts
//            values that sit on an edge into the neighbouring bucket) counted
//            into one LDS histogram per wave, then added to the segment's counts
//            (integer atomics: exact, any order)
//   finish 2 a workgroup per segment: folds the partial squares in a fixed order,
//            writes sq, stddev and the bucket rows
// The data is read twice because the centred squares need the mean and the
// bucket index needs the minimum and the width; the second read of a model's
// parameters (cfg2: 13 MB) finds them in L2 / Infinity Cache.  A thread adds its
// elements in index order, a wave's lanes meet in an xor butterfly, the waves and
// then the tiles are added in index order: the same bits on every call, no
// floating-point atomics.  A chunk whose first element is 16-byte aligned is read
// as float4 (FlatParams aligns every variable), any other with dword loads.
// Only elements of a segment are ever read.
#include "cg_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTsThreads = 256;
constexpr int kTsWaves = kTsThreads / 64;
constexpr int kTsChunk = 4096;       // elements of one tile
constexpr int kTsMaxBuckets = 512;
constexpr int kTsMaxSegments = 65535;
constexpr int kTsMaxGrid = 2048;     // workgroups of a pass; beyond: grid-stride
constexpr int kTsPlanThreads = 1024;

// the workspace: tile_start [nseg + 1] int64 | part1 [tiles][4] f64 (mn, mx, sum,
// nonfinite) | part2 [tiles] f64 | counts [nseg][k] uint32
struct TsLayout {
  long long tiles, part1, part2, counts, bytes;
};

inline TsLayout ts_layout(int nseg, long long total_len, int k) {
  TsLayout l;
  // sum of ceil(len / chunk) <= nseg + floor(total_len / chunk)
  l.tiles = (long long)nseg + total_len / kTsChunk;
  l.part1 = ((long long)nseg + 1) * 8;
  l.part2 = l.part1 + l.tiles * 32;
  l.counts = l.part2 + l.tiles * 8;
  l.bytes = l.counts + (((long long)nseg * k * 4 + 7) & ~7LL);
  return l;
}

// minimum, maximum and the two sums over the workgroup, in every thread.
// sm: [4][kTsWaves]
__device__ __forceinline__ void ts_block_fold(double& mn, double& mx, double& sum,
                                              double& nf, double (*sm)[kTsWaves]) {
  block_fold_put<FoldMin>(mn, sm[0]);
  block_fold_put<FoldMax>(mx, sm[1]);
  double v[2] = {sum, nf};
  block_fold_put<2>(v, &sm[2][threadIdx.x >> 6], kTsWaves);
  __syncthreads();
  mn = block_fold_get<kTsWaves, FoldMin>(sm[0]);
  mx = block_fold_get<kTsWaves, FoldMax>(sm[1]);
  sum = block_fold_get<kTsWaves>(sm[2]);
  nf = block_fold_get<kTsWaves>(sm[3]);
  __syncthreads();  // the slots are free again
}

__device__ __forceinline__ double ts_block_sum(double v, double* sm /*[kTsWaves]*/) {
  block_fold_put(v, sm);
  __syncthreads();
  v = block_fold_get<kTsWaves>(sm);
  __syncthreads();  // the slots are free again
  return v;
}

__device__ __forceinline__ long long ts_tiles_of(long long len) {
  return len > 0 ? (len + (kTsChunk - 1)) / kTsChunk : 0;
}

// the segment of tile t: tile_start[s] <= t < tile_start[s + 1] (t is below
// tile_start[nseg])
__device__ __forceinline__ int ts_segment_of(const long long* __restrict__ tile_start,
                                             int nseg, long long t) {
  int lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// f(x) on the m elements at q, a thread's elements in increasing index order; f
// carries its sums by value (captured by reference they stay in scratch memory)
template <class F>
__device__ __forceinline__ F ts_for_each(const float* __restrict__ q, int m, F f) {
  const int tid = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) {
    const int m4 = m >> 2;
    const float4* __restrict__ q4 = reinterpret_cast<const float4*>(q);
    for (int g = tid; g < m4; g += kTsThreads) {
      const float4 v = q4[g];
      f(v.x);
      f(v.y);
      f(v.z);
      f(v.w);
    }
    for (int i = (m4 << 2) + tid; i < m; i += kTsThreads) f(q[i]);
  } else {
    for (int i = tid; i < m; i += kTsThreads) f(q[i]);
  }
  return f;
}

__device__ __forceinline__ bool ts_nonfinite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

struct TsPass1 {
  double mn, mx, sum, nf;
  // (selects, not branches: hipcc merges the two arms' additions into one
  // through a runtime-indexed slot in scratch memory.  sum is never -0, so
  // adding +0 leaves it as it is)
  __device__ __forceinline__ void operator()(float x) {
    const bool bad = ts_nonfinite(x);
    const double d = (double)x;
    nf = nf + (bad ? 1.0 : 0.0);
    sum = sum + (bad ? 0.0 : d);
    mn = bad ? mn : fmin(mn, d);
    mx = bad ? mx : fmax(mx, d);
  }
};

// the centred squares, and the bucket indices into the wave's LDS histogram
// (hist == nullptr: all values are equal, nothing to count)
struct TsPass2 {
  double sq, mean, mn, w;
  int k;
  unsigned* hist;
  __device__ __forceinline__ void operator()(float x) {
    const double d = (double)x;
    const double c = d - mean;
    sq = sq + c * c;
    if (hist) {
      const double q = (d - mn) / w;
      long long i = (long long)floor(q);
      i = i < k - 1 ? i : k - 1;
      i = i > 0 ? i : 0;
      atomicAdd(&hist[i], 1u);
    }
  }
};

// tile_start[s] = number of tiles before segment s, clamped to the number of
// tiles the workspace was sized for (a total_len below the tables' sum is the
// caller's error; it must not become a write past the workspace)
__global__ __launch_bounds__(kTsPlanThreads) void ts_plan_kernel(
    const long long* __restrict__ seg_len, int nseg, long long max_tiles,
    long long* __restrict__ tile_start) {
  __shared__ long long sm[kTsPlanThreads];
  const int tid = threadIdx.x;
  const int per = (nseg + kTsPlanThreads - 1) / kTsPlanThreads;
  const int lo = min(tid * per, nseg), hi = min(lo + per, nseg);
  long long own = 0;
  for (int i = lo; i < hi; ++i) own += ts_tiles_of(seg_len[i]);
  sm[tid] = own;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < kTsPlanThreads; ++i) {
      const long long t = sm[i];
      sm[i] = run;
      run += t;
    }
    tile_start[nseg] = run < max_tiles ? run : max_tiles;
  }
  __syncthreads();
  long long run = sm[tid];
  for (int i = lo; i < hi; ++i) {
    tile_start[i] = run < max_tiles ? run : max_tiles;
    run += ts_tiles_of(seg_len[i]);
  }
}

__global__ __launch_bounds__(kTsThreads) void ts_pass1_kernel(
    const float* __restrict__ data, const long long* __restrict__ seg_off,
    const long long* __restrict__ seg_len, int nseg,
    const long long* __restrict__ tile_start, double* __restrict__ part1) {
  __shared__ double sm[4][kTsWaves];
  const long long total = tile_start[nseg];
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const int s = ts_segment_of(tile_start, nseg, t);
    const long long begin = (t - tile_start[s]) * kTsChunk;
    const long long left = seg_len[s] - begin;
    const int m = left < kTsChunk ? (int)left : kTsChunk;
    const TsPass1 own = ts_for_each(data + seg_off[s] + begin, m,
                                    TsPass1{INFINITY, -INFINITY, 0.0, 0.0});
    double mn = own.mn, mx = own.mx, sum = own.sum, nf = own.nf;
    ts_block_fold(mn, mx, sum, nf, sm);
    if (threadIdx.x == 0) {
      part1[t * 4 + 0] = mn;
      part1[t * 4 + 1] = mx;
      part1[t * 4 + 2] = sum;
      part1[t * 4 + 3] = nf;
    }
  }
}

__global__ __launch_bounds__(kTsThreads) void ts_finish1_kernel(
    const long long* __restrict__ seg_len, int nseg, int k,
    const long long* __restrict__ tile_start, const double* __restrict__ part1,
    unsigned* __restrict__ counts, double* __restrict__ stats) {
  __shared__ double sm[4][kTsWaves];
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const long long t1 = tile_start[s + 1];
    double mn = INFINITY, mx = -INFINITY, sum = 0.0, nf = 0.0;
    for (long long t = tile_start[s] + tid; t < t1; t += kTsThreads) {
      mn = fmin(mn, part1[t * 4 + 0]);
      mx = fmax(mx, part1[t * 4 + 1]);
      sum = sum + part1[t * 4 + 2];
      nf = nf + part1[t * 4 + 3];
    }
    ts_block_fold(mn, mx, sum, nf, sm);
    for (int j = tid; j < k; j += kTsThreads) counts[(long long)s * k + j] = 0u;
    if (tid == 0) {
      const double n = (double)seg_len[s];
      const bool bad = nf > 0.0;
      double* o = stats + (long long)s * 8;
      o[0] = n;
      o[1] = bad ? NAN : mn;
      o[2] = bad ? NAN : mx + 0.0;  // -0 -> +0, every other value unchanged
      o[3] = bad ? NAN : sum;
      o[4] = bad ? NAN : sum / n;
      o[7] = nf;
    }
  }
}

__global__ __launch_bounds__(kTsThreads) void ts_pass2_kernel(
    const float* __restrict__ data, const long long* __restrict__ seg_off,
    const long long* __restrict__ seg_len, int nseg, int k,
    const long long* __restrict__ tile_start, const double* __restrict__ stats,
    double* __restrict__ part2, unsigned* __restrict__ counts) {
  __shared__ double sm[kTsWaves];
  __shared__ unsigned sm_hist[kTsWaves][kTsMaxBuckets];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long total = tile_start[nseg];
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const int s = ts_segment_of(tile_start, nseg, t);
    const double* st = stats + (long long)s * 8;
    if (st[7] > 0.0) {  // (uniform) a NaN or an infinity: no squares, no buckets
      if (tid == 0) part2[t] = 0.0;
      continue;
    }
    const long long begin = (t - tile_start[s]) * kTsChunk;
    const long long left = seg_len[s] - begin;
    const int m = left < kTsChunk ? (int)left : kTsChunk;
    const double mn = st[1], mean = st[4];
    const double range = st[2] - mn;
    const bool binned = range != 0.0;  // uniform
    const double w = range / (double)k;
    if (binned) {
      for (int j = tid; j < kTsWaves * k; j += kTsThreads) sm_hist[j / k][j % k] = 0u;
      __syncthreads();
    }
    double sq = ts_for_each(data + seg_off[s] + begin, m,
                            TsPass2{0.0, mean, mn, w, k,
                                    binned ? sm_hist[wave] : nullptr}).sq;
    sq = ts_block_sum(sq, sm);  // (its barriers also close the LDS histograms)
    if (tid == 0) part2[t] = sq;
    if (binned) {
      for (int j = tid; j < k; j += kTsThreads) {
        unsigned c = 0u;
#pragma unroll
        for (int v = 0; v < kTsWaves; ++v) c += sm_hist[v][j];
        if (c) atomicAdd(&counts[(long long)s * k + j], c);
      }
      __syncthreads();  // before the next tile zeroes the histograms
    }
  }
}

__global__ __launch_bounds__(kTsThreads) void ts_finish2_kernel(
    int nseg, int k, const long long* __restrict__ tile_start,
    const double* __restrict__ part2, const unsigned* __restrict__ counts,
    double* __restrict__ stats, double* __restrict__ buckets) {
  __shared__ double sm[kTsWaves];
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const long long t1 = tile_start[s + 1];
    double sq = 0.0;
    for (long long t = tile_start[s] + tid; t < t1; t += kTsThreads) sq = sq + part2[t];
    sq = ts_block_sum(sq, sm);
    double* st = stats + (long long)s * 8;
    const double n = st[0], mn = st[1], mx = st[2];
    const bool bad = st[7] > 0.0;
    if (tid == 0) {
      st[5] = bad ? NAN : sq;
      st[6] = bad ? NAN : sqrt(sq / n);
    }
    const double range = mx - mn;
    const double w = range / (double)k;
    for (int j = tid; j < k; j += kTsThreads) {
      double left = 0.0, right = 0.0, count = 0.0;
      if (bad) {
      } else if (range == 0.0) {
        if (j == 0) left = mn - 0.5, right = mn + 0.5, count = n;
      } else {
        const double a = (double)j * w, b = (double)(j + 1) * w;
        left = mn + a;
        right = j + 1 == k ? mx : mn + b;
        count = (double)counts[(long long)s * k + j];
      }
      double* o = buckets + ((long long)s * k + j) * 3;
      o[0] = left;
      o[1] = right;
      o[2] = count;
    }
  }
}

bool ts_valid(int nseg, long long total_len, int k) {
  return nseg >= 1 && nseg <= kTsMaxSegments && k >= 1 && k <= kTsMaxBuckets &&
         total_len >= 1;
}

}  // namespace

extern "C" long long cg_tensor_summary_ws_bytes(int nseg, long long total_len,
                                                int num_buckets) {
  if (!ts_valid(nseg, total_len, num_buckets)) return -1;
  return ts_layout(nseg, total_len, num_buckets).bytes;
}

extern "C" int cg_tensor_summary(const float* data, const long long* seg_off,
                                 const long long* seg_len, int nseg,
                                 long long total_len, int num_buckets,
                                 double* stats, double* buckets, void* ws,
                                 long long ws_bytes, void* stream) {
  if (!data || !seg_off || !seg_len || !stats || !buckets || !ws ||
      !ts_valid(nseg, total_len, num_buckets))
    return CG_EINVAL;
  const TsLayout l = ts_layout(nseg, total_len, num_buckets);
  if (ws_bytes < l.bytes || (reinterpret_cast<uintptr_t>(ws) & 7)) return CG_EINVAL;
  char* base = static_cast<char*>(ws);
  long long* tile_start = reinterpret_cast<long long*>(base);
  double* part1 = reinterpret_cast<double*>(base + l.part1);
  double* part2 = reinterpret_cast<double*>(base + l.part2);
  unsigned* counts = reinterpret_cast<unsigned*>(base + l.counts);
  const int k = num_buckets;
  const dim3 tiles((unsigned)(l.tiles < kTsMaxGrid ? l.tiles : kTsMaxGrid));
  const dim3 segs((unsigned)(nseg < 1024 ? nseg : 1024));
  hipLaunchKernelGGL(ts_plan_kernel, dim3(1), dim3(kTsPlanThreads), 0, cg_stream(stream),
                     seg_len, nseg, l.tiles, tile_start);
  hipLaunchKernelGGL(ts_pass1_kernel, tiles, dim3(kTsThreads), 0, cg_stream(stream), data,
                     seg_off, seg_len, nseg, tile_start, part1);
  hipLaunchKernelGGL(ts_finish1_kernel, segs, dim3(kTsThreads), 0, cg_stream(stream),
                     seg_len, nseg, k, tile_start, part1, counts, stats);
  hipLaunchKernelGGL(ts_pass2_kernel, tiles, dim3(kTsThreads), 0, cg_stream(stream), data,
                     seg_off, seg_len, nseg, k, tile_start, stats, part2, counts);
  hipLaunchKernelGGL(ts_finish2_kernel, segs, dim3(kTsThreads), 0, cg_stream(stream),
                     nseg, k, tile_start, part2, counts, stats, buckets);
  CG_LAUNCH_CHECK();
}
