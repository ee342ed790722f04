// Pattern counts of the surrogate experiment (DESIGN.md 19;
// spike_metrics.pattern_histogram is the numpy statement).  A sample is T time
// steps x C neurons; its code is sum_{t, c} [x[n][t][c] != 0] << (t C + c), and
// counts[code] is the number of samples n < N with that code.  K = T C <=
// CG_PATTERN_HIST_MAX_BITS.
//
// Two launches per call:
//   zero    counts[0 .. 2^K) = 0 (a kernel, not a memset node)
//   count   a workgroup takes the tiles blockIdx, blockIdx + gridDim, ... of
//           CG_PATTERN_HIST_BLOCK_SAMPLES samples, one sample per thread and
//           tile.  The per-bit element offsets arrive as kernel arguments
//           (uniform: scalar registers).
//           gather   K single loads, four in flight at a time: any strides
//           packed   K / 4 16-byte loads: a sample whose K frames fill K
//                    consecutive elements in some order (the (n, L, C) layout
//                    and the (n, C, L) one read as its (n, L, C) view), K a
//                    multiple of 4, sample starts 16-byte aligned.  Element j
//                    of the sample sets bit pos[j].
//           K <= CG_PATTERN_HIST_LDS_BITS: the workgroup counts into a 32-bit
//           table in LDS and adds its non-zero entries to counts once, at the
//           end.  Above: every count goes to global memory.
// All additions are integer atomics (HIP's atomicAdd): any order gives the same
// counts.  Combining equal codes within a wave before the add (the first
// pending lane's code broadcast, its holders counted by a ballot, up to four
// rounds) was measured and is not here: 1 - 5 % slower on a draw of the
// dichotomised-Gaussian model and no faster on an input of equal samples
// (DESIGN.md 19.3).
#include "cg_common.h"

namespace {

constexpr int kPtThreads = CG_PATTERN_HIST_BLOCK_SAMPLES;
constexpr int kPtLdsSize = 1 << CG_PATTERN_HIST_LDS_BITS;
constexpr int kPtZeroThreads = 256;
constexpr int kPtZeroMaxBlocks = 2048;
// a workgroup's 32-bit LDS counts hold its share of N below this
constexpr long long kPtMaxSamples = 1ll << 40;
static_assert(kPtThreads % 64 == 0 && kPtThreads <= 1024, "one sample per thread");
static_assert(CG_PATTERN_HIST_MAX_BITS % 4 == 0 && CG_PATTERN_HIST_MAX_BITS < 32,
              "four bits at a time into a 32-bit code");
static_assert(kPtMaxSamples / CG_PATTERN_HIST_MAX_BLOCKS +
                      CG_PATTERN_HIST_BLOCK_SAMPLES < (1ll << 32),
              "32-bit counts per workgroup");

struct PtOffsets {
  long long o[CG_PATTERN_HIST_MAX_BITS];  // element offset of bit k; 0 for k >= K
  int pos[CG_PATTERN_HIST_MAX_BITS];      // packed: the bit element j sets
};

__global__ __launch_bounds__(kPtZeroThreads) void pattern_zero_kernel(
    long long* __restrict__ counts, long long size) {
  for (long long i = (long long)blockIdx.x * kPtZeroThreads + threadIdx.x; i < size;
       i += (long long)gridDim.x * kPtZeroThreads)
    counts[i] = 0;
}

template <bool PACKED>
__device__ __forceinline__ unsigned pattern_code(const float* __restrict__ p,
                                                 const PtOffsets& off, int K) {
  unsigned code = 0;
  if (PACKED) {
    constexpr int kVecs = CG_PATTERN_HIST_MAX_BITS / 4;
    float4 v[kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j)
      if (4 * j < K) v[j] = *reinterpret_cast<const float4*>(p + 4 * j);  // uniform
#pragma unroll
    for (int j = 0; j < kVecs; ++j)
      if (4 * j < K) {
        code |= (unsigned)(v[j].x != 0.0f) << off.pos[4 * j];
        code |= (unsigned)(v[j].y != 0.0f) << off.pos[4 * j + 1];
        code |= (unsigned)(v[j].z != 0.0f) << off.pos[4 * j + 2];
        code |= (unsigned)(v[j].w != 0.0f) << off.pos[4 * j + 3];
      }
    return code;
  }
#pragma unroll
  for (int k0 = 0; k0 < CG_PATTERN_HIST_MAX_BITS; k0 += 4) {
    if (k0 >= K) break;  // uniform
    float v[4];
    // (bits K .. k0 + 3 read the sample's first frame again and are masked off)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[off.o[k0 + j]];
#pragma unroll
    for (int j = 0; j < 4; ++j) code |= (unsigned)(v[j] != 0.0f) << (k0 + j);
  }
  return code & ((1u << K) - 1u);
}

template <bool LDS, bool PACKED>
__global__ __launch_bounds__(kPtThreads) void pattern_count_kernel(
    const float* __restrict__ x, long long N, long long s_n, PtOffsets off, int K,
    unsigned long long* __restrict__ counts) {
  __shared__ unsigned sm[LDS ? kPtLdsSize : 1];
  const int tid = threadIdx.x;
  const int size = 1 << K;
  if (LDS) {
    for (int i = tid; i < size; i += kPtThreads) sm[i] = 0;
    __syncthreads();
  }
  const long long tiles = (N + kPtThreads - 1) / kPtThreads;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long n = tile * kPtThreads + tid;
    if (n < N) {
      const unsigned code = pattern_code<PACKED>(x + n * s_n, off, K);
      if (LDS)
        atomicAdd(&sm[code], 1u);
      else
        atomicAdd(&counts[code], 1ull);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = tid; i < size; i += kPtThreads) {
      const unsigned v = sm[i];
      if (v) atomicAdd(&counts[i], (unsigned long long)v);
    }
  }
}

inline bool pattern_shape_ok(long long N, int T, int C) {
  return N >= 1 && N <= kPtMaxSamples && T >= 1 && C >= 1 &&
         (long long)T * C <= CG_PATTERN_HIST_MAX_BITS;
}

}  // namespace

extern "C" long long cg_pattern_hist_ws_bytes(long long N, int T, int C) {
  // both forms add into counts itself, zeroed by the call's first launch
  return pattern_shape_ok(N, T, C) ? 0 : -1;
}

extern "C" int cg_pattern_histogram(const float* spikes, long long N, int T, int C,
                                    long long s_n, long long s_t, long long s_c,
                                    long long* counts, void* ws,
                                    long long ws_bytes, void* stream) {
  (void)ws;
  if (!spikes || !counts || !pattern_shape_ok(N, T, C) ||
      ws_bytes < cg_pattern_hist_ws_bytes(N, T, C))
    return CG_EINVAL;
  const int K = T * C;
  PtOffsets off;
  // packed: the offsets are a permutation of 0 .. K - 1
  bool packed = K % 4 == 0 && s_n % 4 == 0 &&
                reinterpret_cast<uintptr_t>(spikes) % 16 == 0;
  for (int k = 0; k < CG_PATTERN_HIST_MAX_BITS; ++k) off.pos[k] = -1;
  for (int k = 0; k < CG_PATTERN_HIST_MAX_BITS; ++k) {
    off.o[k] = k < K ? (k / C) * s_t + (k % C) * s_c : 0;
    if (k >= K) continue;
    if (off.o[k] < 0 || off.o[k] >= K || off.pos[off.o[k]] >= 0)
      packed = false;
    else
      off.pos[off.o[k]] = k;
  }
  const long long size = 1ll << K;
  const long long zb = (size + kPtZeroThreads - 1) / kPtZeroThreads;
  hipLaunchKernelGGL(pattern_zero_kernel,
                     dim3((unsigned)(zb < kPtZeroMaxBlocks ? zb : kPtZeroMaxBlocks)),
                     dim3(kPtZeroThreads), 0, cg_stream(stream), counts, size);
  const long long tiles = (N + kPtThreads - 1) / kPtThreads;
  const dim3 grid((unsigned)(tiles < CG_PATTERN_HIST_MAX_BLOCKS
                                 ? tiles
                                 : CG_PATTERN_HIST_MAX_BLOCKS));
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
#define CG_PT_LAUNCH(LDS, PACKED)                                               \
  hipLaunchKernelGGL((pattern_count_kernel<LDS, PACKED>), grid,                 \
                     dim3(kPtThreads), 0, cg_stream(stream), spikes, N, s_n, off, K, out)
  if (K <= CG_PATTERN_HIST_LDS_BITS) {
    if (packed) CG_PT_LAUNCH(true, true); else CG_PT_LAUNCH(true, false);
  } else {
    if (packed) CG_PT_LAUNCH(false, true); else CG_PT_LAUNCH(false, false);
  }
#undef CG_PT_LAUNCH
  CG_LAUNCH_CHECK();
}
