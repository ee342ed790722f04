// Cross-correlograms and population counts of binary spike trains (DESIGN.md
// 21; spike_metrics.cross_correlogram / population_count_histogram are the
// numpy statements).
//
//   ccg[b][tau][i][j] = sum_{t = 0}^{T - 1 - tau} s_i(t) s_j(t + tau)
//
// One workgroup owns a 64 x 64 block (P, Q) of neurons of one sample and a group
// of kCcgLags consecutive lags tau0 .. tau0 + 7, tau0 a multiple of 8, and walks
// the whole of T in chunks of kCcgChunk frames with the accumulators in
// registers: every output element is written once, by one workgroup, with no
// atomics, no workspace and nothing zeroed beforehand.  A chunk is staged in LDS
// neuron-major as bf16 {0, 1}: the rows of block P from frame t0 (the A side),
// the rows of block Q from frame t0 + tau0 with 8 frames more (the B side);
// frames >= T and neurons >= C are zeros, so a product that the definition does
// not hold vanishes by itself and a lag >= T gives zeros.  Time is the K
// dimension of v_mfma_f32_16x16x32_bf16: lane l holds 8 consecutive frames from
// 8 (l >> 4) of neuron l & 15 on either side.  The B fragment of lag tau0 + r
// starts r frames later: two aligned 16-byte reads hold the 16 frames all eight
// shifts lie in, and a funnel shift (v_alignbit_b32 for an odd r) forms each.
// Wave w takes the row tile w of the block against its four column tiles: one A
// read and eight B reads feed 32 MFMAs.  0 and 1 are exact in bf16 and an f32
// sum of at most 2^24 such products is exact, so the conversion to int32 does
// not round and the order of the sum does not matter.
//
// The population histogram: one workgroup per sample, an aligned group of lanes
// per frame (group_sum_n of cg_common.h), the counts in an LDS table.
#include "cg_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 ccg_bf16x8;

constexpr int kCcgThreads = 256;
constexpr int kCcgWaves = kCcgThreads / 64;
constexpr int kCcgBlock = 64;                  // neurons of a row / column block
constexpr int kCcgTiles = kCcgBlock / 16;      // 16-neuron tiles of a block
static_assert(kCcgWaves == kCcgTiles, "one row tile per wave");
constexpr int kCcgLags = 8;                    // lags of one workgroup
constexpr int kCcgChunk = 128;                 // frames per LDS chunk
// LDS row of one neuron: the chunk and the 8 frames the shifted fragments reach
// into.  272 bytes: rows r and r + 1 lie one 16-byte slot apart modulo the
// 256-byte bank row, so the 16 rows of a ds_read_b128 lane group (and of a
// staging write) fall on 16 distinct slots
constexpr int kCcgRow = kCcgChunk + kCcgLags;  // bf16 elements
static_assert(kCcgRow * 2 % 256 == 16, "row pitch one slot past a bank row");
constexpr int kCcgMaxT = 1 << 24;
constexpr unsigned kBf16One = 0x3F80u;

// Rows n0 .. n0 + 63 of the sample, frames f0 .. f0 + 8 GROUPS, as bf16 {0, 1}:
// lane n of wave w takes neuron n0 + n and the groups of 8 frames w, w + 4, ...
// Every load is issued before the first is looked at, from an address clamped
// into the sample (neuron 0 for a row past C, frame T - 1 past the end); what
// was clamped is stored as zero.  (A load under its own bounds test makes hipcc
// wait for each in turn: a chunk then costs 72 round trips to the L2.)
template <int GROUPS>
__device__ __forceinline__ void ccg_stage(uint4* __restrict__ sm,
                                          const float* __restrict__ sp,
                                          long long s_t, long long s_c, int n0,
                                          int f0, int T, int C, int wave) {
  constexpr int kIters = (GROUPS + kCcgWaves - 1) / kCcgWaves;
  const int n = threadIdx.x & 63;
  const bool live = n0 + n < C;
  const float* row = sp + (long long)(live ? n0 + n : 0) * s_c;
  float v[kIters][8];
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int fg = wave + it * kCcgWaves;
    if ((it + 1) * kCcgWaves <= GROUPS || fg < GROUPS) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        v[it][e] = row[(long long)min(f0 + fg * 8 + e, T - 1) * s_t];
    }
  }
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int fg = wave + it * kCcgWaves;
    if ((it + 1) * kCcgWaves <= GROUPS || fg < GROUPS) {
      unsigned h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        h[e] = (live && f0 + fg * 8 + e < T && v[it][e] != 0.f) ? kBf16One : 0u;
      uint4 w;
      w.x = h[0] | h[1] << 16;
      w.y = h[2] | h[3] << 16;
      w.z = h[4] | h[5] << 16;
      w.w = h[6] | h[7] << 16;
      sm[n * (kCcgRow / 8) + fg] = w;
    }
  }
}

// elements R .. R + 7 of the 16 bf16 in (lo, hi)
// (R a constant once the caller's loop is unrolled)
__device__ __forceinline__ ccg_bf16x8 ccg_shift(const uint4& lo, const uint4& hi,
                                                const int R) {
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint4 o;
  if (R % 2 == 0) {
    o.x = w[R / 2]; o.y = w[R / 2 + 1]; o.z = w[R / 2 + 2]; o.w = w[R / 2 + 3];
  } else {
    o.x = __builtin_amdgcn_alignbit(w[R / 2 + 1], w[R / 2], 16);
    o.y = __builtin_amdgcn_alignbit(w[R / 2 + 2], w[R / 2 + 1], 16);
    o.z = __builtin_amdgcn_alignbit(w[R / 2 + 3], w[R / 2 + 2], 16);
    o.w = __builtin_amdgcn_alignbit(w[R / 2 + 4], w[R / 2 + 3], 16);
  }
  return __builtin_bit_cast(ccg_bf16x8, o);
}

// One staged chunk into the accumulators of a wave: acc[c][r] += A_w B_c(r) for
// the four column tiles c and the eight lags r in one unbranched stream.  (A
// column tile past C holds zeros, and a lag past max_lag is computed and not
// written: hipcc keeps the accumulators in place only without branches here.)
__device__ __forceinline__ void ccg_chunk(f32x4 (&acc)[kCcgTiles][kCcgLags],
                                          const uint4* __restrict__ sm_a,
                                          const uint4* __restrict__ sm_b, int wave,
                                          int lane) {
#pragma unroll
  for (int kk = 0; kk < kCcgChunk / 32; ++kk) {
    // row (column) l & 15, frames 8 (l >> 4) ..
    const int at = (lane & 15) * (kCcgRow / 8) + kk * 4 + (lane >> 4);
    const ccg_bf16x8 a =
        __builtin_bit_cast(ccg_bf16x8, sm_a[(wave * 16) * (kCcgRow / 8) + at]);
#pragma unroll
    for (int c = 0; c < kCcgTiles; ++c) {
      const uint4 lo = sm_b[(c * 16) * (kCcgRow / 8) + at];
      const uint4 hi = sm_b[(c * 16) * (kCcgRow / 8) + at + 1];
#pragma unroll
      for (int r = 0; r < kCcgLags; ++r)
        acc[c][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, ccg_shift(lo, hi, r), acc[c][r], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(kCcgThreads, 2) void spike_ccg_kernel(
    const float* __restrict__ spikes, long long s_b, long long s_t, long long s_c,
    int T, int C, int max_lag, long long items, int* __restrict__ ccg) {
  __shared__ uint4 sm_a[kCcgBlock * kCcgRow / 8];
  __shared__ uint4 sm_b[kCcgBlock * kCcgRow / 8];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NB = (C + kCcgBlock - 1) / kCcgBlock;
  const int NG = max_lag / kCcgLags + 1;
  const int per_sample = NB * NB * NG;
  // item -> (sample, lag group, P, Q), the blocks of a sample next to each other
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long b = item / per_sample;
    int rem = (int)(item - b * per_sample);
    const int lg = rem / (NB * NB);
    rem -= lg * NB * NB;
    const int P = rem / NB, Q = rem - P * NB;
    const int tau0 = lg * kCcgLags;
    const int nl = min(kCcgLags, max_lag + 1 - tau0);  // lags of this group
    const float* sp = spikes + b * s_b;
    const int i0 = P * kCcgBlock + wave * 16;          // this wave's row tile
    const bool rows = i0 < C;

    f32x4 acc[kCcgTiles][kCcgLags];
#pragma unroll
    for (int c = 0; c < kCcgTiles; ++c)
#pragma unroll
      for (int r = 0; r < kCcgLags; ++r) acc[c][r] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t0 = 0; t0 < T; t0 += kCcgChunk) {
      ccg_stage<kCcgChunk / 8>(sm_a, sp, s_t, s_c, P * kCcgBlock, t0, T, C, wave);
      ccg_stage<kCcgRow / 8>(sm_b, sp, s_t, s_c, Q * kCcgBlock, t0 + tau0, T, C,
                             wave);
      __syncthreads();
      if (rows) {
        ccg_chunk(acc, sm_a, sm_b, wave, lane);
      }
      __syncthreads();
    }

    // C/D: column lane & 15, row 4 (lane >> 4) + reg
    if (rows) {
#pragma unroll
      for (int r = 0; r < kCcgLags; ++r) {
        if (r < nl) {
          int* plane = ccg + ((b * (max_lag + 1) + tau0 + r) * C) * (long long)C;
#pragma unroll
          for (int c = 0; c < kCcgTiles; ++c) {
            const int j = Q * kCcgBlock + c * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int i = i0 + 4 * (lane >> 4) + reg;
              if (i < C && j < C) plane[(long long)i * C + j] = (int)acc[c][r][reg];
            }
          }
        }
      }
    }
  }
}

// hist[b][k]: frames of sample b with exactly k spikes.  N lanes per frame.
constexpr int kPhThreads = 1024;
template <int N>
__global__ __launch_bounds__(kPhThreads) void population_hist_kernel(
    const float* __restrict__ spikes, long long s_b, long long s_t, long long s_c,
    int T, int C, int* __restrict__ hist) {
  __shared__ int sm[CG_CCG_MAX_C + 1];
  const int tid = threadIdx.x;
  for (int k = tid; k <= C; k += kPhThreads) sm[k] = 0;
  __syncthreads();
  const float* sp = spikes + (long long)blockIdx.x * s_b;
  const int sub = tid & (N - 1), slot = tid / N;
  // (every lane goes through every pass: the group sums are cross-lane moves)
  for (int t0 = 0; t0 < T; t0 += kPhThreads / N) {
    const int t = t0 + slot;
    float n = 0.f;  // at most 1024: exact
    if (t < T) {
      const float* p = sp + (long long)t * s_t;
      for (int c = sub; c < C; c += N) n += p[(long long)c * s_c] != 0.f ? 1.f : 0.f;
    }
    n = group_sum_n(n, N);
    if (sub == 0 && t < T) atomicAdd(&sm[(int)n], 1);
  }
  __syncthreads();
  int* out = hist + (long long)blockIdx.x * (C + 1);
  for (int k = tid; k <= C; k += kPhThreads) out[k] = sm[k];
}

inline bool ccg_shape_ok(int B, int T, int C) {
  return B >= 1 && T >= 1 && C >= 1 && T <= kCcgMaxT && C <= CG_CCG_MAX_C;
}

}  // namespace

extern "C" int cg_spike_ccg(const float* spikes, int B, int T, int C,
                            long long s_b, long long s_t, long long s_c,
                            int max_lag, int* ccg, void* stream) {
  if (!spikes || !ccg || !ccg_shape_ok(B, T, C) || max_lag < 0 ||
      max_lag > CG_CCG_MAX_LAG)
    return CG_EINVAL;
  const long long NB = (C + kCcgBlock - 1) / kCcgBlock;
  const long long items = (long long)B * NB * NB * (max_lag / kCcgLags + 1);
  const long long cap = 1ll << 30;
  hipLaunchKernelGGL(spike_ccg_kernel, dim3((unsigned)(items < cap ? items : cap)),
                     dim3(kCcgThreads), 0, cg_stream(stream), spikes, s_b, s_t, s_c,
                     T, C, max_lag, items, ccg);
  CG_LAUNCH_CHECK();
}

extern "C" int cg_spike_population_hist(const float* spikes, int B, int T, int C,
                                        long long s_b, long long s_t,
                                        long long s_c, int* hist, void* stream) {
  if (!spikes || !hist || !ccg_shape_ok(B, T, C)) return CG_EINVAL;
  if (C <= 16)
    hipLaunchKernelGGL(population_hist_kernel<16>, dim3(B), dim3(kPhThreads), 0,
                       cg_stream(stream), spikes, s_b, s_t, s_c, T, C, hist);
  else
    hipLaunchKernelGGL(population_hist_kernel<64>, dim3(B), dim3(kPhThreads), 0,
                       cg_stream(stream), spikes, s_b, s_t, s_c, T, C, hist);
  CG_LAUNCH_CHECK();
}
