// Power spectra of calcium traces on the device (compute_metrics.py
// --spectral_metrics): per neuron the periodogram of the mean-removed,
// Hann-windowed trace, summed over the trials of a batch,
//   cg_trace_psd  totals[k][c] = sum_b |sum_t y_t e^{-2 pi i k t / T}|^2,
//                 y_t = (x[b][t][c] - m) w_t, k = 0 .. T / 2
// m = float32(sum_t float64(x_t) / T), w_t = float32(0.5 - 0.5 cospi(2 t / T)),
// the difference and the product each rounded to float32.  The numpy statement
// is signals_metrics.trace_power_spectrum.
//
// Shaped as ifft.hip: 512 threads, the stages of fft_stages.h on the swizzled
// [T][G] LDS image, G = min(16, 8192 / T), at most 1024 workgroups walking the
// items grid-stride.  What differs:
//   pairs   the image's real parts hold neuron c0 + 2 g, its imaginary parts
//           neuron c0 + 2 g + 1 (a global row of 2 G consecutive floats goes to
//           one LDS row of 2 G floats as it lies).  With W the transform of
//           z = a + i b, W' that of bin T - k:  |A_k|^2 = |W' + conj W|^2 / 4,
//           |B_k|^2 = |W' - conj W|^2 / 4 -- the same whichever sign the
//           stages' twiddles have, so nothing is conjugated.  A workgroup
//           transforms 2 G neurons in the LDS passes ifft.hip spends on G.  An
//           odd last neuron pairs with zeros.
//   item    one group of 2 G neurons x one chunk of consecutive trials.  A lane
//           owns up to 8 (row, column) positions with bin < T / 2 (row p holds
//           bin u = ifft_time_of_row(p); u < T / 2 is bit 1 of p clear), lanes
//           0 .. G - 1 also row 2 (bin T / 2), and keeps two float64 sums per
//           position over the chunk's trials, in trial order.  They go to
//           partial[chunk][u][c] in the workspace; a second launch adds the
//           chunks in index order and applies the 1/4 (exact).  The chunking is
//           a function of (B, T, C) alone and every partial element is written:
//           the same bits every call, nothing zeroed beforehand, no atomics.
//   mean    a lane's loads all belong to one column (512 is a multiple of 2 G):
//           it sums them in float64 as they arrive, the lanes of a column meet
//           by an xor butterfly inside the wave and the 8 waves' values are
//           added in wave order.  The window is then applied in place.
//   NaN     a non-finite sample would reach its partner through the packed
//           transform.  The column sum of such a trace is not finite (finite
//           float32 values cannot overflow a float64 sum): zeros are transformed
//           in its place and the neuron's partials are written as NaN.
//   zero    a trial whose y is all zero (a constant trace) adds exact zeros:
//           what the transform leaves in its half of the unpacking is the
//           partner's rounding error, not its own.
// LDS: the image (<= 64 KiB), T / 4 twiddles, T / 2 + 1 window values (w_t =
// w_{T - t}), the row of bin T - u for every row of a bin u < T / 2 (16 bits
// each) and 2.6 KiB of reduction slots: 79 KiB at T = 2048, two workgroups a
// CU; 106 KiB at T = 8192, one.
#include "cg_common.h"

#include "fft_stages.h"

namespace {

constexpr int kPsdWaves = kPsdThreads / 64;
constexpr int kPsdMaxGrid = 1024;      // workgroups; beyond: grid-stride
constexpr int kPsdMaxCols = 2 * kIfftMaxGroup;
// positions with bin < T / 2 per lane at most, and the one of bin T / 2
constexpr int kPsdSlots = kIfftTraceElems / 2 / kPsdThreads;
// chunking: about kPsdTargetItems items (two workgroups on each of 256 CUs), at
// most kPsdMaxChunks partial images, at least kPsdMinChunk trials between two
// writes of a partial image
constexpr int kPsdTargetItems = 512;
constexpr int kPsdMaxChunks = 64;
constexpr int kPsdMinChunk = 4;
constexpr int kPsdLoadBatch = 4;
constexpr int kPsdFinishThreads = 256;

struct PsdPlan {
  int groups, chunk_len, chunks;
};

inline PsdPlan psd_plan(int B, int T, int C) {
  PsdPlan p;
  const int cols = 2 * ifft_group(T);
  p.groups = (C - 1) / cols + 1;
  int want = (kPsdTargetItems - 1) / p.groups + 1;
  if (want > kPsdMaxChunks) want = kPsdMaxChunks;
  p.chunk_len = (B - 1) / want + 1;
  if (p.chunk_len < kPsdMinChunk) p.chunk_len = kPsdMinChunk;
  if (p.chunk_len > B) p.chunk_len = B;
  p.chunks = (B - 1) / p.chunk_len + 1;
  return p;
}

// (x - m) w, the difference and the product each rounded to float32
__device__ __forceinline__ float psd_window(float x, float m, float w) {
#pragma clang fp contract(off)
  float a = x - m;
  a = a * w;
  return a;
}

struct PsdArgs {
  const float* x;
  long long s_b, s_t, s_c;
  double* partial;  // [chunks][T / 2 + 1][C]
  int B, T, C, groups, chunk_len, chunks, odd;
  long long items;  // chunks * groups
};

__global__ __launch_bounds__(kPsdThreads, 4) void trace_psd_kernel(PsdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char psd_lds[];
  const int T = a.T, G = ifft_group(T), rows_mask = 32 / G - 1;
  cf32* buf = reinterpret_cast<cf32*>(psd_lds);    // [T][G]
  float* fbuf = reinterpret_cast<float*>(psd_lds);  // [T][2 G]
  cf32* tw = buf + (size_t)T * G;                   // [T / 4]
  float* win = reinterpret_cast<float*>(tw + T / 4);  // [T / 2 + 1] (+ 1 pad)
  double* red = reinterpret_cast<double*>(win + T / 2 + 2);  // [waves][32]
  float* mean = reinterpret_cast<float*>(red + kPsdWaves * kPsdMaxCols);
  int* bad = reinterpret_cast<int*>(mean + kPsdMaxCols);  // in any trial so far
  int* cur = bad + kPsdMaxCols;                           // in this trial
  int* nonzero = cur + kPsdMaxCols;  // y of this trial has a non-zero value
  unsigned short* mrow = reinterpret_cast<unsigned short*>(nonzero + kPsdMaxCols);
  const int tid = threadIdx.x;
  const int gshift = __builtin_ctz(G), cshift = gshift + 1, cols = 2 * G;
  const int elems = T * G;  // 512 at least, a power of two
  const int floats = 2 * elems;
  const int bins = T / 2 + 1;

  fft_fill_twiddles<kPsdThreads>(tw, T, tid);
  for (int k = tid; k <= T / 2; k += kPsdThreads)
    win[k] = (float)(0.5 - 0.5 * cospi(2.0 * (double)k / (double)T));

  // mrow[j]: the LDS row of bin T - u for the j-th row with bin u < T / 2
  for (int j = tid; j < T / 2; j += kPsdThreads) {
    const int u = ifft_time_of_row(psd_low_row(j), T, a.odd);
    mrow[j] = (unsigned short)ifft_phys(
        ifft_row_of_time((T - u) & (T - 1), T, a.odd), rows_mask);
  }
  // the neuron pair of every position of the lane (512 is a multiple of G)
  const int gl = tid & (G - 1);
  const int self = ifft_phys(2, rows_mask) * G + gl;  // bin T / 2: row 2
  // the lane's column of the [T][2 G] image, in every load it makes
  const int col = tid & (cols - 1);
  const int lane = tid & 63, wave = tid >> 6;

  // (consecutive items are neighbouring neuron groups of one chunk)
  for (long long item = cg_xcd_first_item(); item < a.items; item += gridDim.x) {
    const int chunk = (int)(item / a.groups);
    const int c0 = (int)(item - (long long)chunk * a.groups) * cols;
    const int b0 = chunk * a.chunk_len;
    const int b1 = b0 + a.chunk_len < a.B ? b0 + a.chunk_len : a.B;
    const bool live = c0 + col < a.C;
    // a neuron past the last reads the last one's (valid) address
    const long long coff = (long long)(live ? c0 + col : a.C - 1) * a.s_c;
    double acc[kPsdSlots + 1][2];
#pragma unroll
    for (int s = 0; s <= kPsdSlots; ++s) acc[s][0] = acc[s][1] = 0.0;
    if (tid < kPsdMaxCols) bad[tid] = 0;  // (read after this trial's barriers)

    for (int b = b0; b < b1; ++b) {
      // (the trial's index arithmetic starts from a value the compiler cannot
      // see through: hoisted out of this loop, the stages' LDS addresses alone
      // take more registers than two workgroups a CU leave a lane)
      int lt = tid;
      asm volatile("" : "+v"(lt));
      const float* xb = a.x + (long long)b * a.s_b + coff;
      double sum = 0.0;
      for (int first = lt; first < floats; first += kPsdThreads * kPsdLoadBatch) {
        float v[kPsdLoadBatch];
#pragma unroll
        for (int u = 0; u < kPsdLoadBatch; ++u) {
          const int idx = first + u * kPsdThreads;
          if (idx < floats)  // (the same in every lane)
            v[u] = xb[(long long)(idx >> cshift) * a.s_t];
        }
#pragma unroll
        for (int u = 0; u < kPsdLoadBatch; ++u) {
          const int idx = first + u * kPsdThreads;
          if (idx < floats) {
            const float val = live ? v[u] : 0.f;
            sum += (double)val;
            fbuf[ifft_phys(idx >> cshift, rows_mask) * cols + col] = val;
          }
        }
      }
      for (int o = 32; o >= cols; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (lane < cols) red[wave * kPsdMaxCols + lane] = sum;
      __syncthreads();
      if (lt < cols) {
        double s = red[lt];
#pragma unroll
        for (int w = 1; w < kPsdWaves; ++w) s += red[w * kPsdMaxCols + lt];
        const bool finite = s - s == 0.0;
        mean[lt] = (float)(s / (double)T);
        cur[lt] = !finite;
        nonzero[lt] = 0;
        if (!finite) bad[lt] = 1;
      }
      __syncthreads();

      {
        const float m = mean[col];
        const bool zero = cur[col] != 0;
        bool any = false;
        for (int first = lt; first < floats; first += kPsdThreads * kPsdLoadBatch) {
          float v[kPsdLoadBatch];
#pragma unroll
          for (int u = 0; u < kPsdLoadBatch; ++u) {
            const int idx = first + u * kPsdThreads;
            if (idx < floats)
              v[u] = fbuf[ifft_phys(idx >> cshift, rows_mask) * cols + col];
          }
#pragma unroll
          for (int u = 0; u < kPsdLoadBatch; ++u) {
            const int idx = first + u * kPsdThreads;
            if (idx < floats) {
              const int t = idx >> cshift;
              const float w = win[t <= T / 2 ? t : T - t];
              const float y = zero ? 0.f : psd_window(v[u], m, w);
              any |= y != 0.f;
              fbuf[ifft_phys(t, rows_mask) * cols + col] = y;
            }
          }
        }
        if (any) nonzero[col] = 1;  // (every writer stores the same value)
      }
      __syncthreads();

      // fft_run_stages<kPsdThreads, kPsdBflyBatch>(..., lt), written out: called
      // through the driver the stages are the same and two spills fewer, but
      // hipcc then fuses dr * dr + si * si of the unpacking below as fma(si, si,
      // dr * dr) in every slot, where this text gets fma(dr, dr, si * si) in the
      // later ones, and a few totals in a thousand move by an ulp
      // (profiles/fft_schedule_once.txt).
      int N = T;
      if (a.odd) {
        const int count = elems / 2;
        for (int first = lt; first < count; first += kPsdThreads * kPsdBflyBatch) {
          IfftBfly f[kPsdBflyBatch];
#pragma unroll
          for (int u = 0; u < kPsdBflyBatch; ++u) {
            const int idx = first + u * kPsdThreads;
            if (idx < count)
              ifft_radix2_load(f[u], buf, T, G, rows_mask, idx >> gshift, idx & (G - 1));
          }
#pragma unroll
          for (int u = 0; u < kPsdBflyBatch; ++u)
            if (first + u * kPsdThreads < count) ifft_radix2_finish(f[u], tw, T);
        }
        __syncthreads();
        N = T / 2;
      }
      for (; N >= 4; N >>= 2) {
        const int count = elems / 4;
        for (int first = lt; first < count; first += kPsdThreads * kPsdBflyBatch) {
          IfftBfly f[kPsdBflyBatch];
#pragma unroll
          for (int u = 0; u < kPsdBflyBatch; ++u) {
            const int idx = first + u * kPsdThreads;
            if (idx < count)
              ifft_radix4_load(f[u], buf, G, rows_mask, N, idx >> gshift, idx & (G - 1));
          }
#pragma unroll
          for (int u = 0; u < kPsdBflyBatch; ++u)
            if (first + u * kPsdThreads < count) ifft_radix4_finish(f[u], tw, T, N);
        }
        __syncthreads();
      }

      // An all-zero y adds exact zeros: its partner's rounding errors are not
      // mirror images of each other and would leave ~1e-14 of its power here.
      const bool add_a = nonzero[2 * gl] != 0, add_b = nonzero[2 * gl + 1] != 0;
#pragma unroll
      for (int s = 0; s <= kPsdSlots; ++s) {
        const int idx = lt + s * kPsdThreads;
        if (s < kPsdSlots ? idx < elems / 2 : lt < G) {
          const int j = idx >> gshift;
          const cf32 w1 = buf[s < kPsdSlots
                                  ? ifft_phys(psd_low_row(j), rows_mask) * G + gl
                                  : self];
          const cf32 w2 = buf[s < kPsdSlots ? (int)mrow[j] * G + gl : self];
          const double sr = (double)w2.re + (double)w1.re;
          const double di = (double)w2.im - (double)w1.im;
          const double dr = (double)w2.re - (double)w1.re;
          const double si = (double)w2.im + (double)w1.im;
          acc[s][0] += add_a ? sr * sr + di * di : 0.0;
          acc[s][1] += add_b ? dr * dr + si * si : 0.0;
        }
      }
      __syncthreads();  // the next trial's load overwrites buf
    }

    double* part = a.partial + (long long)chunk * bins * a.C;
#pragma unroll
    for (int s = 0; s <= kPsdSlots; ++s) {
      const int idx = tid + s * kPsdThreads;
      if (s < kPsdSlots ? idx < elems / 2 : tid < G) {
        const int p = s < kPsdSlots ? psd_low_row(idx >> gshift) : 2;
        const int u = ifft_time_of_row(p, T, a.odd);
        const int c = c0 + 2 * gl;
        double* dst = part + (long long)u * a.C + c;
        if (c < a.C) dst[0] = bad[2 * gl] ? __builtin_nan("") : acc[s][0];
        if (c + 1 < a.C) dst[1] = bad[2 * gl + 1] ? __builtin_nan("") : acc[s][1];
      }
    }
    __syncthreads();  // the next item clears bad
  }
}

// totals[e] = (1/4) sum over the chunks, in index order
__global__ __launch_bounds__(kPsdFinishThreads) void trace_psd_finish_kernel(
    const double* partial, int chunks, long long n, double* totals) {
  for (long long e = (long long)blockIdx.x * kPsdFinishThreads + threadIdx.x; e < n;
       e += (long long)gridDim.x * kPsdFinishThreads) {
    double s = partial[e];
    for (int ch = 1; ch < chunks; ++ch) s += partial[(long long)ch * n + e];
    totals[e] = 0.25 * s;
  }
}

inline size_t psd_lds_bytes(int T) {
  return fft_lds_bytes(T) + (size_t)(T / 2 + 2) * sizeof(float) +
         (size_t)kPsdWaves * kPsdMaxCols * sizeof(double) +
         (size_t)kPsdMaxCols * (sizeof(float) + 3 * sizeof(int)) +
         (size_t)(T / 2) * sizeof(unsigned short);
}

inline bool psd_shape_ok(int B, int T, int C) {
  return B >= 1 && C >= 1 && fft_length_ok(T);
}

}  // namespace

extern "C" long long cg_trace_psd_ws_bytes(int B, int T, int C) {
  if (!psd_shape_ok(B, T, C)) return -1;
  return (long long)psd_plan(B, T, C).chunks * (T / 2 + 1) * C *
         (long long)sizeof(double);
}

extern "C" int cg_trace_psd(const float* x, int B, int T, int C,
                            long long s_b, long long s_t, long long s_c,
                            double* totals, void* ws, void* stream) {
  if (!x || !totals || !ws || !psd_shape_ok(B, T, C) ||
      (reinterpret_cast<uintptr_t>(ws) & 7))
    return CG_EINVAL;
  const PsdPlan plan = psd_plan(B, T, C);
  PsdArgs a;
  a.x = x; a.s_b = s_b; a.s_t = s_t; a.s_c = s_c;
  a.partial = static_cast<double*>(ws);
  a.B = B; a.T = T; a.C = C;
  a.groups = plan.groups; a.chunk_len = plan.chunk_len; a.chunks = plan.chunks;
  a.odd = __builtin_ctz((unsigned)T) & 1;
  a.items = (long long)plan.chunks * plan.groups;
  // up to 106 KiB of dynamic LDS (T = 8192): above the 64 KiB a kernel gets unasked
  if (int e = cg_allow_dynamic_lds<&trace_psd_kernel>((int)psd_lds_bytes(kFftMaxT)))
    return e;
  const unsigned grid =
      (unsigned)(a.items < kPsdMaxGrid ? a.items : kPsdMaxGrid);
  hipLaunchKernelGGL(trace_psd_kernel, dim3(grid), dim3(kPsdThreads),
                     psd_lds_bytes(T), cg_stream(stream), a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long long n = (long long)(T / 2 + 1) * C;
  const long long blocks = (n - 1) / kPsdFinishThreads + 1;
  hipLaunchKernelGGL(trace_psd_finish_kernel,
                     dim3((unsigned)(blocks < kPsdMaxGrid ? blocks : kPsdMaxGrid)),
                     dim3(kPsdFinishThreads), 0, cg_stream(stream),
                     a.partial, plan.chunks, n, totals);
  CG_LAUNCH_CHECK();
}
