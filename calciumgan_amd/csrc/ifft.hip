// Inverse FFT of generated spectra on the device (FFT datasets: the reference's
// generate_tfrecords.py --fft stores each neuron's trace as its spectrum along
// time, channels [real | imag]; utils.reverse_preprocessing inverts it per
// (sample, neuron) and keeps the real part -- gan/utils/utils.py:35-63):
//   cg_ifft_channels  y[b][t][c] = Re((1/T) sum_k (xr_k + i xi_k) e^{+2 pi i k t/T})
//                     xr_k = x[b][k][c] scale + offset, xi_k = x[b][k][C+c] ...
// The numpy statement is utils.ifft_channels.
//
// One workgroup (512 threads) owns one sample and G consecutive neurons, G =
// min(16, 8192 / T):
// at most 64 KiB of complex traces in LDS (T = 2048: G = 4) plus a quarter-circle
// twiddle table of 2 T bytes, so two workgroups share a CU up to T = 8192.
//   load    time row t -> LDS row t: consecutive lanes read G consecutive reals,
//           then G consecutive imaginaries, of one global row
//   stages  decimation in frequency, in place: one radix-2 stage first when
//           log2 T is odd, then radix-4 stages with leg distance h = N / 4 =
//           ... 16, 4, 1; a lane owns one butterfly of one neuron, the neuron
//           index running fastest over the lanes
//   store   LDS row p holds time u = the mixed-radix digit reversal of p; the
//           rows are walked in LDS order and written to global row u (a global
//           row is G floats whichever order the rows go in), times 1/T (exact)
// LDS image: element (t, g) is the float2 at row phys(t) = t ^ ((t >> 2) & (M -
// 1)), column g, M = 32 / G rows making up the 64 banks one ds_read_b64 lane
// group (32 lanes) sweeps.  The G lanes of one butterfly leg share a row; the M
// butterflies of a lane group have consecutive j, so their rows differ in bits
// 0 .. 2s-1 and 2s+2 .. of t (h = 4^s): without the XOR the late stages (h < M)
// put them on M / 4 .. 1 distinct bank positions.  With it the low bits of
// phys, t_i ^ t_{i+2}, are a bijection of the varying bits in every stage, the
// radix-2 one and the row-order walks of load and store included.
// Twiddles: e^{2 pi i k / T}, k < T / 4, by sincospi in float64 rounded once to
// float32 (0.5 ulp); the other three quadrants are sign / component swaps.
#include "cg_common.h"

#include "fft_stages.h"

namespace {

constexpr int kIfftMaxGrid = 1024;      // workgroups; beyond: grid-stride

// x scale + offset, the product and the sum rounded to float32 one after the
// other (utils.denormalize of a float32 array; deconvolve_signals_device's
// convention)
CG_IFFT_FN float ifft_denorm(float v, float scale, float offset) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float a = v * scale;
  a = a + offset;
  return a;
}

struct IfftArgs {
  const float* x;
  long long s_b, s_t, s_c;
  float* y;
  long long y_sb, y_st, y_sc;
  int B, T, C, groups, odd;
  long long items;  // B * groups
  float scale, offset, inv_T;
};

// (a lane issues the global loads, or the LDS reads, of kIfftLoadBatch elements
// before it uses the first, as with the butterflies of kIfftBflyBatch)
constexpr int kIfftLoadBatch = 8;

__global__ __launch_bounds__(kIfftThreads) void ifft_channels_kernel(IfftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ifft_lds[];
  const int T = a.T, G = ifft_group(T), rows_mask = 32 / G - 1;
  cf32* buf = reinterpret_cast<cf32*>(ifft_lds);  // [T][G]
  cf32* tw = buf + (size_t)T * G;                 // [T / 4]
  const int tid = threadIdx.x;
  const int gshift = __builtin_ctz(G);
  const int elems = T * G;  // 512 at least, a power of two

  fft_fill_twiddles<kIfftThreads>(tw, T, tid);

  // (consecutive items are neighbouring neuron groups of one sample: at G = 4
  // eight of them share every 128-byte line of a time row)
  for (long long item = cg_xcd_first_item(); item < a.items; item += gridDim.x) {
    const int b = (int)(item / a.groups);
    const int c0 = (int)(item - (long long)b * a.groups) * G;
    const float* xb = a.x + (long long)b * a.s_b;
    float* yb = a.y + (long long)b * a.y_sb;

    for (int first = tid; first < elems; first += kIfftThreads * kIfftLoadBatch) {
      float re[kIfftLoadBatch], im[kIfftLoadBatch];
#pragma unroll
      for (int u = 0; u < kIfftLoadBatch; ++u) {
        const int idx = first + u * kIfftThreads;
        if (idx < elems) {  // (the same in every lane)
          const int g = idx & (G - 1), t = idx >> gshift;
          // a neuron past the last reads the last one's (valid) address
          const int c = c0 + g < a.C ? c0 + g : a.C - 1;
          const float* p = xb + (long long)t * a.s_t;
          re[u] = p[(long long)c * a.s_c];
          im[u] = p[((long long)a.C + c) * a.s_c];
        }
      }
#pragma unroll
      for (int u = 0; u < kIfftLoadBatch; ++u) {
        const int idx = first + u * kIfftThreads;
        if (idx < elems) {
          const int g = idx & (G - 1), t = idx >> gshift;
          cf32 v{0.f, 0.f};
          if (c0 + g < a.C) {
            v.re = ifft_denorm(re[u], a.scale, a.offset);
            v.im = ifft_denorm(im[u], a.scale, a.offset);
          }
          buf[ifft_phys(t, rows_mask) * G + g] = v;
        }
      }
    }
    __syncthreads();

    fft_run_stages<kIfftThreads, kIfftBflyBatch>(buf, tw, T, G, rows_mask, a.odd,
                                                 tid);

    for (int first = tid; first < elems; first += kIfftThreads * kIfftLoadBatch) {
      float v[kIfftLoadBatch];
#pragma unroll
      for (int u = 0; u < kIfftLoadBatch; ++u) {
        const int idx = first + u * kIfftThreads;
        if (idx < elems)
          v[u] = buf[ifft_phys(idx >> gshift, rows_mask) * G + (idx & (G - 1))].re;
      }
#pragma unroll
      for (int u = 0; u < kIfftLoadBatch; ++u) {
        const int idx = first + u * kIfftThreads;
        const int c = c0 + (idx & (G - 1));
        if (idx < elems && c < a.C) {
          const int t = ifft_time_of_row(idx >> gshift, T, a.odd);
          yb[(long long)t * a.y_st + (long long)c * a.y_sc] = v[u] * a.inv_T;
        }
      }
    }
    __syncthreads();  // the next item's load overwrites buf
  }
}

}  // namespace

extern "C" int cg_ifft_channels(const float* x, int B, int T, int C,
                                long long s_b, long long s_t, long long s_c,
                                float scale, float offset, float* y,
                                long long y_sb, long long y_st, long long y_sc,
                                void* stream) {
  if (!x || !y || B < 1 || C < 1 || !fft_length_ok(T))
    return CG_EINVAL;
  const int G = ifft_group(T);
  IfftArgs a;
  a.x = x; a.s_b = s_b; a.s_t = s_t; a.s_c = s_c;
  a.y = y; a.y_sb = y_sb; a.y_st = y_st; a.y_sc = y_sc;
  a.B = B; a.T = T; a.C = C;
  a.groups = (C - 1) / G + 1;
  a.odd = __builtin_ctz((unsigned)T) & 1;
  a.items = (long long)B * a.groups;
  a.scale = scale; a.offset = offset;
  a.inv_T = 1.0f / (float)T;  // a power of two: exact
  // up to 80 KiB of dynamic LDS (T = 8192): above the 64 KiB a kernel gets unasked
  if (int e = cg_allow_dynamic_lds<&ifft_channels_kernel>(
          (int)fft_lds_bytes(kFftMaxT)))
    return e;
  const unsigned grid =
      (unsigned)(a.items < kIfftMaxGrid ? a.items : kIfftMaxGrid);
  hipLaunchKernelGGL(ifft_channels_kernel, dim3(grid), dim3(kIfftThreads),
                     fft_lds_bytes(T), cg_stream(stream), a);
  CG_LAUNCH_CHECK();
}
