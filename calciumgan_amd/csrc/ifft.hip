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

#if defined(__HIPCC__)
#define CG_IFFT_FN __host__ __device__ __forceinline__
#else
#define CG_IFFT_FN static inline
#endif

namespace {

inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kIfftThreads = 512;
constexpr int kIfftMinT = 32, kIfftMaxT = 8192;
constexpr int kIfftMaxGroup = 16;       // neurons per workgroup at most
constexpr int kIfftTraceElems = 8192;   // complex elements of LDS per workgroup
constexpr int kIfftMaxGrid = 1024;      // workgroups; beyond: grid-stride

struct cf32 {
  float re, im;
};

CG_IFFT_FN int ifft_group(int T) {
  const int g = kIfftTraceElems / T;
  return g > kIfftMaxGroup ? kIfftMaxGroup : g;
}

// LDS row of logical row t; rows_mask = 32 / G - 1
CG_IFFT_FN int ifft_phys(int t, int rows_mask) { return t ^ ((t >> 2) & rows_mask); }

// e^{+2 pi i k / T}, k < T, from the first quadrant's table (quarter = T / 4)
CG_IFFT_FN cf32 ifft_twiddle(const cf32* tw, int k, int quarter) {
  const cf32 w = tw[k & (quarter - 1)];
  const int q = k >> __builtin_ctz((unsigned)quarter);
  cf32 r;
  r.re = q == 0 ? w.re : q == 1 ? -w.im : q == 2 ? -w.re : w.im;
  r.im = q == 0 ? w.im : q == 1 ? w.re : q == 2 ? -w.im : -w.re;
  return r;
}

CG_IFFT_FN cf32 cmul(cf32 a, cf32 w) {
  cf32 r;
  r.re = a.re * w.re - a.im * w.im;
  r.im = a.re * w.im + a.im * w.re;
  return r;
}
CG_IFFT_FN cf32 cadd(cf32 a, cf32 b) { return cf32{a.re + b.re, a.im + b.im}; }
CG_IFFT_FN cf32 csub(cf32 a, cf32 b) { return cf32{a.re - b.re, a.im - b.im}; }
// i a
CG_IFFT_FN cf32 cmul_i(cf32 a) { return cf32{-a.im, a.re}; }

// A butterfly in two halves, so that a lane has the LDS reads of several
// butterflies in flight before it finishes the first (a stage's butterflies
// touch disjoint rows).
struct IfftBfly {
  cf32* p[4];
  cf32 a[4];
  int r;
};

// Butterfly j < T / 2 of neuron column g of the radix-2 stage over the whole
// trace: (a0 + a1, (a0 - a1) w_T^j) at rows j, j + T / 2.
CG_IFFT_FN void ifft_radix2_load(IfftBfly& f, cf32* buf, int T, int G,
                                 int rows_mask, int j, int g) {
  f.p[0] = buf + ifft_phys(j, rows_mask) * G + g;
  f.p[1] = buf + ifft_phys(j + T / 2, rows_mask) * G + g;
  f.a[0] = *f.p[0];
  f.a[1] = *f.p[1];
  f.r = j;
}
CG_IFFT_FN void ifft_radix2_finish(const IfftBfly& f, const cf32* tw, int T) {
  *f.p[0] = cadd(f.a[0], f.a[1]);
  *f.p[1] = cmul(csub(f.a[0], f.a[1]), ifft_twiddle(tw, f.r, T / 4));
}
CG_IFFT_FN void ifft_radix2(cf32* buf, const cf32* tw, int T, int G, int rows_mask,
                            int j, int g) {
  IfftBfly f;
  ifft_radix2_load(f, buf, T, G, rows_mask, j, g);
  ifft_radix2_finish(f, tw, T);
}

// Butterfly j < T / 4 of neuron column g of the radix-4 stage on blocks of N
// rows (h = N / 4): block j / h, r = j % h, legs a_k at rows block N + r + k h,
//   b_q = w_N^{q r} sum_k a_k i^{k q}   left at row block N + r + q h.
CG_IFFT_FN void ifft_radix4_load(IfftBfly& f, cf32* buf, int G, int rows_mask,
                                 int N, int j, int g) {
  const int h = N >> 2;
  const int r = j & (h - 1);
  const int base = (j - r) * 4 + r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f.p[k] = buf + ifft_phys(base + k * h, rows_mask) * G + g;
    f.a[k] = *f.p[k];
  }
  f.r = r;
}
CG_IFFT_FN void ifft_radix4_finish(const IfftBfly& f, const cf32* tw, int T, int N) {
  const cf32 s02 = cadd(f.a[0], f.a[2]), d02 = csub(f.a[0], f.a[2]);
  const cf32 s13 = cadd(f.a[1], f.a[3]), d13 = cmul_i(csub(f.a[1], f.a[3]));
  cf32 b0 = cadd(s02, s13), b1 = cadd(d02, d13);
  cf32 b2 = csub(s02, s13), b3 = csub(d02, d13);
  if (N > 4) {  // (N == 4: r = 0, every twiddle is 1)
    const int k = f.r * (T / N);
    b1 = cmul(b1, ifft_twiddle(tw, k, T / 4));
    b2 = cmul(b2, ifft_twiddle(tw, 2 * k, T / 4));
    b3 = cmul(b3, ifft_twiddle(tw, 3 * k, T / 4));
  }
  *f.p[0] = b0;
  *f.p[1] = b1;
  *f.p[2] = b2;
  *f.p[3] = b3;
}
CG_IFFT_FN void ifft_radix4(cf32* buf, const cf32* tw, int T, int G, int rows_mask,
                            int N, int j, int g) {
  IfftBfly f;
  ifft_radix4_load(f, buf, G, rows_mask, N, j, g);
  ifft_radix4_finish(f, tw, T, N);
}

// Time index held by row p after the last stage: with u = q0 + 2 (q1 + 4 (q2 +
// ...)) (q0 only when log2 T is odd), p = q0 T/2 + q1 T/8 + q2 T/32 + ...
CG_IFFT_FN int ifft_time_of_row(int p, int T, int odd) {
  int u = 0, shift = 0, bits = __builtin_ctz((unsigned)T);
  if (odd) {
    bits -= 1;
    u = p >> bits;
    p &= (1 << bits) - 1;
    shift = 1;
  }
  while (bits > 0) {
    bits -= 2;
    u |= (p >> bits) << shift;
    p &= (1 << bits) - 1;
    shift += 2;
  }
  return u;
}

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

// (batches: a lane issues the global loads, or the LDS reads, of kIfft*Batch
// elements before it uses the first -- at 16 waves a CU nothing else hides
// their latency)
constexpr int kIfftLoadBatch = 8;
constexpr int kIfftBflyBatch = 4;

__global__ __launch_bounds__(kIfftThreads) void ifft_channels_kernel(IfftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ifft_lds[];
  const int T = a.T, G = ifft_group(T), rows_mask = 32 / G - 1;
  cf32* buf = reinterpret_cast<cf32*>(ifft_lds);  // [T][G]
  cf32* tw = buf + (size_t)T * G;                 // [T / 4]
  const int tid = threadIdx.x;
  const int gshift = __builtin_ctz(G);
  const int elems = T * G;  // 512 at least, a power of two

  for (int k = tid; k < T / 4; k += kIfftThreads) {
    double s, c;
    sincospi(2.0 * (double)k / (double)T, &s, &c);
    tw[k] = cf32{(float)c, (float)s};
  }

  // Consecutive items are neighbouring neuron groups of one sample: at G = 4
  // eight of them share every 128-byte line of a time row.  Workgroups go to
  // the 8 XCDs (one L2 each) in turn, so the grid is renumbered to give the
  // workgroups that share an L2 a run of consecutive items (speed only: any
  // placement computes the same).
  int first_item = blockIdx.x;
  if ((gridDim.x & 7) == 0)
    first_item = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  for (long long item = first_item; item < a.items; item += gridDim.x) {
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

    int N = T;
    if (a.odd) {
      const int count = elems / 2;
      for (int first = tid; first < count; first += kIfftThreads * kIfftBflyBatch) {
        IfftBfly f[kIfftBflyBatch];
#pragma unroll
        for (int u = 0; u < kIfftBflyBatch; ++u) {
          const int idx = first + u * kIfftThreads;
          if (idx < count)
            ifft_radix2_load(f[u], buf, T, G, rows_mask, idx >> gshift, idx & (G - 1));
        }
#pragma unroll
        for (int u = 0; u < kIfftBflyBatch; ++u)
          if (first + u * kIfftThreads < count) ifft_radix2_finish(f[u], tw, T);
      }
      __syncthreads();
      N = T / 2;
    }
    for (; N >= 4; N >>= 2) {
      const int count = elems / 4;
      for (int first = tid; first < count; first += kIfftThreads * kIfftBflyBatch) {
        IfftBfly f[kIfftBflyBatch];
#pragma unroll
        for (int u = 0; u < kIfftBflyBatch; ++u) {
          const int idx = first + u * kIfftThreads;
          if (idx < count)
            ifft_radix4_load(f[u], buf, G, rows_mask, N, idx >> gshift, idx & (G - 1));
        }
#pragma unroll
        for (int u = 0; u < kIfftBflyBatch; ++u)
          if (first + u * kIfftThreads < count) ifft_radix4_finish(f[u], tw, T, N);
      }
      __syncthreads();
    }

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

inline size_t ifft_lds_bytes(int T) {
  return ((size_t)T * ifft_group(T) + T / 4) * sizeof(cf32);
}

}  // namespace

extern "C" int cg_ifft_channels(const float* x, int B, int T, int C,
                                long long s_b, long long s_t, long long s_c,
                                float scale, float offset, float* y,
                                long long y_sb, long long y_st, long long y_sc,
                                void* stream) {
  if (!x || !y || B < 1 || C < 1 || T < kIfftMinT || T > kIfftMaxT ||
      (T & (T - 1)))
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
  static CgPerDeviceFlag attr_set;
  if (!attr_set.test()) {
    hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&ifft_channels_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)ifft_lds_bytes(kIfftMaxT));
    if (e != hipSuccess) return (int)e;
    attr_set.mark();
  }
  const unsigned grid =
      (unsigned)(a.items < kIfftMaxGrid ? a.items : kIfftMaxGrid);
  hipLaunchKernelGGL(ifft_channels_kernel, dim3(grid), dim3(kIfftThreads),
                     ifft_lds_bytes(T), S_(stream), a);
  CG_LAUNCH_CHECK();
}
