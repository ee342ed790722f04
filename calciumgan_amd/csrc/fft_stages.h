// What the three FFT kernels share -- the inverse transform of generated spectra
// (ifft.hip), the forward transform of recording windows (windows.hip) and the
// trace power spectra (trace_psd.hip): radix-4 decimation in frequency in LDS
// with one radix-2 stage when log2 T is odd, on the swizzled [T][G] image and
// with the quarter-circle twiddle table described at the top of ifft.hip.  The
// twiddles are e^{+2 pi i k / T}: the forward transform of a real trace runs the
// same stages and conjugates the result.  The butterflies, the index functions,
// the order of the stages (fft_for_each_stage) and a lane's walk through one
// stage (fft_stage) are stated here once; tests/fft_stages_host.cc runs them on
// the host as the kernels do.  (trace_psd.hip keeps the walk written out, and
// says why.)
#ifndef CG_FFT_STAGES_H_
#define CG_FFT_STAGES_H_

#include <stddef.h>

#if defined(__HIPCC__)
#define CG_IFFT_FN __host__ __device__ __forceinline__
#else
#define CG_IFFT_FN static inline
#endif

namespace {

constexpr int kIfftMaxGroup = 16;       // neurons per workgroup at most
constexpr int kIfftTraceElems = 8192;   // complex elements of LDS per workgroup
constexpr int kFftMinT = 32, kFftMaxT = 8192;
// Lanes of a workgroup, and the butterflies whose LDS reads a lane has in flight
// before it finishes the first (at 16 waves a CU nothing else hides their
// latency), of ifft.hip, windows.hip and trace_psd.hip
constexpr int kIfftThreads = 512, kIfftBflyBatch = 4;
constexpr int kWinFftThreads = 512, kWinBflyBatch = 4;
constexpr int kPsdThreads = 512, kPsdBflyBatch = 2;

struct cf32 {
  float re, im;
};

// the lengths the kernels take: a power of two in kFftMinT .. kFftMaxT
CG_IFFT_FN bool fft_length_ok(int T) {
  return T >= kFftMinT && T <= kFftMaxT && !(T & (T - 1));
}

CG_IFFT_FN int ifft_group(int T) {
  const int g = kIfftTraceElems / T;
  return g > kIfftMaxGroup ? kIfftMaxGroup : g;
}

// bytes of the [T][G] image and the T / 4 twiddles behind it
CG_IFFT_FN size_t fft_lds_bytes(int T) {
  return ((size_t)T * ifft_group(T) + T / 4) * sizeof(cf32);
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

// The stages in their order: f(0) for the radix-2 stage over the whole trace
// when log2 T is odd, then f(N) for the radix-4 stages on blocks of N = T or
// T / 2, ..., 16, 4 rows.
template <class F>
CG_IFFT_FN void fft_for_each_stage(int T, int odd, F&& f) {
  int N = T;
  if (odd) {
    f(0);
    N = T / 2;
  }
  for (; N >= 4; N >>= 2) f(N);
}

// One stage as lane `lane` of THREADS runs it: butterfly idx = j G + g is that
// of ifft_radix2_load / ifft_radix4_load (the neuron index running fastest over
// the lanes); the lane takes lane + u THREADS, u < BATCH, issues their loads
// together, finishes them, and strides on by THREADS BATCH.
template <int THREADS, int BATCH>
CG_IFFT_FN void fft_stage(cf32* buf, const cf32* tw, int T, int G, int rows_mask,
                          int stage, int lane) {
  const int gshift = __builtin_ctz((unsigned)G);
  const int count = T * G / (stage ? 4 : 2);
  for (int first = lane; first < count; first += THREADS * BATCH) {
    IfftBfly f[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const int idx = first + u * THREADS;
      if (idx < count) {  // (the same in every lane)
        if (stage)
          ifft_radix4_load(f[u], buf, G, rows_mask, stage, idx >> gshift, idx & (G - 1));
        else
          ifft_radix2_load(f[u], buf, T, G, rows_mask, idx >> gshift, idx & (G - 1));
      }
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u)
      if (first + u * THREADS < count) {
        if (stage)
          ifft_radix4_finish(f[u], tw, T, stage);
        else
          ifft_radix2_finish(f[u], tw, T);
      }
  }
}

// between two stages every lane of the workgroup meets (the host runs the
// lanes of a stage one after the other)
CG_IFFT_FN void fft_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

// Every stage in order, each followed by the barrier, for one lane.
template <int THREADS, int BATCH>
CG_IFFT_FN void fft_run_stages(cf32* buf, const cf32* tw, int T, int G,
                               int rows_mask, int odd, int lane) {
  fft_for_each_stage(T, odd, [&](int stage) {
    fft_stage<THREADS, BATCH>(buf, tw, T, G, rows_mask, stage, lane);
    fft_barrier();
  });
}

#if defined(__HIPCC__)
// tw[k] = e^{2 pi i k / T}, k < T / 4: sincospi in float64 rounded once to
// float32 (the caller's barrier comes before the first stage)
template <int THREADS>
__device__ __forceinline__ void fft_fill_twiddles(cf32* tw, int T, int lane) {
  for (int k = lane; k < T / 4; k += THREADS) {
    double s, c;
    sincospi(2.0 * (double)k / (double)T, &s, &c);
    tw[k] = cf32{(float)c, (float)s};
  }
}
#endif

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

// The row that holds time (or bin) u after the last stage: the inverse of
// ifft_time_of_row.
CG_IFFT_FN int ifft_row_of_time(int u, int T, int odd) {
  int p = 0, bits = __builtin_ctz((unsigned)T);
  if (odd) {
    bits -= 1;
    p = (u & 1) << bits;
    u >>= 1;
  }
  while (bits > 0) {
    bits -= 2;
    p |= (u & 3) << bits;
    u >>= 2;
  }
  return p;
}

// the j-th row whose bin is below T / 2 (trace_psd.hip): bit 1 of the row is
// the top bit of its bin (the last radix-4 digit)
CG_IFFT_FN int psd_low_row(int j) { return ((j >> 1) << 2) | (j & 1); }

}  // namespace

#endif  // CG_FFT_STAGES_H_
