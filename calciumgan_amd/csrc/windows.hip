// Recording datasets: cut one batch of windows out of the resident (T_raw, C)
// recording, straight into the batch buffer train() reads (the reference's
// generate_tfrecords.py materialises every stride-2 window instead: each row of
// the recording about L / 2 times on disk, in host RAM and in HBM):
//   cg_window_batch  fft == 0: y[b][t][c] = (raw[row(b, t)][c] - sub) / div
//                    fft != 0: y[b][k][c], y[b][k][C + c] = (Re, Im of
//                      sum_t raw[row(b, t)][c] e^{-2 pi i k t / L}, each - sub) / div
//   row(b, t) = clamp(starts[b] + t, 0, T_raw - 1)
// The numpy statement is dataset_helper.window_batch.
//
// Plain: one item is 1024 consecutive elements of one window's (L, C) block,
// 4 per lane of a 256-thread workgroup, at most 2048 workgroups (8 per CU: 8
// waves a SIMD), grid-stride beyond.  The recording is a few MB and is read
// about L / stride times an epoch, so it sits in L2 / Infinity Cache: the
// stores are the traffic.  A lane's 4 elements move as one 16-byte load and
// store where they are contiguous and 16-byte aligned on both sides:
//   rows   unit channel strides, C % 4 == 0, every pitch a multiple of 4: a
//          chunk lies in one row, whichever row the clamp picks
//   flat   unit channel strides, row pitch C on both sides (C = 102: rows of
//          408 bytes), the window inside the recording and starts[b] * C % 4
//          == 0 (every even start): the window is one span of L * C floats
// and one by one otherwise (a stored (C, T) recording viewed transposed, a
// window past an end, an odd start with C % 4 != 0).  The choice is the same
// in every lane of a workgroup.
//
// FFT: shaped as ifft.hip -- one 512-thread workgroup per (window, G
// neurons), G = min(16, 8192 / L), at most 1024 workgroups, the stages of
// fft_stages.h on the swizzled LDS image.  The real window is loaded as the
// real part with a zero imaginary part; the stages run with e^{+2 pi i k / L}
// and the result is conjugated on the way out (the DFT of a real trace is the
// conjugate of its unscaled inverse transform).  LDS row p holds bin u = the
// digit reversal of p: both blocks are stored in LDS row order to global row u.
// An all-zero trace stays exactly zero through every butterfly.
#include "cg_common.h"

#include "fft_stages.h"

namespace {

constexpr int kWinThreads = 256;       // plain
constexpr int kWinItemElems = 4 * kWinThreads;
constexpr int kWinMaxGrid = 2048;      // workgroups; beyond: grid-stride
constexpr int kWinFftMaxGrid = 1024;   // workgroups; beyond: grid-stride

// (v - sub) / div: the float32 difference, then the IEEE float32 quotient
__device__ __forceinline__ float win_affine(float v, float sub, float div) {
#pragma clang fp contract(off)
  float a = v - sub;
  a = a / div;
  return a;
}

__device__ __forceinline__ long long win_row(long long start, int t, long long T_raw) {
  const long long r = start + t;
  return r < 0 ? 0 : r >= T_raw ? T_raw - 1 : r;
}

struct WinArgs {
  const float* raw;
  long long T_raw, r_st, r_sc;
  const int* starts;
  float* y;
  long long y_sb, y_st, y_sc;
  int B, L, C;
  float sub, div;
  // plain
  long long win_elems;      // L * C
  long long items_per_win;  // ceil(win_elems / kWinItemElems)
  int rows_ok, flat_ok;     // the 16-byte paths the layout admits
  // fft
  int groups, odd;
  long long items;          // plain: B * items_per_win; fft: B * groups
};

__global__ __launch_bounds__(kWinThreads) void window_gather_kernel(WinArgs a) {
  const int tid = threadIdx.x;
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int b = (int)(item / a.items_per_win);
    const long long part = item - (long long)b * a.items_per_win;
    const long long i0 = part * kWinItemElems + 4 * tid;  // within the window
    if (i0 >= a.win_elems) continue;
    const long long start = a.starts[b];
    float* yb = a.y + (long long)b * a.y_sb;
    if (a.rows_ok) {  // (C % 4 == 0: i0 .. i0 + 3 are channels c .. c + 3 of row t)
      const int t = (int)(i0 / a.C), c = (int)(i0 - (long long)t * a.C);
      const float4 v = *reinterpret_cast<const float4*>(
          a.raw + win_row(start, t, a.T_raw) * a.r_st + c);
      float4 o;
      o.x = win_affine(v.x, a.sub, a.div);
      o.y = win_affine(v.y, a.sub, a.div);
      o.z = win_affine(v.z, a.sub, a.div);
      o.w = win_affine(v.w, a.sub, a.div);
      *reinterpret_cast<float4*>(yb + (long long)t * a.y_st + c) = o;
      continue;
    }
    const bool flat = a.flat_ok && start >= 0 && start + a.L <= a.T_raw &&
                      ((start * a.C) & 3) == 0;
    if (flat && i0 + 4 <= a.win_elems) {
      const float4 v =
          *reinterpret_cast<const float4*>(a.raw + start * a.C + i0);
      float4 o;
      o.x = win_affine(v.x, a.sub, a.div);
      o.y = win_affine(v.y, a.sub, a.div);
      o.z = win_affine(v.z, a.sub, a.div);
      o.w = win_affine(v.w, a.sub, a.div);
      *reinterpret_cast<float4*>(yb + i0) = o;
      continue;
    }
    int t = (int)(i0 / a.C), c = (int)(i0 - (long long)t * a.C);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u < a.win_elems) {
        const float v =
            a.raw[win_row(start, t, a.T_raw) * a.r_st + (long long)c * a.r_sc];
        yb[(long long)t * a.y_st + (long long)c * a.y_sc] =
            win_affine(v, a.sub, a.div);
      }
      if (++c == a.C) {
        c = 0;
        ++t;
      }
    }
  }
}

// (as in ifft.hip, a lane issues the global loads, or the LDS reads, of a batch
// before it uses the first)
constexpr int kWinLoadBatch = 8;

__global__ __launch_bounds__(kWinFftThreads) void window_fft_kernel(WinArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char win_lds[];
  const int T = a.L, G = ifft_group(T), rows_mask = 32 / G - 1;
  cf32* buf = reinterpret_cast<cf32*>(win_lds);  // [T][G]
  cf32* tw = buf + (size_t)T * G;                // [T / 4]
  const int tid = threadIdx.x;
  const int gshift = __builtin_ctz(G);
  const int elems = T * G;  // 512 at least, a power of two

  fft_fill_twiddles<kWinFftThreads>(tw, T, tid);

  // (consecutive items are neighbouring neuron groups of one window)
  for (long long item = cg_xcd_first_item(); item < a.items; item += gridDim.x) {
    const int b = (int)(item / a.groups);
    const int c0 = (int)(item - (long long)b * a.groups) * G;
    const long long start = a.starts[b];
    float* yb = a.y + (long long)b * a.y_sb;

    for (int first = tid; first < elems; first += kWinFftThreads * kWinLoadBatch) {
      float re[kWinLoadBatch];
#pragma unroll
      for (int u = 0; u < kWinLoadBatch; ++u) {
        const int idx = first + u * kWinFftThreads;
        if (idx < elems) {  // (the same in every lane)
          const int g = idx & (G - 1), t = idx >> gshift;
          // a neuron past the last reads the last one's (valid) address
          const int c = c0 + g < a.C ? c0 + g : a.C - 1;
          re[u] = a.raw[win_row(start, t, a.T_raw) * a.r_st + (long long)c * a.r_sc];
        }
      }
#pragma unroll
      for (int u = 0; u < kWinLoadBatch; ++u) {
        const int idx = first + u * kWinFftThreads;
        if (idx < elems) {
          const int g = idx & (G - 1), t = idx >> gshift;
          buf[ifft_phys(t, rows_mask) * G + g] =
              cf32{c0 + g < a.C ? re[u] : 0.f, 0.f};
        }
      }
    }
    __syncthreads();

    fft_run_stages<kWinFftThreads, kWinBflyBatch>(buf, tw, T, G, rows_mask, a.odd,
                                                  tid);

    for (int first = tid; first < elems; first += kWinFftThreads * kWinLoadBatch) {
      cf32 v[kWinLoadBatch];
#pragma unroll
      for (int u = 0; u < kWinLoadBatch; ++u) {
        const int idx = first + u * kWinFftThreads;
        if (idx < elems)
          v[u] = buf[ifft_phys(idx >> gshift, rows_mask) * G + (idx & (G - 1))];
      }
#pragma unroll
      for (int u = 0; u < kWinLoadBatch; ++u) {
        const int idx = first + u * kWinFftThreads;
        const int c = c0 + (idx & (G - 1));
        if (idx < elems && c < a.C) {
          const int k = ifft_time_of_row(idx >> gshift, T, a.odd);
          float* p = yb + (long long)k * a.y_st;
          p[(long long)c * a.y_sc] = win_affine(v[u].re, a.sub, a.div);
          p[((long long)a.C + c) * a.y_sc] = win_affine(-v[u].im, a.sub, a.div);
        }
      }
    }
    __syncthreads();  // the next item's load overwrites buf
  }
}

inline bool win_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace

extern "C" int cg_window_batch(const float* raw, long long T_raw, int C,
                               long long r_st, long long r_sc,
                               const int* starts, int B, int L,
                               int fft, float sub, float div,
                               float* y, long long y_sb, long long y_st,
                               long long y_sc, void* stream) {
  if (!raw || !starts || !y || T_raw < 1 || C < 1 || B < 1 || L < 1 ||
      div == 0.0f)
    return CG_EINVAL;
  if (fft && !fft_length_ok(L)) return CG_EINVAL;
  WinArgs a;
  a.raw = raw; a.T_raw = T_raw; a.r_st = r_st; a.r_sc = r_sc;
  a.starts = starts;
  a.y = y; a.y_sb = y_sb; a.y_st = y_st; a.y_sc = y_sc;
  a.B = B; a.L = L; a.C = C;
  a.sub = sub; a.div = div;
  a.win_elems = (long long)L * C;
  a.items_per_win = (a.win_elems - 1) / kWinItemElems + 1;
  a.rows_ok = a.flat_ok = 0;
  a.groups = a.odd = 0;
  if (!fft) {
    const bool unit = r_sc == 1 && y_sc == 1 && win_aligned16(raw) &&
                      win_aligned16(y) && (y_sb & 3) == 0;
    a.rows_ok = unit && (C & 3) == 0 && (r_st & 3) == 0 && (y_st & 3) == 0;
    a.flat_ok = unit && r_st == C && y_st == C;
    a.items = (long long)B * a.items_per_win;
    const unsigned grid =
        (unsigned)(a.items < kWinMaxGrid ? a.items : kWinMaxGrid);
    hipLaunchKernelGGL(window_gather_kernel, dim3(grid), dim3(kWinThreads), 0,
                       cg_stream(stream), a);
    CG_LAUNCH_CHECK();
  }
  const int G = ifft_group(L);
  a.groups = (C - 1) / G + 1;
  a.odd = __builtin_ctz((unsigned)L) & 1;
  a.items = (long long)B * a.groups;
  // up to 80 KiB of dynamic LDS (L = 8192): above the 64 KiB a kernel gets unasked
  if (int e = cg_allow_dynamic_lds<&window_fft_kernel>(
          (int)fft_lds_bytes(kFftMaxT)))
    return e;
  const unsigned grid =
      (unsigned)(a.items < kWinFftMaxGrid ? a.items : kWinFftMaxGrid);
  hipLaunchKernelGGL(window_fft_kernel, dim3(grid), dim3(kWinFftThreads),
                     fft_lds_bytes(L), cg_stream(stream), a);
  CG_LAUNCH_CHECK();
}
