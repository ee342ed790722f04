// float32 Dense kernels of the MLP model (gan/models/mlp.py:15-77 of the
// reference) with counter-based dropout, and the float32 forms of the WGAN-GP
// step's small kernels.  Everything here is float32 and independent of the
// build's activation type.
//
// Every layer of the model is a Dense over rows: h = drop(act(x W + b)) with
// W row-major (in, out) -- the Keras kernel layout -- and act(z) = max(z, a z).
// One tiled kernel serves the forward modes and the input gradient: a workgroup
// of 256 threads owns a block of 32 rows and walks the output columns in tiles
// of 64; per tile it adds K in panels of 32, the panels of x and of W staged in
// LDS, every thread holding 2 x 4 accumulators.  The sum over K of one output
// is a single chain of fmaf in index order: the same bits on every launch.
//
// Dropout: the keep decision of element e of a layer's (rows x out) output is
// word e & 3 of the Philox4x32-10 block with counter (e >> 2, stream id) and
// key (seed): a pure function of its arguments, so no mask is stored.  The
// backward kernels read the decision back from the stored h: h > 0 is a kept
// element of slope 1, h < 0 one of slope alpha, and a stored zero of EITHER sign
// counts as dropped (mask_of gives 0).  A KEPT element is stored as zero in three
// cases: every z < 0 under alpha = 0 (as -0.0; its factor s alpha is 0 anyway),
// z exactly 0, and alpha z underflowing to -0.0; in the last two the backward
// gives 0 where the derivative is s alpha (tests/test_hip_mlp_parity.py pins
// the rule at +0.0 and -0.0).
#include "cg_common.h"

namespace {

constexpr int kBM = 32;   // rows of a workgroup's block
constexpr int kBN = 64;   // output columns per tile
constexpr int kBK = 32;   // K panel
constexpr int kThreads = 256;

// -- Philox4x32-10 (Salmon et al., SC'11; Random123) --------------------------
struct Philox4 { uint32_t w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1,
                                                 uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

struct DropArgs {
  uint32_t seed_lo, seed_hi, stream_lo, stream_hi;
  uint32_t threshold;  // keep iff word >= threshold; 0: no dropout
  float scale;         // float32(1 / (1 - p))
};

__device__ __forceinline__ bool drop_keep(const DropArgs& d, uint64_t e) {
  const uint64_t blk = e >> 2;
  const Philox4 r = philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32),
                                  d.stream_lo, d.stream_hi, d.seed_lo, d.seed_hi);
  return r.w[e & 3] >= d.threshold;
}

// s * keep * act'(z) read back from the stored h = drop(act(z))
__device__ __forceinline__ float mask_of(float h, float alpha, float scale) {
  return h > 0.f ? scale : (h < 0.f ? scale * alpha : 0.f);
}

inline DropArgs make_drop(double p, long long seed, long long stream_id) {
  DropArgs d;
  d.seed_lo = (uint32_t)(uint64_t)seed;
  d.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  d.stream_lo = (uint32_t)(uint64_t)stream_id;
  d.stream_hi = (uint32_t)((uint64_t)stream_id >> 32);
  d.threshold = (uint32_t)(p * 4294967296.0);  // floor(p 2^32), 0 <= p < 1
  d.scale = (float)(1.0 / (1.0 - p));
  return d;
}

__global__ void mlp_mask_kernel(uint8_t* keep, long long n, DropArgs d) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) keep[e] = drop_keep(d, (uint64_t)e) ? 1 : 0;
}

// -- the tiled Dense -----------------------------------------------------------
// out[r][j] = epilogue(sum_k a[r][k] * B[k][j]) for r < rows, j < N, k < K.
//   forward  (TRANS = false): a = x (row pitch a_pitch), B = W [K][N]
//   dgrad    (TRANS = true):  a = prologue(dh, h) [rows][K] dense, B[k][j] =
//                             W[j][k], W [N][K]; the masked a is also written
//                             to dz (by the pass over the first column tile)
struct DenseArgs {
  const float* a;
  long long a_pitch;
  const float* a_aux;   // dgrad: the stored h (MASK) / y (SIGMOID)
  float* dz;            // dgrad: masked a
  const float* W;
  const float* bias;    // forward ACT / SIGMOID, or null
  const float* h_mask;  // forward TANGENT: the stored h
  float* out;           // [rows][N] dense, or null (dgrad: dz only)
  long long rows;
  int K, N;
  int mode;
  float alpha;
  DropArgs drop;
};

template <bool TRANS>
__global__ __launch_bounds__(kThreads) void mlp_dense_kernel(DenseArgs p) {
  __shared__ float As[kBM][kBK + 1];
  __shared__ float Bs[kBK][kBN + 4];
  const int t = threadIdx.x;
  const int tx = t & 15, ty = t >> 4;
  const long long r0 = (long long)blockIdx.x * kBM;
  const int ntile = p.out ? (p.N + kBN - 1) / kBN : 1;
  for (int ct = 0; ct < ntile; ++ct) {
    const int j0 = ct * kBN;
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < p.K; k0 += kBK) {
      // panel of a: 32 x 32, four elements per thread, k fastest
#pragma unroll
      for (int i = 0; i < (kBM * kBK) / kThreads; ++i) {
        const int idx = t + i * kThreads;
        const int rr = idx / kBK, kk = idx % kBK;
        const long long r = r0 + rr;
        const int k = k0 + kk;
        float v = 0.f;
        if (r < p.rows && k < p.K) {
          v = p.a[r * p.a_pitch + k];
          if (TRANS) {
            if (p.mode == CG_MLP_BWD_MASK) {
              v *= mask_of(p.a_aux[r * (long long)p.K + k], p.alpha, p.drop.scale);
            } else if (p.mode == CG_MLP_BWD_SIGMOID) {
              const float y = p.a_aux[r * (long long)p.K + k];
              v *= y * (1.f - y);
            }
            if (ct == 0) p.dz[r * (long long)p.K + k] = v;
          }
        }
        As[rr][kk] = v;
      }
      if (p.out) {
        // panel of B: 32 x 64, eight elements per thread
#pragma unroll
        for (int i = 0; i < (kBK * kBN) / kThreads; ++i) {
          const int idx = t + i * kThreads;
          int kk, jj;
          if (TRANS) { kk = idx % kBK; jj = idx / kBK; }
          else       { jj = idx % kBN; kk = idx / kBN; }
          const int k = k0 + kk, j = j0 + jj;
          float v = 0.f;
          if (k < p.K && j < p.N)
            v = TRANS ? p.W[(long long)j * p.K + k] : p.W[(long long)k * p.N + j];
          Bs[kk][jj] = v;
        }
      }
      __syncthreads();
      if (p.out) {
#pragma unroll 8
        for (int kk = 0; kk < kBK; ++kk) {
          const float a0 = As[ty * 2][kk], a1 = As[ty * 2 + 1][kk];
          const float b0 = Bs[kk][tx * 4], b1 = Bs[kk][tx * 4 + 1],
                      b2 = Bs[kk][tx * 4 + 2], b3 = Bs[kk][tx * 4 + 3];
          acc[0][0] = fmaf(a0, b0, acc[0][0]);
          acc[0][1] = fmaf(a0, b1, acc[0][1]);
          acc[0][2] = fmaf(a0, b2, acc[0][2]);
          acc[0][3] = fmaf(a0, b3, acc[0][3]);
          acc[1][0] = fmaf(a1, b0, acc[1][0]);
          acc[1][1] = fmaf(a1, b1, acc[1][1]);
          acc[1][2] = fmaf(a1, b2, acc[1][2]);
          acc[1][3] = fmaf(a1, b3, acc[1][3]);
        }
      }
      __syncthreads();
    }
    if (!p.out) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long r = r0 + ty * 2 + i;
      if (r >= p.rows) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx * 4 + c;
        if (j >= p.N) continue;
        const long long e = r * (long long)p.N + j;
        float v = acc[i][c];
        if (!TRANS) {
          if (p.mode == CG_MLP_FWD_TANGENT) {
            v *= mask_of(p.h_mask[e], p.alpha, p.drop.scale);
          } else {
            if (p.bias) v += p.bias[j];
            if (p.mode == CG_MLP_FWD_SIGMOID) {
              v = 1.f / (1.f + expf(-v));
            } else {
              v = fmaxf(v, p.alpha * v);
              if (p.drop.threshold)
                v = drop_keep(p.drop, (uint64_t)e) ? v * p.drop.scale : 0.f;
            }
          }
        }
        p.out[e] = v;
      }
    }
  }
}

// -- weight and bias gradient: ordered two-stage sums --------------------------
// stage 1: block (tile, chunk) adds x^T dz over the rows of its chunk for a
// 64 x 64 tile of dW (and, in the tiles of the first tile row, the column sums
// of dz) and STORES them in the chunk's slice of ws; a chunk lies inside ONE
// segment.  Stage 2 adds each segment's slices in chunk order and then the
// segments' sums times their coefficients, every product and sum rounded on
// its own: terms that cancel in exact arithmetic -- the head's bias gradient is
// -(1/B) B + (1/B) B -- cancel to exactly 0 here as well (Adam would turn a
// residue of 1e-8 into a full step).  No atomics: the same bits on every call.
constexpr int kWT = 64;   // tile edge of dW
constexpr int kWR = 16;   // rows staged per pass

struct WgradArgs {
  const float* x;
  long long x_pitch;
  const float* x_tail;  // rows >= tail_row0 read x_tail[(r - tail_row0)][Cin]
  long long tail_row0;
  const float* dz;
  long long rows, seg_rows, bias_rows, chunk_rows;
  int Cin, Cout, tiles_j, cps;  // cps: chunks per segment
  float* ws;
};

__global__ __launch_bounds__(kThreads) void mlp_wgrad_kernel(WgradArgs p) {
  __shared__ float Xs[kWR][kWT];
  __shared__ float Ds[kWR][kWT];
  __shared__ float Db[kWR][kWT];  // dz of the rows that carry a bias gradient
  const int t = threadIdx.x;
  const int tx = t & 15, ty = t >> 4;
  const int i0 = (blockIdx.x / p.tiles_j) * kWT;
  const int j0 = (blockIdx.x % p.tiles_j) * kWT;
  const int seg = blockIdx.y / p.cps;
  const long long seg_end = seg == 2 ? p.rows : (seg + 1) * p.seg_rows;
  const long long rb = seg * p.seg_rows + (long long)(blockIdx.y % p.cps) * p.chunk_rows;
  long long re = rb + p.chunk_rows;
  if (re > seg_end) re = seg_end;
  if (re > p.rows) re = p.rows;
  const bool want_bias = i0 == 0;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  float bsum = 0.f;
  for (long long rr0 = rb; rr0 < re; rr0 += kWR) {
#pragma unroll
    for (int i = 0; i < (kWR * kWT) / kThreads; ++i) {
      const int idx = t + i * kThreads;
      const int rr = idx / kWT, cc = idx % kWT;
      const long long r = rr0 + rr;
      float xv = 0.f, dv = 0.f, bv = 0.f;
      if (r < re) {
        if (i0 + cc < p.Cin) {
          xv = (p.x_tail && r >= p.tail_row0)
                   ? p.x_tail[(r - p.tail_row0) * (long long)p.Cin + i0 + cc]
                   : p.x[r * p.x_pitch + i0 + cc];
        }
        if (j0 + cc < p.Cout) {
          dv = p.dz[r * (long long)p.Cout + j0 + cc];
          if (r < p.bias_rows) bv = dv;
        }
      }
      Xs[rr][cc] = xv;
      Ds[rr][cc] = dv;
      Db[rr][cc] = bv;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < kWR; ++rr) {
      float xa[4], db[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xa[a] = Xs[rr][ty * 4 + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) db[b] = Ds[rr][tx * 4 + b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xa[a], db[b], acc[a][b]);
    }
    if (want_bias && t < kWT) {
#pragma unroll
      for (int rr = 0; rr < kWR; ++rr) bsum += Db[rr][t];
    }
    __syncthreads();
  }
  const long long slice = (long long)p.Cin * p.Cout + p.Cout;
  float* w = p.ws + (long long)blockIdx.y * slice;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ty * 4 + a;
    if (i >= p.Cin) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tx * 4 + b;
      if (j < p.Cout) w[(long long)i * p.Cout + j] = acc[a][b];
    }
  }
  if (want_bias && t < kWT && j0 + t < p.Cout)
    w[(long long)p.Cin * p.Cout + j0 + t] = bsum;
}

__global__ void mlp_wgrad_finish_kernel(const float* ws, int nseg, int cps,
                                        float c0, float c1, float c2,
                                        long long nW, int Cout, float* dW,
                                        float* db) {
  // (no fused multiply-add here: a product must round before it is added)
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long slice = nW + Cout;
  if (e >= slice) return;
  float total = 0.f;
  for (int k = 0; k < nseg; ++k) {
    float s = 0.f;
    for (int c = 0; c < cps; ++c) s += ws[(long long)(k * cps + c) * slice + e];
    const float term = (k == 0 ? c0 : (k == 1 ? c1 : c2)) * s;
    total = k == 0 ? term : total + term;
  }
  if (e < nW) dW[e] = total;
  else if (db) db[e - nW] = total;
}

inline long long wgrad_chunk_rows(long long rows) {
  // at most 64 chunks, each a multiple of the staged pass and >= 64 rows
  long long c = (rows + 63) / 64;
  if (c < 64) c = 64;
  return (c + kWR - 1) / kWR * kWR;
}

// -- the float32 small steps of the WGAN-GP schedule ----------------------------
__global__ void mlp_interp_kernel(const float* real, const float* fake,
                                  const float* alpha, float* out, int B,
                                  long long n) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)B * n;
  if (e >= total) return;
  const float a = alpha[e / n];
  const float r = real[e], f = fake[e];
  out[e] = r;
  out[total + e] = f;
  out[2 * total + e] = a * r + (1.f - a) * f;
}

// (an LDS tree, not cg_common.h's block fold: its order of additions differs
// from wave-then-index, and moving it would change the MLP step's bits)
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// one workgroup: per-sample norms (a chain per sample), gp, v and the losses
__global__ __launch_bounds__(kThreads) void mlp_gp_loss_kernel(
    const float* g, const float* d_out, float* norm, float* gp, float* coef,
    float* v, float* loss, int B, long long n, float penalty) {
  __shared__ float red[kThreads];
  const int t = threadIdx.x;
  float s_gp = 0.f, s_real = 0.f, s_fake = 0.f;
  for (int b = t; b < B; b += kThreads) {
    const float* gb = g + (long long)b * n;
    float ss = 0.f;
    for (long long i = 0; i < n; ++i) ss = fmaf(gb[i], gb[i], ss);
    const float nr = sqrtf(ss);
    const float d = nr - 1.f;
    const float c = penalty * 2.f * d / ((float)B * nr);
    norm[b] = nr;
    coef[b] = c;
    s_gp += d * d;
    s_real += d_out[b];
    s_fake += d_out[B + b];
    if (v)
      for (long long i = 0; i < n; ++i) v[(long long)b * n + i] = c * gb[i];
  }
  const float t_gp = block_sum_256(s_gp, red);
  const float t_real = block_sum_256(s_real, red);
  const float t_fake = block_sum_256(s_fake, red);
  if (t == 0) {
    const float inv = 1.f / (float)B;
    const float gpv = t_gp * inv;
    gp[0] = gpv;
    loss[0] = -t_real * inv + t_fake * inv + penalty * gpv;
    loss[1] = -t_fake * inv;
  }
}

inline bool widths_ok(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return false;
  if (Cin > CG_MLP_MAX_FLAT || Cout > CG_MLP_MAX_FLAT) return false;
  // one side may be a flattened (time x width) axis, the other is a layer width
  return (Cin < Cout ? Cin : Cout) <= CG_MLP_MAX_WIDTH;
}

inline bool p_ok(double p) { return p >= 0.0 && p < 1.0; }

}  // namespace

extern "C" {

int cg_mlp_dropout_mask(void* keep, long long n, long long seed,
                        long long stream_id, double p, void* stream) {
  if (!keep || n <= 0 || !p_ok(p)) return CG_EINVAL;
  const DropArgs d = make_drop(p, seed, stream_id);
  const long long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return CG_EINVAL;
  hipLaunchKernelGGL(mlp_mask_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, (uint8_t*)keep, n, d);
  CG_LAUNCH_CHECK();
}

int cg_mlp_dense_fwd(const float* x, long long x_pitch, const float* W,
                     const float* b, const float* h_mask, float* h,
                     long long rows, int Cin, int Cout, int mode, float alpha,
                     double p, long long seed, long long stream_id,
                     void* stream) {
  if (!x || !W || !h || rows <= 0 || !widths_ok(Cin, Cout) || x_pitch < Cin ||
      !p_ok(p))
    return CG_EINVAL;
  if (mode != CG_MLP_FWD_ACT && mode != CG_MLP_FWD_TANGENT &&
      mode != CG_MLP_FWD_SIGMOID)
    return CG_EINVAL;
  if (mode == CG_MLP_FWD_TANGENT && !h_mask) return CG_EINVAL;
  const long long blocks = (rows + kBM - 1) / kBM;
  if (blocks > 0x7fffffffLL) return CG_EINVAL;
  DenseArgs a = {};
  a.a = x;
  a.a_pitch = x_pitch;
  a.W = W;
  a.bias = mode == CG_MLP_FWD_TANGENT ? nullptr : b;
  a.h_mask = h_mask;
  a.out = h;
  a.rows = rows;
  a.K = Cin;
  a.N = Cout;
  a.mode = mode;
  a.alpha = alpha;
  a.drop = make_drop(mode == CG_MLP_FWD_SIGMOID ? 0.0 : p, seed, stream_id);
  hipLaunchKernelGGL(mlp_dense_kernel<false>, dim3((unsigned)blocks),
                     dim3(kThreads), 0, (hipStream_t)stream, a);
  CG_LAUNCH_CHECK();
}

int cg_mlp_dense_dgrad(const float* dh, const float* h, const float* W,
                       float* dz, float* dx, long long rows, int Cin, int Cout,
                       int mode, float alpha, double p, void* stream) {
  if (!dh || !W || !dz || rows <= 0 || !widths_ok(Cin, Cout) ||
      !p_ok(p) || dz == dh)
    return CG_EINVAL;
  if (mode != CG_MLP_BWD_MASK && mode != CG_MLP_BWD_SIGMOID &&
      mode != CG_MLP_BWD_NONE)
    return CG_EINVAL;
  if (mode != CG_MLP_BWD_NONE && !h) return CG_EINVAL;
  const long long blocks = (rows + kBM - 1) / kBM;
  if (blocks > 0x7fffffffLL) return CG_EINVAL;
  DenseArgs a = {};
  a.a = dh;
  a.a_pitch = Cout;
  a.a_aux = h;
  a.dz = dz;
  a.W = W;
  a.out = dx;
  a.rows = rows;
  a.K = Cout;
  a.N = Cin;
  a.mode = mode;
  a.alpha = alpha;
  a.drop = make_drop(p, 0, 0);
  hipLaunchKernelGGL(mlp_dense_kernel<true>, dim3((unsigned)blocks),
                     dim3(kThreads), 0, (hipStream_t)stream, a);
  CG_LAUNCH_CHECK();
}

long long cg_mlp_wgrad_ws_elems(long long rows, int Cin, int Cout) {
  if (rows <= 0 || !widths_ok(Cin, Cout)) return 0;
  // up to three segments of at most `rows` rows, each cut into its own chunks
  const long long cr = wgrad_chunk_rows(rows);
  const long long nchunks = 3 * ((rows + cr - 1) / cr);
  return nchunks * ((long long)Cin * Cout + Cout);
}

int cg_mlp_dense_wgrad(const float* x, long long x_pitch, const float* x_tail,
                       long long tail_row0, const float* dz, float* dW,
                       float* db, long long rows, int Cin, int Cout,
                       long long seg_rows, float c0, float c1, float c2,
                       long long bias_rows, float* ws, void* stream) {
  if (!x || !dz || !dW || !ws || rows <= 0 || !widths_ok(Cin, Cout) ||
      x_pitch < Cin || seg_rows <= 0 || tail_row0 < 0 || bias_rows < 0)
    return CG_EINVAL;
  WgradArgs a = {};
  a.x = x;
  a.x_pitch = x_pitch;
  a.x_tail = x_tail;
  a.tail_row0 = tail_row0;
  a.dz = dz;
  a.rows = rows;
  a.seg_rows = seg_rows;
  a.bias_rows = bias_rows;
  // segments [0, seg_rows), [seg_rows, 2 seg_rows), [2 seg_rows, rows); the
  // chunking is that of the whole row count (cg_mlp_wgrad_ws_elems' bound)
  const int nseg = rows <= seg_rows ? 1 : (rows <= 2 * seg_rows ? 2 : 3);
  long long longest = nseg == 1 ? rows : seg_rows;
  if (nseg == 3 && rows - 2 * seg_rows > longest) longest = rows - 2 * seg_rows;
  a.chunk_rows = wgrad_chunk_rows(rows);
  a.cps = (int)((longest + a.chunk_rows - 1) / a.chunk_rows);
  a.Cin = Cin;
  a.Cout = Cout;
  a.tiles_j = (Cout + kWT - 1) / kWT;
  a.ws = ws;
  const int nchunks = nseg * a.cps;
  const long long tiles = (long long)((Cin + kWT - 1) / kWT) * a.tiles_j;
  hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((unsigned)tiles, (unsigned)nchunks),
                     dim3(kThreads), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long long nW = (long long)Cin * Cout;
  const long long total = nW + Cout;
  hipLaunchKernelGGL(mlp_wgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, (const float*)ws, nseg,
                     a.cps, c0, c1, c2, nW, Cout, dW, db);
  CG_LAUNCH_CHECK();
}

int cg_mlp_interp(const float* real, const float* fake, const float* alpha,
                  float* out, int B, long long n, void* stream) {
  if (!real || !fake || !alpha || !out || B <= 0 || n <= 0) return CG_EINVAL;
  const long long blocks = ((long long)B * n + 255) / 256;
  if (blocks > 0x7fffffffLL) return CG_EINVAL;
  hipLaunchKernelGGL(mlp_interp_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, real, fake, alpha, out, B, n);
  CG_LAUNCH_CHECK();
}

int cg_mlp_gp_loss(const float* g, const float* d_out, float* norm, float* gp,
                   float* coef, float* v, float* loss, int B, long long n,
                   float penalty, void* stream) {
  if (!g || !d_out || !norm || !gp || !coef || !loss || B <= 0 || n <= 0)
    return CG_EINVAL;
  hipLaunchKernelGGL(mlp_gp_loss_kernel, dim3(1), dim3(kThreads), 0,
                     (hipStream_t)stream, g, d_out, norm, gp, coef, v, loss, B,
                     n, penalty);
  CG_LAUNCH_CHECK();
}

}  // extern "C"
