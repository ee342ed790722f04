// van Rossum kernel sums and distances between the binary trains of a trial on
// the float64 matrix pipe (spike_metrics.van_rossum_gram_frames is
// the numpy statement).
//
//   S_ij = sum_{k in i, l in j} a^|f_k - f_l| = G_ij + G_ji,  G = M' Sp^T
//
// with Sp the (C, T) trains and M' the half-weighted causal filter
//   h = s[t] / 2;  m' = fl(fl(a m) + h);  M'[t] = m';  m = fl(m' + h)
// One workgroup owns a 128 x 128 block (P, Q), P <= Q, of one sample's matrix
// (C <= 128: the whole sample).  It walks time in chunks of kVrChunk frames: one
// lane per train advances the recursion through the chunk and leaves M' (f64)
// and the train (f32 {0, 1}) in LDS, then the eight waves run
// v_mfma_f64_16x16x4_f64 over the chunk into accumulators that stay in
// registers for the whole of T: per pair of 16-train tiles (I, J) one
// accumulator for G_IJ (A = M'_I, B = Sp_J) and one for G_JI^T (A = Sp_I, B =
// M'_J).  At the end S = G + G^T is one addition per element; the element
// (j, i) is a copy of (i, j), brought to its place through LDS.  No M' array in
// global memory, no atomics, no zeroed buffer: the same bits every call.
// An off-diagonal block also forms the diagonal tiles of its row and column
// block (the S_ii of the distances): the same instructions on the same data as
// in the diagonal block, hence the same bits.
#include "cg_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kVrThreads = 512;
constexpr int kVrWaves = kVrThreads / 64;
constexpr int kVrBlock = 128;  // trains of a row / column block: 8 tiles of 16
constexpr int kVrTiles = kVrBlock / 16;
constexpr int kVrChunk = 16;   // frames per LDS chunk (spike_metrics.VAN_ROSSUM_CHUNK)
// LDS row of one frame: the row block's trains, then the column block's; 16
// columns of padding put the rows of lanes l and l + 16 on disjoint banks
// (272 * 8 B = 32 banks of 64 further for ds_read_b64, 272 * 4 B = 16 of 32 for
// ds_read_b32)
constexpr int kVrStride = 2 * kVrBlock + 16;
// tile pairs per wave: 64 cross pairs + 16 diagonal tiles over 8 waves (a
// diagonal block has 36 pairs: 5 per wave at most)
constexpr int kVrMaxPairs = 10;
constexpr int kVrScratch = 16 * 17;  // one tile, rows padded by one element
constexpr int kVrMaxC = 4096;
constexpr int kVrMaxT = 1 << 24;

// One train through one chunk.  p: frame 0 of the train, or null for a padding
// column (train >= C), which leaves exact zeros.  Frames >= T leave zeros too.
// No fused multiply-add: every operation rounds on its own, as numpy's do.
__device__ __forceinline__ double vr_filter_chunk(const float* p, long long s_t,
                                                  int t0, int T, double a, double m,
                                                  double* mcol, float* scol) {
#pragma clang fp contract(off)
  float v[kVrChunk];
#pragma unroll
  for (int f = 0; f < kVrChunk; ++f)
    v[f] = (p && t0 + f < T) ? p[(long long)(t0 + f) * s_t] : 0.f;
#pragma unroll
  for (int f = 0; f < kVrChunk; ++f) {
    const double s = v[f] != 0.f ? 1.0 : 0.0;
    const double h = 0.5 * s;
    double mp = a * m;
    mp = mp + h;
    mcol[f * kVrStride] = t0 + f < T ? mp : 0.0;
    scol[f * kVrStride] = (float)s;
    m = mp + h;
  }
  return m;
}

__device__ __forceinline__ void vr_emit(double* __restrict__ gram,
                                        double* __restrict__ dist, long long at,
                                        double s, double sii, double sjj) {
#pragma clang fp contract(off)
  if (gram) gram[at] = s;
  if (dist) {
    double d2 = sii + sjj;
    d2 = d2 - 2.0 * s;
    dist[at] = sqrt(fmax(d2, 0.0));
  }
}

__global__ __launch_bounds__(kVrThreads) void van_rossum_kernel(
    const float* __restrict__ spikes, long long s_b, long long s_t, long long s_c,
    int T, int C, double decay, double* __restrict__ gram,
    double* __restrict__ dist) {
  __shared__ double sm_m[kVrChunk * kVrStride];
  __shared__ float sm_s[kVrChunk * kVrStride];
  __shared__ double sm_diag[2 * kVrBlock];
  static_assert(kVrWaves * kVrScratch <= kVrChunk * kVrStride, "scratch in sm_m");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // blockIdx.y -> (P, Q), P <= Q, row by row
  const int NB = (C + kVrBlock - 1) / kVrBlock;
  int P = 0, rem = blockIdx.y;
  while (rem >= NB - P) { rem -= NB - P; ++P; }
  const int Q = P + rem;
  const bool diag = P == Q;
  const float* sp = spikes + (long long)blockIdx.x * s_b;
  // LDS column -> train: [0, 128) the row block, [128, 256) the column block
  auto train_of = [&](int col) {
    return (col < kVrBlock ? P : Q) * kVrBlock + (col & (kVrBlock - 1));
  };

  // the recursion: 16 (32) lanes of every wave take the wave's share of the 128
  // (256) columns
  const int per = (diag ? kVrBlock : 2 * kVrBlock) / kVrWaves;
  const int mycol = lane < per ? wave * per + lane : -1;
  const float* mine = nullptr;
  if (mycol >= 0 && train_of(mycol) < C) mine = sp + (long long)train_of(mycol) * s_c;

  // this wave's tile pairs: pair wave + 8 q
  int ra[kVrMaxPairs], cb[kVrMaxPairs];
  unsigned valid = 0, store = 0;
#pragma unroll
  for (int q = 0; q < kVrMaxPairs; ++q) {
    const int p = wave + kVrWaves * q;
    int a = 0, b = 0;
    bool ok = false, st = false;
    if (diag) {
      if (p < kVrTiles * (kVrTiles + 1) / 2) {
        int I = 0, r = p;
        while (r >= kVrTiles - I) { r -= kVrTiles - I; ++I; }
        a = I * 16; b = (I + r) * 16; ok = st = true;
      }
    } else if (p < kVrTiles * kVrTiles) {
      a = (p / kVrTiles) * 16; b = kVrBlock + (p % kVrTiles) * 16; ok = st = true;
    } else if (p < kVrTiles * kVrTiles + 2 * kVrTiles) {
      // the diagonal tiles of both blocks, for the S_ii only
      a = b = (p - kVrTiles * kVrTiles) * 16; ok = true;
    }
    ok = ok && train_of(a) < C && train_of(b) < C;
    ra[q] = __builtin_amdgcn_readfirstlane(a);
    cb[q] = __builtin_amdgcn_readfirstlane(b);
    if (ok) valid |= 1u << q;
    if (ok && st) store |= 1u << q;
  }
  valid = __builtin_amdgcn_readfirstlane(valid);
  store = __builtin_amdgcn_readfirstlane(store);

  f64x4 accG[kVrMaxPairs], accH[kVrMaxPairs];
#pragma unroll
  for (int q = 0; q < kVrMaxPairs; ++q) {
    accG[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    accH[q] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  double m = 0.0;
  const int nchunks = (T + kVrChunk - 1) / kVrChunk;
  for (int ch = 0; ch < nchunks; ++ch) {
    if (mycol >= 0)
      m = vr_filter_chunk(mine, s_t, ch * kVrChunk, T, decay, m, sm_m + mycol,
                          sm_s + mycol);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kVrChunk / 4; ++kk) {
      // A: row lane & 15, k = lane >> 4; B: k = lane >> 4, column lane & 15
      const int at = (kk * 4 + (lane >> 4)) * kVrStride + (lane & 15);
#pragma unroll
      for (int q = 0; q < kVrMaxPairs; ++q) {
        if (valid >> q & 1) {
          const double ma = sm_m[at + ra[q]], mb = sm_m[at + cb[q]];
          const double sa = (double)sm_s[at + ra[q]], sb = (double)sm_s[at + cb[q]];
          accG[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, sb, accG[q], 0, 0, 0);
          accH[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, mb, accH[q], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // S = G + G^T; C/D layout: column lane & 15, row (lane >> 4) + 4 r
#pragma unroll
  for (int q = 0; q < kVrMaxPairs; ++q) accG[q] = accG[q] + accH[q];
#pragma unroll
  for (int q = 0; q < kVrMaxPairs; ++q) {
    if ((valid >> q & 1) && ra[q] == cb[q]) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((lane >> 4) + 4 * r == (lane & 15)) sm_diag[ra[q] + (lane & 15)] = accG[q][r];
    }
  }
  __syncthreads();

  double* scr = sm_m + wave * kVrScratch;  // (the chunks are done with sm_m)
  const long long ob = (long long)blockIdx.x * C * C;
#pragma unroll
  for (int q = 0; q < kVrMaxPairs; ++q) {
    const bool act = store >> q & 1;
    const int gi0 = train_of(ra[q]), gj0 = train_of(cb[q]);
    const bool same = gi0 == gj0;  // a diagonal tile: its upper triangle counts
    if (act) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = (lane >> 4) + 4 * r, j = lane & 15;
        scr[i * 17 + j] = accG[q][r];
        if (gi0 + i < C && gj0 + j < C && (!same || i <= j))
          vr_emit(gram, dist, ob + (long long)(gi0 + i) * C + (gj0 + j), accG[q][r],
                  sm_diag[ra[q] + i], sm_diag[cb[q] + j]);
      }
    }
    __syncthreads();
    if (act) {
      // element (j, i) is element (i, j): rows of the mirrored tile run along
      // the lanes again
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = (lane >> 4) + 4 * r, i = lane & 15;
        if (gi0 + i < C && gj0 + j < C && (!same || i < j))
          vr_emit(gram, dist, ob + (long long)(gj0 + j) * C + (gi0 + i),
                  scr[i * 17 + j], sm_diag[ra[q] + i], sm_diag[cb[q] + j]);
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int cg_van_rossum(const float* spikes, int B, int T, int C,
                             long long s_b, long long s_t, long long s_c,
                             double decay, double* gram, double* dist,
                             void* stream) {
  if (!spikes || (!gram && !dist) || B < 1 || T < 1 || C < 1 || T > kVrMaxT ||
      C > kVrMaxC || !(decay >= 0.0 && decay <= 1.0))
    return CG_EINVAL;
  const int NB = (C + kVrBlock - 1) / kVrBlock;
  hipLaunchKernelGGL(van_rossum_kernel, dim3(B, NB * (NB + 1) / 2),
                     dim3(kVrThreads), 0, cg_stream(stream), spikes, s_b, s_t, s_c, T, C,
                     decay, gram, dist);
  CG_LAUNCH_CHECK();
}
