// Population states of spike trains and their nearest neighbours (DESIGN.md 25;
// spike_metrics.population_states / state_neighbours are the numpy statements).
//
// A state is the vector of spike counts of the C neurons in one bin of `bin`
// frames: integers 0 .. bin <= 127, which bf16 holds exactly.  A set of states
// is a row-major bf16 matrix whose rows are padded with zeros to a multiple of
// CG_STATE_K_STEP = 32 elements, the K step of v_mfma_f32_16x16x32_bf16.
//
//   d2(a_i, b_j) = |a_i|^2 + |b_j|^2 - 2 a_i . b_j
//
// The products run on the matrix pipe with the neurons as the K dimension:
// every product and every partial sum is an integer of at most C bin^2 <= 2^24,
// which f32 holds exactly in any order, so the conversion to int32 does not
// round.  The norms are int32 sums of a launch of their own.
//
// One workgroup owns kSnRows = 128 states of A (32 a wave) and a run of 64-state
// tiles of B.  B's states are the ROWS of the MFMA and A's the COLUMNS, so a
// lane's four accumulator registers of a tile are four states of B against ONE
// state of A (column lane & 15): the lane keeps the 8 smallest d2 of that state
// of A, ascending, in registers, and its count of d2 <= radius_b[j], and never
// exchanges anything while B streams past.  While C <= 128 the wave's fragments
// of A stay in registers too, and only B's tiles pass through LDS.  At the end
// the four lane groups (lane >> 4) of a state are merged through LDS.  Where A
// has few rows B is split over up to 64 workgroups per row block (sn_plan: a
// function of Sa and Sb alone); their lists and counts go to the workspace and
// a second launch merges them in split order.  The k smallest VALUES of a
// multiset do not depend on the order they are met in and the counts are
// integer sums: no atomics, nothing zeroed beforehand, the same bits every call.
#include "cg_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 sn_bf16x8;

constexpr int kSnThreads = 256;
constexpr int kSnWaves = kSnThreads / 64;
constexpr int kSnWaveTiles = 2;                        // 16-state tiles of A per wave
constexpr int kSnRows = kSnWaves * kSnWaveTiles * 16;  // states of A per workgroup
constexpr int kSnColTiles = 4;
constexpr int kSnCols = kSnColTiles * 16;              // states of B per tile
constexpr int kSnChunk = 128;                          // K elements per LDS chunk
constexpr int kSnChunk8 = kSnChunk / 8;                // in 16-byte words
// LDS row: the chunk and one 16-byte slot, so that the 16 rows of a
// ds_read_b128 lane group fall on 16 distinct slots (as spike_ccg.hip)
constexpr int kSnPitch = kSnChunk8 + 1;
static_assert(kSnPitch * 16 % 256 == 16, "row pitch one slot past a bank row");
constexpr int kSnK = CG_STATE_MAX_K;
constexpr int kSnNone = CG_STATE_NONE;
constexpr int kSnMaxSplits = 64;
constexpr int kSnTargetItems = 1024;  // workgroups wanted before B is split less

// v into the ascending list: a no-op for v >= l[kSnK - 1]
__device__ __forceinline__ void sn_insert(int (&l)[kSnK], int v) {
#pragma unroll
  for (int e = 0; e < kSnK; ++e) {
    const int lo = min(l[e], v);
    v = max(l[e], v);
    l[e] = lo;
  }
}

__device__ __forceinline__ unsigned sn_bf16_bits(int n) {  // 0 <= n < 256: exact
  return __float_as_uint((float)n) >> 16;
}
__device__ __forceinline__ int sn_bf16_int(unsigned bits) {
  return (int)__uint_as_float(bits << 16);
}

// states[row][c] for row = n nb + b: spikes of neuron c in frames b bin ..
// (b + 1) bin - 1 of trial n.  One thread per pair of columns of a row, the
// padding columns included; every input element is read once.
__global__ __launch_bounds__(256) void population_states_kernel(
    const float* __restrict__ trains, long long s_b, long long s_t, long long s_c,
    int nb, int C, int half, int bin, long long total,
    unsigned* __restrict__ states) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total;
       e += gridDim.x * 256ll) {
    const long long row = e / half;
    const int c = (int)(e - row * half) * 2;
    const long long n = row / nb;
    const int b = (int)(row - n * nb);
    const float* p = trains + n * s_b + (long long)b * bin * s_t;
    int n0 = 0, n1 = 0;
    if (c < C) {
      const float* q = p + (long long)c * s_c;
      for (int t = 0; t < bin; ++t) n0 += q[(long long)t * s_t] != 0.f ? 1 : 0;
    }
    if (c + 1 < C) {
      const float* q = p + (long long)(c + 1) * s_c;
      for (int t = 0; t < bin; ++t) n1 += q[(long long)t * s_t] != 0.f ? 1 : 0;
    }
    states[e] = sn_bf16_bits(n0) | sn_bf16_bits(n1) << 16;
  }
}

// norms[row] = sum_c states[row][c]^2, 16 lanes per row
__global__ __launch_bounds__(256) void state_norms_kernel(
    const uint4* __restrict__ states, int S, int Cp8, int* __restrict__ norms) {
  const int sub = threadIdx.x & 15;
  const long long row = (blockIdx.x * 256ll + threadIdx.x) >> 4;
  int sum = 0;
  if (row < S) {
    const uint4* p = states + row * Cp8;
    for (int q = sub; q < Cp8; q += 16) {
      const uint4 w = p[q];
      const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int lo = sn_bf16_int(u[h] & 0xffffu), hi = sn_bf16_int(u[h] >> 16);
        sum += lo * lo + hi * hi;
      }
    }
  }
  // (every lane goes through the shuffles)
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
  if (sub == 0 && row < S) norms[row] = sum;
}

// Rows r0 .. r0 + ROWS - 1 of a set of S states, 16-byte words q0 .. q0 + 15 of
// each, into LDS; a row >= S and a word >= Cp8 are stored as zeros and read
// from an address clamped into the set.  Every load is issued before the first
// is stored.
template <int ROWS>
__device__ __forceinline__ void sn_stage(uint4* __restrict__ sm,
                                         const uint4* __restrict__ m, int S,
                                         int Cp8, int r0, int q0) {
  constexpr int kIters = ROWS * kSnChunk8 / kSnThreads;
  static_assert(ROWS * kSnChunk8 % kSnThreads == 0, "whole passes");
  uint4 v[kIters];
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int idx = threadIdx.x + it * kSnThreads;
    const int r = idx / kSnChunk8, q = idx % kSnChunk8;
    v[it] = m[(long long)min(r0 + r, S - 1) * Cp8 + min(q0 + q, Cp8 - 1)];
  }
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int idx = threadIdx.x + it * kSnThreads;
    const int r = idx / kSnChunk8, q = idx % kSnChunk8;
    if (r0 + r >= S || q0 + q >= Cp8) v[it] = uint4{0u, 0u, 0u, 0u};
    sm[r * kSnPitch + q] = v[it];
  }
}

// One tile's accumulators into the lists and the counts of a lane.  The lists
// hold e = |b_j|^2 - 2 a_i . b_j, which orders the states of B as d2 = e +
// |a_i|^2 does (the norm of a_i is added once, at the end); d2 <= radius_b[j] is
// (|b_j|^2 - radius_b[j]) - 2 a_i . b_j <= -|a_i|^2 with the bracket staged per
// state of B.  EDGE: the tile holds a state past Sb or the excluded diagonal,
// and every element is masked.
template <bool EDGE>
__device__ __forceinline__ void sn_select(
    const f32x4 (&acc)[kSnWaveTiles][kSnColTiles],
    int (&list)[kSnWaveTiles][kSnK], int (&cnt)[kSnWaveTiles],
    const int (&ai)[kSnWaveTiles], const int (&nai)[kSnWaveTiles],
    const int* __restrict__ snb, const int* __restrict__ scr, int j0, int Sb,
    int exclude_self, bool count, int lane) {
  // C/D: column lane & 15 (the state of A), row 4 (lane >> 4) + reg (of B)
#pragma unroll
  for (int at = 0; at < kSnWaveTiles; ++at) {
#pragma unroll
    for (int bt = 0; bt < kSnColTiles; ++bt) {
      const int jl = bt * 16 + 4 * (lane >> 4);
      const int4 nb4 = *reinterpret_cast<const int4*>(snb + jl);
      const int nbv[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
      int dot[4], e[4];
      bool ok[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        dot[reg] = (int)acc[at][bt][reg];
        e[reg] = nbv[reg] - 2 * dot[reg];
        if (EDGE) {
          const int j = j0 + jl + reg;
          ok[reg] = j < Sb && !(exclude_self && j == ai[at]);
          e[reg] = ok[reg] ? e[reg] : kSnNone;
        }
      }
      if (count) {
        const int4 cr4 = *reinterpret_cast<const int4*>(scr + jl);
        const int crv[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          bool hit = crv[reg] - 2 * dot[reg] <= -nai[at];
          if (EDGE) hit = hit && ok[reg];
          cnt[at] += hit ? 1 : 0;
        }
      }
      if (min(min(e[0], e[1]), min(e[2], e[3])) < list[at][kSnK - 1]) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sn_insert(list[at], e[reg]);
      }
    }
  }
}

// blockIdx.x = row block * splits + split.  out_knn: [splits][Sa][k] (the
// result itself when splits == 1), out_within: [splits][Sa]; either may be NULL.
// ONE: all of K fits one chunk (C <= 128); a wave then keeps the fragments of
// its states of A in registers for the whole of B, and a K step past C
// multiplies staged zeros.
template <bool ONE>
__global__ __launch_bounds__(kSnThreads, 2) void state_neighbours_kernel(
    const uint4* __restrict__ a, int Sa, const uint4* __restrict__ b, int Sb,
    int Cp8, const int* __restrict__ na, const int* __restrict__ nb,
    const int* __restrict__ radius, int exclude_self, int splits,
    int tiles_per_split, int k, int* __restrict__ out_knn,
    int* __restrict__ out_within) {
  __shared__ uint4 sm_a[kSnRows * kSnPitch];
  __shared__ uint4 sm_b[kSnCols * kSnPitch];
  __shared__ __attribute__((aligned(16))) int sm_nb[2][kSnCols];
  __shared__ __attribute__((aligned(16))) int sm_cr[2][kSnCols];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rb = blockIdx.x / splits, split = blockIdx.x - rb * splits;
  const int i0 = rb * kSnRows;
  const int ntiles = (Sb + kSnCols - 1) / kSnCols;
  const int t_begin = split * tiles_per_split;
  const int t_end = min(ntiles, t_begin + tiles_per_split);
  const int nchunks = ONE ? 1 : (Cp8 + kSnChunk8 - 1) / kSnChunk8;
  // state l & 15 of a 16-state tile, elements 8 (l >> 4) .. of a K step
  const int frag = (lane & 15) * kSnPitch + (lane >> 4);

  int list[kSnWaveTiles][kSnK];
  int cnt[kSnWaveTiles], ai[kSnWaveTiles], nai[kSnWaveTiles];
#pragma unroll
  for (int at = 0; at < kSnWaveTiles; ++at) {
#pragma unroll
    for (int e = 0; e < kSnK; ++e) list[at][e] = kSnNone;
    cnt[at] = 0;
    ai[at] = i0 + (wave * kSnWaveTiles + at) * 16 + (lane & 15);
    nai[at] = na[min(ai[at], Sa - 1)];
  }

  sn_bf16x8 fa1[kSnWaveTiles][kSnChunk8 / 4];
  if (ONE) {
    sn_stage<kSnRows>(sm_a, a, Sa, Cp8, i0, 0);
    __syncthreads();
#pragma unroll
    for (int at = 0; at < kSnWaveTiles; ++at)
#pragma unroll
      for (int ks = 0; ks < kSnChunk8 / 4; ++ks)
        fa1[at][ks] = __builtin_bit_cast(
            sn_bf16x8,
            sm_a[(wave * kSnWaveTiles + at) * 16 * kSnPitch + frag + ks * 4]);
  }

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int j0 = tile * kSnCols;
    const int par = tile & 1;
    f32x4 acc[kSnWaveTiles][kSnColTiles];
#pragma unroll
    for (int at = 0; at < kSnWaveTiles; ++at)
#pragma unroll
      for (int bt = 0; bt < kSnColTiles; ++bt)
        acc[at][bt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < nchunks; ++ch) {
      if (!ONE) sn_stage<kSnRows>(sm_a, a, Sa, Cp8, i0, ch * kSnChunk8);
      sn_stage<kSnCols>(sm_b, b, Sb, Cp8, j0, ch * kSnChunk8);
      if (ch == 0 && threadIdx.x < kSnCols) {
        const int j = j0 + threadIdx.x;
        const int nbj = j < Sb ? nb[j] : 0;
        sm_nb[par][threadIdx.x] = nbj;
        // (d2 is in 0 .. 2^25: a radius clamped into -1 .. 2^30 decides the
        // same, and neither difference overflows)
        sm_cr[par][threadIdx.x] =
            (radius != nullptr && j < Sb)
                ? nbj - min(max(radius[j], -1), 1 << 30) : 0;
      }
      __syncthreads();
      if (ONE) {
#pragma unroll
        for (int ks = 0; ks < kSnChunk8 / 4; ++ks) {
          sn_bf16x8 fb[kSnColTiles];
#pragma unroll
          for (int bt = 0; bt < kSnColTiles; ++bt)
            fb[bt] = __builtin_bit_cast(
                sn_bf16x8, sm_b[bt * 16 * kSnPitch + frag + ks * 4]);
#pragma unroll
          for (int at = 0; at < kSnWaveTiles; ++at)
#pragma unroll
            for (int bt = 0; bt < kSnColTiles; ++bt)
              acc[at][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  fb[bt], fa1[at][ks], acc[at][bt], 0, 0, 0);
        }
      } else {
        const int ksteps = min(kSnChunk8 / 4, Cp8 / 4 - ch * (kSnChunk8 / 4));
        for (int ks = 0; ks < ksteps; ++ks) {
          sn_bf16x8 fa[kSnWaveTiles], fb[kSnColTiles];
#pragma unroll
          for (int at = 0; at < kSnWaveTiles; ++at)
            fa[at] = __builtin_bit_cast(
                sn_bf16x8,
                sm_a[(wave * kSnWaveTiles + at) * 16 * kSnPitch + frag + ks * 4]);
#pragma unroll
          for (int bt = 0; bt < kSnColTiles; ++bt)
            fb[bt] = __builtin_bit_cast(
                sn_bf16x8, sm_b[bt * 16 * kSnPitch + frag + ks * 4]);
#pragma unroll
          for (int at = 0; at < kSnWaveTiles; ++at)
#pragma unroll
            for (int bt = 0; bt < kSnColTiles; ++bt)
              acc[at][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  fb[bt], fa[at], acc[at][bt], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    // a tile with a state past Sb or the excluded diagonal in it masks per
    // element; every other tile (uniform over the workgroup) does not
    const bool edge = j0 + kSnCols > Sb ||
                      (exclude_self && j0 < i0 + kSnRows && i0 < j0 + kSnCols);
    if (edge)
      sn_select<true>(acc, list, cnt, ai, nai, sm_nb[par], sm_cr[par], j0, Sb,
                      exclude_self, radius != nullptr, lane);
    else
      sn_select<false>(acc, list, cnt, ai, nai, sm_nb[par], sm_cr[par], j0, Sb,
                       exclude_self, radius != nullptr, lane);
  }

  // the four lane groups of a state of A: [row][group][8 values, count]
  __syncthreads();
  int* sl = reinterpret_cast<int*>(sm_a);
  static_assert(kSnRows * 4 * (kSnK + 1) * 4 <= kSnRows * kSnPitch * 16, "fits");
#pragma unroll
  for (int at = 0; at < kSnWaveTiles; ++at) {
    const int r = (wave * kSnWaveTiles + at) * 16 + (lane & 15);
    int* p = sl + (r * 4 + (lane >> 4)) * (kSnK + 1);
#pragma unroll
    for (int e = 0; e < kSnK; ++e) p[e] = list[at][e];
    p[kSnK] = cnt[at];
  }
  __syncthreads();
  if (threadIdx.x < kSnRows && i0 + (int)threadIdx.x < Sa) {
    const int* p = sl + threadIdx.x * 4 * (kSnK + 1);
    int l[kSnK];
#pragma unroll
    for (int e = 0; e < kSnK; ++e) l[e] = p[e];
    int c = p[kSnK];
#pragma unroll
    for (int g = 1; g < 4; ++g) {
#pragma unroll
      for (int e = 0; e < kSnK; ++e) sn_insert(l, p[g * (kSnK + 1) + e]);
      c += p[g * (kSnK + 1) + kSnK];
    }
    const long long at = (long long)split * Sa + i0 + threadIdx.x;
    if (out_knn != nullptr) {
      const int norm = na[i0 + threadIdx.x];  // the lists hold d2 - |a_i|^2
#pragma unroll
      for (int e = 0; e < kSnK; ++e)
        if (e < k) out_knn[at * k + e] = l[e] == kSnNone ? kSnNone : l[e] + norm;
    }
    if (out_within != nullptr) out_within[at] = c;
  }
}

// the splits' lists and counts of a state of A, in split order
__global__ __launch_bounds__(256) void state_merge_kernel(
    const int* __restrict__ pk, const int* __restrict__ pw, int Sa, int splits,
    int k, int* __restrict__ knn, int* __restrict__ within) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= Sa) return;
  if (knn != nullptr) {
    int l[kSnK];
#pragma unroll
    for (int e = 0; e < kSnK; ++e) l[e] = kSnNone;
    for (int s = 0; s < splits; ++s) {
      const int* p = pk + ((long long)s * Sa + i) * k;
      for (int e = 0; e < k; ++e) sn_insert(l, p[e]);
    }
#pragma unroll
    for (int e = 0; e < kSnK; ++e)
      if (e < k) knn[i * k + e] = l[e];
  }
  if (within != nullptr) {
    int c = 0;
    for (int s = 0; s < splits; ++s) c += pw[(long long)s * Sa + i];
    within[i] = c;
  }
}

inline int sn_padded(int C) {
  return (C + CG_STATE_K_STEP - 1) / CG_STATE_K_STEP * CG_STATE_K_STEP;
}

// every sum of products of two states is an integer f32 holds
inline bool sn_exact(int C, int bin) {
  return C >= 1 && C <= CG_STATE_MAX_C && bin >= 1 && bin <= CG_STATE_MAX_BIN &&
         (long long)C * bin * bin <= CG_STATE_EXACT_SUM;
}

struct SnPlan {
  int rowblocks, tiles_per_split, splits;
};
inline SnPlan sn_plan(int Sa, int Sb) {
  SnPlan p;
  p.rowblocks = (Sa + kSnRows - 1) / kSnRows;
  const int ntiles = (Sb + kSnCols - 1) / kSnCols;
  int want = (kSnTargetItems + p.rowblocks - 1) / p.rowblocks;
  if (want > kSnMaxSplits) want = kSnMaxSplits;
  if (want > ntiles) want = ntiles;
  p.tiles_per_split = (ntiles + want - 1) / want;
  p.splits = (ntiles + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}

inline bool sn_shape_ok(int Sa, int Sb, int C, int bin, int k) {
  return Sa >= 1 && Sb >= 1 && Sa <= CG_STATE_MAX_ROWS &&
         Sb <= CG_STATE_MAX_ROWS && sn_exact(C, bin) && k >= 1 &&
         k <= CG_STATE_MAX_K;
}

inline bool sn_aligned(const void* p, uintptr_t to) {
  return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0;
}

}  // namespace

extern "C" int cg_population_states(const float* trains, int B, int T, int C,
                                    long long s_b, long long s_t, long long s_c,
                                    int bin, void* states, void* stream) {
  if (!trains || !states || !sn_aligned(states, 16) || B < 1 || T < 1 ||
      !sn_exact(C, bin) || T < bin ||
      (long long)B * (T / bin) > CG_STATE_MAX_ROWS)
    return CG_EINVAL;
  const int nb = T / bin;
  const int half = sn_padded(C) / 2;
  const long long total = (long long)B * nb * half;
  const long long blocks = (total + 255) / 256;
  const long long cap = 1ll << 20;
  hipLaunchKernelGGL(population_states_kernel,
                     dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0,
                     cg_stream(stream), trains, s_b, s_t, s_c, nb, C, half, bin,
                     total, static_cast<unsigned*>(states));
  CG_LAUNCH_CHECK();
}

extern "C" long long cg_state_neighbours_ws_bytes(int Sa, int Sb, int C, int bin,
                                                  int k) {
  if (!sn_shape_ok(Sa, Sb, C, bin, k)) return -1;
  const SnPlan p = sn_plan(Sa, Sb);
  long long ints = (long long)Sa + Sb;
  if (p.splits > 1) ints += (long long)p.splits * Sa * (k + 1);
  return ints * 4;
}

extern "C" int cg_state_neighbours(const void* a, int Sa, const void* b, int Sb,
                                   int C, int bin, int k, int exclude_self,
                                   const int* radius_b, int* knn, int* within,
                                   void* ws, void* stream) {
  if (!a || !b || !ws || !sn_aligned(a, 16) || !sn_aligned(b, 16) ||
      !sn_aligned(ws, 16) || !sn_aligned(radius_b, 4) || !sn_aligned(knn, 4) ||
      !sn_aligned(within, 4) || !sn_shape_ok(Sa, Sb, C, bin, k) ||
      (!knn && !within) || (within != nullptr) != (radius_b != nullptr) ||
      (exclude_self && (a != b || Sa != Sb)))
    return CG_EINVAL;
  const SnPlan p = sn_plan(Sa, Sb);
  const int Cp8 = sn_padded(C) / 8;
  int* na = static_cast<int*>(ws);
  int* nb = na + Sa;
  int* pk = nb + Sb;                        // [splits][Sa][k]
  int* pw = pk + (long long)p.splits * Sa * k;  // [splits][Sa]
  const uint4* a4 = static_cast<const uint4*>(a);
  const uint4* b4 = static_cast<const uint4*>(b);
  hipStream_t st = cg_stream(stream);
  hipLaunchKernelGGL(state_norms_kernel, dim3((unsigned)((Sa + 15) / 16)),
                     dim3(256), 0, st, a4, Sa, Cp8, na);
  hipLaunchKernelGGL(state_norms_kernel, dim3((unsigned)((Sb + 15) / 16)),
                     dim3(256), 0, st, b4, Sb, Cp8, nb);
  const bool split = p.splits > 1;
  const dim3 grid((unsigned)(p.rowblocks * p.splits));
  int* out_knn = knn ? (split ? pk : knn) : nullptr;
  int* out_within = within ? (split ? pw : within) : nullptr;
  if (Cp8 <= kSnChunk8)
    hipLaunchKernelGGL(state_neighbours_kernel<true>, grid, dim3(kSnThreads), 0,
                       st, a4, Sa, b4, Sb, Cp8, na, nb, radius_b,
                       exclude_self ? 1 : 0, p.splits, p.tiles_per_split, k,
                       out_knn, out_within);
  else
    hipLaunchKernelGGL(state_neighbours_kernel<false>, grid, dim3(kSnThreads), 0,
                       st, a4, Sa, b4, Sb, Cp8, na, nb, radius_b,
                       exclude_self ? 1 : 0, p.splits, p.tiles_per_split, k,
                       out_knn, out_within);
  if (split)
    hipLaunchKernelGGL(state_merge_kernel, dim3((unsigned)((Sa + 255) / 256)),
                       dim3(256), 0, st, pk, pw, Sa, p.splits, k, knn, within);
  CG_LAUNCH_CHECK();
}
