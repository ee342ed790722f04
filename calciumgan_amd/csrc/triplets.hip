// Third-order spike counts of binarised population states (DESIGN.md 26;
// spike_metrics.binary_states / triplet_counts are the numpy statements).
//
// A state is one bit per neuron: whether it fired at all in one bin of `bin`
// frames.  cg_binary_words packs the states of a neuron 32 to a uint32 word,
// neuron-major: words[c][n wpt + w], wpt = ceil(nb / 32) words per trial, bit
// b % 32 of word b / 32 the state of bin b; the tail bits of a trial's last word
// are zero and so count nothing.  Then
//
//   triplets[i < j < k] = sum_w popcount(w_i & w_j & w_k)
//
// and the pair and single counts are the same sum with k == j (and j == i).
//
// cg_triplet_counts cuts the neurons into tiles of kTpTile = 16.  A workgroup of
// kTpThreads = 128 owns one tile triple I <= J <= K and a run of chunks of
// kTpChunk = 64 words, staged in LDS (3 x 16 rows).  A lane holds neuron j of J
// and TWO neurons k, k + 8 of K: per four words it forms w_j & w_k twice (one
// ds_read_b128 each of the three rows) and walks the 16 rows of I as broadcast
// ds_read_b128 into 2 x 16 register accumulators, v_and_b32 then
// v_bcnt_u32_b32, whose add is part of the instruction (the compiler folds the
// two ANDs into one v_bitop3_b32).  Two k per lane: with one, the 18 LDS reads
// per 128 vector instructions keep the LDS array busier than the SIMDs
// (MI355X_MICROARCH.md, LDS: a ds_read_b128 is 4 array cycles a wave); with two
// it is 19 per 256.
// Where the tile triples are few (84 at C = 102) the words are split over up to
// kTpMaxSplits workgroups per triple (tp_plan: a function of C and W alone);
// their 16^3 partial counts go to the workspace and a second launch adds them
// in split order and writes the outputs.  Integer sums: no atomics, nothing
// zeroed beforehand, every output written exactly once, the same bits every
// call.
//
// Who writes what.  Element (i, j, k) of triple (I, J, K), global neurons gi,
// gj, gk < C:
//   gi < gj < gk          triplets[rank(gi, gj, gk)]   (its tiles are sorted, so
//                         exactly one triple holds it)
//   J == K and gj == gk   the pair count of (gi, gj): for I < J both
//                         pairs[gi][gj] and pairs[gj][gi]; for I == J the one
//                         element pairs[gi][gj] (the triple holds both orders),
//                         and singles[gi] where gi == gj
// Everything else a diagonal triple computes is discarded: 10 % of the work at
// C = 512, half of it at C = 102.
#include "cg_common.h"

namespace {

constexpr int kTpTile = 16;
constexpr int kTpThreads = 128;
constexpr int kTpChunk = 64;             // words per LDS chunk
// LDS row: the chunk and one 16-byte slot, so that 16 rows read at one word
// offset by ds_read_b128 fall on 16 distinct slots of four banks
constexpr int kTpPitch = kTpChunk + 4;
static_assert(kTpPitch * 4 % 256 == 16, "row pitch one slot past a bank row");
constexpr int kTpTileElems = kTpTile * kTpTile * kTpTile;
constexpr int kTpMaxSplits = 64;
constexpr int kTpTargetItems = 2048;     // workgroups wanted before W is split less

// trial n, word w of neuron c: bins 32 w .. 32 w + 31 of the trial.  One thread
// per word, the neuron fastest so that the lanes of a wave read neighbouring
// channels; every element of the whole bins is read once.
__global__ __launch_bounds__(256) void binary_words_kernel(
    const float* __restrict__ trains, long long s_b, long long s_t, long long s_c,
    int C, int nb, int wpt, int bin, long long total, long long row_stride,
    unsigned* __restrict__ words) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total;
       e += gridDim.x * 256ll) {
    const int c = (int)(e % C);
    const long long r = e / C;
    const int w = (int)(r % wpt);
    const long long n = r / wpt;
    const float* p = trains + n * s_b + (long long)c * s_c;
    const int b_end = min(nb, 32 * w + 32);
    unsigned word = 0;
    for (int b = 32 * w; b < b_end; ++b) {
      const float* q = p + (long long)b * bin * s_t;
      bool any = false;
      for (int t = 0; t < bin; ++t) any |= q[(long long)t * s_t] != 0.f;
      word |= (any ? 1u : 0u) << (b & 31);
    }
    words[(long long)c * row_stride + n * wpt + w] = word;
  }
}

__host__ __device__ inline long long tp_choose3(long long n) {
  return n * (n - 1) * (n - 2) / 6;
}

// rank of i < j < k < C among the triplets in lexicographic order
__device__ __forceinline__ int tp_rank(int i, int j, int k, int C) {
  const int a = C - i, b = C - i - 1, c = C - j;
  return (int)(tp_choose3(C) - tp_choose3(a)) + b * (b - 1) / 2 -
         c * (c - 1) / 2 + (k - j - 1);
}

// item -> I <= J <= K, K outermost: (K + 1)(K + 2) / 2 triples end in K
__device__ __forceinline__ void tp_triple(int item, int& I, int& J, int& K) {
  K = 0;
  while (item >= (K + 1) * (K + 2) / 2) {
    item -= (K + 1) * (K + 2) / 2;
    ++K;
  }
  J = 0;
  while (item >= J + 1) {
    item -= J + 1;
    ++J;
  }
  I = item;
}

__device__ __forceinline__ void tp_emit(int I, int J, int K, int i, int j, int k,
                                        int v, int C, int* __restrict__ singles,
                                        int* __restrict__ pairs,
                                        int* __restrict__ triplets) {
  const int gi = I * kTpTile + i, gj = J * kTpTile + j, gk = K * kTpTile + k;
  if (gi >= C || gj >= C || gk >= C) return;
  if (gi < gj && gj < gk) {
    triplets[tp_rank(gi, gj, gk, C)] = v;
  } else if (gj == gk) {
    pairs[gi * C + gj] = v;
    if (I < J) pairs[gj * C + gi] = v;
    if (gi == gj) singles[gi] = v;
  }
}

// blockIdx.x = item * splits + split.  partial: [splits][items][16][16][16], or
// NULL with splits == 1, when the outputs are written here.
__global__ __launch_bounds__(kTpThreads) void triplet_counts_kernel(
    const unsigned* __restrict__ words, int C, int W, long long row_stride,
    int splits, int chunks_per_split, int* __restrict__ partial,
    int* __restrict__ singles, int* __restrict__ pairs,
    int* __restrict__ triplets) {
  __shared__ __attribute__((aligned(16))) unsigned sm[3][kTpTile][kTpPitch];
  const int item = blockIdx.x / splits, split = blockIdx.x - item * splits;
  int I, J, K;
  tp_triple(item, I, J, K);
  const int tiles[3] = {I, J, K};
  const int j = threadIdx.x >> 3, k0 = threadIdx.x & 7, k1 = k0 + 8;
  const int w_begin = split * chunks_per_split * kTpChunk;
  const int w_end = min(W, w_begin + chunks_per_split * kTpChunk);

  int acc0[kTpTile], acc1[kTpTile];
#pragma unroll
  for (int i = 0; i < kTpTile; ++i) acc0[i] = acc1[i] = 0;

  for (int w0 = w_begin; w0 < w_end; w0 += kTpChunk) {
    // 3 x 16 rows of 64 words; a neuron >= C and a word >= w_end are zeros and
    // are read from an address clamped into the matrix
    constexpr int kIters = 3 * kTpTile * kTpChunk / kTpThreads;
    unsigned v[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int idx = threadIdx.x + it * kTpThreads;
      const int row = idx / kTpChunk, w = idx % kTpChunk;
      const int c = tiles[row / kTpTile] * kTpTile + row % kTpTile;
      v[it] = words[(long long)min(c, C - 1) * row_stride + min(w0 + w, W - 1)];
      if (c >= C || w0 + w >= w_end) v[it] = 0u;
    }
    __syncthreads();  // the chunk before is read out
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int idx = threadIdx.x + it * kTpThreads;
      const int row = idx / kTpChunk, w = idx % kTpChunk;
      sm[row / kTpTile][row % kTpTile][w] = v[it];
    }
    __syncthreads();
    const int steps = (min(kTpChunk, w_end - w0) + 3) / 4;
    for (int s = 0; s < steps; ++s) {
      const uint4 a = *reinterpret_cast<const uint4*>(&sm[1][j][4 * s]);
      const uint4 b0 = *reinterpret_cast<const uint4*>(&sm[2][k0][4 * s]);
      const uint4 b1 = *reinterpret_cast<const uint4*>(&sm[2][k1][4 * s]);
      const unsigned m0[4] = {a.x & b0.x, a.y & b0.y, a.z & b0.z, a.w & b0.w};
      const unsigned m1[4] = {a.x & b1.x, a.y & b1.y, a.z & b1.z, a.w & b1.w};
#pragma unroll
      for (int i = 0; i < kTpTile; ++i) {
        const uint4 x4 = *reinterpret_cast<const uint4*>(&sm[0][i][4 * s]);
        const unsigned x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          acc0[i] += __builtin_popcount(x[h] & m0[h]);
          acc1[i] += __builtin_popcount(x[h] & m1[h]);
        }
      }
    }
  }

  if (partial != nullptr) {
    int* p = partial + ((long long)split * (gridDim.x / splits) + item) *
                           kTpTileElems + j * kTpTile;
#pragma unroll
    for (int i = 0; i < kTpTile; ++i) {
      p[i * kTpTile * kTpTile + k0] = acc0[i];
      p[i * kTpTile * kTpTile + k1] = acc1[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < kTpTile; ++i) {
      tp_emit(I, J, K, i, j, k0, acc0[i], C, singles, pairs, triplets);
      tp_emit(I, J, K, i, j, k1, acc1[i], C, singles, pairs, triplets);
    }
  }
}

// the splits' partial counts of one element of a tile triple, in split order;
// blockIdx.x = item * 16 + i, threadIdx.x = j * 16 + k
__global__ __launch_bounds__(256) void triplet_merge_kernel(
    const int* __restrict__ partial, int items, int splits, int C,
    int* __restrict__ singles, int* __restrict__ pairs,
    int* __restrict__ triplets) {
  const int item = blockIdx.x / kTpTile, i = blockIdx.x % kTpTile;
  int I, J, K;
  tp_triple(item, I, J, K);
  const int* p = partial + (long long)item * kTpTileElems +
                 i * kTpTile * kTpTile + threadIdx.x;
  int sum = 0;
  for (int s = 0; s < splits; ++s)
    sum += p[(long long)s * items * kTpTileElems];
  tp_emit(I, J, K, i, threadIdx.x / kTpTile, threadIdx.x % kTpTile, sum, C,
          singles, pairs, triplets);
}

struct TpPlan {
  int items, chunks_per_split, splits;
};
inline TpPlan tp_plan(int C, int W) {
  TpPlan p;
  const int nt = (C + kTpTile - 1) / kTpTile;
  p.items = nt * (nt + 1) * (nt + 2) / 6;
  const int nchunks = (W + kTpChunk - 1) / kTpChunk;
  int want = (kTpTargetItems + p.items - 1) / p.items;
  if (want > kTpMaxSplits) want = kTpMaxSplits;
  if (want > nchunks) want = nchunks;
  p.chunks_per_split = (nchunks + want - 1) / want;
  p.splits = (nchunks + p.chunks_per_split - 1) / p.chunks_per_split;
  return p;
}

inline bool tp_shape_ok(int C, long long W) {
  return C >= 3 && C <= CG_TRIPLET_MAX_C && W >= 1 && W <= CG_TRIPLET_MAX_WORDS;
}

inline bool tp_aligned(const void* p, uintptr_t to) {
  return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0;
}

}  // namespace

extern "C" int cg_binary_words(const float* trains, int B, int T, int C,
                               long long s_b, long long s_t, long long s_c,
                               int bin, void* words, long long row_stride,
                               void* stream) {
  if (!trains || !tp_aligned(words, 16) || B < 1 || T < 1 || bin < 1 || T < bin)
    return CG_EINVAL;
  const int nb = T / bin, wpt = (nb + 31) / 32;
  const long long W = (long long)B * wpt;
  if (!tp_shape_ok(C, W) || row_stride < W) return CG_EINVAL;
  const long long total = W * C;
  const long long blocks = (total + 255) / 256;
  const long long cap = 1ll << 20;
  hipLaunchKernelGGL(binary_words_kernel,
                     dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0,
                     cg_stream(stream), trains, s_b, s_t, s_c, C, nb, wpt, bin,
                     total, row_stride, static_cast<unsigned*>(words));
  CG_LAUNCH_CHECK();
}

extern "C" long long cg_triplet_counts_ws_bytes(int C, int W) {
  if (!tp_shape_ok(C, W)) return -1;
  const TpPlan p = tp_plan(C, W);
  if (p.splits == 1) return 16;
  return (long long)p.splits * p.items * kTpTileElems * 4;
}

extern "C" int cg_triplet_counts(const void* words, int C, int W,
                                 long long row_stride, int* singles, int* pairs,
                                 int* triplets, void* ws, void* stream) {
  if (!tp_aligned(words, 16) || !tp_aligned(ws, 16) || !tp_aligned(singles, 4) ||
      !tp_aligned(pairs, 4) || !tp_aligned(triplets, 4) || !tp_shape_ok(C, W) ||
      row_stride < W)
    return CG_EINVAL;
  const TpPlan p = tp_plan(C, W);
  hipStream_t st = cg_stream(stream);
  int* partial = p.splits > 1 ? static_cast<int*>(ws) : nullptr;
  hipLaunchKernelGGL(triplet_counts_kernel, dim3((unsigned)(p.items * p.splits)),
                     dim3(kTpThreads), 0, st,
                     static_cast<const unsigned*>(words), C, W, row_stride,
                     p.splits, p.chunks_per_split, partial, singles, pairs,
                     triplets);
  if (partial != nullptr)
    hipLaunchKernelGGL(triplet_merge_kernel, dim3((unsigned)(p.items * kTpTile)),
                       dim3(256), 0, st, partial, p.items, p.splits, C, singles,
                       pairs, triplets);
  CG_LAUNCH_CHECK();
}
