// Inter-spike intervals and spike counts of packed spike trains (DESIGN.md 27;
// spike_metrics.interval_counts is the numpy statement).
//
// A train is one neuron in one trial: wpt words as cg_binary_words writes them
// at bin = 1, bit t % 32 of word t / 32 the frame t.  With its spikes at t_1 <
// ... < t_m and I_k = t_{k+1} - t_k, a neuron's outputs are sums over its
// trains: the histogram of the I_k (bins 1 .. max_isi and one overflow bin),
// the six moments (spikes, intervals, sum I, sum I^2, consecutive pairs, sum
// I_k I_{k+1}) and the spikes of every train.
//
// A workgroup of kIvThreads = 256 owns one neuron and a run of trials; each of
// its four waves takes a trial at a time and walks it in chunks of kIvChunk =
// 64 words, a word a lane (one coalesced 256-byte read).  A lane needs the two
// spikes before its word.  No scan is run for them: the ballot of the
// non-empty words gives every lane the nearest non-empty lane below it by
// count-leading-zeros, and three ds_bpermute reads fetch
//   p1 = that lane's last spike
//   p2 = that lane's second-to-last spike where it holds two, else ITS p1
// -- the associative combine of (count, last, second-to-last) summaries,
// unrolled: only a non-empty lane is ever asked, so one step back reaches the
// answer.  Below the lowest non-empty lane the chunk's carry (last, second to
// last of the trial so far; -1 where there is none, reset per trial) stands in,
// and the highest non-empty lane leaves the next carry.  Then the lane walks
// its set bits with count-trailing-zeros: an integer add into the neuron's
// histogram in LDS (ds_add_u32: the order cannot matter) and int64 register
// sums.
// Where the neurons are few the trials are split over up to kIvMaxSplits
// workgroups a neuron (iv_plan: a function of C and the trials alone); their
// histograms and moments go to the workspace and a second launch adds them in
// split order.  counts[n][c] has one owner either way.  No global atomics,
// nothing zeroed beforehand, every output written exactly once, the same bits
// every call.
#include "cg_common.h"

namespace {

constexpr int kIvThreads = 256;
constexpr int kIvWaves = kIvThreads / 64;
constexpr int kIvChunk = 64;             // words of a trial a wave reads at once
constexpr int kIvMoments = 6;
constexpr int kIvMaxSplits = 64;
// workgroups the grid is held to while the trials are split: one round of the 8
// a CU that the 16.5 KB of LDS and 51 registers admit, on 256 CUs -- a wave's
// chunks are a chain of load, ballot and cross-lane reads, so the time is
// latency over waves, and a second round costs more than it spreads
constexpr int kIvTargetItems = 2048;

// blockIdx.x = c * splits + split.  part_hist [splits][C][H] and part_mom
// [splits][C][6], or NULL with splits == 1, when the outputs are written here.
__global__ __launch_bounds__(kIvThreads) void spike_intervals_kernel(
    const unsigned* __restrict__ words, int C, int trials, int wpt,
    long long row_stride, int max_isi, int splits, int trials_per_split,
    int* __restrict__ part_hist, long long* __restrict__ part_mom,
    int* __restrict__ hist, long long* __restrict__ moments,
    int* __restrict__ counts) {
  __shared__ int sh_hist[CG_INTERVAL_MAX_ISI + 1];
  __shared__ long long sh_fold[kIvMoments][kIvWaves];
  const int c = blockIdx.x / splits, split = blockIdx.x - c * splits;
  const int H = max_isi + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < H; d += kIvThreads) sh_hist[d] = 0;
  __syncthreads();

  const int n_begin = split * trials_per_split;
  const int n_end = min(trials, n_begin + trials_per_split);
  const unsigned* row = words + (long long)c * row_stride;
  // lanes below this one
  const unsigned long long below = (1ull << lane) - 1ull;

  long long acc[kIvMoments] = {0, 0, 0, 0, 0, 0};
  for (int n = n_begin + wave; n < n_end; n += kIvWaves) {
    const unsigned* trial = row + (long long)n * wpt;
    int carry1 = -1, carry2 = -1;   // last and second-to-last spike so far
    int spikes = 0;
    for (int w0 = 0; w0 < wpt; w0 += kIvChunk) {
      const int w = w0 + lane;
      unsigned word = w < wpt ? trial[w] : 0u;
      const unsigned long long mask = __ballot(word != 0u);
      if (mask == 0ull) continue;   // (wave-uniform)
      const int base = w * 32;
      const int cnt = __builtin_popcount(word);
      // own last and second-to-last spike; -1 where there is none
      int last = -1, second = -1;
      if (word != 0u) {
        const int top = 31 - __builtin_clz(word);
        last = base + top;
        const unsigned rest = word & ~(1u << top);
        if (rest != 0u) second = base + 31 - __builtin_clz(rest);
      }
      const unsigned long long lower = mask & below;
      const int src = lower != 0ull ? 63 - __builtin_clzll(lower) : 0;
      const int got1 = __shfl(last, src, 64);
      int p1 = lower != 0ull ? got1 : carry1;
      // what a lane above is told of this one's second-to-last spike
      const int out2 = cnt >= 2 ? second : p1;
      const int got2 = __shfl(out2, src, 64);
      int p2 = lower != 0ull ? got2 : carry2;
      const int top_lane = 63 - __builtin_clzll(mask);
      carry1 = __shfl(last, top_lane, 64);
      carry2 = __shfl(out2, top_lane, 64);

      spikes += cnt;
      while (word != 0u) {
        const int t = base + __builtin_ctz(word);
        word &= word - 1u;
        if (p1 >= 0) {
          const long long I = t - p1;
          atomicAdd(&sh_hist[(int)min(I, (long long)H) - 1], 1);
          acc[1] += 1;
          acc[2] += I;
          acc[3] += I * I;
          if (p2 >= 0) {
            acc[4] += 1;
            acc[5] += I * (long long)(p1 - p2);
          }
        }
        p2 = p1;
        p1 = t;
      }
    }
    acc[0] += spikes;
    spikes = wave_fold(spikes);
    if (lane == 0) counts[(long long)n * C + c] = spikes;
  }

  block_fold_put<kIvMoments>(acc, &sh_fold[0][wave], kIvWaves);
  __syncthreads();   // the histogram and the waves' sums are in LDS
  int* h_out = part_hist != nullptr
                   ? part_hist + ((long long)split * C + c) * H
                   : hist + (long long)c * H;
  for (int d = threadIdx.x; d < H; d += kIvThreads) h_out[d] = sh_hist[d];
  if (threadIdx.x < kIvMoments) {
    long long* m_out = part_mom != nullptr
                           ? part_mom + ((long long)split * C + c) * kIvMoments
                           : moments + (long long)c * kIvMoments;
    m_out[threadIdx.x] = block_fold_get<kIvWaves>(&sh_fold[threadIdx.x][0]);
  }
}

// the splits' partial results of one neuron, in split order; blockIdx.x = c
__global__ __launch_bounds__(kIvThreads) void spike_intervals_merge_kernel(
    const int* __restrict__ part_hist, const long long* __restrict__ part_mom,
    int C, int H, int splits, int* __restrict__ hist,
    long long* __restrict__ moments) {
  const int c = blockIdx.x;
  for (int d = threadIdx.x; d < H; d += kIvThreads) {
    int sum = 0;
    for (int s = 0; s < splits; ++s)
      sum += part_hist[((long long)s * C + c) * H + d];
    hist[(long long)c * H + d] = sum;
  }
  if (threadIdx.x < kIvMoments) {
    long long sum = 0;
    for (int s = 0; s < splits; ++s)
      sum += part_mom[((long long)s * C + c) * kIvMoments + threadIdx.x];
    moments[(long long)c * kIvMoments + threadIdx.x] = sum;
  }
}

struct IvPlan {
  int trials_per_split, splits;
  long long hist_bytes;   // of the partial histograms, the moments behind them
};
inline IvPlan iv_plan(int C, int trials, int max_isi) {
  IvPlan p;
  int want = kIvTargetItems / C;
  if (want < 1) want = 1;
  if (want > kIvMaxSplits) want = kIvMaxSplits;
  // a wave a trial: a split of fewer than kIvWaves trials leaves waves idle
  const int most = (trials + kIvWaves - 1) / kIvWaves;
  if (want > most) want = most;
  p.trials_per_split = (trials + want - 1) / want;
  p.splits = (trials + p.trials_per_split - 1) / p.trials_per_split;
  const long long bytes = (long long)p.splits * C * (max_isi + 1) * 4;
  p.hist_bytes = (bytes + 15) / 16 * 16;
  return p;
}

inline bool iv_shape_ok(int C, int trials, int wpt, int max_isi) {
  return C >= 1 && C <= CG_INTERVAL_MAX_C && trials >= 1 && wpt >= 1 &&
         (long long)trials * wpt <= CG_TRIPLET_MAX_WORDS && max_isi >= 1 &&
         max_isi <= CG_INTERVAL_MAX_ISI;
}

inline bool iv_aligned(const void* p, uintptr_t to) {
  return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0;
}

}  // namespace

extern "C" long long cg_spike_intervals_ws_bytes(int C, int trials, int wpt,
                                                 int max_isi) {
  if (!iv_shape_ok(C, trials, wpt, max_isi)) return -1;
  const IvPlan p = iv_plan(C, trials, max_isi);
  if (p.splits == 1) return 16;
  return p.hist_bytes + (long long)p.splits * C * kIvMoments * 8;
}

extern "C" int cg_spike_intervals(const void* words, int C, int trials, int wpt,
                                  long long row_stride, int max_isi, int* hist,
                                  long long* moments, int* counts, void* ws,
                                  void* stream) {
  if (!iv_aligned(words, 16) || !iv_aligned(ws, 16) || !iv_aligned(hist, 4) ||
      !iv_aligned(counts, 4) || !iv_aligned(moments, 8) ||
      !iv_shape_ok(C, trials, wpt, max_isi) ||
      row_stride < (long long)trials * wpt)
    return CG_EINVAL;
  const IvPlan p = iv_plan(C, trials, max_isi);
  hipStream_t st = cg_stream(stream);
  int* part_hist = p.splits > 1 ? static_cast<int*>(ws) : nullptr;
  long long* part_mom =
      p.splits > 1 ? reinterpret_cast<long long*>(static_cast<char*>(ws) +
                                                  p.hist_bytes)
                   : nullptr;
  hipLaunchKernelGGL(spike_intervals_kernel, dim3((unsigned)(C * p.splits)),
                     dim3(kIvThreads), 0, st,
                     static_cast<const unsigned*>(words), C, trials, wpt,
                     row_stride, max_isi, p.splits, p.trials_per_split,
                     part_hist, part_mom, hist, moments, counts);
  if (part_hist != nullptr)
    hipLaunchKernelGGL(spike_intervals_merge_kernel, dim3((unsigned)C),
                       dim3(kIvThreads), 0, st, part_hist, part_mom, C,
                       max_isi + 1, p.splits, hist, moments);
  CG_LAUNCH_CHECK();
}
