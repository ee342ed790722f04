// Victor-Purpura edit distances between the binary trains of a trial (DESIGN.md
// 13; spike_metrics.victor_purpura_distance_frames is the numpy statement).
//
//   G[k][0] = k, G[0][l] = l,
//   G[k][l] = min(G[k-1][l] + 1, G[k][l-1] + 1,
//                 G[k-1][l-1] + fl(qf |f_a[k-1] - f_b[l-1]|)),   D_ab = G[n_a][n_b]
//
// on the ascending frame indices f of the non-zero entries of each train, every
// operation rounded to float64 on its own.  The programme only adds and takes
// minima of non-NaN values, so any traversal of the cells gives the statement's
// bits.  Two launches:
//
//  vp_compact_kernel  one wave per train walks T in steps of 64 frames; the
//                     ballot of v != 0 and a prefix popcount place the frame
//                     indices (uint16, pitch T) and the count in the workspace.
//                     It also writes the zero diagonal.
//  vp_pairs_kernel    one 16-lane DPP row per pair (i < j), four pairs per wave,
//                     a fixed grid of row slots that walks the pairs.  The
//                     shorter train lies along the lanes in strips of 16
//                     columns, the longer one along the steps.  A strip is swept
//                     skewed: at step t lane c works on row k = t - c + 1 of its
//                     column.  It keeps its own previous value (G[k-1][l]),
//                     receives G[k][l-1] and the frame f_a[k-1] from lane c - 1
//                     by row_shr:1, and last step's received value is
//                     G[k-1][l-1].  Lane 0 receives the previous strip's last
//                     column (k itself in the first strip), lane 15 hands its
//                     column on.  That boundary column (n_a + 1 float64) lives
//                     in the slot's workspace line, not in LDS (at T = 2048 it
//                     would be 16 KB a pair): it moves 16 values at a time
//                     through a 16-entry LDS ring per row, one load issued a
//                     block of 16 steps ahead and one store per block.  A
//                     strip's store of row k follows its own load of row k by
//                     data dependence (the load was consumed a block earlier),
//                     so the line is updated in place.  The frames of the longer
//                     train travel through the same ring.
//
// No atomics, nothing zeroed beforehand, no hipMemset: the same bits every call.
// The mirrored element (j, i) is a second store of the same register.
#include "cg_common.h"

namespace {

constexpr int kVpThreads = 256;
constexpr int kVpRows = kVpThreads / 16;  // pairs in flight per workgroup
// workgroups of the pair kernel at most: two per CU of an MI355X (8 waves a CU);
// the workspace holds one boundary line per row slot
constexpr int kVpMaxGroups = 512;
constexpr int kVpMaxB = 65536;
constexpr int kVpMaxT = 16384;  // frame indices are uint16
constexpr int kVpMaxC = 4096;

// workspace: [slots][T + 1] float64 boundary lines, [B C] int32 counts,
// [B C][T] uint16 frame indices -- in this order, so that nothing needs padding
struct VpLayout {
  long long pairs, groups, bnd_pitch, off_counts, off_frames, bytes;
};
inline VpLayout vp_layout(int B, int T, int C) {
  VpLayout L;
  L.pairs = (long long)B * C * (C - 1) / 2;
  L.groups = (L.pairs + kVpRows - 1) / kVpRows;
  if (L.groups > kVpMaxGroups) L.groups = kVpMaxGroups;
  L.bnd_pitch = (long long)T + 1;
  L.off_counts = L.groups * kVpRows * L.bnd_pitch * 8;
  L.off_frames = L.off_counts + (long long)B * C * 4;
  L.bytes = L.off_frames + (long long)B * C * T * 2;
  return L;
}
inline bool vp_shape_ok(int B, int T, int C) {
  return B >= 1 && T >= 1 && C >= 1 && B <= kVpMaxB && T <= kVpMaxT && C <= kVpMaxC;
}

__global__ __launch_bounds__(kVpThreads) void vp_compact_kernel(
    const float* __restrict__ spikes, long long s_b, long long s_t, long long s_c,
    int B, int T, int C, unsigned short* __restrict__ frames,
    int* __restrict__ counts, double* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const long long train = (long long)blockIdx.x * (kVpThreads / 64) + (threadIdx.x >> 6);
  if (train >= (long long)B * C) return;  // (the whole wave)
  const long long b = train / C, c = train % C;
  const float* p = spikes + b * s_b + c * s_c;
  unsigned short* out = frames + train * T;
  int cnt = 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const bool sp = t < T && p[(long long)t * s_t] != 0.f;
    const unsigned long long m = __ballot(sp);
    if (sp) out[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)t;
    cnt += __popcll(m);
  }
  if (lane == 0) {
    counts[train] = cnt;
    dist[(b * C + c) * C + c] = 0.0;
  }
}

// lane c of a 16-lane row receives `v` of lane c - 1; lane 0 keeps `first`
__device__ __forceinline__ int vp_shr1(int v, int first) {
  return __builtin_amdgcn_update_dpp(first, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ double vp_shr1(double v, double first) {
  const int lo = vp_shr1(__double2loint(v), __double2loint(first));
  const int hi = vp_shr1(__double2hiint(v), __double2hiint(first));
  return __hiloint2double(hi, lo);
}
// max over the four rows of a wave of a value that is uniform within a row
__device__ __forceinline__ int vp_rows_max(int v) {
  const int a = max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
  const int b = max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48));
  return max(a, b);
}

__global__ __launch_bounds__(kVpThreads) void vp_pairs_kernel(
    const unsigned short* __restrict__ frames, const int* __restrict__ counts,
    double* bnd, long long bnd_pitch, int T, int C, long long per_trial,
    long long npairs, double qf, double* __restrict__ dist) {
  __shared__ double sm_in[kVpRows][16];   // boundary column, this block's 16 rows
  __shared__ int sm_f[kVpRows][16];       // frames of the long train, likewise
  __shared__ double sm_out[kVpRows][16];  // lane 15's column, this block's steps
  const int c = threadIdx.x & 15;
  const int row = threadIdx.x >> 4;
  const long long nslots = (long long)gridDim.x * kVpRows;
  const long long slot = (long long)blockIdx.x * kVpRows + row;
  double* line = bnd + slot * bnd_pitch;

  // the four rows of a wave take four consecutive pairs; the loop is uniform
  // over the wave, rows without a pair idle under masks
  for (long long p0 = slot - (row & 3); p0 < npairs; p0 += nslots) {
    const long long p = p0 + (row & 3);
    const bool have = p < npairs;
    int na = 0, nb = 0;  // spikes of the longer / the shorter train
    const unsigned short *fa = frames, *fb = frames;
    long long o_ij = 0, o_ji = 0;
    if (have) {
      const long long b = p / per_trial;
      const int r = (int)(p - b * per_trial);
      // r -> (i, j), i < j, row by row: row i starts at i (2 C - 1 - i) / 2
      const double w = 2.0 * C - 1.0;
      int i = (int)((w - sqrt(w * w - 8.0 * r)) * 0.5);
      i = min(max(i, 0), C - 2);
      while (i + 1 <= C - 2 && (long long)(i + 1) * (2 * C - 2 - i) / 2 <= r) ++i;
      while (i > 0 && (long long)i * (2 * C - 1 - i) / 2 > r) --i;
      const int j = i + 1 + (r - (int)((long long)i * (2 * C - 1 - i) / 2));
      const long long ti = b * C + i, tj = b * C + j;
      const int ni = counts[ti], nj = counts[tj];
      const bool swap = nj > ni;
      na = swap ? nj : ni;
      nb = swap ? ni : nj;
      fa = frames + (swap ? tj : ti) * T;
      fb = frames + (swap ? ti : tj) * T;
      o_ij = ti * C + j;
      o_ji = tj * C + i;
    }
    const int strips = (nb + 15) >> 4;
    double res = (double)na;  // nb == 0: the other count, without a sweep
    const int max_strips = vp_rows_max(strips);
    for (int s = 0; s < max_strips; ++s) {
      const bool on = s < strips;
      const bool carry_in = s > 0, carry_out = on && s + 1 < strips;
      const int l = 16 * s + c + 1;  // this lane's column
      const int fbv = (on && l <= nb) ? (int)fb[l - 1] : 0;
      double up = (double)l;          // G[k-1][l], G[0][l] first
      double diag = (double)(l - 1);  // G[k-1][l-1]
      double cur = up;                // what lane c + 1 receives next step
      int fcur = 0;
      const int nblk = (vp_rows_max(on ? na + 15 : 0) + 15) >> 4;
      // rows t0 + 1 + c of the boundary and frames t0 + c, a block ahead
      double pre_g = 0.0;
      int pre_f = 0;
      if (on) {
        if (c < na) pre_f = fa[c];
        if (carry_in && c + 1 <= na) pre_g = line[c + 1];
      }
      for (int blk = 0; blk < nblk; ++blk) {
        const int t0 = blk * 16;
        if (on) {
          sm_in[row][c] = pre_g;
          sm_f[row][c] = pre_f;
          const int idx = t0 + 16 + c;
          pre_f = idx < na ? (int)fa[idx] : 0;
          pre_g = (carry_in && idx + 1 <= na) ? line[idx + 1] : 0.0;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int tt = 0; tt < 16; ++tt) {
          const int t = t0 + tt;
          const int k = t - c + 1;
          const double first = carry_in ? sm_in[row][tt] : (double)(t + 1);
          // (the moves stay outside the branch: a lane reads its neighbour
          // whether or not either of them has a cell this step)
          const double left = vp_shr1(cur, first);
          fcur = vp_shr1(fcur, sm_f[row][tt]);
          if (on && k >= 1 && k <= na) {
#pragma clang fp contract(off)
            const double d = (double)abs(fcur - fbv);
            double shift = qf * d;
            shift = diag + shift;
            const double v = fmin(fmin(up + 1.0, left + 1.0), shift);
            up = v;
            cur = v;
            diag = left;
          }
          if (carry_out && c == 15) sm_out[row][tt] = cur;
        }
        __builtin_amdgcn_wave_barrier();
        if (carry_out) {
          const int k = t0 + c - 14;  // lane 15's row at step t0 + c
          if (k >= 1 && k <= na) line[k] = sm_out[row][c];
        }
      }
      if (on && s + 1 == strips) res = up;  // G[na][l]
      // the next strip's loads see this strip's stores (other lanes of the wave)
      __threadfence_block();
    }
    if (have && c == (nb > 0 ? (nb - 1) & 15 : 0)) {
      dist[o_ij] = res;
      dist[o_ji] = res;
    }
  }
}

}  // namespace

extern "C" long long cg_victor_purpura_ws_bytes(int B, int T, int C) {
  if (!vp_shape_ok(B, T, C)) return -1;
  return vp_layout(B, T, C).bytes;
}

extern "C" int cg_victor_purpura(const float* spikes, int B, int T, int C,
                                 long long s_b, long long s_t, long long s_c,
                                 double qf, double* dist, void* ws,
                                 long long ws_bytes, void* stream) {
  if (!spikes || !dist || !ws || !vp_shape_ok(B, T, C) || !(qf >= 0.0))
    return CG_EINVAL;
  const VpLayout L = vp_layout(B, T, C);
  if (ws_bytes < L.bytes || (reinterpret_cast<uintptr_t>(ws) & 7)) return CG_EINVAL;
  char* base = static_cast<char*>(ws);
  double* bnd = reinterpret_cast<double*>(base);
  int* counts = reinterpret_cast<int*>(base + L.off_counts);
  unsigned short* frames = reinterpret_cast<unsigned short*>(base + L.off_frames);
  const long long trains = (long long)B * C;
  const int waves = kVpThreads / 64;
  hipLaunchKernelGGL(vp_compact_kernel, dim3((unsigned)((trains + waves - 1) / waves)),
                     dim3(kVpThreads), 0, cg_stream(stream), spikes, s_b, s_t, s_c, B, T,
                     C, frames, counts, dist);
  if (L.pairs > 0)
    hipLaunchKernelGGL(vp_pairs_kernel, dim3((unsigned)L.groups), dim3(kVpThreads), 0,
                       cg_stream(stream), frames, counts, bnd, L.bnd_pitch, T, C,
                       (long long)C * (C - 1) / 2, L.pairs, qf, dist);
  CG_LAUNCH_CHECK();
}
