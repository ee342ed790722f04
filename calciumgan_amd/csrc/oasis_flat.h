/* One trace of OASIS AR(1) with s_min as ONE flat loop -- the form the batched
 * device kernel (spikes.hip) runs per lane, compiled for the host too
 * (oasis_ar1.c: cg_oasis_ar1_flat) so that a CPU build can be checked against
 * cg_oasis_ar1 bit for bit.
 *
 * Same pools (v, w, l) and the same float64 operations in the same order as
 * cg_oasis_ar1 with lam = 0 (a pool's start time is the sum of the lengths below
 * it, so t is not stored).  Differences of form only:
 *   - an iteration either merges the top pool into the one below or takes the
 *     next frame (lanes of a wave that merge different numbers of times stay in
 *     the same loop body);
 *   - the top pool and the two below it live in registers with their quotient
 *     r = v / w and their power p = g^l; the stack below the top is in memory
 *     at sv / sw / sl[depth * sstride] (interleaved by trace on the device);
 *   - g^l comes from a table filled by the host's pow (cg_oasis_pow_table):
 *     device pow and glibc pow are different functions;
 *   - c is not kept: s[t] = c[t] - g c[t-1] is formed while the pools are
 *     walked.
 * No fused multiply-add may be formed here (the host library is plain x86-64
 * code without FMA): contraction is switched off for this function only.
 *
 * Termination: an iteration merges (at most T - 1 times in all: every merge
 * removes a pool a frame opened), takes a frame (T - 1 times) or leaves; a NaN
 * compares false and takes a frame.  The loop is bounded by 2 T besides.
 */
#ifndef CG_OASIS_FLAT_H_
#define CG_OASIS_FLAT_H_

#if defined(__HIPCC__)
#define CG_OASIS_FN __device__ __forceinline__
#else
#define CG_OASIS_FN static inline
#endif

typedef struct {
  double v, w; /* value sum, weight sum */
  double r, p; /* v / w, g^l */
  int l;       /* frames */
} cg_oasis_pool;

/* y[t] = (double)(x[t] * scale + offset), the product and the sum rounded to
 * float32 one after the other (utils.denormalize on a float32 array) */
CG_OASIS_FN double cg_oasis_frame(const float* x, long long sx_t, int t,
                                  int affine, float scale, float offset) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float a = x[(long long)t * sx_t];
  if (affine) {
    a = a * scale;
    a = a + offset;
  }
  return (double)a;
}

/* x: frames at stride sx_t.  gpow[0 .. T]: g^l by the host's pow.  Stack: T
 * entries per trace at stride sstride.  spikes at stride so_t; c_out / s_out
 * (T contiguous doubles each) may be null. */
CG_OASIS_FN void cg_oasis_flat(const float* x, long long sx_t, int affine,
                               float scale, float offset, int T, double g,
                               double s_min, double threshold,
                               const double* gpow, double* sv, double* sw,
                               int* sl, long long sstride, float* spikes,
                               long long so_t, double* c_out, double* s_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p1 = gpow[1];
  cg_oasis_pool top, prev, prev2;
  top.v = cg_oasis_frame(x, sx_t, 0, affine, scale, offset);
  top.w = 1.0;
  top.r = top.v; /* v / 1 */
  top.p = p1;
  top.l = 1;
  prev = top;  /* (valid from depth 1) */
  prev2 = top; /* (valid from depth 2) */
  int i = 0;   /* stack index of the top pool */
  int t = 1;   /* next frame */
  double ynext = T > 1 ? cg_oasis_frame(x, sx_t, 1, affine, scale, offset) : 0.0;
  for (int it = 0; it < 2 * T; ++it) {
    if (i > 0 && prev.r * prev.p + s_min > top.r) {
      const double gl = prev.p;
      top.v = prev.v + top.v * gl;
      top.w = prev.w + top.w * gl * gl;
      top.l = prev.l + top.l;
      top.r = top.v / top.w;
      top.p = gpow[top.l];
      --i;
      prev = prev2;
      if (i >= 2) {
        const long long o = (long long)(i - 2) * sstride;
        prev2.v = sv[o];
        prev2.w = sw[o];
        prev2.l = sl[o];
        prev2.r = prev2.v / prev2.w;
        prev2.p = gpow[prev2.l];
      }
    } else {
      if (t >= T) break;
      const long long o = (long long)i * sstride; /* i <= T - 2 here */
      sv[o] = top.v;
      sw[o] = top.w;
      sl[o] = top.l;
      prev2 = prev;
      prev = top;
      top.v = ynext;
      top.w = 1.0;
      top.r = ynext;
      top.p = p1;
      top.l = 1;
      ++i;
      ++t;
      if (t < T) ynext = cg_oasis_frame(x, sx_t, t, affine, scale, offset);
    }
  }
  /* pools 0 .. i - 1 are in the stack, pool i is `top` */
  int j = 0, k = 0;
  int len = i == 0 ? top.l : sl[0];
  double tmp = i == 0 ? top.r : sv[0] / sw[0];
  if (tmp < 0.0) tmp = 0.0;
  double cprev = 0.0;
  for (t = 0; t < T; ++t) {
    if (k == len && j < i) {
      ++j;
      if (j == i) {
        len = top.l;
        tmp = top.r;
      } else {
        const long long o = (long long)j * sstride;
        len = sl[o];
        tmp = sv[o] / sw[o];
      }
      if (tmp < 0.0) tmp = 0.0;
      k = 0;
    }
    const double c = tmp;
    const double s = t == 0 ? 0.0 : c - g * cprev;
    spikes[(long long)t * so_t] = s > threshold ? 1.0f : 0.0f;
    if (c_out) c_out[t] = c;
    if (s_out) s_out[t] = s;
    cprev = c;
    tmp = tmp * g;
    ++k;
  }
}

#endif /* CG_OASIS_FLAT_H_ */
