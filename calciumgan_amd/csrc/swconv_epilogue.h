// The output tails of the cg_swconv kernels, each rule stated once: the
// pointwise epilogues over the eight consecutive values a lane stores, the row
// target of the output-side PhaseShuffle adjoint, the fused LayerNorm row and
// the commit of a workgroup's share of the penalty norm.  Included by swconv.hip
// and swconv_swp.hip only.  Every function is a pure function of its arguments
// (the software-pipelined epilogues re-derive their lane ids and keep no
// register alive across the K loop: nothing here may capture kernel state).
// How the eight values reach a lane, where bias / gamma / beta are read from,
// the cross-lane sums, the barriers and the stores stay with the kernels.
// tests/swconv_ref.py is the float64 statement of the same rules.
#pragma once
#include "swconv_args.h"

// LeakyReLU
__device__ __forceinline__ void epi_lrelu8(float (&v)[8], float alpha) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], alpha * v[e]);
}

// With an output shift the gradient is rounded to the activation type before it
// is masked: the unfused form stores it in that type and cg_unshuffle masks what
// it reads back.
__device__ __forceinline__ void epi_round8(float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = act2f(f2act(v[e]));
}

// LeakyReLU' from the mask source's eight activations (four packed words): > 0
// alone selects 1, everything else -- -0, +0, NaN -- the slope.
__device__ __forceinline__ void epi_mask8(float (&v)[8], uint32_t h0, uint32_t h1,
                                          uint32_t h2, uint32_t h3, float alpha,
                                          bool round_first) {
  const uint32_t hw[4] = {h0, h1, h2, h3};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (round_first) v[e] = act2f(f2act(v[e]));  // (epi_round8, element by element)
    const uint16_t hv = (uint16_t)(hw[e >> 1] >> ((e & 1) * 16));
    v[e] *= (act2f(hv) > 0.f) ? 1.f : alpha;
  }
}

__device__ __forceinline__ void epi_sigmoid8(float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = 1.f / (1.f + __expf(-v[e]));
}

// The run-time selection among CG_EPI_NONE / LRELU / MASK / SIGMOID.  to_side: a
// reflected row of the output shift, which goes unmasked to the side buffer;
// out_shifts: the launch's output shifts or null (non-null: round first);
// mask_words() gives the row's four packed words and is only called when the
// mask applies (a load inside it stays conditional).  SIGMOID = false leaves
// the branch out where the host refuses it (split-K).
template <bool SIGMOID = true, class MaskWords>
__device__ __forceinline__ void epi_apply8(float (&v)[8], int epilogue, float alpha,
                                           bool to_side, const int* out_shifts,
                                           MaskWords&& mask_words) {
  if (epilogue == CG_EPI_LRELU) {
    epi_lrelu8(v, alpha);
  } else if (epilogue == CG_EPI_MASK && !to_side) {
    if (out_shifts) epi_round8(v);
    const uint4 h = mask_words();
    epi_mask8(v, h.x, h.y, h.z, h.w, alpha, false);
  } else if (SIGMOID && epilogue == CG_EPI_SIGMOID) {
    epi_sigmoid8(v);
  }
}

// channel padding [N, Cy) stays exactly zero: v[0..3] are columns n0 .., v[4..7]
// columns n4 .. (n0 + 4 unless an f32 store splits the eight in two groups)
__device__ __forceinline__ void epi_zero_pad8(float (&v)[8], int n0, int n4, int N) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (n0 + e >= N) v[e] = 0.f;
    if (n4 + e >= N) v[4 + e] = 0.f;
  }
}
__device__ __forceinline__ void epi_zero_pad8(float (&v)[8], int n0, int N) {
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (n0 + e >= N) v[e] = 0.f;
}

// the penalty norm squares the f32 epilogue result BEFORE the store's rounding
__device__ __forceinline__ void epi_add_squares8(const float (&v)[8], float& ssq) {
#pragma unroll
  for (int e = 0; e < 8; ++e) ssq += v[e] * v[e];
}

// eight values as one 16-byte store of the activation type
__device__ __forceinline__ uint4 epi_pack8(const float (&v)[8]) {
  return make_uint4(pack2act(v[0], v[1]), pack2act(v[2], v[3]), pack2act(v[4], v[5]),
                    pack2act(v[6], v[7]));
}

// Output-side PhaseShuffle adjoint (cg_conv_desc.out_shifts): row t of a sample
// of Ly rows lands on t + s, except the |s| rows that the reflection folds back
// -- the last s for s > 0, the first |s| for s < 0 -- which go to row
// t - (Ly - s) / t of the side buffer.  (Ly by reference: a kernel then reads it
// from its argument block where the rule does, inside the s > 0 branch; read
// ahead of the call it costs the LayerNorm instantiations of the
// software-pipelined kernel two VGPRs and with them an occupancy step.)
__device__ __forceinline__ int out_shift_row(int t, int s, const int& Ly, bool& to_side) {
  if (s > 0) {
    to_side = t >= Ly - s;
    return to_side ? t - (Ly - s) : t + s;
  }
  to_side = t < -s;
  return to_side ? t : t + s;
}
// (the predicate alone)
__device__ __forceinline__ bool out_shift_reflected(int t, int s, const int& Ly) {
  bool to_side;
  out_shift_row(t, s, Ly, to_side);
  return to_side;
}

// Fused LayerNorm row, step 1: statistics of the STORED pre-activation (rounded
// to the activation type), as the separate cg_ln_lrelu_fwd pass sees it.  v
// becomes the rounded values (0 past N), s1 / s2 gain their sum and squares.
__device__ __forceinline__ void ln_row_stats8(float (&v)[8], const float (&bv)[8],
                                              int n0, int N, float& s1, float& s2) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v[e] = n0 + e < N ? act2f(f2act(v[e] + bv[e])) : 0.f;
    s1 += v[e];
    s2 += v[e] * v[e];
  }
}
// step 2: mean and reciprocal standard deviation from the row's joined sums
__device__ __forceinline__ void ln_row_moments(float s1, float s2, float invn, float eps,
                                               float& mean, float& rstd) {
  mean = s1 * invn;
  const float var = fmaxf(s2 * invn - mean * mean, 0.f);
  rstd = rsqrtf(var + eps);
}
// step 3: normalise, affine, LeakyReLU.  (channel padding stays +0 whatever the
// row holds: with NaN / inf statistics the zero gamma / beta of a padding column
// give NaN)
__device__ __forceinline__ void ln_row_act8(const float (&v)[8], float (&hv)[8], float mean,
                                            float rstd, const f32x4& g0, const f32x4& g1,
                                            const f32x4& b0, const f32x4& b1, int n0, int N,
                                            float alpha) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t =
        (v[e] - mean) * rstd * (e < 4 ? g0[e] : g1[e - 4]) + (e < 4 ? b0[e] : b1[e - 4]);
    hv[e] = n0 + e < N ? fmaxf(t, alpha * t) : 0.f;
  }
}

// A workgroup's sum of squares (the whole tile belongs to one sample: nseg == 1,
// checked on the host): a plain store into its own slot of the ordered sum,
// which the finishing launch adds in slot order, or ONE f32 atomic per
// workgroup -- the atomics of a sample all hit one address and serialise in the
// L2 (measured 24 us of an 88 us launch with one per wave).
__device__ __forceinline__ void ssq_commit(float t, float* ssq_ws, long long slot,
                                           float* rowsumsq, int b) {
  if (ssq_ws) ssq_ws[slot] = t;
  else atomicAdd(rowsumsq + b, t);
}
