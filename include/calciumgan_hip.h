/* calciumgan_hip.h -- C ABI of the MI355X (gfx950) CalciumGAN hot-path kernels.
 *
 * Drop-in boundary: the reference has no FFI; the device ops
 * it executes are whatever TensorFlow dispatches for the Keras layers named
 * below.  Each entry point here replaces the device work of one reference
 * call site (file:line relative to the reference repo) and is what a
 * maintainer would bind (ctypes stub in INTEGRATION.md).
 *
 * Conventions for every function:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless
 *     the parameter is a `const cg_*_desc*` (host struct, read at call time);
 *   - activations are channels-last bf16 [nB][L][Cp], Cp = channel pitch, a
 *     multiple of 8; channels [C, Cp) are kept zero by every kernel;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are async,
 *     re-entrant per stream, allocate nothing and keep no global state;
 *   - the return value is a hipError_t (0 = success) or CG_EINVAL for a
 *     shape the kernels do not support (nothing is launched in that case).
 */
#ifndef CALCIUMGAN_HIP_H_
#define CALCIUMGAN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CG_EINVAL 100001
#define CG_ABI_VERSION 20

/* epilogue selectors of cg_swconv */
#define CG_EPI_NONE 0     /* y = acc (+bias) */
#define CG_EPI_LRELU 1    /* y = leaky_relu(acc + bias, alpha) */
#define CG_EPI_MASK 2     /* y = acc * (mask_src > 0 ? 1 : alpha) */
#define CG_EPI_SIGMOID 3  /* y = sigmoid(acc + bias) */
#define CG_EPI_LN_LRELU 4 /* y = acc + bias; ln_h = leaky_relu(layernorm(y)) */

/* workgroup tile of cg_swconv (rows x columns of y per workgroup); the _M32
 * tiles run v_mfma_f32_32x32x16_bf16 and need CK % 32 == 0, the others
 * v_mfma_f32_16x16x32_bf16.  Every tile gives the same result up to the f32
 * summation order inside one 32-deep K-step. */
#define CG_TILE_256x64 0
#define CG_TILE_64x64 1
#define CG_TILE_128x64 2
#define CG_TILE_256x64_M32 3
#define CG_TILE_128x64_M32 4
#define CG_TILE_256x128_M32 5
#define CG_TILE_128x128_M32 6
#define CG_TILE_256x128 7
#define CG_TILE_128x128 8
/* Software-pipelined tiles (swconv_swp.hip): two waves per SIMD (one 8-wave
 * workgroup or two 4-wave workgroups per CU), fragments double-buffered in
 * registers at K-step granularity, the source window and the weight ring both
 * filled by LDS-DMA.  v_mfma_f32_16x16x32, CK == 32, exactly twelve taps per
 * source-row parity (24 taps at stride 2 with a parity-major operand, 12 per
 * phase at stride 1), at least 16 rows of a sample per wave subtile and at most
 * eight samples per row tile; split-K over whole channel chunks; the LayerNorm
 * epilogue on the 128-column tiles.
 * Same results as the tiles above. */
#define CG_TILE_SWP_512x64 9
#define CG_TILE_SWP_256x64 10
#define CG_TILE_SWP_256x128 11
#define CG_TILE_SWP_128x128 12
#define CG_TILE_SWP_128x64 13  /* 4 waves x (32 x 64): short launches (more workgroups) */
#define CG_TILE_SWP_256x64_W8 14  /* 8 waves x (32 x 64): two workgroups = 4 waves per SIMD */
#define CG_TILE_SWP_128x128_W8 15 /* 8 waves x (32 x 64), 4 x 2: the same for 128 columns */
#define CG_NUM_TILES 16

int cg_abi_version(void);
/* Storage type of activations / activation gradients / packed operands this
 * build of the library computes with (everything the comments below call
 * "bf16"): libcalciumgan_hip.so is the bf16 build, libcalciumgan_hip_f16.so the
 * IEEE fp16 build (-DCG_ACT_F16=1; the reference's mixed_float16 policy,
 * main.py:22-30, with the loss scaling entry points at the end of this file).
 * Accumulators, statistics, losses, master weights and Adam state are f32 in
 * both. */
#define CG_DTYPE_BF16 0
#define CG_DTYPE_F16 1
int cg_act_dtype(void);
/* sizeof() of the descriptor structs as this library was compiled
 * (which: 0 cg_conv_desc, 1 cg_pack_desc, 2 cg_wgrad_desc; else -1): a binding
 * checks its own struct layout against it before the first launch. */
int cg_struct_size(int which);
/* rows / columns of a CG_TILE_* value (host helper; CG_EINVAL if unknown) */
int cg_tile_shape(int tile, int* rows, int* cols);

/* Measurement hook (the one piece of process-wide state in this library; not
 * for use while a stream is being captured into a hipGraph).  After
 * cg_profile_enable(n) the next n cg_swconv / cg_wgrad launches are issued with
 * a HIP event pair that carries the kernel's own begin / end timestamps;
 * cg_profile_collect waits for them, writes each launch's duration (ms) and
 * family (0 = cg_swconv, 1 = cg_wgrad) in launch order, returns the count
 * (negative hipError_t on failure) and disables the hook.  bench.py's roofline
 * leg is its only user. */
/* Development switch (process-wide, like the hook below): the specialised
 * epilogues of the 32-row software-pipelined tiles (swconv_swp.hip, kEpi*) on
 * (1) / off (0); < 0 only queries.  Returns the previous setting.  Off by
 * default (CALCIUMGAN_SWP_LEAN_EPI=1 turns them on at load): same results bit
 * for bit, no faster. */
int cg_debug_lean_epilogue(int on);
/* Form of cg_wgrad_batched for launches whose layers all take the ring-staged
 * 24-tap kernel with `partials` (round 5, ABI 18): 0 the K'-split forms, 1
 * (default; env CALCIUMGAN_WGRAD_FLEX) the flex form -- layers side by side,
 * equal contiguous K' shares -- when every team's share is worth its set-up, 2
 * the flex form whatever the size (tests).  Returns the previous mode; any
 * other argument only reads it.  Results are identical on exactly representable
 * data; in floating point the forms differ in summation order. */
int cg_debug_wgrad_flex(int mode);

int cg_profile_enable(int max_launches);
int cg_profile_collect(float* ms, int* family, int capacity);

/* ---------------------------------------------------------------------------
 * Sliding-window convolution as an implicit GEMM on MFMA (bf16 in, f32 acc).
 *
 *   y[b, y_stride*u + y_off, n] = epi( bias[n] +
 *        sum_{tap<taps} sum_{c<Cx} xs[b, stride*u + off + tap, c] * Wl[tap][c][n] )
 *
 * for u in [0, Lu), n in [0, N); rows of xs outside [0, Lx) read as zero
 * (TF 'same' padding) and xs = phase_shuffle(x, shifts[b / seg_size]) when
 * `shifts` is non-NULL (reflect gather fused into the LDS staging).
 * With nphase == 2 the launch computes two output phases z = 0,1 using
 * w + z*w_phase_stride, off + z*off_phase_step, y_off + z*yoff_phase_step
 * (the two 12-tap phases of a stride-2 transposed convolution).
 *
 * Replaces: layers.Conv1D fwd (gan/models/calciumgan.py:145-185) [stride 2,
 * taps k]; its input-gradient / Conv1DTranspose fwd (gan/models/utils.py:86-89)
 * [stride 1, taps k/2, two phases]; Conv1DTranspose input-gradient [stride 2];
 * layers.Dense on the last axis (calciumgan.py:32,96) [taps 1].
 *
 * `w` is the packed operand produced by cg_pack_weights for the same
 * (taps, Cx, CK).  Supported: stride in {1,2}; taps even when stride == 2;
 * Cx % CK == 0, CK % 8 == 0, CK >= 32; Lu a power-of-two divisor or any
 * multiple of the row tile (cg_tile_shape).
 * ------------------------------------------------------------------------- */
typedef struct cg_conv_desc {
  const void* x;        /* bf16 [nB][Lx][Cx] */
  const void* w;        /* bf16 packed [ceil(N/128)*128][Kpack] per phase */
  void* y;              /* bf16 or f32 [nB][Ly][Cy] */
  const float* bias;    /* f32 [N] or NULL */
  const void* mask_src; /* bf16, geometry of y; CG_EPI_MASK only */
  const int* shifts;    /* int32 [ceil(nB/seg_size)] or NULL */
  int nB, Lx, Cx, seg_size;
  int taps, stride, off, Lu;
  int N, Ly, Cy, y_stride, y_off;
  int CK;
  int epilogue, out_f32;
  float alpha;          /* leaky slope */
  int nphase;
  long long w_phase_stride; /* elements */
  int off_phase_step, yoff_phase_step;
  int tile;             /* CG_TILE_* */
  int stage_ksteps;     /* 0: choose; 2 or 4: MFMA K-steps per weight stage */
  float* rowsumsq;      /* optional f32 [nB]: += sum over (row, n) of y^2 per
                           sample (penalty norm, wgan_gp.py:49); needs Lu >= tile.
                           The value squared is the f32 epilogue result, BEFORE
                           it is rounded to a bf16 / fp16 y */
  int w_parity_major;   /* stride 2: `w` was packed with parity_major = 1 */
  int split_parity;     /* stride 2 + w_parity_major: stage one source-row
                           parity at a time (half the LDS window, twice the
                           staging phases; results identical) */
  /* CG_EPI_LN_LRELU only (layers.LayerNormalization + LeakyReLU after
   * Conv1DTranspose, calciumgan.py:68-70 fused into the producing launch):
   * y receives the bf16 pre-activation, ln_h = lrelu(LN(y)), ln_mean / ln_rstd
   * the per-row statistics (indexed like rows of y) cg_ln_lrelu_bwd consumes.
   * Needs stride 1, N <= 128, bf16 output and a 128-column tile (cg_tile_shape).
   * ln_mean = ln_rstd = NULL: forward only -- neither the statistics nor the
   * pre-activation y are stored (y may then be any non-NULL pointer). */
  const float* ln_gamma; /* f32 [N] */
  const float* ln_beta;  /* f32 [N] */
  void* ln_h;            /* bf16, geometry of y */
  float* ln_mean;        /* f32 [nB*Ly] */
  float* ln_rstd;        /* f32 [nB*Ly] */
  float ln_eps;
  /* Output-side PhaseShuffle adjoint (input gradient of a layer whose input
   * was shuffled, calciumgan.py:117-138): output row t of sample b belongs to
   * source row r = shuffle_src(t, out_shifts[b / out_seg_size], Ly).  Rows on
   * the direct branch are stored at r (bias / mask epilogues read row r); rows
   * on the reflected branch (at most |shift| per sample) go unmasked to
   * side[b][j] and are folded in by cg_unshuffle_fixup, which also zeroes the
   * |shift| rows nothing maps to.  NULL: rows are stored where they are
   * computed.  bf16 output only.
   * side == NULL with out_shifts: the folded form -- the launch itself adds each
   * reflected row onto its target and zeroes the empty rows, y ends up bit for
   * bit what the launch with `side` followed by cg_unshuffle_fixup leaves, and
   * there is no side buffer and no second launch.  A reflected row and the
   * direct row of its target are mirrors of equal parity among the first / last
   * |shift| + 1 rows of their phase, i.e. registers of one wave; so it is
   * admitted only where that holds: CG_EPI_MASK on the software-pipelined tiles
   * with 32-row waves (CG_TILE_SWP_128x64, _256x64_W8, _128x128_W8), stride 1,
   * two interleaved phases (y_stride 2, y_off 0, yoff_phase_step 1, Ly = 2 Lu),
   * Lu % 32 == 0, side_rows (still the bound on |shift|) <= 31, no row_scale.
   * CG_EINVAL everywhere else. */
  int w_narrow_last;    /* `w` was packed with narrow_last = 1 (stride 2,
                           w_parity_major, CK == 32) */
  const int* out_shifts;
  int out_seg_size;
  void* side;           /* bf16 [nB][side_rows][Cy]; NULL: the folded form */
  int side_rows;        /* >= max |shift| */
  /* Split-K for launches with few output tiles (the penalty's tangent chain:
   * one 128-sample segment): ksplit > 1 workgroups share an output tile, each
   * walking Cx/CK/ksplit channel chunks and storing f32 partial sums to
   * split_ws[z]; a finishing launch adds them, applies bias / LeakyReLU / mask
   * and writes the bf16 y.  Needs (Cx/CK) % ksplit == 0, bf16 output,
   * epilogue NONE / LRELU / MASK, no rowsumsq / out_shifts.  0 or 1: off. */
  int ksplit;
  float* split_ws;      /* f32 [ksplit][nB][Ly][Cy] */
  long long split_ws_elems;
  /* Per-sample scale applied before the epilogue: y = epi((acc + bias) *
   * row_scale[sample]).  The penalty's tangent chain starts from v = coef_b * g:
   * with this, its first launch reads g itself and the 134 MB pass that scaled
   * it is gone (wgan_gp.py, _critic_compute).  Software-pipelined tiles only,
   * no split-K, not with the fused LayerNorm; null: off. */
  const float* row_scale;
  /* Ordered penalty norm: with a workspace of >= cg_rowsumsq_ws_elems(d) floats
   * every workgroup STORES its share of a sample's sum of squares in its own
   * slot and a finishing launch adds a sample's slots in slot order and stores
   * rowsumsq[b] -- the same bits every run, no zeroed buffer -- instead of one
   * f32 atomic per workgroup into rowsumsq[b].  NULL: atomics (+=). */
  float* rowsumsq_ws;
  long long rowsumsq_ws_elems;
  /* 1: leave the slots in rowsumsq_ws and do NOT launch the finishing pass --
   * the caller's next launch adds them (cg_gp_loss_scale reads the slots
   * itself: one launch fewer per critic update).  Needs rowsumsq_ws. */
  int rowsumsq_defer;
} cg_conv_desc;

int cg_swconv(const cg_conv_desc* d, void* stream);
/* floats of cg_conv_desc.rowsumsq_ws for this descriptor's tile (0: no rowsumsq;
 * < 0: invalid descriptor) */
long long cg_rowsumsq_ws_elems(const cg_conv_desc* d);
/* Validate a descriptor exactly as cg_swconv would (geometry, tile, LDS budget,
 * epilogue / split-K constraints) without launching anything: 0 or CG_EINVAL.
 * The host uses it before adopting a tile choice from a saved table. */
int cg_swconv_check(const cg_conv_desc* d);

/* Streaming form of the 1-tap case with f32 output (the generator's last
 * layers.Dense + sigmoid, calciumgan.py:96-101; HBM-bound):
 *   y[r, n] = epi(bias[n] + sum_c x[r, c] * W[c][n]),  y[r, n >= N] = 0
 * x bf16 / fp16 (the build's activation type) [rows][Cx], y f32 [rows][Cy]; `w`
 * is the cg_pack_weights operand for
 * (taps 1, Cx, CK 32).  Epilogue CG_EPI_NONE or CG_EPI_SIGMOID.  Two forms:
 * Cx in {32, 64, 96, 128} and N <= Cy <= 128 (Cy % 4 == 0): every wave holds W
 * in registers; otherwise Cx in {128, 256, 384, 512}, any N <= Cy (Cy % 8 == 0):
 * a workgroup holds one 128-column panel of W in LDS (BASELINE configs[4]:
 * 512 -> 512). */
int cg_dense_rows(const void* x, const void* w, const float* bias, float* y,
                  long long rows, int Cx, int N, int Cy, int epilogue,
                  void* stream);
/* cg_dense_rows for the fake batches of ALL n critic updates of one train() -- x
 * bf16 / fp16 [n * B * L][Cx], the generator's last hidden layer over n * B samples --
 * fused with cg_interp_pack.  Register form: Cx in {32, 64, 96, 128}, N <= 128, Cp =
 * 128.  LDS-panel form (ABI 19; BASELINE configs[4]): Cx in {128, 256, 384, 512}
 * with Cx > 128 or N > 128, Cp >= N a multiple of 8, B * L % 32 == 0; without x^
 * (alpha == NULL) the Dense only stores its fake segments and a second launch
 * reads `real` once for the n real segments.
 * x0[k] (bf16 / fp16 [3 B][L][Cp]) receives [real | fake_k | x^_k], x^ =
 * alpha[k * B + b] * real + (1 - alpha) * fake (wgan_gp.py:38-41, interpolation
 * in f32 on the f32 Dense output as the reference does).  The f32 fake batch
 * never reaches HBM and `real` (f32 [B][L][Cr]) is read once.  L % 16 == 0,
 * n <= 8.  The bytes of x0[k] equal those of cg_dense_rows + cg_interp_pack.
 * alpha == NULL (ABI 19): the x^ segment is left untouched -- the caller forms the
 * critic's first layer on x^ with cg_lrelu_mix and never reads x^ itself. */
int cg_dense_rows_interp(const void* x, const void* w, const float* bias,
                         const float* real, const float* alpha, void* const* x0,
                         int n, int B, int L, int Cx, int N, int Cr, int Cp,
                         int epilogue, void* stream);
/* The same contraction with an activation-typed (bf16 / fp16) output, no bias,
 * no epilogue -- the input gradient of that Dense: dh[r, c] = sum_n dz[r, n] *
 * W[c][n] with `w` the operand packed from W transposed.  Cx in {128, 256, 384,
 * 512}, N <= Cy, Cy % 8 == 0; columns [N, Cy) are written as zeros. */
int cg_dense_rows_act(const void* x, const void* w, void* y, long long rows,
                      int Cx, int N, int Cy, void* stream);
/* Weight gradient of that Dense, dW f32 [Cx_real][Cg_real] row-major (the Keras
 * kernel layout), x [rows][Cx], g [rows][Cg] bf16 / fp16, pitches multiples of
 * 8.  Streaming form: 128 x 128 tiles of dW x row ranges, K'-major operands
 * through LDS transpose reads.  ws == NULL: the row ranges' partial tiles meet
 * through f32 atomics, dW[cx][cg] += sum_r x[r][cx] * g[r][cg] (the caller
 * zeroes dW).  With a workspace of cg_dense_wgrad_ws_elems(...) floats: plain
 * stores and a reducing launch that adds the ranges in a fixed order and STORES
 * dW -- the only sensible form when dW has at most four tiles (a thousand
 * workgroups' atomics on the same addresses serialise), and the deterministic
 * one for any size. */
long long cg_dense_wgrad_ws_elems(long long rows, int Cx_real, int Cg_real);
int cg_dense_wgrad(const void* x, const void* g, float* dw, long long rows,
                   int Cx, int Cg, int Cx_real, int Cg_real, float* ws,
                   long long ws_elems, void* stream);
/* elements (bf16) of one packed phase operand for (N, taps, Cx, CK) */
long long cg_packed_elems(int N, int taps, int Cx, int CK);

/* ---------------------------------------------------------------------------
 * Pack an f32 master weight (TensorFlow layout, arbitrary strides) into the
 * bf16 operand cg_swconv consumes:
 *   Wl[tap][c][n] = src[(tap0 + tap*tap_step)*s_tap + c*s_c + n*s_n]
 * for tap<taps, c<C_real, n<N_real; zero elsewhere (channel / row padding).
 * Replaces nothing in the reference (TF keeps one layout); it is the
 * MI355X-side operand preparation run after each optimizer update.
 * ------------------------------------------------------------------------- */
typedef struct cg_pack_desc {
  const float* src;
  void* dst; /* bf16, cg_packed_elems(N_real, taps, Cx, CK) elements */
  int taps, tap0, tap_step;
  long long s_tap, s_c, s_n;
  int C_real, N_real, Cx, CK;
  int parity_major; /* 0: taps in order; 1 (even taps only): the even taps first,
                       then the odd ones -- the order in which a stride-2 launch
                       with w_parity_major walks them (one source-row parity
                       at a time) */
  int narrow_last;  /* 1 (needs parity_major, CK == 32, 6 <= taps <= 32, Cx >= 64
                       and Cx - 32 < C_real <= Cx - 24: the last channel chunk
                       holds at most 8 real channels): that chunk is packed as
                       one 8-channel group per tap -- 16 slots per tap parity,
                       K = 32 groups instead of taps*4 -- for launches with
                       cg_conv_desc.w_narrow_last, which then skip the chunk's
                       all-zero channel groups */
} cg_pack_desc;
int cg_pack_weights(const cg_pack_desc* d, void* stream);
/* Batched form (one launch for all operands of a model).  Host side:
 *   blocks = cg_pack_plan_build(descs, n, NULL, 0);            (sizing pass)
 *   bytes  = cg_pack_plan_bytes(n, blocks);
 *   cg_pack_plan_build(descs, n, host_buf, bytes);             (fills host_buf)
 * copy host_buf to device memory once, then after every optimizer update
 *   cg_pack_batched(dev_plan, n, blocks, stream). */
long long cg_pack_plan_bytes(int n, long long total_blocks);
long long cg_pack_plan_build(const cg_pack_desc* descs, int n, void* host_buf,
                             long long host_bytes);
int cg_pack_batched(const void* dev_plan, int n, long long blocks, void* stream);

/* ---------------------------------------------------------------------------
 * Weight gradient of the sliding-window convolution (f32 accumulate, f32
 * atomics into dw, which the caller zeroes):
 *   dw[tap][cx][cg] += sum_{b,u} xs[b, stride*u + off + tap, cx] * g[b, u, cg]
 * dw is dense f32 [taps][Cx_real][Cg_real].  Replaces the autodiff
 * weight-gradient of Conv1D / Conv2DTranspose / Dense taken by
 * tape.gradient in gan/algorithms/optimizer.py:31-34.
 * Supported: (stride 2, even taps <= 24) or (stride 1, taps 1).
 * ------------------------------------------------------------------------- */
typedef struct cg_wgrad_desc {
  const void* x;     /* bf16 [nB][Lx][Cx] */
  const void* g;     /* bf16 [nB][Lu][Cg] */
  float* dw;         /* f32 [taps][Cx_real][Cg_real] */
  const int* shifts; /* phase shuffle applied to x rows, or NULL */
  int nB, Lx, Cx, seg_size;
  int Lu, Cg;
  int taps, stride, off;
  int Cx_real, Cg_real;
  int nsplit;        /* 0 = choose */
  int tile_rows;     /* 0 = choose; 64 or 128 rows of (b,u) per staged tile */
  int no_xcd_group;  /* 1: plain block order instead of the XCD-grouped one (A/B runs) */
  int classic_staging; /* 1: register-staged tiles instead of the LDS-DMA ring (A/B runs) */
  float* dbias;      /* optional f32 [Cg_real]: += sum of g over its first
                        bias_rows (b,u) rows -- the conv bias gradient, taken
                        from the g tiles already staged in LDS */
  long long bias_rows;
  float* partials;   /* optional workspace of >= cg_wgrad_partials_elems(d) f32:
                        the K' splits then leave their partial sums (dw tiles
                        and, with dbias, their bias column sums) with plain
                        stores and a second kernel adds them in split order (one
                        owner per element: deterministic), instead of every
                        split adding into dw / dbias with f32 atomics.  NULL:
                        atomics. */
  long long partials_elems;
  int store;         /* with `partials`: dw (and dbias) are STORED, not added to
                        (no zeroed buffer needed).  0: += as before. */
} cg_wgrad_desc;
int cg_wgrad(const cg_wgrad_desc* d, void* stream);
/* f32 elements of `partials` this descriptor needs (0: the taps == 1 form, which
 * adds each dw element once per K' split with atomics -- one split, nsplit = 1,
 * is deterministic); < 0: error */
long long cg_wgrad_partials_elems(const cg_wgrad_desc* d);
/* n weight gradients (independent layers of one backward pass) as ONE launch
 * when they are all the pipelined stride-2 form with the same tap count (the
 * accumulator flush of one layer then overlaps the next layer's main loop);
 * otherwise the same as n cg_wgrad calls.  Results as cg_wgrad (f32 atomics:
 * the summation order differs); descriptors with `partials` are reduced by one
 * extra launch for all layers. */
int cg_wgrad_batched(const cg_wgrad_desc* descs, int n, void* stream);
/* The flex form's share plan for inspection (host only, nothing is launched):
 * returns the number of ints of the table -- items [workgroups][8][6] = (layer
 * or -1, bx, by, first K' tile, tiles, slot), then per layer [gx * gy][2] =
 * (first slot, slots) -- and copies it to `out` when out_ints suffices; info
 * (>= 16 ints): team size, teams, workgroups, items, slots of layer 0..5, int
 * offsets of the layers' tile tables.  < 0: not the flex form under `mode`. */
long long cg_wgrad_flex_plan(const cg_wgrad_desc* descs, int n, int mode, int* out,
                             long long out_ints, int* info);

/* Second half of cg_conv_desc.out_shifts: per sample with shift s,
 *   delta[b, r, :] = 0 for the |s| rows r no output row maps to, and
 *   delta[b, r, :] += side[b, j, :] * (h[b, r, :] > 0 ? 1 : alpha) for the |s|
 * reflected rows.  delta / h bf16 [nB][w][Cp], side bf16 [nB][side_rows][Cp]. */
int cg_unshuffle_fixup(const void* side, const void* h, void* delta,
                       const int* shifts, int nB, int w, int Cp, int seg_size,
                       int side_rows, float alpha, void* stream);

/* ---------------------------------------------------------------------------
 * LayerNormalization(axis=-1, eps) + LeakyReLU.  Replaces
 * layers.LayerNormalization + activation_fn (calciumgan.py:44-46 etc.) and
 * their autodiff backward.  Activations are of the build's activation type
 * (bf16 or fp16), [rows][Cp] with C real channels; Cp % 8 == 0, Cp <= 512,
 * C <= Cp, rows >= 1 (else CG_EINVAL, nothing launched).  A row is covered by
 * the lanes of part of a wavefront (8 channels per lane), several rows per wave.
 *   mean / var: over the C real channels, two passes (mean, then the mean of
 *     (y - mean)^2, biased); rstd = 1 / sqrt(var + eps);
 *   h = lrelu((y - mean) rstd gamma + beta), lrelu(t) = t > 0 ? t : alpha t.
 * Channels [C, Cp) of y_pre are never read into a result (they may hold
 * anything, NaN included); channels [C, Cp) of h are stored as +0.  gamma / beta
 * are read for c < C only.  mean / rstd may each be NULL: that statistic is not
 * stored, h is the same.
 * ------------------------------------------------------------------------- */
int cg_ln_lrelu_fwd(const void* y_pre /*act [rows][Cp]*/, const float* gamma,
                    const float* beta, void* h /*act [rows][Cp]*/,
                    float* mean /*[rows] or NULL*/, float* rstd /*[rows] or NULL*/,
                    long long rows, int C, int Cp, float eps, float alpha,
                    void* stream);
/* Ordered reductions.  The functions below that reduce over rows take a
 * workspace `ws` of cg_reduce_ws_elems() floats (one size for every function and
 * shape; launches are stream-ordered, so one buffer serves them all).  With it,
 * every block STORES a partial row and a finishing launch adds the rows in a
 * fixed order and STORES the result: the same bits every run and no zeroed
 * output.  ws == NULL: blocks meet through f32 atomics (+= into outputs the
 * caller zeroed; the order, and so the last bits, vary from run to run). */
long long cg_reduce_ws_elems(void);
/* Deferred finishing launches (round 5): between cg_finish_defer(1) and
 * cg_finish_flush(stream) on the calling thread, the finishing launch of every
 * ordered reduction above is queued instead of issued, and the flush adds all
 * queued reductions in ONE launch (up to 12 per launch; the same sums in the same
 * order).  Every queued call must have been given its own workspace region -- its
 * partial rows are read at the flush -- and nothing between may read the outputs
 * (cg_bn_bwd does: not deferrable).  cg_finish_defer returns the previous mode. */
int cg_finish_defer(int on);
int cg_finish_flush(void* stream);
/* Backward of cg_ln_lrelu_fwd (same limits on Cp, C, rows).  mean / rstd [rows]
 * are used AS GIVEN (not recomputed from y_pre).  With mask = h > 0 ? 1 : alpha
 * (h = +0, -0 and NaN take alpha), do = dh mask, xhat = (y_pre - mean) rstd,
 * dyh = do gamma and mean_c the mean over the C real channels:
 *   dy = rstd (dyh - mean_c(dyh) - xhat mean_c(dyh xhat))
 *   dgamma[c] = sum_rows do xhat, dbeta[c] = sum_rows do, and, when dbias !=
 *   NULL, dbias[c] = sum_rows of the STORED (rounded) dy: the bias gradient of
 *   the producing conv.
 * The three sums are stored (ws) or accumulated with f32 atomics onto outputs
 * the caller zeroed (ws == NULL), for c < C only.  Channels [C, Cp) of dh, h and
 * y_pre are never read into a result; channels [C, Cp) of dy are stored as +0. */
int cg_ln_lrelu_bwd(const void* dh /*act*/, const void* h /*act*/,
                    const void* y_pre /*act*/, const float* mean,
                    const float* rstd, const float* gamma, void* dy /*act*/,
                    float* dgamma, float* dbeta, float* dbias, long long rows,
                    int C, int Cp, float alpha, float* ws, void* stream);

/* ---------------------------------------------------------------------------
 * BatchNormalization(axis=-1) of a generator block (calciumgan.py:42-43 etc.;
 * Keras defaults: momentum 0.99, epsilon 1e-3, biased batch variance) -- single
 * rank only (batch statistics would need a cross-rank reduction).  All three
 * need the workspace of cg_reduce_ws_elems() floats (ordered column sums).
 *   cg_bn_stats: mean[c] / var[c] over the rows of y; with moving_mean /
 *     moving_var (training): moving = moving * momentum + batch * (1 - momentum).
 *   cg_bn_apply: out = f((y - mean) * rsqrt(var + eps) * gamma + beta), f(t) =
 *     max(t, alpha t) (alpha = 1: no activation); inference passes the moving
 *     statistics.
 *   cg_bn_bwd: do = dout * (act ? lrelu'(h) : 1); dbeta = sum do, dgamma = sum
 *     do * xhat (both STORED); dy = gamma rstd (do - dbeta / R - xhat dgamma / R),
 *     rstd = rsqrt(var + eps), xhat = (y - mean) rstd, R = rows, lrelu'(h) = h > 0
 *     ? 1 : alpha (h = +0, -0 and NaN take alpha); act == 0: h is not read (NULL).
 * y / out / dout / h / dy are of the build's activation type, [rows][Cp] with C
 * real channels; Cp % 8 == 0, C <= Cp, rows >= 1, and Cp <= 2048 for cg_bn_stats
 * and cg_bn_bwd (cg_bn_apply takes any pitch).  A NULL among the required
 * pointers, one of moving_mean / moving_var without the other, or act != 0 with
 * h == NULL: CG_EINVAL, nothing launched.  Channels [C, Cp) of the inputs are
 * never read into a result (they may hold anything, NaN included); channels
 * [C, Cp) of out / dy are stored as +0; the f32 vectors are read and written
 * for c < C only.
 * ------------------------------------------------------------------------- */
int cg_bn_stats(const void* y, long long rows, int C, int Cp, float* mean,
                float* var, float* moving_mean /* or NULL */,
                float* moving_var /* or NULL */, float momentum, float* ws,
                void* stream);
int cg_bn_apply(const void* y, const float* mean, const float* var,
                const float* gamma, const float* beta, void* out, long long rows,
                int C, int Cp, float eps, float alpha, void* stream);
int cg_bn_bwd(const void* dout, const void* h /* act != 0 */, const void* y,
              const float* mean, const float* var, const float* gamma, void* dy,
              float* dgamma, float* dbeta, long long rows, int C, int Cp,
              float eps, float alpha, int act, float* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Discriminator head: Flatten + Dense(1) (calciumgan.py:188-190).
 * ------------------------------------------------------------------------- */
/* h is bf16 [nB][Lt][Cp]; w is the f32 Keras kernel [Lt*C] (flatten index
 * t*C + c, calciumgan.py:188), used rounded to bf16.
 * out[b] = bias[0] + sum_{t,c<C} h[b][t][c] * bf16(w[t*C+c]) */
int cg_dense1_fwd(const void* h, const float* w, const float* bias,
                  float* out /*[nB]*/, int nB, int Lt, int C, int Cp,
                  void* stream);
/* cg_dense1_fwd and cg_dense1_bwd in one pass over h (the seed of the backward
 * chain does not depend on the head's output) */
int cg_dense1_fwd_bwd(const void* h, const float* w, const float* bias,
                      float* out /*[nB]*/, const float* coef /*device [nseg]*/,
                      void* delta /*bf16*/, int nB, int Lt, int C, int Cp,
                      int seg_size, float alpha, void* stream);
/* delta[b][t][c] = coef[b / seg_size] * bf16(w[t*C+c]) * lrelu'(h[b][t][c]) */
int cg_dense1_bwd(const float* w, const float* coef /*device [nseg]*/,
                  const void* h, void* delta /*bf16*/, int nB, int Lt, int C,
                  int Cp, int seg_size, float alpha, void* stream);
/* dw[t*C+c] += sum_b coef[b / seg_size] * x[b][t][c];
 * db[0] += sum_b bias_coef[b / seg_size]  (bias_coef may be NULL);
 * with ws: = instead of += (ordered reduction, see cg_reduce_ws_elems) */
int cg_dense1_wgrad(const void* x /*bf16 [nB][Lt][Cp]*/, const float* coef,
                    const float* bias_coef /*device [nseg]*/, float* dw,
                    float* db, int nB, int Lt, int C, int Cp, int seg_size,
                    float* ws, void* stream);

/* Head of the vanilla (BCE) GAN step (gan.py:43-56, 72-85; ABI 20).  h holds
 * 2B samples [fake | real] (fake segment first).  Per sample, x = the logit of
 * cg_dense1_fwd (same sum order) -> out[b]; with s the sigmoid and y = 0 on the
 * fake segment, 1 on the real one:
 *   coef_d[b] = S_d * (s(x_b) - y_b) / B             (NULL: not written)
 *   coef_g[b] = S_g * (s(x_b) - 1) / B, b < B        (NULL: not written)
 *   delta_d[b][t][c] = coef_d[b] * bf16(w[t*C+c]) * lrelu'(h[b][t][c])  (2B rows)
 *   delta_g[b][t][c] = coef_g[b] * bf16(w[t*C+c]) * lrelu'(h[b][t][c])  (B rows)
 * (delta_d NULL: no seeds; delta_g NULL: no generator seeds; channels [C, Cp)
 * of both are stored as +0; lrelu'(h) = h > 0 ? 1 : alpha).  S_d / S_g are
 * device scalars (the fp16 loss scales; NULL = 1).  Keras BCE from logits,
 * max(x,0) - x y + log1p(exp(-|x|)), averaged per segment:
 *   loss[0] = mean_fake BCE(1, x)                      (generator loss)
 *   loss[1] = mean_real BCE(1, x) + mean_fake BCE(0, x) (discriminator loss)
 * With ws (3B floats of it) the means are an ordered reduction and stored;
 * without, they are added with atomics onto a zeroed loss. */
int cg_dense1_bce(const void* h /*[2B][Lt][Cp]*/, const float* w,
                  const float* bias, float* out /*[2B]*/, float* coef_d /*[2B]*/,
                  float* coef_g /*[B]*/, void* delta_d, void* delta_g,
                  float* loss /*[2]*/, const float* scale_d,
                  const float* scale_g, int B, int Lt, int C, int Cp,
                  float alpha, float* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Backward of LeakyReLU + PhaseShuffle between discriminator layers:
 *   delta[b][r][c] = lrelu'(h[b][r][c]) * sum_{t: src(t)=r} e[b][t][c]
 * where src is the reflect gather of PhaseShuffle (calciumgan.py:117-138): a
 * row has no, one or two sources; the f32 sum times the mask is rounded once.
 * lrelu'(h) = h > 0 ? 1 : alpha (h = +0, -0 and NaN take alpha).  Sample b takes
 * shifts[b / seg_size] (|shift| < w; shifts == NULL: 0 everywhere).  e / h /
 * delta are of the build's activation type; Cp % 8 == 0.  There is no channel
 * count: all Cp channels are computed, so zero padding in e gives +0 padding in
 * delta.
 * ------------------------------------------------------------------------- */
int cg_unshuffle_mask(const void* e /*act [nB][w][Cp]*/, const void* h,
                      void* delta, const int* shifts, int nB, int w, int Cp,
                      int seg_size, float alpha, void* stream);

/* ---------------------------------------------------------------------------
 * WGAN-GP elementwise / reduction pieces (gan/algorithms/wgan_gp.py).
 * ------------------------------------------------------------------------- */
/* x0[0:B]=bf16(real), x0[B:2B]=bf16(fake), x0[2B:3B]=bf16(alpha*real+(1-alpha)*fake)
 * (wgan_gp.py:38-41); real f32 [B][L][Cr], fake f32 [B][L][Cf] (row pitches,
 * C valid channels), x0 bf16 [3B][L][Cp].  alpha == NULL (ABI 19): the third
 * segment is left untouched (see cg_lrelu_mix). */
int cg_interp_pack(const float* real, const float* fake, const float* alpha,
                   void* x0, int B, int L, int C, int Cr, int Cf, int Cp,
                   int write_real /* 0: x0[0:B] already holds bf16(real) */,
                   void* stream);
/* dst bf16 [rows][Cp] = src f32 [rows][Cs] (C valid channels), pad zero */
int cg_cast_pad(const float* src, void* dst, long long rows, int C, int Cs,
                int Cp, void* stream);
/* norm[b] = ||g[b]||_2 over n elements (wgan_gp.py:49), g bf16 [B][n] (the
 * layer-1 input gradient, stored like every other activation gradient) */
int cg_rownorm(const void* g, float* norm, int B, long long n,
               float* ws /* ordered reduction, or NULL */, void* stream);
/* gp = mean((norm-1)^2) (wgan_gp.py:50); coef[b] = scale*2*(norm-1)/(B*norm).
 * squared != 0: `norm` holds sums of squares on entry and is replaced by their
 * square roots. */
int cg_gp_finalize(float* norm, float* gp, float* coef, int B, float scale,
                   int squared, void* stream);
/* a0 bf16 [B][n] = coef[b] * g[b], g bf16 [B][n] */
int cg_scale_rows(const void* g, const float* coef, void* a0, int B,
                  long long n, void* stream);
/* out[0] = -mean(d_out[0:B]) + mean(d_out[B:2B]) + penalty*gp[0]  (wgan_gp.py:58-61)
 * out[1] = -mean(d_out[B:2B]) (generator_loss of the same fake batch) */
int cg_critic_loss(const float* d_out, const float* gp, float penalty,
                   float* out, int B, void* stream);
/* cg_gp_finalize followed by cg_critic_loss as ONE launch: coef additionally
 * multiplied by coef_mul; loss[0] / loss[1] as cg_critic_loss's out. */
int cg_gp_critic_loss(float* norm, float* gp, float* coef, const float* d_out,
                      float* loss /*[2]*/, int B, float penalty, int squared,
                      float coef_mul, void* stream);
/* The penalty's finalisation as ONE launch (wgan_gp.py:43-62): adds the slots a
 * cg_swconv launch with rowsumsq_defer left in ssq_ws ([B][P] floats, P =
 * cg_rowsumsq_ws_elems / nB) in slot order, norm[b] = sqrt of that, gp / coef /
 * loss exactly as cg_gp_critic_loss(squared = 1), and -- g non-null -- dst[b] =
 * coef[b] * g[b] for bf16 [B][n] rows (cg_scale_rows: every workgroup forms its
 * sample's coefficient from the same slots, bit for bit the value coef[] gets). */
int cg_gp_loss_scale(const float* ssq_ws, int P, float* norm, float* gp,
                     float* coef, const float* d_out, float* loss /*[2]*/, int B,
                     float penalty, float coef_mul, const void* g, void* dst,
                     long long n, void* stream);
/* out[0] = -mean(d_out[0:B])  (wgan_gp.py:19-20) */
int cg_neg_mean(const float* d_out, float* out, int B, void* stream);

/* out f32[C] += column sums of x bf16 [rows][Cp] (bias gradients); with ws:
 * = instead of += (ordered reduction) */
int cg_colsum(const void* x, float* out, long long rows, int C, int Cp,
              float* ws, void* stream);
/* dz = dfake * s * (1 - s)  (sigmoid backward; calciumgan.py:98-99) */
int cg_sigmoid_bwd(const void* dfake /*bf16 [rows][Cp]*/,
                   const float* fake /*f32 [rows][Cf]*/,
                   void* dz /*bf16 [rows][Cp]*/, long long rows, int C, int Cf,
                   int Cp, void* stream);
/* dpre = dh * lrelu'(h), all bf16 [n] */
int cg_lrelu_bwd(const void* dh, const void* h, void* dpre, long long n,
                 float alpha, void* stream);
/* out[b] = act(mix[b] * act^-1(h_a[b]) + (1 - mix[b]) * act^-1(h_b[b])), all bf16
 * [B][n_per_sample], act(y) = max(y, alpha y) with 0 < alpha <= 1: the critic's first
 * layer on x^ = a real + (1 - a) fake (gan/algorithms/wgan_gp.py:41-47 feeding
 * gan/models/calciumgan.py:159-166) from that layer's outputs on real and fake -- the
 * convolution is linear, so the x^ segment needs no convolution of its own. */
int cg_lrelu_mix(const void* h_a, const void* h_b, const float* mix, void* out,
                 int B, long long n_per_sample, float alpha, void* stream);

/* ---------------------------------------------------------------------------
 * Keras Adam (gan/algorithms/optimizer.py:9; tf.keras.optimizers.Adam):
 *   g = grad*grad_scale; m = b1*m + (1-b1)g; v = b2*v + (1-b2)g^2;
 *   p -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t)
 * ------------------------------------------------------------------------- */
int cg_adam(float* p, const float* grad, float* m, float* v, long long n,
            float lr_t, float beta1, float beta2, float eps, float grad_scale,
            const float* lr_t_dev /* device scalar overriding lr_t, or NULL
                                     (lets a captured hipGraph vary the step) */,
            void* stream);

/* ---------------------------------------------------------------------------
 * Exponential moving average of a flat f32 parameter buffer (--ema_decay;
 * gan/algorithms/averaging.py), TF's assign_moving_average:
 *   ema[i] = ema[i] - fl(fl(ema[i] - p[i]) * om),   om = 1 - decay
 * three f32 operations, each rounded on its own (never an fma): the bits of
 * averaging.update_statement, the same on every call.  p is only read.  Any
 * n >= 1 and any 4-byte aligned pointers; 16-byte loads and stores where ema
 * and p are both 16-byte aligned.  ema and p must not overlap.  No atomics, no
 * workspace.  CG_EINVAL, nothing launched: ema or p NULL, n < 1, om outside
 * [0, 1] or NaN.
 * ------------------------------------------------------------------------- */
int cg_ema_update(float* ema, const float* p, long long n, float om,
                  void* stream);

/* ---------------------------------------------------------------------------
 * Dynamic loss scaling of the mixed_float16 mode -- mixed_precision.
 * LossScaleOptimizer(Adam, 'dynamic') (gan/algorithms/optimizer.py:10-12,23-29):
 * the loss is multiplied by S before the backward pass, the gradients divided by
 * S before Adam; non-finite gradients skip the update and halve S (floor 1);
 * `growth_interval` consecutive finite updates double it [TF: initial 2^15,
 * interval 2000].  The state is four DEVICE floats, so a captured graph carries
 * it without host round trips:
 *   ls[0] = S, ls[1] = consecutive finite updates, ls[2] = applied Adam steps t,
 *   ls[3] = 1 while the gradients of the update in progress look finite.
 * One update = cg_grad_finite (clears ls[3] on any inf / nan; n % 4 == 0)
 *           -> cg_adam_scaled (no-op when ls[3] == 0; g = grad*grad_scale/S;
 *              lr_t from t = ls[2] + 1 as in cg_adam)
 *           -> cg_loss_scale_update (advances S / counters, sets ls[3] = 1).
 * ------------------------------------------------------------------------- */
int cg_grad_finite(const float* grad, long long n, float* ls, void* stream);
int cg_adam_scaled(float* p, const float* grad, float* m, float* v, long long n,
                   float lr, float beta1, float beta2, float eps,
                   float grad_scale, const float* ls, void* stream);
int cg_loss_scale_update(float* ls, int growth_interval, void* stream);

/* ---------------------------------------------------------------------------
 * GAN.metrics (gan/algorithms/gan.py:32-41, gan/utils/signals_metrics.py:9-28):
 * out[0..3] += sum over rows of squared differences of per-row (min, max,
 * mean, population-std) over channels of denormalised real vs fake; caller
 * zeroes out and divides by rows (ws == NULL); with ws the MEANS over rows are
 * stored (ordered reduction, see cg_reduce_ws_elems).
 * ------------------------------------------------------------------------- */
int cg_signal_metrics(const float* real /*[rows][Cr]*/,
                      const float* fake /*[rows][Cf]*/, float* out,
                      long long rows, int C, int Cr, int Cf, float smin,
                      float smax, float* ws, void* stream);

/* The scalars WGAN_GP.train returns (gan/algorithms/wgan_gp.py:82-95), gathered
 * by one launch: out[0] = gen_loss[0], out[1] = mean_k loss[2 k] (the critic loss
 * of update k; loss is f32 [n][2] as cg_critic_loss writes it), out[2] = mean_k
 * gp[k], out[3..6] = metrics[0..3]. */
int cg_step_outputs(const float* gen_loss, const float* loss, const float* gp,
                    const float* metrics, int n, float* out /*[7]*/,
                    void* stream);

/* ---------------------------------------------------------------------------
 * Spike statistics during validation (spikes.hip; no counterpart on a device in
 * the reference, which deconvolves on the host: main.py:142-154,
 * gan/utils/spike_helper.py:23-54, compute_dg_metrics.py:40-58).  Functions
 * added under ABI 20; the same in both precision builds (nothing here touches
 * an activation type).
 * ------------------------------------------------------------------------- */
/* OASIS AR(1) deconvolution with a minimum spike size (oasisAR1(y, g, s_min),
 * lam = 0), one trace per lane in float64, then spike = s > threshold: bit for
 * bit what the host library computes (csrc/oasis_ar1.c: cg_oasis_ar1 /
 * cg_deconvolve) on the same float64 input.
 *   trace (o, i), o < n_outer, i < n_inner, frame t:
 *     y = (double)x[o * sx_outer + t * sx_t + i * sx_inner]
 *   or, unless scale == 1 and offset == 0, (double)(x * scale + offset) with the
 *   product and the sum each rounded to float32 (denormalisation of a float32
 *   array); strides in elements.  Consecutive lanes take consecutive i: a
 *   (B, L, Cf) batch is read in place with n_inner = C, sx_inner = 1, and a
 *   (rows, T) array with n_outer = 1, n_inner = rows, sx_inner = T.
 *   spikes: float32 {0, 1} with strides of its own; c / s: float64 [traces][T]
 *   (trace = o * n_inner + i) or NULL.
 *   gpow: DEVICE float64 [T + 1], gpow[l] = pow(g, l) as the HOST's libm gives
 *   it (cg_oasis_pow_table of libcalciumgan_host.so), uploaded by the caller.
 *   ws: cg_oasis_ws_bytes(traces, T) bytes, 8-byte aligned: the pool stacks at
 *   full depth (20 bytes x T per trace, interleaved by trace).  A smaller or
 *   larger workspace is legal from 64 traces' worth: the call then walks the
 *   batch in groups of the traces it holds, one launch per group.
 * T <= 2^24.  Never spins: at most 2 T iterations per trace, NaN included. */
long long cg_oasis_ws_bytes(long long traces, int T);
int cg_oasis_ar1_batched(const float* x, int n_outer, int n_inner, int T,
                         long long sx_outer, long long sx_t, long long sx_inner,
                         float scale, float offset, double g, double s_min,
                         double threshold, const double* gpow, float* spikes,
                         long long so_outer, long long so_t, long long so_inner,
                         double* c, double* s, void* ws, long long ws_bytes,
                         void* stream);
/* Per sample b < B of binary trains spikes[b * s_b + t * s_t + c * s_c] (float32,
 * 24 frames per second):
 *   rates[b][c] = sum_t spikes / (T / 24)        (spike_metrics.mean_firing_rate)
 *   cov[b][p]   = unbiased covariance of the 500-ms bin counts of neurons (i, j),
 *                 p running over i <= j in np.triu_indices order
 *                 (spike_metrics.covariance; 12 frames per bin, a trailing
 *                 partial bin dropped, nb = T / 12 bins)
 * rates f32 [B][C], cov f32 [B][C (C + 1) / 2].  The sums are exact integers;
 * only the final quotient rounds.  CG_EINVAL: nb < 2, or 4 C + nb C > 60 KiB
 * (the counts of one sample are kept in LDS). */
int cg_spike_stats(const float* spikes, int B, int T, int C, long long s_b,
                   long long s_t, long long s_c, float* rates, float* cov,
                   void* stream);
/* out[0] = sum |fr_a - fr_b|, out[1] = sum (fr_a - fr_b)^2 over n_fr elements,
 * out[2], out[3] the same for cov over n_cov elements (the sums behind
 * compute_dg_metrics.report's MAE / RMSE / MSE; sums, so that an epoch is formed
 * from its batches).  Ordered two-stage reduction through ws
 * (cg_spike_stats_error_ws_elems floats): the same bits every run. */
long long cg_spike_stats_error_ws_elems(long long n_fr, long long n_cov);
int cg_spike_stats_error(const float* fr_a, const float* fr_b, long long n_fr,
                         const float* cov_a, const float* cov_b, long long n_cov,
                         float* out /*[4]*/, float* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Per-trial correlations and van Rossum distances of the recorded-data report
 * (compute_metrics.py:306-480 of the reference, which takes them from Elephant
 * on the host; here compute_metrics.py --device gpu).  Functions added under
 * ABI 20; the same in both precision builds (nothing here touches an
 * activation type).  Strides in elements, as for cg_spike_stats: a (B, T, C)
 * batch inside a pitch-128 buffer and a (rows, T) array are read in place;
 * a frame counts as a spike when it is != 0.
 * ------------------------------------------------------------------------- */
/* Summed kernel matrix and van Rossum distances between the C trains of every
 * sample, on the 24-Hz frame grid (van_rossum.hip; the numpy statement is
 * spike_metrics.van_rossum_gram_frames / van_rossum_distance_frames):
 *   gram[b][i][j] = S_ij = sum_{k in i, l in j} decay^|f_k - f_l|
 *                 = G_ij + G_ji, G = M' Sp^T, M' the half-weighted causal filter
 *                   h = s[t] / 2; m' = fl(fl(decay m) + h); M'[t] = m'; m = fl(m' + h)
 *                   (each operation rounded to float64 on its own, m = 0 first)
 *   dist[b][i][j] = sqrt(max(fl(fl(S_ii + S_jj) - 2 S_ij), 0))
 * with decay = exp(-1 / (24 tau)) formed by the caller.  The products run on
 * v_mfma_f64_16x16x4_f64: M' is the statement's bit for bit, only the order of
 * the sum over frames belongs to the matrix pipe (decay 1, 0 and, while T <= 40,
 * 0.5 make every sum exact).  Both outputs are symmetric bit for bit, the
 * diagonal of dist is exactly 0, and the same input gives the same bits every
 * call (no atomics, no scratch memory, nothing zeroed beforehand).
 * gram / dist: float64 [B][C][C]; either may be NULL, not both.
 * CG_EINVAL (nothing launched): a NULL spikes, both outputs NULL, B, T or C < 1,
 * T > 2^24, C > 4096, decay outside [0, 1] (NaN included). */
int cg_van_rossum(const float* spikes, int B, int T, int C, long long s_b,
                  long long s_t, long long s_c, double decay, double* gram,
                  double* dist, void* stream);
/* Pearson correlation of the 500-ms bin counts (12 frames per bin, a trailing
 * partial bin dropped, nb = T / 12) between the C trains of every sample
 * (spike_metrics.correlation_coefficients_exact): with the exact integer sums
 * S_i = sum n_i, S_ij = sum n_i n_j kept in 64 bits,
 *   num = nb S_ij - S_i S_j, v_i = nb S_ii - S_i^2, r_ij = num / sqrt(v_i v_j)
 * (num, v_i, v_j converted to float64 before the product).  NaN where a train's
 * counts do not vary, as np.corrcoef gives.  corr: float64 [B][C][C], symmetric
 * bit for bit.  CG_EINVAL as cg_spike_stats: nb < 2, or 4 C + nb C > 60 KiB. */
int cg_spike_corrcoef(const float* spikes, int B, int T, int C, long long s_b,
                      long long s_t, long long s_c, double* corr, void* stream);
/* Victor-Purpura edit distances between the C trains of every sample, on the
 * 24-Hz frame grid (victor_purpura.hip; the numpy statement is
 * spike_metrics.victor_purpura_distance_frames).  With f_i the ascending frame
 * indices of the non-zero entries of train i and n_i their number,
 *   G[k][0] = k, G[0][l] = l,
 *   G[k][l] = min(G[k-1][l] + 1, G[k][l-1] + 1,
 *                 G[k-1][l-1] + fl(qf |f_a[k-1] - f_b[l-1]|)),
 *   dist[.][a][b] = G[n_a][n_b]   (a, b the two trains of the pair),
 * every operation rounded to float64 on its own (no fused multiply-add), the
 * frame difference an exact integer.  qf = q / 24 is formed by the caller
 * (spike_metrics.victor_purpura_cost).  Only sums and minima of non-NaN values:
 * the result equals the statement bit for bit.  dist: float64 [B][C][C],
 * symmetric bit for bit, diagonal exactly 0, the same bits every call (no
 * atomics; nothing in ws or dist has to be zeroed beforehand).  Two launches on
 * `stream`: the trains are compacted to frame indices in ws, then one 16-lane
 * row per pair sweeps the programme in strips of 16 columns.  A pair costs
 * O(n_a n_b) whatever qf is (no time band).
 * ws: cg_victor_purpura_ws_bytes(B, T, C) bytes, 8-byte aligned: one boundary
 * line of T + 1 float64 per resident pair (at most 8192 of them), 4 B C bytes
 * of counts and 2 B C T bytes of frame indices.  -1 for an unsupported shape.
 * Limits: B <= 65536, T <= 16384 (uint16 frame indices), C <= 4096.
 * CG_EINVAL (nothing launched): a NULL spikes, dist or ws, B, T or C < 1 or over
 * the limits, qf negative or NaN, ws_bytes too small or ws misaligned. */
long long cg_victor_purpura_ws_bytes(int B, int T, int C);
int cg_victor_purpura(const float* spikes, int B, int T, int C, long long s_b,
                      long long s_t, long long s_c, double qf, double* dist,
                      void* ws, long long ws_bytes, void* stream);
/* Histogram counts behind the KL figures of that report (pair_hist.hip; the
 * numpy statement is spike_metrics.pair_histograms).  Added under ABI 20.  For
 * pair p, side a is the set of a[p][i][j] with i < j that are not NaN, side b
 * the same from b; valid[p] holds the two set sizes.  The pooled values are cut
 * exactly as pandas.cut(pooled, bins=num_bins) cuts them (right-closed bins):
 *   mn, mx the pooled minimum and maximum (a zero maximum is taken as +0)
 *   mn == mx:  mn -= (mn != 0 ? 0.001 |mn| : 0.001),
 *              mx += (mx != 0 ? 0.001 |mx| : 0.001)
 *   otherwise: adj = (mx - mn) 0.001
 *   step = (mx - mn) / num_bins
 *   e[k] = fl(fl(k step) + mn)  (step == 0: fl(fl(fl(k / num_bins) (mx - mn)) + mn))
 *   e[num_bins] = mx;  mn != mx: e[0] -= adj
 *   id(x) = number of edges < x;  x counts in bin id - 1 when 1 <= id <= num_bins
 * every operation rounded to float64 on its own (no fused multiply-add).  The
 * bin comes from comparing x with the edges, not from (x - mn) / step.
 * status[p] is a bit set: 1 a side is empty, 2 a pooled value is infinite, 4 two
 * edges coincide (looked for only when there is a value and none is infinite).
 * With status != 0 the pair's counts and edges are written as zeros, valid as
 * counted.  counts: int32 [P][2][num_bins]; valid: int32 [P][2]; edges: float64
 * [P][num_bins + 1] or NULL; status: int32 [P].  One launch, one workgroup per
 * pair; every output element is written (nothing has to be zeroed beforehand),
 * no global atomics, no workspace, the same bits every call.  Strides in
 * elements, any sign.
 * CG_EINVAL (nothing launched): a NULL a, b, counts, valid or status, P < 1,
 * C < 2 or C > 4096, num_bins < 1 or num_bins > 256. */
int cg_pair_histogram(const double* a, long long a_sp, long long a_si,
                      long long a_sj, const double* b, long long b_sp,
                      long long b_si, long long b_sj, int P, int C, int num_bins,
                      int* counts, int* valid, double* edges, int* status,
                      void* stream);
/* Cross-correlograms of the C trains of every sample (spike_ccg.hip; the numpy
 * statement is spike_metrics.cross_correlogram).  Added under ABI 20.  With
 * s_i(t) = [spikes[b * s_b + t * s_t + i * s_c] != 0] (a NaN is a spike, -0.0 is
 * not),
 *   ccg[b][tau][i][j] = sum_{t = 0}^{T - 1 - tau} s_i(t) s_j(t + tau),
 *                       tau = 0 .. max_lag
 * -- how often neuron j fires tau frames after neuron i; a lag tau >= T gives
 * zeros, and frames of sample b never pair with frames of sample b + 1.  The
 * diagonal of the plane tau = 0 holds the spike counts, the diagonals of the
 * others the autocorrelograms.  ccg: int32 [B][max_lag + 1][C][C].
 * The products run on v_mfma_f32_16x16x32_bf16 with time as the K dimension: 0
 * and 1 are exact in bf16 and an f32 sum of at most 2^24 of their products is
 * exact, hence T <= 2^24 and every count is the exact integer.  One launch; a
 * workgroup owns a 64 x 64 block of neurons of one sample at 8 consecutive lags
 * over the whole of T, so every element is written exactly once: nothing has
 * to be zeroed beforehand, no global atomics, no workspace, the same bits every
 * call.
 * CG_EINVAL (nothing launched): a NULL spikes or ccg, B, T or C < 1, T > 2^24,
 * C > CG_CCG_MAX_C, max_lag < 0 or max_lag > CG_CCG_MAX_LAG. */
#define CG_CCG_MAX_C 1024
#define CG_CCG_MAX_LAG 256
int cg_spike_ccg(const float* spikes, int B, int T, int C, long long s_b,
                 long long s_t, long long s_c, int max_lag, int* ccg,
                 void* stream);
/* Population counts (spike_ccg.hip; spike_metrics.population_count_histogram):
 *   hist[b][k] = number of frames t < T of sample b in which exactly k of the C
 *                neurons fire, k = 0 .. C
 * hist: int32 [B][C + 1]; every row sums to T.  One workgroup per sample counts
 * into a table in LDS and writes every element: nothing has to be zeroed
 * beforehand, no global atomics, the same bits every call.
 * CG_EINVAL (nothing launched): a NULL spikes or hist, B, T or C < 1, T > 2^24,
 * C > CG_CCG_MAX_C. */
int cg_spike_population_hist(const float* spikes, int B, int T, int C,
                             long long s_b, long long s_t, long long s_c,
                             int* hist, void* stream);

/* Pattern counts of the surrogate experiment (patterns.hip; the numpy statement
 * is spike_metrics.pattern_histogram).  Added under ABI 20.  A sample is T time
 * steps x C neurons, K = T C bits:
 *   bit(n, t, c) = spikes[n * s_n + t * s_t + c * s_c] != 0
 *                  (the spike kernels' convention: a NaN is a spike, -0.0 is not)
 *   code(n)      = sum_{t, c} bit(n, t, c) << (t * C + c)
 *   counts[code] = number of samples n < N with that code, int64 [1 << K]
 * Strides in elements, any sign: a (n, neurons, L) array is read in place as
 * its (n, L, neurons) view.  Every element of counts is written by the call
 * (its first launch zeroes them; no memset node), nothing has to be zeroed
 * beforehand, and the same input gives the same bits every call: the additions
 * are integer atomics.
 * K <= CG_PATTERN_HIST_LDS_BITS: each workgroup counts into a private table in
 * LDS and adds its non-zero entries to counts once.  Above: every count goes
 * straight to global memory.  A workgroup takes CG_PATTERN_HIST_BLOCK_SAMPLES
 * samples at a time and the grid has at most CG_PATTERN_HIST_MAX_BLOCKS
 * workgroups, so one pass of the grid covers their product.
 * ws: cg_pattern_hist_ws_bytes(N, T, C) bytes (0 for both present forms, which
 * add into counts itself: ws may then be NULL; -1 for a shape the call refuses).
 * CG_EINVAL (nothing launched, counts untouched): a NULL spikes or counts,
 * N < 1 or N > 2^40 (a workgroup's table is 32-bit), T < 1, C < 1,
 * K > CG_PATTERN_HIST_MAX_BITS, ws_bytes smaller than
 * cg_pattern_hist_ws_bytes reports. */
#define CG_PATTERN_HIST_MAX_BITS 24
#define CG_PATTERN_HIST_LDS_BITS 13
#define CG_PATTERN_HIST_BLOCK_SAMPLES 1024
#define CG_PATTERN_HIST_MAX_BLOCKS 512
long long cg_pattern_hist_ws_bytes(long long N, int T, int C);
int cg_pattern_histogram(const float* spikes, long long N, int T, int C,
                         long long s_n, long long s_t, long long s_c,
                         long long* counts, void* ws, long long ws_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------
 * FFT datasets (ifft.hip; the reference's generate_tfrecords.py --fft stores a
 * trace as its spectrum along time, channels [real | imag], and inverts it on
 * the host in utils.reverse_preprocessing, gan/utils/utils.py:35-63).  Added
 * under ABI 20; the same float32 code in both precision builds.
 * ------------------------------------------------------------------------- */
/* Real part of the inverse DFT along time of every (sample, neuron) of a
 * (B, T, >= 2 C) float32 batch (the numpy statement is utils.ifft_channels):
 *   y[b][t][c] = Re((1/T) sum_k (xr_k + i xi_k) e^{+2 pi i k t / T})
 *   xr_k = x[b * s_b + k * s_t + c * s_c] * scale + offset
 *   xi_k = x[b * s_b + k * s_t + (C + c) * s_c] * scale + offset
 * the product and the sum each rounded to float32 and not contracted (the
 * denormalisation of a float32 array, as for cg_oasis_ar1_batched), y at
 * y[b * y_sb + t * y_st + c * y_sc].  Strides in elements, any values: a
 * channel-padded generator output and permuted views are read in place, and
 * only the B T C elements of y are written.  x and y must not overlap.
 * One launch on `stream`, one workgroup per (sample, group of min(16, 8192 / T)
 * neurons) up to 1024 workgroups, grid-stride beyond; radix-4 (one radix-2
 * stage when log2 T is odd) decimation in frequency in LDS, twiddles by float64
 * sincospi rounded to float32, the 1/T scale exact.  No atomics, no workspace,
 * the same bits every call.
 * CG_EINVAL (nothing launched): a NULL x or y, B, T or C < 1, T not a power of
 * two or outside 32 .. 8192. */
int cg_ifft_channels(const float* x, int B, int T, int C,
                     long long s_b, long long s_t, long long s_c,
                     float scale, float offset,
                     float* y, long long y_sb, long long y_st, long long y_sc,
                     void* stream);

/* ---------------------------------------------------------------------------
 * Power spectra of calcium traces (trace_psd.hip; compute_metrics.py
 * --spectral_metrics: not in the reference, whose reports look at the traces
 * only after deconvolution).  Added under ABI 20; the same float32 / float64
 * code in both precision builds.
 * ------------------------------------------------------------------------- */
/* Periodogram of every neuron of a (B, T, C) float32 batch, summed over the
 * trials (the numpy statement is signals_metrics.trace_power_spectrum):
 *   m = float32(sum_t float64(x_t) / T)
 *   w_t = float32(0.5 - 0.5 cospi(2 t / T))            (periodic Hann)
 *   y_t = (x_t - m) w_t, the difference and the product each rounded to float32
 *   totals[k * C + c] = sum_b |sum_t y_t e^{-2 pi i k t / T}|^2,  k = 0 .. T / 2
 * x_t = x[b * s_b + t * s_t + c * s_c], strides in elements, any values (a
 * stored (B, C, T) array viewed (B, T, C) and a padded channel pitch are read in
 * place), every element read once.  totals is float64 (T / 2 + 1, C),
 * contiguous and un-normalised: divide by B sum_t w_t^2 = B 3 T / 8 for a
 * spectrum in which white noise of variance s^2 has the level s^2.
 * The transform is float32 (the stages of cg_ifft_channels, two neurons packed
 * into one complex trace: a neuron's error is relative to the larger norm of
 * its pair); |.|^2 and every sum over trials are float64.  A neuron with a
 * non-finite sample in any trial has NaN in all its totals and changes no other
 * neuron's bits: zeros are transformed in place of such a trace.  A constant
 * trace gives exact zeros.
 * Two launches on `stream`: one workgroup per (group of 2 min(16, 8192 / T)
 * neurons, chunk of consecutive trials) up to 1024, grid-stride beyond, writes
 * float64 partial sums [chunks][T / 2 + 1][C] to ws; the second adds the chunks
 * in index order.  The chunking depends on (B, T, C) alone and every partial
 * element is written: nothing has to be zeroed, no atomics, no host sync, the
 * same bits every call.  Only the (T / 2 + 1) C elements of totals are written.
 * cg_trace_psd_ws_bytes: bytes of `ws` (8-byte aligned; contents do not
 * matter), -1 for arguments cg_trace_psd refuses.
 * CG_EINVAL (nothing launched): a NULL x, totals or ws, ws not 8-byte aligned,
 * B or C < 1, T not a power of two or outside 32 .. 8192. */
long long cg_trace_psd_ws_bytes(int B, int T, int C);
int cg_trace_psd(const float* x, int B, int T, int C,
                 long long s_b, long long s_t, long long s_c,
                 double* totals, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Nearest stretch of the recording to every trial (nearest_stretch.hip;
 * compute_metrics.py --novelty_metrics: not in the reference, none of whose
 * figures tells a generator that replays the recording from one that learned
 * it).  Added under ABI 20; the same float32 / float64 code in both precision
 * builds.
 * ------------------------------------------------------------------------- */
/* Squared distances from N query trials (N, L, C) to every stretch of L rows of
 * a (T_raw, C) float32 recording that starts on the grid s_j = j step, j < S =
 * (T_raw - L) / step + 1 (the numpy statement is
 * signals_metrics.nearest_stretch):
 *   d2[n * S + j] = sum_{t, c} (q[n][t][c] - raw[s_j + t][c])^2
 * evaluated as (|q_n|^2 + W_j) - 2 sum q r with every term float64 (the float32
 * products are exact there), clamped at 0; within 4 K 2^-53 (|q_n|^2 + W_j), K =
 * L C, of the difference form, and equal to it bit for bit on data whose sums
 * are exact.  A non-finite d2 is stored as NaN: a non-finite sample of a query
 * spoils that query's row, a non-finite row of the recording the offsets whose
 * stretch covers it, nothing else.
 *   nearest[n] = the least finite d2[n][j] over the admitted j, index[n] the
 *   lowest j that attains it; NaN and -1 where no admitted d2 is finite.
 * Offset j is left out for query n when exclude is non-NULL, exclude[n] >= 0
 * and |s_j - exclude[n]| < exclude_len (exclude: device int32 [N] of start
 * rows, negative for none).  d2 holds every offset's distance, admitted or not.
 * q at q[n * q_sn + t * q_st + c * q_sc], raw at raw[row * r_st + c * r_sc],
 * strides in elements, any values; nothing is copied or padded.  d2 (may be
 * NULL: then nothing of size N S is written outside ws) is float64 (N, S),
 * nearest float64 [N], index int32 [N], all contiguous and written whole.
 * Five launches on `stream`: squared norms of the queries and of the
 * recording's rows, W_j as the sum of its own L rows (no difference of running
 * sums), the products on v_mfma_f64_16x16x4_f64 with the recording's rows of a
 * tile of 64 offsets staged in LDS once per chunk of K (while 63 step C + 64
 * <= 18432; read from global memory beyond) and K split over up to 16
 * workgroups whose partial sums [splits][N][S rounded up to 64] go to ws, their
 * sum in split order with the minimum of every 1024 offsets, and an ordered
 * pass over those.  The plan depends on the shape alone: no atomics, nothing to
 * zero beforehand, no host sync, the same bits every call.
 * cg_nearest_stretch_ws_bytes: bytes of `ws` (8-byte aligned; contents do not
 * matter), -1 for a shape cg_nearest_stretch refuses.
 * CG_EINVAL (nothing launched, nothing written): a NULL q, raw, nearest, index
 * or ws, ws not 8-byte aligned, N, L, C or step < 1, L > T_raw, exclude_len <
 * 0, N > 65535, L C > 2^30, T_raw C > 2^40, T_raw >= 2^31 - 64 (so S < 2^31),
 * step > 2^20. */
long long cg_nearest_stretch_ws_bytes(int N, int L, int C, long long T_raw,
                                      int step);
int cg_nearest_stretch(const float* q, int N, int L, int C,
                       long long q_sn, long long q_st, long long q_sc,
                       const float* raw, long long T_raw,
                       long long r_st, long long r_sc, int step,
                       const int* exclude, int exclude_len,
                       double* d2, double* nearest, int* index,
                       void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Population states and their nearest neighbours (state_neighbours.hip;
 * compute_metrics.py --state_metrics: improved precision / recall and coverage
 * of the generated population states against the recorded ones; not in the
 * reference, whose figures all compare averages over trials).  Added under ABI
 * 20; the same code in both precision builds.
 * ------------------------------------------------------------------------- */
/* A state is the vector of spike counts of the C neurons of a trial in one bin
 * of `bin` frames (the numpy statement is spike_metrics.population_states):
 *   x[n * nb + b][c] = #{t in [b bin, (b + 1) bin) : trains[n * s_b + t * s_t +
 *                        c * s_c] != 0},   nb = T / bin (a partial bin is dropped)
 * (a NaN is a spike, -0.0 is not).  Strides in elements, any values; every
 * element of the bins is read once.  states: bf16 [B nb][Cp], Cp = C rounded up
 * to CG_STATE_K_STEP, 16-byte aligned, written whole: the counts 0 .. bin are
 * exact in bf16 and columns C .. Cp - 1 are zeros.  One launch, no atomics.
 * CG_EINVAL (nothing launched, nothing written): a NULL trains or states,
 * states not 16-byte aligned, B, T or C < 1, bin < 1 or > CG_STATE_MAX_BIN,
 * T < bin, C > CG_STATE_MAX_C, C bin^2 > CG_STATE_EXACT_SUM, B nb >
 * CG_STATE_MAX_ROWS. */
#define CG_STATE_K_STEP 32
#define CG_STATE_MAX_BIN 127
#define CG_STATE_MAX_C 4096
#define CG_STATE_MAX_ROWS 16777216
#define CG_STATE_EXACT_SUM 16777216
#define CG_STATE_MAX_K 8
#define CG_STATE_NONE 2147483647
int cg_population_states(const float* trains, int B, int T, int C,
                         long long s_b, long long s_t, long long s_c, int bin,
                         void* states, void* stream);
/* Neighbour query of a set A of Sa states against a set B of Sb states, both as
 * cg_population_states writes them (values 0 .. bin; the numpy statement is
 * spike_metrics.state_neighbours).  d2(x, y) = sum_c (x_c - y_c)^2, an integer.
 *   knn[i * k + 0 .. k - 1] = the k smallest d2(a_i, b_j) over the admitted j,
 *                             ascending; CG_STATE_NONE where fewer are admitted
 *   within[i] = #{admitted j : d2(a_i, b_j) <= radius_b[j]}
 * Every j < Sb is admitted, except j == i when exclude_self != 0 (by index: a
 * duplicate of a_i elsewhere counts, at distance 0).  knn int32 [Sa][k], within
 * int32 [Sa], radius_b int32 [Sb]; knn or within may be NULL (not both), within
 * and radius_b are given together or not at all.
 * d2 = |a_i|^2 + |b_j|^2 - 2 a_i . b_j with the products on
 * v_mfma_f32_16x16x32_bf16 (K = the neurons): every partial sum is an integer
 * of at most C bin^2 <= CG_STATE_EXACT_SUM = 2^24, which f32 holds, so every d2
 * is the exact integer.  Hence the limits: C <= CG_STATE_MAX_C with C bin^2 <=
 * 2^24 (C <= 1040 at bin 127, bin <= 64 at C 4096), Sa and Sb <=
 * CG_STATE_MAX_ROWS.
 * Launches on `stream`: the int32 squared norms of both sets (to ws); the
 * fused launch, in which a workgroup owns 128 states of A and a run of 64-state
 * tiles of B and every lane keeps the 8 smallest d2 and the count of one state
 * of A in registers -- nothing of size Sa Sb exists in memory; where A has few
 * states B is split over up to 64 workgroups per 128 states of A (a function of
 * Sa and Sb alone) whose lists and counts go to ws, and one more launch merges
 * them in split order.  No atomics, nothing to zero beforehand, no host sync,
 * the same bits every call.
 * cg_state_neighbours_ws_bytes: bytes of `ws` (16-byte aligned; contents do not
 * matter), -1 for a shape cg_state_neighbours refuses.
 * CG_EINVAL (nothing launched, nothing written): a NULL a, b or ws; a, b or ws
 * not 16-byte aligned; radius_b, knn or within not 4-byte aligned; knn and
 * within both NULL; one of within and radius_b NULL and the other not; Sa, Sb or
 * C < 1; Sa or Sb > CG_STATE_MAX_ROWS; C > CG_STATE_MAX_C; bin < 1 or >
 * CG_STATE_MAX_BIN; C bin^2 > CG_STATE_EXACT_SUM; k < 1 or > CG_STATE_MAX_K;
 * exclude_self with a != b or Sa != Sb. */
long long cg_state_neighbours_ws_bytes(int Sa, int Sb, int C, int bin, int k);
int cg_state_neighbours(const void* a, int Sa, const void* b, int Sb, int C,
                        int bin, int k, int exclude_self, const int* radius_b,
                        int* knn, int* within, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Third-order spike counts of binarised population states (triplets.hip;
 * compute_metrics.py --triplet_metrics: the connected third-order correlation
 * of all neuron triplets; not in the reference, whose figures stop at pairs).
 * Added under ABI 20; the same code in both precision builds.
 * ------------------------------------------------------------------------- */
/* The binary state of neuron c in bin b of trial n (the numpy statement is
 * spike_metrics.binary_states):
 *   x[n * nb + b][c] = 1 iff some t in [b bin, (b + 1) bin) has trains[n * s_b +
 *                      t * s_t + c * s_c] != 0,   nb = T / bin (a partial bin is
 *                      dropped)
 * (a NaN is a spike, -0.0 is not), packed 32 states to a word, neuron-major:
 *   words[c * row_stride + n * wpt + w], wpt = ceil(nb / 32), bit b % 32 of word
 *   b / 32 of trial n is x[n * nb + b][c]; the tail bits of a trial's last word
 *   are zero.
 * Strides in elements, any values; every element of the whole bins is read once.
 * words: uint32, 16-byte aligned.  One launch; every word of the C x B wpt block
 * is written exactly once by a plain store and nothing else is written; nothing
 * has to be zeroed beforehand.
 * CG_EINVAL (nothing launched, nothing written): a NULL trains or words, words
 * not 16-byte aligned, B or T < 1, bin < 1, T < bin, C outside 3 ..
 * CG_TRIPLET_MAX_C, B wpt > CG_TRIPLET_MAX_WORDS, row_stride < B wpt. */
#define CG_TRIPLET_MAX_C 512
#define CG_TRIPLET_MAX_WORDS 67108863
int cg_binary_words(const float* trains, int B, int T, int C, long long s_b,
                    long long s_t, long long s_c, int bin, void* words,
                    long long row_stride, void* stream);
/* Counts of the states in which one, two and three neurons are active together,
 * from W words a neuron as cg_binary_words writes them (the numpy statement is
 * spike_metrics.triplet_counts):
 *   singles[i]      = sum_w popcount(w_i)                      int32 [C]
 *   pairs[i * C + j] = sum_w popcount(w_i & w_j)               int32 [C][C],
 *                      symmetric, the singles on the diagonal
 *   triplets[r]     = sum_w popcount(w_i & w_j & w_k)          int32 [C(C,3)],
 *                      r the rank of i < j < k in lexicographic order
 * A zero bit counts nothing, so padding bits may sit anywhere.  Every count is
 * at most 32 W < 2^31 (CG_TRIPLET_MAX_WORDS = 2^26 - 1): exact, no other bound.
 * The neurons are cut into tiles of 16; a workgroup owns one tile triple I <= J
 * <= K over a run of 64-word chunks staged in LDS, a lane two (j, k) pairs whose
 * AND it forms once per word, walking the 16 words of I as broadcast LDS reads
 * into 32 register accumulators (v_and_b32, v_bcnt_u32_b32).  Where the tile
 * triples are few the words are split over up to 64 workgroups a triple (a
 * function of C and W alone), whose partial counts go to ws, and one more
 * launch adds them in split order.  No atomics, nothing to zero beforehand, no
 * host sync, every output written exactly once, the same bits every call.
 * cg_triplet_counts_ws_bytes: bytes of `ws` (16-byte aligned; contents do not
 * matter), -1 for a shape cg_triplet_counts refuses.
 * CG_EINVAL (nothing launched, nothing written): a NULL words, ws, singles,
 * pairs or triplets; words or ws not 16-byte aligned; an output not 4-byte
 * aligned; C outside 3 .. CG_TRIPLET_MAX_C; W outside 1 ..
 * CG_TRIPLET_MAX_WORDS; row_stride < W. */
long long cg_triplet_counts_ws_bytes(int C, int W);
int cg_triplet_counts(const void* words, int C, int W, long long row_stride,
                      int* singles, int* pairs, int* triplets, void* ws,
                      void* stream);

/* ---------------------------------------------------------------------------
 * Inter-spike intervals and spike counts of spike trains (spike_intervals.hip;
 * compute_metrics.py --interval_metrics: ISI histogram, CV, serial correlation,
 * Fano factor and count correlations; not in the reference).  Added under ABI
 * 20; the same code in both precision builds.
 * ------------------------------------------------------------------------- */
/* From the words of cg_binary_words at bin = 1 (uint32, row c at c *
 * row_stride, trial n's wpt words at n * wpt, bit t % 32 of word t / 32 the
 * frame t; a zero bit is no spike, so padding bits may sit anywhere).  Train
 * (n, c) has its spikes at t_1 < ... < t_m and the intervals I_k = t_{k+1} -
 * t_k; no interval runs from one trial into the next.  The numpy statement is
 * spike_metrics.interval_counts:
 *   hist[c * (max_isi + 1) + d - 1]  intervals of neuron c equal to d, 1 <= d <=
 *                                    max_isi, over its trials; [.. + max_isi]
 *                                    those > max_isi       int32 [C][max_isi + 1]
 *   moments[c * 6 + 0 .. 5]          spikes, intervals, sum I, sum I^2,
 *                                    consecutive pairs, sum I_k I_{k+1} (an
 *                                    overflow interval with its true length)
 *                                                          int64 [C][6]
 *   counts[n * C + c]                spikes of train (n, c)   int32 [trials][C]
 * trials wpt <= CG_TRIPLET_MAX_WORDS keeps every int32 below 2^31 and every
 * int64 below 2^62: exact, no other bound.
 * A workgroup owns a neuron and a run of trials, a wave a trial at a time in
 * chunks of 64 words, a word a lane; the two spikes before a lane's word come
 * from the ballot of the non-empty words and three cross-lane reads (a carry
 * between chunks), the set bits are walked by count-trailing-zeros into an LDS
 * histogram and register sums.  Where the neurons are few the trials are split
 * over up to 64 workgroups a neuron (a function of C and trials alone), whose
 * partial results go to ws, and one more launch adds them in split order.  No
 * global atomics, nothing to zero beforehand, no host sync, every output
 * written exactly once, the same bits every call.
 * cg_spike_intervals_ws_bytes: bytes of `ws` (16-byte aligned; contents do not
 * matter; at least 16), -1 for a shape cg_spike_intervals refuses.
 * CG_EINVAL (nothing launched, nothing written): a NULL words, ws, hist,
 * moments or counts; words or ws not 16-byte aligned; hist or counts not 4-byte
 * aligned; moments not 8-byte aligned; C outside 1 .. CG_INTERVAL_MAX_C; trials
 * or wpt < 1; trials wpt > CG_TRIPLET_MAX_WORDS; max_isi outside 1 ..
 * CG_INTERVAL_MAX_ISI; row_stride < trials wpt. */
#define CG_INTERVAL_MAX_C 4096
#define CG_INTERVAL_MAX_ISI 4095
long long cg_spike_intervals_ws_bytes(int C, int trials, int wpt, int max_isi);
int cg_spike_intervals(const void* words, int C, int trials, int wpt,
                       long long row_stride, int max_isi, int* hist,
                       long long* moments, int* counts, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Recording datasets (windows.hip; the reference's generate_tfrecords.py cuts a
 * (neurons, T) recording into overlapping stride-2 windows and writes each one
 * out; here the recording stays resident and every step's windows are cut
 * straight into the batch buffer).  Added under ABI 20; the same float32 code
 * in both precision builds.
 * ------------------------------------------------------------------------- */
/* One batch of B windows of L rows of a float32 (T_raw, C) recording (the numpy
 * statement is dataset_helper.window_batch).  Row t of window b is raw row
 * clamp(starts[b] + t, 0, T_raw - 1): nothing outside raw is ever read,
 * whatever starts holds, and a window past either end repeats the edge row.
 * raw at raw[row * r_st + c * r_sc], strides in elements, any values (a stored
 * (C, T) array viewed transposed is read in place); starts is a device int32[B].
 *   fft == 0: y is (B, L, C), y[b * y_sb + t * y_st + c * y_sc] = (v - sub) / div
 *             with v the raw value; 16-byte accesses where r_sc == y_sc == 1 and
 *             the alignment allows, one element at a time otherwise
 *   fft != 0: y is (B, L, 2 C); channel c is the real and channel C + c the
 *             imaginary part of sum_t x_t e^{-2 pi i k t / L} (unscaled; the
 *             layout of utils.fft_channels), each written as (v - sub) / div.
 *             Shaped as cg_ifft_channels: one workgroup per (window, group of
 *             min(16, 8192 / L) neurons) up to 1024, grid-stride beyond.  An
 *             all-zero trace gives an all-zero spectrum.
 * (v - sub) / div is the float32 difference, then the IEEE float32 quotient,
 * not contracted, no reciprocal: v itself, bit for bit, with sub = 0, div = 1.
 * One launch on `stream`; no atomics, no workspace, no host sync, the same bits
 * every call; only the window elements of y are written.  raw and y must not
 * overlap.
 * CG_EINVAL (nothing launched): a NULL raw, starts or y, T_raw, C, B or L < 1,
 * div == 0, with fft an L that is not a power of two in 32 .. 8192. */
int cg_window_batch(const float* raw, long long T_raw, int C,
                    long long r_st, long long r_sc,
                    const int* starts, int B, int L,
                    int fft, float sub, float div,
                    float* y, long long y_sb, long long y_st, long long y_sc,
                    void* stream);

/* ---------------------------------------------------------------------------
 * Weight summaries (summary.hip; --plot_weights: the reference's
 * Summary.plot_weights, gan/utils/summary_helper.py:523-557, logs mean, stddev,
 * min, max and a histogram of every trainable variable once per epoch).  Added
 * under ABI 20; the same float32 / float64 code in both precision builds.
 * ------------------------------------------------------------------------- */
/* Statistics and equal-width histogram buckets of nseg segments of one float32
 * buffer, in one call (the numpy statements are summary_helper.
 * variable_statistics and summary_helper.histogram_buckets).  Segment s is the
 * n = seg_len[s] values at data + seg_off[s]; seg_off and seg_len are DEVICE
 * int64 tables [nseg] in elements.  Offsets are arbitrary (a 16-byte aligned
 * segment is read as float4), segments may overlap or repeat, the input is
 * only read, and no element outside a segment is read.  total_len is the sum of
 * seg_len, from the caller (it sizes the workspace; the per-segment work is laid
 * out on the device).  seg_len[s] must be in 1 .. 2^31 - 1: the tables are
 * device memory, a violation is the caller's error.
 * For a segment whose values are all finite, with d = (double)x and every
 * operation rounded to float64 on its own (no fused multiply-add):
 *   mn = min d, mx = max d (by value; a zero maximum is returned as +0)
 *   sum = sum of d, mean = sum / n, sq = sum of (d - mean)^2,
 *   stddev = sqrt(sq / n), range = mx - mn, k = num_buckets
 *   range == 0:  one bucket (mn - 0.5, mn + 0.5, n)
 *   otherwise:   w = range / k
 *                idx(d) = min((long)floor((d - mn) / w), k - 1)
 *                e[j] = mn + fl(j w) for j < k, e[k] = mx
 *                bucket j = (e[j], e[j + 1], (double)#{d : idx(d) = j})
 * which is what the TensorBoard histogram summary (v2) computes for buckets =
 * 30.  (d - mn) / w is the correctly rounded float64 quotient.
 * stats: float64 [nseg][8] = {n, mn, mx, sum, mean, sq, stddev, nonfinite},
 * nonfinite the number of NaN or +-Inf values of the segment; buckets: float64
 * [nseg][num_buckets][3] = (left, right, count).  range == 0: row 0 holds the
 * single bucket, the other rows zeros.  nonfinite > 0: stats[1 .. 6] are NaN and
 * every bucket row is zero; other segments are unaffected.
 * Every element of stats and buckets is written (nothing has to be zeroed
 * beforehand; what the workspace needs zeroed is zeroed by a kernel of the
 * call).  Five launches on `stream` whatever nseg is: a segment is cut into
 * chunks of 4096 elements, one workgroup per chunk, and the chunks' partial
 * results are folded per segment in index order -- no floating-point atomics
 * (the counts meet through integer atomics, which are exact), the same bits
 * every call.
 * cg_tensor_summary_ws_bytes: bytes of `ws` (8-byte aligned; contents do not
 * matter), -1 for arguments cg_tensor_summary refuses.
 * CG_EINVAL (nothing launched): a NULL pointer, nseg outside 1 .. 65535,
 * num_buckets outside 1 .. 512, total_len < 1, ws_bytes too small or ws not
 * 8-byte aligned. */
long long cg_tensor_summary_ws_bytes(int nseg, long long total_len,
                                     int num_buckets);
int cg_tensor_summary(const float* data, const long long* seg_off,
                      const long long* seg_len, int nseg, long long total_len,
                      int num_buckets, double* stats, double* buckets, void* ws,
                      long long ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The MLP model (gan/models/mlp.py:15-77): float32 Dense over rows with
 * counter-based dropout (mlp.hip).  Everything in this section is float32 in
 * both builds.  Operands are row-major; W is the Keras kernel (in, out); inputs
 * are read through a row pitch (in floats) and outputs are written densely.
 * act(z) = max(z, alpha z), alpha in {0.3, 0, 1}.
 *
 * Dropout.  The keep decision of element e of a layer's (rows x Cout) output is
 * word e & 3 of the Philox4x32-10 block with counter words (lo(e >> 2),
 * hi(e >> 2), lo(stream_id), hi(stream_id)) and key (lo(seed), hi(seed)):
 * kept iff word >= floor(p 2^32).  Kept elements are multiplied by
 * float32(1 / (1 - p)), the others are exactly 0.  p == 0 runs no generator.
 * Nothing is stored between launches: the backward kernels read the decision
 * back from the stored h (h > 0: slope 1, h < 0: slope alpha, h == 0: dropped).
 *
 * Limits: Cin, Cout >= 1, the smaller of the two <= CG_MLP_MAX_WIDTH (a layer
 * width) and the larger <= CG_MLP_MAX_FLAT (the flattened time x width side of
 * the generator's first Dense and of the critic's head); 0 <= p < 1.  Outside
 * them, for rows <= 0 and for a NULL pointer where one is needed the functions
 * return CG_EINVAL before anything touches HIP: nothing is written.
 * ------------------------------------------------------------------------- */
#define CG_MLP_MAX_WIDTH 1024
#define CG_MLP_MAX_FLAT 65536
/* cg_mlp_dense_fwd modes */
#define CG_MLP_FWD_ACT 0      /* h = drop(act(x W + b)) */
#define CG_MLP_FWD_TANGENT 1  /* h = m(h_mask) * (x W): no bias, no act; m = the
                                 stored h's s * keep * act' (the tangent chain of
                                 the penalty's second backward) */
#define CG_MLP_FWD_SIGMOID 2  /* h = sigmoid(x W + b), no dropout */
/* cg_mlp_dense_dgrad modes */
#define CG_MLP_BWD_MASK 0     /* dz = dh * m(h) */
#define CG_MLP_BWD_SIGMOID 1  /* dz = dh * h (1 - h), h the sigmoid's output */
#define CG_MLP_BWD_NONE 2     /* dz = dh */

/* keep[e] = 1 / 0 for e < n: the keep mask of (seed, stream_id, p), one byte
 * per element (for tests; the Dense kernels store no mask) */
int cg_mlp_dropout_mask(void* keep, long long n, long long seed,
                        long long stream_id, double p, void* stream);
/* h [rows][Cout] from x [rows][x_pitch >= Cin]; b may be NULL (no bias);
 * h_mask [rows][Cout] is read by CG_MLP_FWD_TANGENT only. */
int cg_mlp_dense_fwd(const float* x, long long x_pitch, const float* W,
                     const float* b, const float* h_mask, float* h,
                     long long rows, int Cin, int Cout, int mode, float alpha,
                     double p, long long seed, long long stream_id,
                     void* stream);
/* dz [rows][Cout] = dh masked on the way in (mode; h [rows][Cout] the stored
 * output of the layer), dx [rows][Cin] = dz W^T.  dx may be NULL (a first
 * layer: dz only); dz must not alias dh. */
int cg_mlp_dense_dgrad(const float* dh, const float* h, const float* W,
                       float* dz, float* dx, long long rows, int Cin, int Cout,
                       int mode, float alpha, double p, void* stream);
/* dW [Cin][Cout] = sum_r c(r) x[r]^T dz[r], db [Cout] = sum_{r < bias_rows}
 * c(r) dz[r] (db may be NULL), c(r) = c0 / c1 / c2 for row r in segment
 * min(r / seg_rows, 2).  Rows >= tail_row0 read their x from x_tail (dense
 * [rows - tail_row0][Cin]) when it is non-NULL: [h_real | h_fake | tangent].
 * Ordered two-stage sums through ws (cg_mlp_wgrad_ws_elems floats, contents do
 * not matter): no atomics, the same bits on every call; dW and db are stored.
 * Each segment is summed on its own and the result is c0 S0 + c1 S1 + c2 S2
 * with every product and sum rounded separately, so S0 == S1 under c0 == -c1
 * (the head's bias gradient) gives exactly 0. */
long long cg_mlp_wgrad_ws_elems(long long rows, int Cin, int Cout);
int cg_mlp_dense_wgrad(const float* x, long long x_pitch, const float* x_tail,
                       long long tail_row0, const float* dz, float* dW,
                       float* db, long long rows, int Cin, int Cout,
                       long long seg_rows, float c0, float c1, float c2,
                       long long bias_rows, float* ws, void* stream);
/* out [3][B][n] = [real | fake | alpha_b real + (1 - alpha_b) fake]
 * (wgan_gp.py:38-41), all float32 [B][n] */
int cg_mlp_interp(const float* real, const float* fake, const float* alpha,
                  float* out, int B, long long n, void* stream);
/* norm[b] = ||g[b]||, gp = mean((norm - 1)^2), coef[b] = penalty * 2 (norm - 1)
 * / (B norm), v[b] = coef[b] g[b] (= penalty * dgp/dg; v may be NULL) and
 * loss[0] / loss[1] as cg_critic_loss's out from d_out [3B]; g, v float32
 * [B][n].  One launch, ordered sums. */
int cg_mlp_gp_loss(const float* g, const float* d_out, float* norm, float* gp,
                   float* coef, float* v, float* loss /*[2]*/, int B,
                   long long n, float penalty, void* stream);

/* ---------------------------------------------------------------------------
 * Added under ABI 20: latent correlations of the dichotomised-Gaussian model
 * of a recording (dg_fit.hip; the numpy statement is data/dg_fit.py
 * gauss_correlation, a restatement of the reference's
 * DGOptimise.get_gauss_correlation).  Everything is float64 in both builds.
 *
 * For every pair i > j, with h = gamma[i], k = gamma[j], S = cov[i][j] (the
 * lower triangle is the one that is read) and
 *   f(l) = Phi_2(h, k; l) - fl32(fl32(rates[i]) fl32(rates[j])) - S
 * (the reference's script multiplies float32 means in float32):
 *   |S| <= 1e-10                      corr 0,        status 1
 *   |f(-0.99999)| < tol               corr -0.99999, status 2
 *   else |f(0.99999)| < tol           corr 0.99999,  status 3
 *   else f(-0.99999) f(0.99999) > tol corr 0,        status 4
 *   else bisection from [-0.99999, 0.99999]: l = (l0 + l1) / 2, f = f(l),
 *     f > 0: l1 = l, f < 0: l0 = l, until |f| <= tol (status 0, iterations =
 *     evaluations of the loop) or maxiters evaluations (status 5).  A midpoint
 *     equal to an end of its bracket would be repeated by every later
 *     iteration: the pair stops there with status 5 and iterations = maxiters.
 * Phi_2 is Plackett's integral over 64 uniform panels of a 16-point
 * Gauss-Legendre rule in asin(l) u, its 1024 terms added in a fixed order
 * (sixteen runs of 64 consecutive nodes, then a tree over neighbouring runs);
 * within 1e-11 of the exact value for |h|, |k| <= 3.8.
 * corr float64, status and iterations int32, all dense [C][C]: every element is
 * written, both triangles, the diagonal 1 / 0 / 0.  cov is read through its
 * strides (in elements).  One launch: one 16-lane row per pair, a grid of at
 * most CG_DG_FIT_MAX_BLOCKS workgroups of CG_DG_FIT_BLOCK_PAIRS pairs that
 * walks the pairs.  No atomics, no workspace: the same bits every call.
 * CG_EINVAL (nothing launched): a NULL pointer, C < 2 or C > 4096, tol <= 0 (or
 * NaN), maxiters < 1. */
#define CG_DG_FIT_MAX_BLOCKS 1024
#define CG_DG_FIT_BLOCK_PAIRS 4
int cg_dg_correlation(const double* rates, const double* gamma,
                      const double* cov, long long cov_s0, long long cov_s1,
                      int C, double tol, int maxiters, double* corr,
                      int* status, int* iterations, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CALCIUMGAN_HIP_H_ */
