/*
 * tem_hip.h -- C ABI of libtem_hip.so, the MI355X (gfx950) implementation of the
 * arithmetic that transfer_em's CycleGAN hot path delegates to TensorFlow.
 *
 * The reference (janelia-flyem/transfer_em) has no FFI of its own: its hot path is
 * Python calling tf.keras layers.  Each entry point below replaces
 * the TF kernels behind the cited reference call sites (paths relative to the
 * reference root).  Conventions for every function:
 *
 *   - plain C types only; all pointers are DEVICE pointers owned by the caller;
 *   - activations are float32, channels-last (N,D,H,W,C); 2-D data is D == 1, kd == 1;
 *   - work is enqueued on `stream` (a hipStream_t); nothing allocates, frees or
 *     synchronises, so every call can be captured into a hipGraph;
 *   - returns 0 on success, a negative TEM_E* code for a rejected argument, or a
 *     positive hipError_t from the launch.
 *
 * INTEGRATION.md shows the ctypes binding the reference-side Python would add.
 */
#ifndef TEM_HIP_H
#define TEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEM_ABI_VERSION 1

#define TEM_OK            0
#define TEM_EINVAL       -1   /* malformed descriptor (NULL pointer, negative dim, ...) */
#define TEM_EUNSUPPORTED -2   /* channel count / kernel size outside the compiled set   */
#define TEM_ESHAPE       -3   /* tensor extents inconsistent with the operator geometry  */

typedef void *tem_stream_t;   /* hipStream_t */

/* Strided view of a float32 NDHWC tensor.  Strides are in elements; the channel
 * stride is 1.  A crop is a view (ptr offset + parent strides); a channel slice is
 * a view with C smaller than sW. */
typedef struct tem_view {
  float  *ptr;
  int32_t N, D, H, W, C;
  int64_t sN, sD, sH, sW;
} tem_view;

/* Fused epilogue shared by the convolution entry points.  With acc the convolution
 * result for one output element of out0 (bias already added):
 *
 *     v = acc + add[element - add_off]        (if add.ptr; zero outside add's window)
 *     v = gate > 0 ? v : gate_slope * v       (if gate.ptr: LeakyReLU *gradient*,
 *                                              gated on the saved forward output)
 *     v = keep(element) ? 2 v : 0             (if dropout: Philox4x32-10 stream
 *                                              (seed, site, step); element = dense
 *                                              NDHWC index in out0, or in the
 *                                              full tensor out0 is a window of)
 *     v = v > 0 ? v : slope * v               (forward LeakyReLU; slope 1 = linear)
 *
 * Channels written to out1 (the second half of a split output) skip add/gate/
 * dropout/slope and receive the raw accumulator.
 *
 * Replaces: tf.keras.layers.LeakyReLU (models/utils.py:77,83,126,135;
 * generator.py:57,99,109; discriminator.py:53,74,94), Dropout(0.5)
 * (models/utils.py:134) and their gradients, Cropping/Concatenate gradients
 * (generator.py:74-86).
 */
typedef struct tem_epilogue {
  const float *bias;          /* [C_out] or NULL (discriminator.py:97-99 only)        */
  float        slope;
  tem_view     gate;          /* same extents as out0, or ptr == NULL                 */
  float        gate_slope;
  tem_view     add;           /* window placed at add_off inside out0, or ptr == NULL */
  int32_t      add_off[3];
  int32_t      dropout;       /* 0 / 1                                                */
  uint64_t     seed;
  uint32_t     site;
  uint32_t     step;
  const uint32_t *step_dev;   /* if non-NULL the step is read from device memory
                                 (graph replay) and `step` is ignored               */
  /* When out0 is a window of a larger logical tensor (region-restricted execution of the cycle
   * path), the dropout element index is taken in the frame of that full tensor: voxel
   * (z,y,x) of out0 is voxel (z,y,x) + drop_org of a tensor with spatial extents drop_dims.
   * drop_dims[0] == 0: out0 itself is the full tensor. */
  int32_t      drop_org[3];
  int32_t      drop_dims[3];
  /* Optional keep mask of the dropout stream: one bit per element of the dropout frame, bit (e & 7) of byte
   * (e >> 3) for dense element index e (C_out a multiple of 8: a voxel's channels start on a byte).
   *   keep_mode 1: the kernel also WRITES the bits it draws (the forward pass of Dropout);
   *   keep_mode 2: the kernel MAY read the bits instead of re-running Philox (the matching input-gradient; a
   *                pure speed hint -- the bits are the same either way);
   *   keep_mode 0 / keep_mask NULL: no mask.
   * Mode 1 is honoured or the call returns TEM_EUNSUPPORTED. */
  uint8_t     *keep_mask;
  int32_t      keep_mode;
} tem_epilogue;

/* Weight addressing for tem_conv: element (tap, c_in, c_out) of the operator's
 * kernel is w[tap' * C_a * C_b + ...] with
 *   TEM_W_TAP_CI_CO : w[tap][c_in][c_out]                  (Keras Conv kernel, forward;
 *                                                           Keras ConvTranspose kernel
 *                                                           used as its own input-grad)
 *   TEM_W_FLIP_CO_CI: w[ntap-1-tap][c_out][c_in]           (input-gradient of a
 *                                                           stride-1 Keras Conv)       */
#define TEM_W_TAP_CI_CO  0
#define TEM_W_FLIP_CO_CI 1
/* TEM_W_WINOGRAD: `w` is the layer's kernel in the Winograd F(2x2, 3x3) domain of the (y, x) axes as tem_winograd_weights wrote it
 * (k 3, s 1, operator channel pairs C_in -> C_out in {8->8, 8->16, 16->8, 16->16, 16->32, 32->16, 32->32}, epilogues LeakyReLU /
 * LeakyReLU' gate, and for 16->16 and 32->32 gate + keep bits + split output; the call returns TEM_EUNSUPPORTED
 * otherwise -- ask tem_conv_is_tiled first).  Same operator and epilogue; the result differs from the direct form by fp32 rounding. */
#define TEM_W_WINOGRAD   2

typedef struct tem_conv_args {
  tem_view in0, in1;          /* logical input = concat(in0, in1) on C; in1.ptr may be NULL */
  const float *w;
  int32_t w_layout;
  int32_t kd, kh, kw;         /* kernel extents, each in {1,3,4}                       */
  int32_t sd, sh, sw;         /* strides, each in {1,2}                                */
  int32_t pd, ph, pw;         /* zero padding; negative == crop                        */
  tem_view out0, out1;        /* output channels [0,out0.C) and [out0.C, out0.C+out1.C) */
  tem_epilogue ep;
} tem_conv_args;

/* out[n,o,co] = sum_{tap,ci} in[n, o*s + tap - p, ci] * W(tap,ci,co)   (cross-correlation)
 *
 * Replaces the TF kernels behind tf.keras.layers.Conv2D/Conv3D forward
 * (models/utils.py:73,80,122; generator.py:54,96,108,110; discriminator.py:45,78,97),
 * Conv3DBackpropInput for the stride-1 layers (TEM_W_FLIP_CO_CI, p = k-1-p_fwd), and
 * Conv3DTranspose's input-gradient (a stride-2 convolution, models/utils.py:129). */
int tem_conv(const tem_conv_args *a, tem_stream_t stream);

/* out[n,o,co] = sum over (j,tap) with o == j*s + tap - p of in[n,j,ci] * w[tap][co][ci]
 *
 * Replaces tf.keras.layers.Conv3DTranspose forward (models/utils.py:129-130; 'same'
 * padding with k 4, s 2 is p = 1) and Conv3DBackpropInput of the stride-2 layers
 * (models/utils.py:80; p = 0, Keras kernel (tap,C_in,C_out) read as [tap][co][ci]).
 * w_layout is ignored. */
int tem_conv_transpose(const tem_conv_args *a, tem_stream_t stream);

/* The shape-generic VALU implementations behind tem_conv / tem_conv_transpose, exported so
 * that tests can compare them with the LDS/MFMA-tiled kernels the dispatcher prefers. */
int tem_conv_direct(const tem_conv_args *a, tem_stream_t stream);
int tem_conv_transpose_direct(const tem_conv_args *a, tem_stream_t stream);

/* 1 if tem_conv / tem_conv_transpose would run these arguments on the LDS/MFMA-tiled kernel
 * (then `name`, if non-NULL, receives the kernel's template name as rocprofv3 prints it), 0 if
 * on the direct kernel.  Used by bench.py to label its per-kernel timings. */
int tem_conv_is_tiled(const tem_conv_args *a, int32_t transposed, char *name, int32_t name_len);

typedef struct tem_bww_args {
  tem_view in0, in1;          /* forward input (concat on C)                           */
  tem_view dout;              /* gradient w.r.t. the pre-activation output             */
  int32_t kd, kh, kw, sd, sh, sw, pd, ph, pw;
  float  *slabs;              /* partial sums: slab s starts at slabs + s*slab_stride   */
  int64_t slab_stride;        /* elements between slabs; 0 == ntap*C_in*C_out (dense).
                                 A whole network shares one [nslab][n_params] workspace
                                 by passing slabs = ws + param_offset, stride = n_params */
  int32_t nslab;              /* number of partial slabs the voxel range is split into */
  int32_t accumulate;         /* 0: slabs are overwritten, 1: added to                 */
} tem_bww_args;

/* slab[s][tap][ci][co] (+)= sum over the s-th share of (n,o) of
 *                           in[n, o*s + tap - p, ci] * dout[n, o, co]
 *
 * Replaces Conv3DBackpropFilter (all Conv layers) and, with in := upstream gradient
 * and dout := the layer input, the kernel gradient of Conv3DTranspose in its Keras
 * layout (tap, C_out, C_in).  The split over slabs is deterministic; tem_reduce_slabs
 * finishes the sum. */
int tem_conv_bwd_weight(const tem_bww_args *a, tem_stream_t stream);

/* Workspace sizing: with a->nslab = the largest split the caller is willing to hold, returns the
 * number of slabs (<= a->nslab) the launch should be given for best occupancy of the 256 CUs
 * (the LDS-tiled kernel writes one slab per workgroup).  Pass the returned value as nslab to
 * tem_conv_bwd_weight.  a->slabs may be NULL here.  Negative: TEM_E*. */
int tem_conv_bwd_weight_nslab(const tem_bww_args *a);

/* Same as tem_conv_is_tiled for tem_conv_bwd_weight (a->nslab must be the value the launch will use). */
int tem_bww_is_tiled(const tem_bww_args *a, char *name, int32_t name_len);

/* out[i] = (accumulate ? out[i] : 0) + scale * sum_s slabs[s*slab_stride + i]
 * (slab_stride 0 == n) */
int tem_reduce_slabs(const float *slabs, int32_t nslab, int64_t n, int64_t slab_stride,
                     float *out, int32_t accumulate, float scale, tem_stream_t stream);

/* One work item of tem_reduce_slabs_multi: out[i] = scale * sum_{s < nslab} slabs[s*stride + i]
 * for i < count (count <= 64). */
typedef struct tem_reduce_item {
  const float *slabs;
  int64_t      stride;
  int32_t      nslab;
  int32_t      count;
  float       *out;
} tem_reduce_item;

/* Finishes the split-K sums of a whole network in ONE launch: `items_dev` is a device array of
 * `nitems` work items (one workgroup each) covering every kernel of the network. */
int tem_reduce_slabs_multi(const tem_reduce_item *items_dev, int32_t nitems, float scale,
                           tem_stream_t stream);

/* The discriminator's 1x1x1 head as one launch per direction (reference discriminator.py:78-99; the launch plans of
 * models/discriminator.py use it in place of two tem_conv, two tem_conv_bwd_weight, one tem_channel_sum and two
 * input-gradient launches on the 8^3 logits map):
 *   forward : p1[v][co] = LeakyReLU_slope(sum_ci e6[v][ci] w1[ci][co]);  z[v] = sum_co p1[v][co] w2[co] + bias[0]
 *   backward: g_p1 = (p1 > 0 ? 1 : slope_p1) dz w2;  g_e6 = (e6 > 0 ? 1 : slope_e6) (g_p1 . w1^T)   (g_e6 may be NULL
 *             only with slabs); with slab_w1 != NULL every workgroup b < nslab writes its partial kernel gradients
 *             slab_w1[b][32*32] (sum_v e6 (x) g_p1), slab_w2[b][32] (sum_v p1 dz), slab_b[b] (sum_v dz) -- rows of the
 *             layers' ordinary slab sets (tem_reduce_slabs_multi sums them); nslab = tem_disc_head_nslab(nvox).
 * All tensors dense float32, channels last, 32 channels (the reference hard-codes them, discriminator.py:60,72,78). */
typedef struct tem_head_bwd_args {
  const float *dz, *e6, *p1, *w1, *w2;
  float *g_e6;
  float slope_p1, slope_e6;
  float *slab_w1, *slab_w2, *slab_b;
  int32_t nslab;
  int64_t nvox;
} tem_head_bwd_args;
int tem_disc_head_nslab(int64_t nvox);
int tem_disc_head_fwd(const float *e6, const float *w1, const float *w2, const float *bias, float *p1, float *z,
                      int64_t nvox, float slope, tem_stream_t stream);
int tem_disc_head_bwd(const tem_head_bwd_args *a, tem_stream_t stream);

/* out[c] = (accumulate ? out[c] : 0) + sum over all (n,d,h,w) of g[...,c]   (bias gradient,
 * discriminator.py:97-99) */
int tem_channel_sum(const tem_view *g, float *out, int32_t accumulate, tem_stream_t stream);

/* tfa.losses.SigmoidFocalCrossEntropy(from_logits=True, alpha=0.5, gamma) with
 * Reduction.AUTO, as used by generator_loss / discriminator_loss (cgan.py:78-79,110-120).
 *   L = mean over z of 0.5 * (1-p_t)^gamma * BCEWithLogits(target, z)
 * losses[k] += loss_scale * L for every bit k set in slot_mask (losses is double[8]);
 * if dz.ptr: dz = grad_scale * dL/dz. */
int tem_focal_logits(const tem_view *z, int32_t target, float gamma,
                     double *losses, uint32_t slot_mask, float loss_scale,
                     const tem_view *dz, float grad_scale, tem_stream_t stream);

/* identity_loss / calc_cycle_loss (cgan.py:122-142): t = 1 - |a-b|/2,
 *   L = mean of 0.5 * (1-t)^gamma * -log(clip(t,eps,1-eps)+eps)   (from_logits=False form)
 * losses[k] += loss_scale * L; if db.ptr: db = grad_scale * dL/db (db has b's extents). */
int tem_focal_match(const tem_view *a, const tem_view *b, float gamma,
                    double *losses, uint32_t slot_mask, float loss_scale,
                    const tem_view *db, float grad_scale, tem_stream_t stream);

/* tf.keras.optimizers.Adam dense update (cgan.py:69-73,218-228), Keras/TF2 form:
 *   t = *step_dev + 1;  lr_t = lr*sqrt(1-b2^t)/(1-b1^t)
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  theta -= lr_t * m / (sqrt(v) + eps)
 * g = grad_scale * grad.  step_dev is NOT incremented here (see tem_step_tick). */
int tem_adam_keras(float *theta, const float *grad, float *m, float *v, int64_t n,
                   float lr, float beta1, float beta2, float eps, float grad_scale,
                   const uint32_t *step_dev, tem_stream_t stream);

/* *step_dev += 1 (one thread). */
int tem_step_tick(uint32_t *step_dev, tem_stream_t stream);

/* Keep bits of (up to two) Dropout(0.5) layers (models/utils.py:134) for one step, written ahead of the transposed
 * convolutions that apply them: bit e of mask = keep(element e) of the Philox4x32-10 stream (seed, site, step) that
 * tem_epilogue.dropout draws from -- the layout tem_epilogue.keep_mask (keep_mode 2) reads.  nbytes = ceil(elements / 128)
 * * 16 (whole Philox blocks; 16-byte aligned); mask1 may be NULL.  step_dev (device counter) overrides step when non-NULL. */
int tem_dropout_masks(uint8_t *mask0, int64_t nbytes0, uint32_t site0, uint8_t *mask1, int64_t nbytes1, uint32_t site1,
                      uint64_t seed, const uint32_t *step_dev, uint32_t step, tem_stream_t stream);

/* datasets.py:193-202 + 157-163: out = ((float)in / 127.5 - 1 - mean) / std */
int tem_u8_to_f32_std(const uint8_t *in, float *out, int64_t n, float mean, float std,
                      tem_stream_t stream);

/* utils.py:109,118: out = (uint8) rint((y*std + mean + 1) * 127.5)  (wraps mod 256).
 * `y` is a view (tile interior), `out` a dense-by-strides uint8 block with element
 * strides oD,oH,oW (batch 1, channel 0). */
int tem_f32_unstd_to_u8(const tem_view *y, uint8_t *out, int64_t oD, int64_t oH, int64_t oW,
                        float mean, float std, tem_stream_t stream);

/* Tiled inference, input side (utils.py:77-89 with the cloud fetch replaced by a resident uint8 volume
 * vol[Z][Y][X]): tile t of out[ntile][edge][edge][edge] = the window of `vol` at origin
 * (z,y,x) = origins_dev[3t..3t+2] -- voxels outside the volume read as 0 -- converted as tem_u8_to_f32_std. */
int tem_u8_tiles_to_f32_std(const uint8_t *vol, int32_t Z, int32_t Y, int32_t X, const int32_t *origins_dev,
                            int32_t ntile, int32_t edge, float *out, float mean, float std, tem_stream_t stream);

/* Tiled inference, output side (utils.py:107-126): the interior of tile t of y[ntile][yedge]^3 (`tpad` voxels
 * stripped per face, utils.py:113-116) is converted as tem_f32_unstd_to_u8 and written into the uint8 volume
 * out[OZ][OY][OX] at (z,y,x) = index_dev[3t..3t+2].  The caller guarantees the blocks lie inside `out`. */
int tem_f32_tiles_unstd_to_u8(const float *y, int32_t ntile, int32_t yedge, int32_t tpad, const int32_t *index_dev,
                              uint8_t *out, int32_t OZ, int32_t OY, int32_t OX, float mean, float std,
                              tem_stream_t stream);

/* Tiled inference of the 2-D networks, input side: tile t of out[ntile][edge][edge] = the edge x edge window of
 * section z of the uint8 volume vol[Z][Y][X] at origin (z,y,x) = origins_dev[3t..3t+2] -- pixels outside the volume
 * (sections outside [0, Z) included) read as 0 -- converted as tem_u8_to_f32_std.  Any ntile; no z halo. */
int tem_u8_tiles2d_to_f32_std(const uint8_t *vol, int32_t Z, int32_t Y, int32_t X, const int32_t *origins_dev,
                              int32_t ntile, int32_t edge, float *out, float mean, float std, tem_stream_t stream);

/* Tiled inference with a boundary mode at the volume's faces.  tem_u8_tiles_to_f32_std / tem_u8_tiles2d_to_f32_std
 * read a voxel outside the volume as 0; these read, on every axis, index fold(i, n) of an axis of extent n:
 *   TEM_BOUNDARY_EDGE      clamp(i, 0, n-1)
 *   TEM_BOUNDARY_REFLECT   n == 1: 0; else m = 2(n-1), r = i mod m (non-negative), r < n ? r : m - r
 * (numpy.pad's "edge" and "reflect" for any pad width).  The volume has extents (Z, Y, X); `blk`[BZ][BY][BX] holds
 * its box at (lz, ly, lx), which must lie inside it (the resident form: blk = the volume, l = 0).  Tile t is the
 * window at block-relative origin (z,y,x) = origins_dev[3t..3t+2]: its voxel p has volume coordinate l + origin + p
 * (|l + origin| + edge must stay below 2^31), is folded against (Z, Y, X) and reads blk[folded - l], converted as
 * tem_u8_to_f32_std.  A folded coordinate outside the block reads 0 and touches no memory.  A tile wholly inside the
 * volume takes the path of the zero-mode kernels.  The 2-D form folds its section too.  edge <= 46340.
 * TEM_EINVAL, without a launch: another mode, a zero extent, a block outside the volume. */
#define TEM_BOUNDARY_REFLECT 1
#define TEM_BOUNDARY_EDGE 2
int tem_u8_tiles_to_f32_std_bc(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly,
                               int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode, const int32_t *origins_dev,
                               int32_t ntile, int32_t edge, float *out, float mean, float std, tem_stream_t stream);
int tem_u8_tiles2d_to_f32_std_bc(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly,
                                 int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode, const int32_t *origins_dev,
                                 int32_t ntile, int32_t edge, float *out, float mean, float std, tem_stream_t stream);

/* Tiled inference under a symmetry of the cube (self-ensemble over the training orientations).  A symmetry is
 * (p0,p1,p2, f0,f1,f2) in tem_augment_f32's convention over a tile's axes (z, y, x):
 *   T(v) = reverse(transpose(v, perm = (p0,p1,p2)), axes a with f_a != 0), i.e. T(v)[q] = v[j(q)] with
 *   j[perm[a]] = f_a ? n - 1 - q[a] : q[a]   (n = the tile's edge; 2-D tiles: p0 == 0, f0 == 0, j[0] = q[0] = 0).
 * Gather: the arguments of the `_bc` gathers plus the symmetry; `mode` may also be 0 (a voxel outside the block reads
 * 0, as tem_u8_tiles_to_f32_std on blk[BZ][BY][BX]; the block must still lie inside (Z, Y, X) at (lz, ly, lx):
 * the resident form passes the block as the volume).  Voxel q of tile t of `out` = the value the corresponding gather
 * (zero-mode or `_bc`) writes at voxel j(q): out[t] = T(tile t), bit for bit.
 * Accumulate: acc[t][j(q)] = (first ? y[t][q] : acc[t][j(q)] + y[t][q]), then / (float)divisor when divisor > 1 (one
 * fp32 addition, one fp32 division): acc (+)= T^-1(y[t]).  y and acc are [ntile][yedge]^3 (2-D: ^2) and must not
 * alias; with `first` acc is written without being read.  Every acc element is written by exactly one thread.
 * TEM_EINVAL, without a launch: what the `_bc` gathers reject (mode 0 allowed), a perm that is no permutation of
 * (0,1,2), a flag outside {0,1}, a 2-D symmetry with p0 != 0 or f0 != 0, first outside {0,1}, divisor < 1. */
int tem_u8_tiles_to_f32_std_sym(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly,
                                int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode, const int32_t *origins_dev,
                                int32_t ntile, int32_t edge, int32_t p0, int32_t p1, int32_t p2, int32_t f0, int32_t f1,
                                int32_t f2, float *out, float mean, float std, tem_stream_t stream);
int tem_u8_tiles2d_to_f32_std_sym(const uint8_t *blk, int32_t BZ, int32_t BY, int32_t BX, int32_t lz, int32_t ly,
                                  int32_t lx, int32_t Z, int32_t Y, int32_t X, int32_t mode, const int32_t *origins_dev,
                                  int32_t ntile, int32_t edge, int32_t p0, int32_t p1, int32_t p2, int32_t f0,
                                  int32_t f1, int32_t f2, float *out, float mean, float std, tem_stream_t stream);
int tem_f32_tiles_sym_accum(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1, int32_t p2, int32_t f0,
                            int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor, tem_stream_t stream);
int tem_f32_tiles2d_sym_accum(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1, int32_t p2,
                              int32_t f0, int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor,
                              tem_stream_t stream);

/* Tiled inference of the 2-D networks, output side: the interior of tile t of y[ntile][yedge][yedge] (`tpad` pixels
 * stripped per side) is converted as tem_f32_unstd_to_u8 and written into section z of the uint8 volume
 * out[OZ][OY][OX] at (z,y,x) = index_dev[3t..3t+2].  Pixels that fall outside `out` are dropped.  Any ntile. */
int tem_f32_tiles2d_unstd_to_u8(const float *y, int32_t ntile, int32_t yedge, int32_t tpad, const int32_t *index_dev,
                                uint8_t *out, int32_t OZ, int32_t OY, int32_t OX, float mean, float std,
                                tem_stream_t stream);

/* Spread of the self-ensemble: how much the members disagree at a voxel, as a uint8 map beside the mean.
 * Accumulate: the arguments of tem_f32_tiles*_sym_accum plus three more arrays of y's extents.  acc is updated exactly
 * as by that entry point (same `first` and `divisor`); in the same launch, at the same element j(q), with yv = y[t][q]:
 *   first:      ref = yv, s1 = 0, s2 = 0                      (written without being read)
 *   otherwise:  d = yv - ref;  s1 = s1 + d;  p = d * d;  s2 = s2 + p
 * the moments about the first member, every operation one rounded fp32 operation (no fused multiply-add).  y is read
 * once.  TEM_EINVAL, without a launch: what tem_f32_tiles*_sym_accum refuses, a null pointer, and any two of y, acc,
 * ref, s1, s2 that overlap.
 * Finish and scatter: from the moments of `count` members, k = (float)count,
 *   t = (s1 * s1) / k;  v = max(s2 - t, 0) / k;  sd = sqrt(v)   (population standard deviation, correctly rounded)
 *   out = (uint8) rint(min(((sd * |std_y|) * 127.5f) * gain, 255.0f))      (saturates)
 * again one rounded fp32 operation each: the members' standard deviation in grey levels of the output, times `gain`.
 * It is written where tem_f32_tiles*_unstd_to_u8 writes the prediction: each tile's interior, `tpad` stripped, at
 * index_dev[3t..3t+2] of out[OZ][OY][OX], and nowhere else.
 * TEM_EINVAL, without a launch: what those scatters refuse, count < 1, a gain that is not finite or not above 0. */
int tem_f32_tiles_sym_accum_spread(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1, int32_t p2,
                                   int32_t f0, int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor,
                                   float *ref, float *s1, float *s2, tem_stream_t stream);
int tem_f32_tiles2d_sym_accum_spread(const float *y, int32_t ntile, int32_t yedge, int32_t p0, int32_t p1, int32_t p2,
                                     int32_t f0, int32_t f1, int32_t f2, float *acc, int32_t first, int32_t divisor,
                                     float *ref, float *s1, float *s2, tem_stream_t stream);
int tem_f32_tiles_spread_to_u8(const float *s1, const float *s2, int32_t ntile, int32_t yedge, int32_t tpad,
                               const int32_t *index_dev, uint8_t *out, int32_t OZ, int32_t OY, int32_t OX, int32_t count,
                               float std_y, float gain, tem_stream_t stream);
int tem_f32_tiles2d_spread_to_u8(const float *s1, const float *s2, int32_t ntile, int32_t yedge, int32_t tpad,
                                 const int32_t *index_dev, uint8_t *out, int32_t OZ, int32_t OY, int32_t OX,
                                 int32_t count, float std_y, float gain, tem_stream_t stream);

/* One level of a mip pyramid of a uint8 block (tiled inference, after the scatter).  src[D][H][W] is dense; only its
 * box [0, vD) x [0, vH) x [0, vW) is valid (0 <= v <= dim: a block of whole tiles holds predictions past the ROI).
 * dst is dense [ceil(D / fz)][ceil(H / 2)][ceil(W / 2)]: y and x pool by 2, z by fz = 2 (3-D models) or 1 (2-D models:
 * sections are not pooled).  dst voxel (z, y, x) is the mean of its children (fz z + a, 2y + b, 2x + c), a < fz,
 * b, c < 2, that lie inside the valid box -- cnt = 1, 2, 4 or 8 of them -- rounded half up in integers:
 *   dst = (sum + (cnt >> 1)) >> log2(cnt);   no valid child: 0
 * Source bytes outside the valid box are never read.  Every byte of dst is written exactly once and nothing outside
 * dst is touched; src and dst must not overlap.  Any alignment of src, dst and W (aligned rows take wider loads and
 * stores; the bytes are the same).  A further level is a further call on dst with the valid extents
 * (ceil(vD / fz), ceil(vH / 2), ceil(vW / 2)).
 * TEM_EINVAL, without a launch: a null pointer, a dimension below 1, a valid extent outside [0, dim], fz not 1 or 2. */
int tem_u8_pool2(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t vD, int32_t vH, int32_t vW, int32_t fz,
                 uint8_t *dst, tem_stream_t stream);

/* Intensity histogram of a box of a uint8 block (tiled inference: of a volume before it, of the prediction after the
 * scatter).  src[D][H][W] is dense.  counts[v] += the number of voxels of the box [z0, z1) x [y0, y1) x [x0, x1) whose
 * byte is v: counts holds 256 entries, or with per_section = 1 (z1 - z0) rows of 256, row z - z0 counting section z.
 * The kernel ADDS (64-bit global atomic adds): the caller clears counts once and any number of calls, from any number
 * of streams, accumulate into it.  Source bytes outside the box are never read and nothing but counts is written.  Any
 * alignment of src, W and the box (16-byte lines that lie inside a row of the box take one wide load, a row's cut
 * ends byte loads; the counts are the same); counts must be 8-byte aligned.  An empty box (lo == hi on an axis)
 * returns TEM_OK without a launch.
 * TEM_EINVAL, without a launch: a null pointer, counts off 8-byte alignment, a dimension below 1, a box outside
 * [0, dim] or with lo > hi, per_section outside {0, 1}, and a box too large for the workgroups' 32-bit counters: the
 * box's (z1 - z0)(y1 - y0) rows are dealt in equal contiguous runs to at most 1024 workgroups, and
 *   ceil(rows / workgroups) x max(x1 - x0, (x1 - x0 + 30) / 16)  must stay below 2^31
 * (a workgroup flushes at the end of its run, and with per_section at every change of section: no counter can see
 * more voxels than that).  A box of fewer than 2^40 voxels always passes. */
int tem_u8_hist(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t z1, int32_t y0, int32_t y1,
                int32_t x0, int32_t x1, uint64_t *counts, int32_t per_section, tem_stream_t stream);

/* Joint histogram of two uint8 blocks (a prediction against its ground truth): a[Da][Ha][Wa] and b[Db][Hb][Wb] are
 * dense, each with its own dims, row stride and pointer alignment.
 *   counts[256 u + v] += #{(z, y, x) in [0, nz) x [0, ny) x [0, nx) :
 *                          a[az0 + z][ay0 + y][ax0 + x] == u  and  b[bz0 + z][by0 + y][bx0 + x] == v}
 * counts holds 65,536 entries, 8-byte aligned.  The kernel ADDS (64-bit global atomic adds, one per non-zero bin and
 * workgroup): the caller clears counts once and any number of calls, from any number of streams, accumulate into it.
 * Exact for any data -- a constant pair (every lane on one bin) and a pair that fills all 65,536 bins included.  Bytes
 * outside the two boxes are never counted and nothing but counts is written; a load touches only naturally aligned
 * words (up to 16 bytes) that hold at least one byte of that side's box.  An empty box (nz, ny or nx == 0) returns
 * TEM_OK without a launch.
 * TEM_EINVAL, without a launch: a null pointer, counts off 8-byte alignment, a dimension below 1, a negative origin
 * or extent, a box that leaves either block, and a box too large for the workgroups' 32-bit counters.  The table is
 * split by the high bit of a, and each half's workgroups see every voxel of their run: with rows = nz * ny and
 * S = (nx + 30) / 16 segments per row, the rows are dealt in equal contiguous runs of
 *   rpw = ceil(rows / P),  P = min(128, max(1, ceil(rows * S / 4096)))
 * rows to ceil(rows / rpw) workgroups per half, and
 *   rpw x max(nx, S)  must stay below 2^31
 * (a workgroup flushes once, at the end of its run: no counter can see more voxels than that, and its 32-bit index of
 * (row, segment) items, split exactly for every value below 2^31, stays in range).  A box of fewer than 2^37 voxels
 * always passes. */
int tem_u8_hist2(const uint8_t *a, int32_t Da, int32_t Ha, int32_t Wa, int32_t az0, int32_t ay0, int32_t ax0,
                 const uint8_t *b, int32_t Db, int32_t Hb, int32_t Wb, int32_t bz0, int32_t by0, int32_t bx0,
                 int32_t nz, int32_t ny, int32_t nx, uint64_t *counts, tem_stream_t stream);

/* Windowed structural similarity (SSIM) of two uint8 blocks, the structural companion of tem_u8_hist2: a[Da][Ha][Wa]
 * and b[Db][Hb][Wb] are dense, each with its own dims, row stride and pointer alignment; the voxel box has extents
 * (nz, ny, nx) at origin (az0, ay0, ax0) of a and (bz0, by0, bx0) of b.  Windows are uniform boxes of wz x win x win
 * voxels, win odd in 3...11, wz = win (volumetric) or 1 (flat != 0: section by section), N = wz win win; only windows
 * that lie wholly inside the box count: the window box is (nz - wz + 1, ny - win + 1, nx - win + 1), a window named by
 * its first voxel.  Per window, from the integer sums Sa, Sb, Saa, Sbb, Sab over its voxels, all in int64:
 *   A1 = 20000 Sa Sb           + 65025 N^2        B1 = 10000 (Sa^2 + Sb^2)                     + 65025 N^2
 *   A2 = 20000 (N Sab - Sa Sb) + 585225 N (N - 1) B2 = 10000 ((N Saa - Sa^2) + (N Sbb - Sb^2)) + 585225 N (N - 1)
 *   l = double(A1) / double(B1)      cs = double(A2) / double(B2)      s = l cs
 *   q_x = (int64) rint(x 2^30)  for x in (s, l, cs)                    (round half to even)
 * -- Wang's SSIM with a uniform window, the sample covariance (N - 1), data range 255, K1 = 0.01, K2 = 0.03
 * (C1 = 6.5025, C2 = 58.5225, carried x 10^4).  A1...B2 stay below 2^53 for win <= 11, so the conversions are exact;
 * B1, B2 > 0; the value is two correctly rounded divisions, one multiplication and a scaling by a power of two.
 *   sums[3 z + 0, 1, 2] += the q_s, q_l, q_cs of all windows whose first section is z       (z < nz - wz + 1)
 *   map[z][y][x] = (255 max(q_s, 0) + 2^29) >> 30      dense [nz - wz + 1][ny - win + 1][nx - win + 1]; may be null
 * The kernel ADDS to sums (signed: s < 0 for an anti-correlated pair) with 64-bit global atomic adds, one per workgroup,
 * window-section and quantity: the caller clears sums once and any number of calls, from any number of streams,
 * accumulate.  Integer adds: the result does not depend on how the box is cut or launched.  No byte outside the two
 * boxes is read and nothing but sums and map is written.  Any alignment of a, b, map, Wa and Wb; sums must be 8-byte
 * aligned.  A box in which no window fits (nz < wz, ny < win or nx < win; an empty box included) returns TEM_OK
 * without a launch.
 * TEM_EINVAL, without a launch: a null a, b or sums, sums off 8-byte alignment, win even or outside 3...11, a
 * dimension below 1, a negative origin or extent, a box that leaves either block, and a window box of more workgroups
 * than one launch holds: a workgroup takes 8 x 32 window origins over (y, x) and a run of 32 window-sections, and
 *   ceil((ny - win + 1) / 8) x ceil((nx - win + 1) / 32) x ceil((nz - wz + 1) / 32)  must stay below 2^24
 * (its 256 threads then stay below 2^32 per launch; the workgroup index is split in 32 bits, every byte offset is 64
 * bits).  A box of fewer than 2^34 voxels with no extent below 32 always passes. */
int tem_u8_ssim(const uint8_t *a, int32_t Da, int32_t Ha, int32_t Wa, int32_t az0, int32_t ay0, int32_t ax0,
                const uint8_t *b, int32_t Db, int32_t Hb, int32_t Wb, int32_t bz0, int32_t by0, int32_t bx0,
                int32_t nz, int32_t ny, int32_t nx, int32_t win, int32_t flat, int64_t *sums, uint8_t *map,
                tem_stream_t stream);

/* A uint8 volume brought onto a grid of another voxel size: intensities only (labels need nearest or majority).  Each
 * axis has a step p / q in lowest terms, the output voxel's edge in source voxels: 1 <= p, q <= 64, 1/8 <= p / q <= 8.
 * An axis of n source voxels gives ceil(n q / p) output voxels, the grid anchored at the volume's voxel 0.  Output j
 * of an axis has integer taps (i, w) and a denominator W:
 *   p >= q, the area average: in units of 1 / q source voxel, j covers [j p, (j + 1) p) and source voxel i covers
 *     [i q, (i + 1) q); w is the length of the overlap, for i from floor(j p / q) while i q < (j + 1) p and i <= n - 1;
 *     W is the sum of the weights kept: p, or less at the far face where n q is not a multiple of p (a voxel that
 *     does not exist never enters a mean: tem_u8_pool2's rule).  At most ceil(p / q) + 1 taps.
 *   p < q, linear between voxel centres: C = (2 j + 1) p - q, i0 = floor(C / (2 q)), f = C - 2 q i0; the taps are
 *     (clamp(i0), 2 q - f) and (clamp(i0 + 1), f), clamp to [0, n - 1]; W = 2 q  (scipy.ndimage.zoom(order=1,
 *     mode="nearest", grid_mode=True) before rounding).
 *   the voxel: S = sum of wz wy wx v over the tap product, Den = Wz Wy Wx, out = (2 S + Den) / (2 Den)  (integers)
 * -- one rounding, half up, at the very end; no pass rounds an intermediate.  2 S + Den <= 511 x 128^3 < 2^31.
 * src[D][H][W] is a dense block of the volume [VZ][VY][VX] with its voxel 0 at (sz0, sy0, sx0); dst[OD][OH][OW] is a
 * dense block of the output grid with its voxel 0 at (oz0, oy0, ox0).  Taps and the far faces are computed in volume
 * coordinates, so a block's bytes do not depend on how the volume was cut.  Every byte of dst is written exactly once
 * and nothing else is written; no source byte outside the hull of the block's taps is read, and a tap of weight 0
 * (f == 0) is no tap: it need not lie in the source block and is not read.  Any alignment of src, dst, W and OW;
 * every byte offset is 64 bits.
 * TEM_EINVAL, without a launch: a null pointer, a dimension below 1, p or q outside 1...64, a step outside [1/8, 8]
 * or not in lowest terms, a negative origin, a source block that leaves the volume, an output block that leaves the
 * grid, an output block one of whose taps lies outside the source block, and an output block of more workgroups than
 * one launch holds: a workgroup takes 8 x 32 outputs over (y, x) and a run of 32 output planes, and
 *   ceil(OH / 8) x ceil(OW / 32) x ceil(OD / 32)  must stay below 2^24
 * (its 256 threads then stay below 2^32 per launch).  A block of fewer than 2^34 voxels with no extent below 32
 * always passes. */
int tem_u8_rescale(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t sy0, int32_t sx0,
                   int32_t VZ, int32_t VY, int32_t VX, int32_t pz, int32_t qz, int32_t py, int32_t qy, int32_t px,
                   int32_t qx, uint8_t *dst, int32_t OD, int32_t OH, int32_t OW, int32_t oz0, int32_t oy0, int32_t ox0,
                   tem_stream_t stream);

/* Intensity remapping of a dense uint8 block in place (tiled inference: the uploaded bytes, ahead of the gather).
 *   per_section = 0:  buf[z][y][x] = lut[buf[z][y][x]]                          lut: 256 bytes
 *   per_section = 1:  buf[z][y][x] = lut[(zsec0 + z) * 256 + buf[z][y][x]]      lut: at least zsec0 + D rows of 256
 * (zsec0: the section of the caller's volume that buf's section 0 is).  A workgroup reads its section's table once
 * into LDS; every byte of buf is read exactly once and written exactly once, and nothing outside buf is touched.  Any
 * alignment of buf, lut and W (16-byte lines inside a section take one wide load and store).
 * TEM_EINVAL, without a launch: a null pointer, a dimension below 1, a negative zsec0, per_section outside {0, 1}. */
int tem_u8_lut(uint8_t *buf, int32_t D, int32_t H, int32_t W, const uint8_t *lut, int32_t per_section, int32_t zsec0,
               tem_stream_t stream);

/* 16-bit volumes, the first link of the preparation chain (utils.volume_histogram16, utils.volume_to_u8): counted in
 * 65,536 bins and brought to uint8 by a table.  A voxel v of a native-endian 16-bit block has the INDEX
 *   u = v             for uint16  (is_signed = 0)
 *   u = v + 32768     for int16   (is_signed = 1):  on the bits v ^ 0x8000, so the order of the values is kept.
 * Histograms and tables are indexed by u and always hold 65,536 entries.
 *
 * tem_u16_hist: src[D][H][W] is dense.  counts[u] += the number of voxels of the box [z0, z1) x [y0, y1) x [x0, x1)
 * whose index is u: counts holds 65,536 entries, or with per_section = 1 (z1 - z0) rows of 65,536, row z - z0 counting
 * section z.  The kernel ADDS (64-bit global atomic adds, one per non-zero bin, workgroup and flush): the caller clears
 * counts once and any number of calls, from any number of streams, accumulate into it.  Exact for any data -- a
 * constant block (every lane on one bin) and a block that fills all 65,536 bins included.  Voxels outside the box are
 * never read and nothing but counts is written; a load touches only naturally aligned words (up to 16 bytes) that hold
 * at least one voxel of the box.  src at any 2-byte alignment, any W (an odd W leaves rows 2-byte aligned only) and any
 * box; counts must be 8-byte aligned.  An empty box (lo == hi on an axis) returns TEM_OK without a launch.
 * TEM_EINVAL, without a launch: a null pointer, src off 2-byte or counts off 8-byte alignment, a dimension below 1, a
 * box outside [0, dim] or with lo > hi, per_section or is_signed outside {0, 1}, and a box too large for the
 * workgroups' 32-bit counters.  The table is split by the high bit of u, and each half's workgroups see every voxel of
 * their run.  The box's rows form nsec stretches of nyd rows that are flushed apart -- the (z1 - z0) sections of
 * (y1 - y0) rows with per_section, else the one box of (z1 - z0)(y1 - y0) rows -- and with S = (2 (x1 - x0) + 29) / 16
 * segments per row a stretch is cut into pieces of
 *   rpp = ceil(nyd / P),  P = min(max(1, 128 / nsec), max(1, ceil(nyd * S / 4096)))
 * rows; a workgroup takes whole pieces and flushes wherever it leaves a stretch, and
 *   rpp x max(x1 - x0, S)  must stay below 2^31
 * (no counter can see more voxels than that between two flushes, and the 32-bit index of (row, segment) items, split
 * exactly for every value below 2^31, stays in range).  Without per_section a box of fewer than 2^37 voxels always
 * passes; with per_section every box whose sections hold fewer than 2^31 voxels each. */
int tem_u16_hist(const uint16_t *src, int32_t D, int32_t H, int32_t W, int32_t z0, int32_t z1, int32_t y0, int32_t y1,
                 int32_t x0, int32_t x1, uint64_t *counts, int32_t per_section, int32_t is_signed, tem_stream_t stream);

/* tem_u16_lut_u8: src is a dense 16-bit block [D][H][W], dst a dense uint8 block [D][H][W]:
 *   per_section = 0:  dst[z][y][x] = lut[u(src[z][y][x])]                            lut: 65,536 bytes
 *   per_section = 1:  dst[z][y][x] = lut[(zsec0 + z) * 65536 + u(src[z][y][x])]      lut: at least zsec0 + D rows
 * (zsec0: the section of the caller's volume that the block's section 0 is).  One table form serves linear windows,
 * gamma, inversion and CDF matching (utils.window_lut16, utils.match_lut16): there is no second arithmetic definition
 * on the device.  Every byte of dst is written exactly once and nothing else is written; no voxel outside src is read.
 * src at any 2-byte alignment and dst at any alignment, independently (8 outputs leave as one 8-byte store where dst
 * allows it, their 16 source bytes arrive as one load where src does too); every byte offset is 64 bits.  src and dst
 * must not overlap.  A workgroup serves one section's table: tem_u16_lut_u8 stages its 64 KiB in LDS once and looks up
 * there, tem_u16_lut_u8_direct looks up in global memory (the baseline the staged form is measured against; the same
 * bytes for the same arguments).
 * TEM_EINVAL, without a launch: a null pointer, src off 2-byte alignment, a dimension below 1, a negative zsec0,
 * per_section or is_signed outside {0, 1}, and a block of more workgroups than one launch holds: a section (the whole
 * block without per_section) of n voxels goes to min(ceil(512 / nsec), ceil(ceil((n + 14) / 8) / 16384)) workgroups
 * and their total must stay below 2^31 -- which it does for every D an int32_t holds, so no block is refused for it. */
int tem_u16_lut_u8(const uint16_t *src, int32_t D, int32_t H, int32_t W, uint8_t *dst, const uint8_t *lut,
                   int32_t per_section, int32_t zsec0, int32_t is_signed, tem_stream_t stream);
int tem_u16_lut_u8_direct(const uint16_t *src, int32_t D, int32_t H, int32_t W, uint8_t *dst, const uint8_t *lut,
                          int32_t per_section, int32_t zsec0, int32_t is_signed, tem_stream_t stream);

/* Repair of damaged sections and voxels of a dense uint8 block along z, in place (tiled inference and
 * utils.volume_repair: the uploaded bytes, ahead of everything else).  buf[D][H][W] holds the sections zsec0 ...
 * zsec0 + D - 1 of the caller's volume.  A voxel (d, y, x) is BAD if any source that is given says so:
 *   mask      (dense [D][H][W], or NULL):           mask[d][y][x] != 0
 *   sections  (one flag per section of the volume, or NULL):  sections[zsec0 + d] != 0
 *   missing   (-1: none, or 0 ... 255):             buf[d][y][x] == missing
 * With R = max_gap (1 ... 32), for a bad voxel at plane d of its column (y, x):
 *   d0 = the smallest k in 1 ... R with d - k >= 0 and voxel d - k good,      a = buf[d - d0]
 *   d1 = the smallest k in 1 ... R with d + k <= D - 1 and voxel d + k good,  b = buf[d + d1]
 *   both exist:  out = (2 (a d1 + b d0) + n) / (2 n),  n = d0 + d1     (integers: linear between the two, half up)
 *   one exists:  out = that value;      neither: the voxel stays as it is.
 * Good voxels are never changed and a bad voxel is never a source, so a voxel's result depends on the planes
 * [d - R, d + R] of its own column only.  Only the core planes [c0, c1) are written; the planes around them are the
 * halo that the core's voxels read, and the caller lets the block reach R planes past the core on each side or to the
 * volume's face -- then the core's bytes do not depend on how the volume was cut.  Nothing outside buf is written,
 * nothing outside buf, mask and sections[zsec0 ... zsec0 + D) is read.  Any alignment of buf, mask and W (a plane
 * stride H W that is a multiple of 4, with mask congruent to buf mod 4, takes dword loads and stores).
 * counts (8-byte aligned, or NULL): counts[0] += bad core voxels that were repaired, counts[1] += bad core voxels
 * left as they are (one 64-bit global atomic add each per workgroup at most; the caller clears them).
 * TEM_EINVAL, without a launch: a null buf, a dimension below 1, a negative zsec0, max_gap outside 1 ... 32, a core
 * that is not 0 <= c0 <= c1 <= D, missing outside -1 ... 255, no source at all, counts off 8-byte alignment.
 * TEM_EUNSUPPORTED: D above 2^21, or more than 2^31 - 1 workgroups per plane.  An empty core launches nothing. */
int tem_u8_repair_z(uint8_t *buf, int32_t D, int32_t H, int32_t W, int32_t zsec0, int32_t c0, int32_t c1,
                    const uint8_t *mask, const uint8_t *sections, int32_t missing, int32_t max_gap, uint64_t *counts,
                    tem_stream_t stream);

/* Contrast-limited adaptive histogram equalisation (CLAHE) of uint8 sections, the two device passes; the tables
 * between them are host work (utils.clahe_tables).  The tile is (th, tw) pixels over (y, x), and the grid of gy x gx
 * tiles is anchored at (0, 0) of the caller's volume.  Both calls cover a dense block [D][H][W] of it whose voxel
 * (d, y, x) sits at in-plane volume coordinates (y_org + y, x_org + x); the last row and column of tiles may be partial.
 *
 * tem_u8_hist_tiles: counts[((d * gy + (y_org + y) / th) * gx + (x_org + x) / tw) * 256 + v] += 1 for every voxel of
 * value v.  counts (4-byte aligned) points at the rows of the block's first section.  The kernel ADDS (32-bit global
 * atomic adds): the caller clears counts once, and blocks that cut a tile between them accumulate into it.  No
 * counter may pass 2^32 - 1; a tile holds at most 2048 x 2048 voxels.
 *
 * tem_u8_clahe: buf is remapped in place by tables[zsec0 + d][i][j][256] (uint8, at least zsec0 + D sections of
 * gy x gx tables).  With v the voxel's value at volume coordinates (y, x):
 *   f = 2 y + 1 - th,  i0 = floor(f / (2 th)),  wy = f - i0 2 th,  i1 = clip(i0 + 1, 0, gy - 1),  i0 = clip(i0, 0, gy - 1)
 * (x likewise with tw and gx: j0, j1, wx), a, b, c, d = T[i0][j0][v], T[i0][j1][v], T[i1][j0][v], T[i1][j1][v],
 * Dn = 4 th tw:
 *   out = ((2 th - wy) ((2 tw - wx) a + wx b) + wy ((2 tw - wx) c + wx d) + Dn / 2) / Dn        (integers)
 * -- bilinear interpolation between the tile centres, rounded half up, clamped to the nearest centre in the half
 * tile along each face; exact for every tile size allowed.  Every byte of buf is read once and written once, and
 * nothing outside buf is touched.  Any alignment of the pointers, W and the origins.
 *
 * TEM_EINVAL, without a launch: a null pointer, a dimension, gy or gx below 1, th or tw outside [1, 2048], a negative
 * origin, a block that reaches past the grid (y_org + H > gy th, x_org + W > gx tw), a negative zsec0, counts off
 * 4-byte alignment.  TEM_EUNSUPPORTED: a remap of more than 2^31 - 1 workgroups (one per section, interpolation cell
 * and run of about 2048 16-byte lines). */
int tem_u8_hist_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t y_org, int32_t x_org, int32_t th,
                      int32_t tw, int32_t gy, int32_t gx, uint32_t *counts, tem_stream_t stream);
int tem_u8_clahe(uint8_t *buf, int32_t D, int32_t H, int32_t W, int32_t zsec0, int32_t y_org, int32_t x_org,
                 const uint8_t *tables, int32_t gy, int32_t gx, int32_t th, int32_t tw, tem_stream_t stream);

/* The sums behind the correlation of every tile of a section with the same tile one section up (utils.section_sums ->
 * section_scores -> find_defects: sections and regions that resemble neither neighbour).  src[D][H][W] is a dense
 * block of a uint8 volume on tem_u8_hist_tiles' tile grid: (th, tw) pixels, gy x gx tiles anchored at the volume's
 * (0, 0), the block's voxel (d, y, x) at in-plane volume coordinates (y_org + y, x_org + x).  Only the core planes
 * [c0, c1) are counted; sums (8-byte aligned) points at the rows of plane c0.  For every core plane d and every voxel
 * of value v in tile (i, j) = ((y_org + y) / th, (x_org + x) / tw), with v+ the voxel at (d + 1, y, x):
 *   q = sums + (((d - c0) * gy + i) * gx + j) * 4
 *   q[0] += v     q[1] += v v     q[2] += v v+  (only if d + 1 < D)     q[3] += 1
 * Plane D - 1 has no pair term: the caller lets the block reach one plane past the core, or the core end at the
 * volume's last section.  The kernel ADDS (64-bit global atomic adds, one per workgroup, plane and quantity): the
 * caller clears sums once, and blocks that cut a tile along y, x or z between them accumulate into it; the adds are
 * integers, so the result does not depend on how the volume was cut or launched.  Nothing but sums is written.  A load
 * touches only naturally aligned words (up to 16 bytes) that hold at least one byte of the block.  Any alignment of
 * src, W and the origins.  No partial can overflow at 255 x 255 = 65025 per voxel: a thread sums at most 64 voxels
 * of a plane in 32 bits (64 x 65025 < 2^23), a wave 64 such partials in 32 bits (< 2^29), a workgroup is given at
 * most 16384 voxels of a plane -- a 2048 x 2048 tile goes to 256 of them -- and adds its four wave sums in 64 bits
 * (16384 x 65025 < 2^31); the 64-bit counter takes a whole such tile per plane (2^22 x 65025 < 2^38) 2^25 times over.
 * TEM_EINVAL, without a launch: a null pointer, sums off 8-byte alignment, a dimension, gy or gx below 1, th or tw
 * outside [1, 2048], a negative origin, a block that reaches past the grid (y_org + H > gy th, x_org + W > gx tw), a
 * core that is not 0 <= c0 <= c1 <= D.  TEM_EUNSUPPORTED: more than 2^31 - 1 workgroups (one per tile of the block,
 * run of rows of about 1024 16-byte pieces, and run of up to 16 core planes).  An empty core launches nothing. */
int tem_u8_zcorr_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t y_org,
                       int32_t x_org, int32_t th, int32_t tw, int32_t gy, int32_t gx, uint64_t *sums,
                       tem_stream_t stream);

/* tem_u8_zcorr_tiles with nlag partners instead of one (utils.section_lag_sums -> lag_scores -> section_spacing: how
 * fast the correlation of a section with those above it decays with the lag is how far the sections sit apart along
 * z).  The tile grid, the block src[D][H][W] at (y_org, x_org), the core [c0, c1), the alignments, the loads, the adds,
 * the argument that no partial overflows and the refusals are tem_u8_zcorr_tiles'; nlag lies in 1...8.  For every core
 * plane d and every voxel of value v in tile (i, j), with v+k the voxel at (d + k, y, x):
 *   q = sums + (((d - c0) * gy + i) * gx + j) * (3 + nlag)
 *   q[0] += v     q[1] += v v     q[2] += 1     q[2 + k] += v v+k  (k = 1...nlag, only if d + k < D)
 * The caller lets the block reach nlag planes past the core, or to the volume's last section.  With nlag = 1 the four
 * quantities are tem_u8_zcorr_tiles', in another column order.  A thread sums at most 64 voxels of a plane and a
 * workgroup is given at most 16384 (nlag <= 4) or 8192 (above) voxels of a plane.
 * TEM_EINVAL, without a launch: what tem_u8_zcorr_tiles refuses, and nlag outside 1...8.  TEM_EUNSUPPORTED: 2^24
 * workgroups or more (one per tile of the block, run of rows of about 1024 or 512 16-byte pieces, and run of up to
 * 24 + 8 nlag core planes; their 256 threads then stay below 2^32 per launch).  An empty core launches nothing. */
int tem_u8_zcorr_lags(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t y_org,
                      int32_t x_org, int32_t th, int32_t tw, int32_t gy, int32_t gx, int32_t nlag, uint64_t *sums,
                      tem_stream_t stream);

/* A uint8 volume resampled along z through a table of taps (utils.volume_resample_z: sections whose measured
 * positions are uneven, brought onto an even grid).  The definition, once: V[VZ][H][W] is the volume, the output has NZ
 * sections, and taps[NZ][2] = (z0, w) per output section, int32, 0 <= z0 <= VZ - 1 and 0 <= w <= 255 (utils.
 * resample_z_taps).  With a = V[z0][y][x] and b = V[min(z0 + 1, VZ - 1)][y][x]:
 *   out = ((256 - w) a + w b + 128) >> 8            (at most 255 x 256 + 128 < 2^16; w = 0 gives a)
 *   nearest = 1 (masks):  out = w < 128 ? a : b
 * A tap of weight 0 -- b where w = 0 -- is no tap: it is not read and need not lie in the block.
 * src[D][H][W] holds sections sz0 ... sz0 + D - 1 of the volume, dst[OD][H][W] output sections oz0 ... oz0 + OD - 1.
 * taps_host points at the whole table on the host, whose rows oz0 ... oz0 + OD - 1 are validated without a launch;
 * taps_dev at the same table on the device, which the kernel reads.  The kernel clamps every z0 it reads into the
 * block and every w to 0...255, so a device table that disagrees with the host's gives wrong bytes, never a fault.
 * Every byte of dst is written exactly once and nothing else is written; no source byte outside the taps' planes is
 * read, and a load touches only naturally aligned words (up to 16 bytes) that hold at least one byte of the block.
 * Any alignment of src, dst and H W, src and dst independently; every byte offset is 64 bits.  A voxel depends on its
 * tap alone, not on how the volume was cut.
 * TEM_EINVAL, without a launch: a null pointer, a dimension below 1, a block outside the volume (sz0 < 0, sz0 + D > VZ)
 * or outside the output (oz0 < 0, oz0 + OD > NZ), nearest outside {0, 1}, a row of the block's with z0 or w out of
 * range, and one whose plane z0, or whose plane min(z0 + 1, VZ - 1) where w > 0, lies outside the source block.
 * TEM_EUNSUPPORTED: 2^24 workgroups or more (one per 4096 bytes of a plane and run of up to 32 output planes; their 256
 * threads then stay below 2^32 per launch).  A block of fewer than 2^34 voxels with planes of 4096 bytes or more
 * always passes. */
int tem_u8_resample_z(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t VZ, uint8_t *dst,
                      int32_t OD, int32_t oz0, int32_t NZ, const int32_t *taps_host, const int32_t *taps_dev,
                      int32_t nearest, tem_stream_t stream);

/* Damaged voxels below the tile: how far a voxel lies outside the range of the voxels below and above it in the nearest
 * good sections (utils.section_outlier_sums -> outlier_thresholds -> volume_outliers -> find_debris: dust, precipitate
 * and knife debris sit on one section).  The definition, once.  V[Z][Y][X] is the uint8 volume; tiles of (th, tw) pixels
 * on tem_u8_hist_tiles' grid, gy x gx of them anchored at the volume's (0, 0).
 *   Neighbours   nbr[Z][2] = (lo, hi) per section, int32 (utils.section_neighbours): either (-1, -1), no verdict, or
 *                lo < z < hi, both in [0, Z), z - lo <= 8 and hi - z <= 8: the nearest good sections below and above.
 *   Deviation    with a = V[lo][y][x], v = V[z][y][x], b = V[hi][y][x]:  e = |v - median(a, v, b)|, that is 0 where
 *                min(a, b) <= v <= max(a, b), else min(|v - a|, |v - b|); e = 0 where the section has no verdict.
 *                0 <= e <= 255.
 *   Tile sums    t[z][i][j] = (sum e, n) over the voxels of tile (i, j) of section z, int64; n is the tile's voxel count
 *                where the section has a verdict, else 0.
 *   Mask         for a radius r in 1...7, Ws(z, y, x) is the sum of e over [y - r, y + r] x [x - r, x + r] cut to the
 *                section and c the number of voxels of the cut window.  With thr[gy][gx], int32 in [1, 65280], in 1/256
 *                grey level, and (i, j) the tile of (y, x):  mask = 1 iff 256 Ws > thr[i][j] c, or where an optional
 *                table tiles[Z][gy][gx] of uint8 is non-zero at [z][i][j]; else 0.  Equality does not flag.
 *                Ws <= 225 x 255 = 57,375; 256 Ws and thr c stay below 2^24: everything fits 32 bits.
 * Both entries take the whole table nbr twice: nbr_host on the host, whose rows for the core planes are validated
 * without a launch, and nbr_dev (4-byte aligned) with the same contents on the device, which the kernel reads.  The
 * block's plane 0 is section sz0 of the stack of Z.  On the device a row with a negative entry is no verdict, and lo
 * and hi of any other row are clamped into the block, as tem_u8_resample_z does with its taps: a device table that
 * disagrees with the host's gives other results, never a read outside the block.
 *
 * tem_u8_zdev_tiles follows tem_u8_zcorr_tiles' contract: the block src[D][H][W] at (y_org, x_org), the core planes
 * [c0, c1), any alignment of src, W and the origins, loads of naturally aligned words that hold a byte of the block,
 * 64-bit sums (8-byte aligned, pointing at the rows of plane c0) that it ADDS to with one 64-bit global atomic add (an
 * ordinary vector atomic) per workgroup, plane and quantity:
 *   q = sums + (((d - c0) * gy + i) * gx + j) * 2        q[0] += e     q[1] += 1    (nothing for a plane without a verdict)
 * so blocks that cut a tile along y, x or z between them accumulate into it.  lo and hi of every core plane with a
 * verdict must lie in the block.  A thread sums at most 64 voxels of a plane (< 2^14), a wave 64 such partials, a
 * workgroup at most 16384 voxels (< 2^22).
 * TEM_EINVAL, without a launch: what tem_u8_zcorr_tiles refuses, a null table, nbr_dev off 4-byte alignment, Z < 1, a
 * block outside the stack (sz0 < 0, sz0 + D > Z), a core row of nbr_host that breaks the rules above or names a
 * section outside the block.  TEM_EUNSUPPORTED: 2^24 workgroups or more (tem_u8_zcorr_tiles' parts and runs of up to 16
 * core planes).  An empty core launches nothing.
 *
 * tem_u8_zdev_mask: src[D][H][W] is a dense block of WHOLE rows (W == X, as tem_u8_zshift_tiles) whose row 0 sits at
 * volume row y_org of a section of Y rows.  It writes dst[c1 - c0][r1 - r0][x1 - x0], dense, for the core planes
 * [c0, c1), core rows [r0, r1) and core columns [x0, x1) of the block: every byte of dst, 0 or 1, and nothing else but
 * count.  The block must hold every row under a core window that the section has -- [0, H) contains
 * [r0 - radius, r1 + radius) cut to [-y_org, Y - y_org) -- and lo and hi of every core plane with a verdict.
 * thr_host[gy][gx] is validated (1...65280); thr_dev (4-byte aligned) is the same table on the device, clamped to that
 * range as it is read.  tiles_dev may be null; it points at the rows of section sz0 + c0: tiles_dev[((d - c0) * gy + i)
 * * gx + j].  count may be null; it is 8-byte aligned, and the number of ones written is ADDED to it with one 64-bit
 * global atomic add (an ordinary vector atomic) per workgroup.  Any alignment of src, dst and W.  A voxel's verdict
 * depends on its window and its section's row alone, not on how the volume was cut.
 * TEM_EINVAL, without a launch: a null src, dst or table, a table or count off its alignment, a dimension, Y, Z, gy or
 * gx below 1, th or tw outside [1, 2048], a radius outside [1, 7], a negative y_org, a block that reaches past the
 * section or the stack, a section past the grid (Y > gy th, W > gx tw), a core that is not 0 <= c0 <= c1 <= D,
 * 0 <= r0 <= r1 <= H, 0 <= x0 <= x1 <= W, an entry of thr_host out of range, a core row of nbr_host that breaks the
 * rules or names a section outside the block, a block without a row that a core window needs.  TEM_EUNSUPPORTED: 2^24
 * workgroups or more (one per core plane and run of up to 64 tiles of 8 x 32 outputs; the run is as long as leaves
 * about 8192 workgroups).  An empty core launches nothing. */
int tem_u8_zdev_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t Z, int32_t c0,
                      int32_t c1, int32_t y_org, int32_t x_org, int32_t th, int32_t tw, int32_t gy, int32_t gx,
                      const int32_t *nbr_host, const int32_t *nbr_dev, uint64_t *sums, tem_stream_t stream);
int tem_u8_zdev_mask(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sz0, int32_t Z, int32_t Y,
                     int32_t y_org, int32_t c0, int32_t c1, int32_t r0, int32_t r1, int32_t x0, int32_t x1, int32_t th,
                     int32_t tw, int32_t gy, int32_t gx, int32_t radius, const int32_t *nbr_host,
                     const int32_t *nbr_dev, const int32_t *thr_host, const int32_t *thr_dev,
                     const uint8_t *tiles_dev, uint8_t *dst, uint64_t *count, tem_stream_t stream);

/* The sums behind the correlation of every tile of a section with the NEXT SECTION DISPLACED by every integer offset
 * within a radius (utils.section_shift_sums -> shift_scores -> section_shifts: how far consecutive sections sit apart
 * in y and x).  The definition: the volume is V[Z][Y][X], uint8; tiles of (th, tw) pixels on tem_u8_hist_tiles' grid,
 * gy x gx of them anchored at the volume's (0, 0); the radius r lies in 1...8 and R = 2 r + 1.  For a section
 * z < Z - 1, a tile (i, j) and an offset (dy, dx) in [-r, r]^2, over the tile's voxels (y, x) whose partner
 * (y + dy, x + dx) lies inside the section -- 0 <= y + dy < Y and 0 <= x + dx < X; it may lie outside the tile --, with
 * v = V[z][y][x] and w = V[z + 1][y + dy][x + dx]:
 *   q[z][i][j][dy + r][dx + r][0..4] = (sum v, sum v v, sum w, sum w w, sum v w)
 * int64; the last section's are all zero.  The number of terms n[i][j][dy + r][dx + r] is geometry only
 * (utils.shift_counts); the kernel does not count.  A full tile of 255s stays below 2^38 per entry.
 *
 * tem_u8_zshift_tiles follows tem_u8_zcorr_tiles' contract, except: src[D][H][W] is a dense block of WHOLE rows
 * (W == X, no x_org) whose row 0 sits at volume row y_org of a section of Y rows.  The voxels counted as v are the core
 * planes [c0, c1) and core rows [r0, r1); the block must hold every partner row of the core that the volume has --
 * [0, H) contains [r0 - radius, r1 + radius) cut to [-y_org, Y - y_org) -- and plane d + 1 for every core plane d,
 * except that a core plane d = D - 1 gets no sums at all.  sums (8-byte aligned) points at the rows of plane c0:
 *   sums[((((d - c0) * gy + i) * gx + j) * R + dy + r) * R + dx + r) * 5 + 0..4] += the five sums above
 * The kernel ADDS (64-bit global atomic adds, ordinary vector atomics: one per workgroup, offset and quantity): the
 * caller clears sums once, and blocks that cut a tile along y or z between them accumulate into it.  Nothing but sums
 * is written.  A load touches only naturally aligned 4-byte words that hold at least one byte of the block.  Any
 * alignment of src and W.  No partial can overflow at 255 x 255 = 65025 per term: a workgroup is given one plane of a
 * part of a tile of at most 4096 voxels (64 rows, 128 columns), so a lane's sums, and the sums of its four waves in
 * LDS, stay below 4096 x 65025 < 2^28 in 32 bits; they are widened to 64 bits for the global add, and the 64-bit
 * counter takes a whole 2048 x 2048 tile per plane (2^22 x 65025 < 2^38) 2^25 times over.
 * TEM_EINVAL, without a launch: a null pointer, sums off 8-byte alignment, a dimension, Y, gy or gx below 1, th or tw
 * outside [1, 2048], a radius outside [1, 8], a negative y_org, a block that reaches past the section or the section
 * past the grid (y_org + H > Y, Y > gy th, W > gx tw), a core that is not 0 <= c0 <= c1 <= D and 0 <= r0 <= r1 <= H, a
 * block without a partner row that the volume has.  TEM_EUNSUPPORTED: more than 2^31 - 1 workgroups (one per core
 * plane with a partner plane, tile and part of it).  An empty core launches nothing. */
int tem_u8_zshift_tiles(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t r0,
                        int32_t r1, int32_t y_org, int32_t Y, int32_t th, int32_t tw, int32_t gy, int32_t gx,
                        int32_t radius, uint64_t *sums, tem_stream_t stream);

/* The sums behind the correlation of every tile of a section with ITSELF displaced by 1...nlag pixels along y and along
 * x (utils.section_plane_sums -> plane_scores -> section_sharpness -> find_blurred: sections and regions that are out of
 * focus; plane_curve -> z_pitch: how many pixels thick a section is).  The definition, once: the volume is V[Z][Y][X],
 * uint8; tiles of (th, tw) pixels on tem_u8_hist_tiles' grid, gy x gx of them anchored at the volume's (0, 0); L = nlag
 * lies in 1...8.  For a section z and a tile (i, j), over the tile's voxels (y, x): the partner of the y lag k is
 * (y + k, x), that of the x lag k is (y, x + k); a pair counts where the partner lies inside the section -- y + k < Y,
 * x + k < X; it may lie outside the tile: tem_u8_zshift_tiles' rule.  With v the voxel and w its partner:
 *   q = sums + ((z * gy + i) * gx + j) * (3 + 2 L)
 *   q[0] += v      q[1] += v v      q[2] += 1
 *   q[2 + k]     += (v - w)^2   for the y lag k = 1...L
 *   q[2 + L + k] += (v - w)^2   for the x lag k = 1...L
 * int64 and exact.  The number of terms per lag is geometry only (utils.plane_lag_counts); the kernel does not count
 * them.  Squared differences, not products: the variogram needs no mean, whose error on a small tile swamps the
 * decay from one pixel to the next.  A full 2048 x 2048 tile of 255s next to 0s stays below 2^38 per entry.
 *
 * tem_u8_zplane_lags follows tem_u8_zshift_tiles' block contract: src[D][H][W] is a dense block of WHOLE rows (W == X)
 * whose row 0 sits at volume row y_org of a section of Y rows.  The voxels counted as v are the core planes [c0, c1) and
 * core rows [r0, r1); the block must hold every partner row of the core that the section has -- [0, H) contains
 * [r0, r1 + nlag) cut to Y - y_org.  No partner plane is needed: every plane of the block may be core.  sums (8-byte
 * aligned) points at the rows of plane c0:
 *   sums[(((d - c0) * gy + i) * gx + j) * (3 + 2 nlag) + 0 .. 2 + 2 nlag] += the sums above
 * The kernel ADDS (64-bit global atomic adds, ordinary vector atomics: one per workgroup, plane and quantity): the
 * caller clears sums once, and blocks that cut a tile along y or z between them accumulate into it.  Nothing but sums
 * is written.  A load touches only naturally aligned words (up to 16 bytes) that hold at least one byte of the block.
 * Any alignment of src and W.  No partial can overflow at (v - w)^2 <= 65025 per term: a thread sums at most 16 rows of
 * 16 bytes, 256 terms, in 32 bits (256 x 65025 < 2^24), a wave 64 such partials (< 2^30); a workgroup is four waves, one
 * plane each, and every wave's sum is widened to 64 bits for its global add; the 64-bit counter takes a whole
 * 2048 x 2048 tile per plane (2^22 x 65025 < 2^38) 2^25 times over.
 * TEM_EINVAL, without a launch: what tem_u8_zshift_tiles refuses (with nlag outside 1...8 in the place of its radius),
 * and a block without a partner row that the section has.  TEM_EUNSUPPORTED: 2^24 workgroups or more (one per four core
 * planes, tile, run of up to 16 x 64 / ceil(columns / 16) rows and 1024 columns of it; their 256 threads then stay
 * below 2^32 per launch).  An empty core launches nothing. */
int tem_u8_zplane_lags(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t r0,
                       int32_t r1, int32_t y_org, int32_t Y, int32_t th, int32_t tw, int32_t gy, int32_t gx,
                       int32_t nlag, uint64_t *sums, tem_stream_t stream);

/* tem_u8_zshift_tiles with the search window of every section and tile CENTRED on an offset of its own instead of on
 * zero (utils.section_shift_sums_at, the device leg of utils.section_shifts_coarse_to_fine: a coarse level's answer,
 * doubled, is the centre of the next finer level's search, so displacements far past the radius are measured).
 * Everything is as above, plus a device table `centers` of int32 (4-byte aligned) laid out [plane][gy][gx][2] =
 * (cy, cx); like sums the pointer addresses the rows of core plane c0.  For a section z, a tile (i, j) with centre
 * (cy, cx) and a local offset (dy, dx) in [-r, r]^2, the sums run over the tile's voxels (y, x) whose partner
 * (y + cy + dy, x + cx + dx) lies inside the section, with v = V[z][y][x] and w = V[z + 1][y + cy + dy][x + cx + dx]:
 *   sums[((((d - c0) * gy + i) * gx + j) * R + dy + r) * R + dx + r) * 5 + 0..4] += (sum v, sum v v, sum w, sum w w, sum v w)
 * The layout, the 64-bit atomic adds, integer exactness and the overflow bounds are unchanged (a part still holds at
 * most 4096 voxels); the number of terms is utils.shift_counts_at.  A tile whose whole window lies outside the section
 * gets nothing added, and nothing is loaded for it.  Zero centres give tem_u8_zshift_tiles' sums, bit for bit.
 * The host promises bounds on the table: cy_lo <= cy <= cy_hi and |cx| <= cx_max, with
 * -1024 <= cy_lo <= 0 <= cy_hi <= 1024 and 0 <= cx_max <= 1024 (utils.SHIFT_MAX_CENTER).  The block must hold every
 * partner row of the core that the volume has: [0, H) contains [r0 - radius + cy_lo, r1 + radius + cy_hi) cut to
 * [-y_org, Y - y_org).  The kernel clamps every centre it reads to the promised bounds, and reads no byte outside the
 * block's rows [0, H) and columns [0, W) whatever the table holds: a table that disagrees with the promise gives
 * other sums (those of the clamped centres), never a read outside the block.
 * TEM_EINVAL as tem_u8_zshift_tiles, and: a null centers or one off 4-byte alignment, bounds outside the ranges
 * above, a block without a partner row of the core, within the bounds, that the volume has.  TEM_EUNSUPPORTED as above. */
int tem_u8_zshift_tiles_at(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t r0,
                           int32_t r1, int32_t y_org, int32_t Y, int32_t th, int32_t tw, int32_t gy, int32_t gx,
                           int32_t radius, const int32_t *centers, int32_t cy_lo, int32_t cy_hi, int32_t cx_max,
                           uint64_t *sums, tem_stream_t stream);

/* tem_u8_zshift_tiles_at over an explicit list of section pairs instead of every core plane and the one above it
 * (utils.section_shift_sums_pairs, the device leg of utils.section_shifts_bridged: a damaged section is skipped and
 * its good neighbours are measured against each other, lag 2 and more; or a few pairs are measured again).
 * src[D][H][W] is a dense block of whole rows as above whose plane 0 is VOLUME section z_org.  `pairs` is a device
 * table of int32 (4-byte aligned) laid out [npairs][2] = (a, b), volume sections with a < b; `centers` is
 * [npairs][gy][gx][2] and sums [npairs][gy][gx][R][R][5]: a row per PAIR.  For pair k = (a, b), a tile (i, j) with
 * centre (cy, cx) and a local offset (dy, dx) in [-r, r]^2, over the tile's voxels (y, x) in the core rows [r0, r1)
 * whose partner (y + cy + dy, x + cx + dx) lies inside the section, with v = src[a - z_org][y][x] and
 * w = src[b - z_org][y + cy + dy][x + cx + dx]:
 *   sums[((((k * gy + i) * gx + j) * R + dy + r) * R + dx + r) * 5 + 0..4] += (sum v, sum v v, sum w, sum w w, sum v w)
 * The five terms, the layout within a row, the 64-bit atomic adds, the overflow bounds, the promised centre bounds
 * (within +-1024) and the partner rows the block must hold are exactly tem_u8_zshift_tiles_at's; a table of
 * (z_org + d, z_org + d + 1) for d = c0 ... c1 - 1 with the same centres gives its sums bit for bit.  The caller
 * promises z_org <= a < b < z_org + D (utils keeps b - a <= SHIFT_MAX_LAG = 8, which bounds the block, not the
 * kernel).  The workgroup reads its pair once and clamps both planes to [0, D - 1], and every centre to the promised
 * bounds: a table that disagrees with the block or the promise gives other sums (those of the clamped table), never
 * a read outside the block.  The same pair may be given in several calls whose core rows or blocks differ: they add.
 * TEM_EINVAL as tem_u8_zshift_tiles_at (all but its core planes), and: a null pairs or one off 4-byte alignment,
 * npairs < 0.  TEM_EUNSUPPORTED: more than 2^31 - 1 workgroups (one per pair, tile and part of it).  npairs == 0 or
 * an empty core launches nothing. */
int tem_u8_zshift_tiles_pairs(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t z_org, int32_t npairs,
                              const int32_t *pairs, int32_t r0, int32_t r1, int32_t y_org, int32_t Y, int32_t th,
                              int32_t tw, int32_t gy, int32_t gx, int32_t radius, const int32_t *centers,
                              int32_t cy_lo, int32_t cy_hi, int32_t cx_max, uint64_t *sums, tem_stream_t stream);

/* Every section of a uint8 volume V[Z][Y][X] resampled through its own affine map (utils.volume_warp: sections aligned
 * by the maps that utils.fit_section_maps fits to the tile offsets of tem_u8_zshift_tiles).  The definition, once: a
 * section's map is six int64 in units of 2^-16, (a_yy, a_yx, b_y, a_xy, a_xx, b_x).  For the output voxel (y, x) of the
 * section, in volume coordinates, in 64-bit integers:
 *   sy = a_yy y + a_yx x + b_y,   sx = a_xy y + a_xx x + b_x
 *   fy = (sy + 128) >> 8,  fx = (sx + 128) >> 8         (arithmetic shifts: the position in 1/256 px, rounded half up)
 *   inside  iff  0 <= fy <= 256 (Y - 1)  and  0 <= fx <= 256 (X - 1);  a voxel that is not inside is `fill` -- no tap
 *           is ever blended with fill
 *   iy = fy >> 8, ty = fy & 255: the taps are rows iy and min(iy + 1, Y - 1) (the clamp is reached only with ty = 0);
 *           ix, tx likewise
 *   out = ((256 - ty) ((256 - tx) v00 + tx v01) + ty ((256 - tx) v10 + tx v11) + 2^15) >> 16      (at most 2^24: one
 *           rounding, half up, at the very end)
 *   nearest = 1 (masks):  out = V[(fy + 128) >> 8][(fx + 128) >> 8]
 * The limits |a_yy - 2^16|, |a_yx|, |a_xy|, |a_xx - 2^16| <= 2^13 (one eighth: seven degrees, or 12 % of scale) and
 * |b| < 2^47 keep every product inside 64 bits and bound the source hull of a 16 x 64 output tile by 27 rows of 75
 * bytes, which is what the kernel stages.
 * src[D][H][W] is a dense block of whole rows [sy0, sy0 + H) of D sections of VY rows and W columns (x is never cut);
 * dst[OD][OH][OW], OD == D, is the output box with its voxel 0 at (oy0, ox0) of the same sections.  maps_host points at
 * the D rows of six on the host, which are validated without a launch; maps_dev at the same rows on the device, which
 * the kernel reads.  The kernel clamps the coefficients it reads to the limits and every load to the block, so a
 * device table that disagrees with the host's gives wrong bytes, never a fault.  Every byte of dst is written exactly
 * once and nothing else is written; a load touches only naturally aligned 4-byte words that hold at least one byte of
 * the block.  Any alignment of src, dst, W and OW; every byte offset is 64 bits.  A voxel depends on its section and
 * its map alone, not on how the volume was cut.
 * TEM_EINVAL, without a launch: a null pointer, a dimension below 1, OD != D, a negative origin, a block that leaves
 * the section (sy0 + H > VY, oy0 + OH > VY, ox0 + OW > W), fill outside 0...255, nearest outside {0, 1}, a coefficient
 * outside the limits, an output block one of whose taps of weight above 0 lies outside the source block -- decided
 * per plane from the block's four corners, where the affine sy takes its extremes: with fy cut to [0, 256 (VY - 1)]
 * the rows fy_min >> 8 ... (fy_max >> 8) + (fy_max & 255 ? 1 : 0), for nearest (fy_min + 128) >> 8 ... (fy_max + 128)
 * >> 8; none where the plane is wholly outside -- and an output block of more workgroups than one launch holds: a
 * workgroup takes 16 x 64 outputs of one plane, and
 *   ceil(OH / 16) x ceil(OW / 64) x D  must stay below 2^24
 * (its 256 threads then stay below 2^32 per launch).  A block of fewer than 2^32 voxels with OH >= 16 and OW >= 64
 * always passes. */
int tem_u8_warp_affine(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY, uint8_t *dst,
                       int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
                       const int64_t *maps_dev, int32_t fill, int32_t nearest, tem_stream_t stream);

/* tem_u8_warp_affine with a smooth displacement field added to every section's map (utils.volume_warp_field: sections
 * aligned elastically by the fields that utils.fit_section_fields fits to what the affine fit leaves over).  The
 * definition, once: the lattice has the spacings Sy = 2^ky and Sx = 2^kx pixels, ky and kx in 4...10; node (i, j) sits
 * at pixel (i Sy, j Sx); there are ny = ((Y - 1) >> ky) + 2 by nx = ((X - 1) >> kx) + 2 nodes, so that every pixel of
 * the section lies in a cell with four nodes; the node values are U[i][j][0..1] = (u_y, u_x), int32 in units of 2^-16
 * px.  For the output voxel (y, x), in 64-bit integers:
 *   i = y >> ky,  ry = y & (Sy - 1);   j = x >> kx,  rx = x & (Sx - 1)
 *   uy = ((Sy - ry) ((Sx - rx) U[i][j][0] + rx U[i][j+1][0])
 *         + ry ((Sx - rx) U[i+1][j][0] + rx U[i+1][j+1][0])) >> (ky + kx)       (arithmetic shift; ux from [..][1])
 *   sy = a_yy y + a_yx x + b_y + uy,   sx = a_xy y + a_xx x + b_x + ux
 * and from sy and sx on everything is tem_u8_warp_affine's definition: fy, inside, the taps, the one rounding, nearest.
 * Consequences, exact: U = 0 gives tem_u8_warp_affine's bytes; a constant U those of the map with b moved by it; a ramp
 * U[i][j][0] = i Sy g those of the map with a_yy + g (the interpolation of a linear lattice is exact and the shift
 * divides an exact multiple), likewise for the other three coefficients.
 * The limits: the affine ones, |U| <= 2^21 (32 px), and two nodes adjacent along y differ by at most Sy 2^13 per
 * component, two adjacent along x by at most Sx 2^13: a gradient of one eighth, the size of the matrix limit.  Inside
 * a cell the exact bilinear value then changes by at most 2^13 per pixel along either axis, it is continuous across
 * cells, and the shift moves it by less than 1, so over a 16 x 64 tile u stays within (8 + 32) 2^13 + 1 of its value
 * at the tile's middle voxel: a range of 10 px on top of the matrix's 15 (1 + 1/8) + 63 / 8 = 24.75 px in sy and 72.75
 * px in sx.  34.75 px span at most 36 rows and the tap below the last makes 37; 82.75 px make 85 columns: the source
 * hull of a tile is at most 37 rows of 85 bytes, which is what the kernel stages (3,256 B of LDS).
 * src, dst, the blocks, maps_host / maps_dev, fill and nearest are tem_u8_warp_affine's; field_host points at the D
 * sections' [ny][nx][2] rows on the host, which are validated without a launch, field_dev at the same rows on the
 * device, which the kernel reads.  The kernel clamps coefficients and node values to the limits and every load to the
 * block, so a device table that disagrees with the host's gives wrong bytes, never a fault.  Every byte of dst is
 * written exactly once and nothing else is written; a load from src touches only naturally aligned 4-byte words that
 * hold at least one byte of the block; any alignment of src, dst, W and OW; every byte offset is 64 bits.
 * TEM_EINVAL, without a launch: everything tem_u8_warp_affine refuses (a null field pointer included); ky or kx
 * outside 4...10; ny or nx that are not the lattice of (VY, W); a node value or a difference of adjacent nodes outside
 * the limits; an output block whose required rows are not in the source block -- decided per plane from a superset of
 * every tap: the extremes of the affine sy at the block's four corners plus the least and the largest U[..][0] over the
 * nodes [oy0 >> ky, ((oy0 + OH - 1) >> ky) + 1] x [ox0 >> kx, ((ox0 + OW - 1) >> kx) + 1] (the interpolated value lies
 * between its nodes, and every shift is monotone), fy cut to the section, the rows fy_min >> 8 ... (fy_max >> 8) +
 * (fy_max & 255 ? 1 : 0), for nearest (fy + 128) >> 8; none where the plane is wholly outside in y or in x by the same
 * bounds -- and more workgroups than one launch holds, as tem_u8_warp_affine. */
int tem_u8_warp_field(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY, uint8_t *dst,
                      int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
                      const int64_t *maps_dev, const int32_t *field_host, const int32_t *field_dev, int32_t ny,
                      int32_t nx, int32_t ky, int32_t kx, int32_t fill, int32_t nearest, tem_stream_t stream);

/* tem_u8_warp_field's baseline for measurements (tests/tools/volume_field_time.py): the same arguments, checks and
 * bytes, computed without LDS -- every output's position from the definition in 64 bits, its taps and nodes as loads
 * from global memory, clamped to the block and the lattice.  Its loads from src are single bytes. */
int tem_u8_warp_field_direct(const uint8_t *src, int32_t D, int32_t H, int32_t W, int32_t sy0, int32_t VY, uint8_t *dst,
                             int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0, const int64_t *maps_host,
                             const int64_t *maps_dev, const int32_t *field_host, const int32_t *field_dev, int32_t ny,
                             int32_t nx, int32_t ky, int32_t kx, int32_t fill, int32_t nearest, tem_stream_t stream);

/* tem_u8_warp_affine and tem_u8_warp_field from a source block that is cut in x as well (utils.predict_volume's and
 * predict_cube's warp= keyword: a prediction chunk's footprint is a box inside sections many times its width, and whole
 * rows would read X / BW times its bytes).  No second definition: the two above are the only ones.  src[D][BH][BW] is
 * the dense box of rows [sy0, sy0 + BH) and columns [sx0, sx0 + BW) of D sections of VY x VX; dst, the output box,
 * maps_host / maps_dev, fill, nearest and stream are tem_u8_warp_affine's.  field_host == field_dev == null: no field
 * (ny, nx, ky, kx are ignored) and the bytes are tem_u8_warp_affine's; otherwise the field pointers and the lattice are
 * tem_u8_warp_field's, and so are the bytes.  With sx0 = 0 and BW = VX the call is the one above, bit for bit.
 * The kernels are the same two with the hull of a tile's taps clamped to the box on all four sides and the row stride
 * BW (a row's shift in LDS is (a0 + r (BW & 3)) & 3): a load touches only naturally aligned 4-byte words that hold at
 * least one byte of the box -- the word before its first byte and the word after its last are such words --, every
 * coefficient, node and tap is clamped as before, and a device table that disagrees with the host's gives wrong bytes,
 * never a read outside the box or LDS.  Any alignment of src, dst, BW, sx0 and OW.
 * TEM_EINVAL, without a launch: everything the entry of the same form refuses (one null field pointer of the two
 * included), a box that leaves the section (sy0 + BH > VY, sx0 + BW > VX, a negative origin), and an output block one
 * of whose taps of weight above 0 lies outside the box in y or in x.  The row rule is the one above; the column rule is
 * its mirror image: the extremes of the affine sx at the block's four corners, plus the least and the largest U[..][1]
 * over the nodes of the cells the block meets, fx cut to [0, 256 (VX - 1)], the columns fx_min >> 8 ... (fx_max >> 8) +
 * (fx_max & 255 ? 1 : 0), for nearest (fx + 128) >> 8.  A plane wholly outside the section in y or in x needs nothing.
 * utils.warp_source_box states the same rule on the host, so a box it planned is never refused. */
int tem_u8_warp_box(const uint8_t *src, int32_t D, int32_t BH, int32_t BW, int32_t sy0, int32_t sx0, int32_t VY,
                    int32_t VX, uint8_t *dst, int32_t OD, int32_t OH, int32_t OW, int32_t oy0, int32_t ox0,
                    const int64_t *maps_host, const int64_t *maps_dev, const int32_t *field_host,
                    const int32_t *field_dev, int32_t ny, int32_t nx, int32_t ky, int32_t kx, int32_t fill,
                    int32_t nearest, tem_stream_t stream);

/* Random augmentation of one cached sample (datasets.py:123-155) with host-drawn parameters:
 *   dst = reverse(transpose(src, perm = (p0,p1,p2)), dims with f_k != 0) * scale + shift
 * src is a dense single-channel (D,H,W) volume (2-D: D == 1, p0 must be 0); dst has extents
 * (dim[p0], dim[p1], dim[p2]) and must not alias src. */
int tem_augment_f32(const float *src, int32_t D, int32_t H, int32_t W, int32_t p0, int32_t p1, int32_t p2,
                    int32_t f0, int32_t f1, int32_t f2, float scale, float shift, float *dst, tem_stream_t stream);

/* debug.warp_tensor (debug.py:7-63) on the device: dst = box blur of src (3 wide per non-unit axis, zero SAME
 * padding); hole seeds ~ Bernoulli(rate) per voxel (Philox stream of `seed`, written to `seeds`, one byte per
 * voxel), dilated by a 4-wide box (SAME: 1 before, 2 after); holes := mean(blurred).  `sum`: one double of
 * workspace.  dst must not alias src. */
int tem_warp_f32(const float *src, int32_t D, int32_t H, int32_t W, float rate, uint64_t seed, float *dst,
                 uint8_t *seeds, double *sum, tem_stream_t stream);

/* One batch of the generator dataset's crops (datasets.py:69-155 over generators.py:59-118), cut in one launch.
 * Source: `src` is uint8 (src_f32 == 0: converted x / 127.5 - 1) or float32 (src_f32 == 1: taken as is); sample b
 * reads src + b * sB with element strides sZ, sY, sX and extents vol[3] (z, y, x).  Crop b is the n[3] box at origin
 * params[12b + 0..2] (z, y, x), REFLECT-padded by pad_lo / pad_hi voxels per axis as np.pad(..., "reflect") (the
 * padding is an index map inside the crop; a crop not inside vol reads NaN).  Then, when enabled:
 * (v - mean) / std (standardize), and dst = reverse(transpose(v, perm), flagged dims) * var_adj + mean_adj
 * (augment; perm = params[12b + 3..5], flips = params[12b + 6..8], var_adj / mean_adj = the float bits of
 * params[12b + 9..10], params[12b + 11] unused).  Every step is one correctly rounded float32 operation, in that order.
 * dst: B dense samples of the padded extents permuted (sample stride = their product), 16-byte aligned.  params is a
 * device pointer. */
typedef struct tem_crop_args {
  const void *src;
  int32_t src_f32;
  int32_t B;
  int64_t sB, sZ, sY, sX;
  int64_t vol[3];
  int32_t n[3], pad_lo[3], pad_hi[3];
  int32_t standardize, augment;
  float mean, std;
  const int32_t *params;
  float *dst;
} tem_crop_args;

int tem_crop_batch(const tem_crop_args *args, tem_stream_t stream);

/* Statistics pass of the dataset (datasets.py:173-190): B dense float32 samples of n elements; block k of sample b
 * writes partials[(b * nblk + k) * 2 + {0, 1}] = float64 {sum, sum of squares} of its grid-strided share. */
int tem_sample_sums_f32(const float *src, int32_t B, int64_t n, int32_t nblk, double *partials, tem_stream_t stream);

/* dst[i] = value */
int tem_fill_f32(float *dst, int64_t n, float value, tem_stream_t stream);

/* dst(view) = src(view) elementwise; same extents (crop / pad / channel-slice copies) */
int tem_copy_view(const tem_view *src, const tem_view *dst, tem_stream_t stream);

/* dst(view) += src(view) */
int tem_add_view(const tem_view *src, const tem_view *dst, tem_stream_t stream);

/* One convolution kernel inside a flat parameter vector: `ntap` taps of a [ci][co] block at element `offset`. */
typedef struct tem_wlayer {
  int64_t offset;
  int32_t ntap, ci, co;
} tem_wlayer;

/* theta_t := theta with every listed kernel's taps reversed and (ci, co) transposed,
 *   theta_t[off + ((ntap-1-t)*co + b)*ci + a] = theta[off + (t*ci + a)*co + b];
 * elements outside the table (biases) are copied.  The input-gradient of a stride-1 convolution is then a plain
 * TEM_W_TAP_CI_CO convolution over theta_t -- same numbers as TEM_W_FLIP_CO_CI over theta, but the kernel-tap
 * fragments are read as contiguous 64-byte runs (measured 27-33 % faster on the LDS-tiled kernels).  One launch
 * per network and step, after the optimizer update (reference: the transposed filter cuDNN/Eigen build inside
 * Conv3DBackpropInputV2).  `layers_dev` is device memory. */
int tem_flip_transpose(const float *theta, float *theta_t, const tem_wlayer *layers_dev, int32_t nlayers,
                       int64_t total, tem_stream_t stream);

/* One kernel of tem_winograd_weights: the 27 taps of a [ci][co] block at theta + src_off (flip = 0: the operator's
 * kernel is theta[tap][ci][co], a forward Conv layer; flip = 1: theta[26-tap][co][ci], its input-gradient) are
 * transformed to U[kz] = G g[kz] G^T on the (y, x) axes (16 points per z tap) and written at u + dst_off in the fragment
 * order of the Winograd kernel: (ci / 8) * ceil(co / 16) * 6144 floats per layer (8 -> 8: 8192), ci, co the operator's
 * channel counts (8, 16 or 32; 32 -> 16 is not built). */
typedef struct tem_wino_layer {
  int64_t src_off, dst_off;
  int32_t ci, co, flip;
} tem_wino_layer;

/* Once per network and step, after the optimizer update (as tem_flip_transpose): the Winograd-domain copies of the
 * listed kernels.  `layers_dev` is device memory.  (The reference leaves the choice of convolution algorithm to
 * TF/cuDNN, which picks Winograd forms for 3x3 kernels the same way.) */
int tem_winograd_weights(const float *theta, float *u, const tem_wino_layer *layers_dev, int32_t nlayers,
                         tem_stream_t stream);

/* Kernel gradient of a k 3, s 1 layer (C_in -> C_out: 16 -> 16, 8 -> 16, 8 -> 8) in the Winograd domain of
 * tem_winograd_weights (2.25x fewer matrix flops than tem_conv_bwd_weight; same operator, fp32 rounding differs).  Same
 * slab contract as tem_conv_bwd_weight: the launch writes exactly tem_conv_bwd_weight_winograd_nslab(a) slabs (query
 * with a->nslab = the caller's upper bound; negative: TEM_E*, e.g. TEM_EUNSUPPORTED for other geometries; `name`, if
 * non-NULL, receives the kernel's name), one per workgroup, already transformed back to [27][ci][co]; pass that value
 * as a->nslab.  Deterministic (fixed summation orders). */
int tem_conv_bwd_weight_winograd_nslab(const tem_bww_args *a, char *name, int32_t name_len);
int tem_conv_bwd_weight_winograd(const tem_bww_args *a, tem_stream_t stream);

/* g(view) = saved(view) > 0 ? g : slope * g, in place: LeakyReLU gradient gated on the saved output where no
 * convolution epilogue can carry it (gradient entering the frozen prior network, discriminator.py:62-66). */
int tem_leaky_gate_view(const tem_view *g, const tem_view *saved, float slope, tem_stream_t stream);

/* ---- bf16 mixed precision (BASELINE config 5; the reference is fp32 only, cgan.py:13-14) -------------------------
 * Activations, gate / add views and the kernel copy are bfloat16: the `float *` fields of tem_view / tem_conv_args
 * carry bf16 pointers, strides stay in ELEMENTS.  `w` is the layer's kernel packed [tap][co][ci] in bf16
 * (tem_pack_weights_bf16); w_layout == TEM_W_FLIP_CO_CI reverses the taps (input-gradient of a stride-1 layer over
 * the un-transposed copy).  Accumulation, bias, LeakyReLU / gate / dropout run in fp32; outputs are rounded to
 * bf16 (nearest even) on store.  Same operator definition and epilogue order as tem_conv.
 * 2-D geometry -- depth-1 views, kd = sd = 1, pd = 0, kh = kw in {3, 4}, sh = sw, ph = pw (is3d=False) -- is accepted by
 * tem_conv_bf16 (k3 s1 and k4 s2), tem_conv_transpose_bf16 (k4 s2) and tem_conv_bwd_weight_bf16 (k3 s1, k4 s2, also
 * the swapped C_out = 1 form with ph = pw = 2) for the channel pairs of the 2-D networks; 1x1 layers arrive as 1x1x1. */
int tem_conv_bf16(const tem_conv_args *a, tem_stream_t stream);

/* TEM_OK and the kernel's name (as rocprofv3 prints it) if tem_conv_bf16 accepts these arguments. */
int tem_conv_bf16_describe(const tem_conv_args *a, char *name, int32_t name_len);

/* bf16 form of tem_conv_transpose (k4 s2 only, 3-D or 2-D geometry): `w` = bf16 kernel [tap][co][ci]. */
int tem_conv_transpose_bf16(const tem_conv_args *a, tem_stream_t stream);
int tem_conv_transpose_bf16_describe(const tem_conv_args *a, char *name, int32_t name_len);

/* bf16 form of tem_conv_bwd_weight: in0 / in1 / dout are bf16 views, the partial slabs are float32 (the split-K
 * finish, the gradient vector and Adam stay fp32).  The launch writes exactly the number of slabs that
 * tem_conv_bwd_weight_bf16_nslab(a) returns for a->nslab = the caller's upper bound (negative: TEM_E*; `name`, if
 * non-NULL, receives the kernel's name); pass that value back as a->nslab. */
int tem_conv_bwd_weight_bf16(const tem_bww_args *a, tem_stream_t stream);
int tem_conv_bwd_weight_bf16_nslab(const tem_bww_args *a, char *name, int32_t name_len);

/* dst[i] = bf16(src[i]) (round to nearest even) */
int tem_cast_f32_to_bf16(const float *src, void *dst, int64_t n, tem_stream_t stream);

/* The per-step bf16 kernel copies of one network: theta_h = bf16(theta), same layout; theta_ht = every kernel of
 * the table with its last two axes transposed ([tap][A][B] -> [tap][B][A]).  tem_conv_bf16 contracts over the LAST
 * axis of the copy it is given: forward of a Conv layer reads theta_ht, its stride-1 input-gradient theta_h with
 * TEM_W_FLIP_CO_CI; a ConvTranspose layer (and the input-gradient of a stride-2 Conv through
 * tem_conv_transpose_bf16) reads theta_h, the ConvTranspose input-gradient theta_ht. */
int tem_pack_weights_bf16(const float *theta, void *theta_h, void *theta_ht, const tem_wlayer *layers_dev,
                          int32_t nlayers, int64_t total, tem_stream_t stream);

/* bf16 forms of tem_focal_logits / tem_focal_match / tem_copy_view / tem_add_view / tem_channel_sum: bf16 views in
 * and out, fp32 arithmetic, double loss sums. */
int tem_focal_logits_bf16(const tem_view *z, int32_t target, float gamma, double *losses, uint32_t slot_mask,
                          float loss_scale, const tem_view *dz, float grad_scale, tem_stream_t stream);
int tem_focal_match_bf16(const tem_view *a, const tem_view *b, float gamma, double *losses, uint32_t slot_mask,
                         float loss_scale, const tem_view *db, float grad_scale, tem_stream_t stream);
int tem_copy_view_bf16(const tem_view *src, const tem_view *dst, tem_stream_t stream);
int tem_add_view_bf16(const tem_view *src, const tem_view *dst, tem_stream_t stream);
int tem_channel_sum_bf16(const tem_view *g, float *out, int32_t accumulate, tem_stream_t stream);

/* InstanceNormalization (models/utils.py:10-38; defined there, every call site commented out at
 * models/utils.py:75-76,81-82,124-125,131): per sample and channel, over the spatial axes,
 *   mean, variance = tf.nn.moments(x);  y = scale[c] * (x - mean) * rsqrt(variance + eps) + offset[c].
 * mean / rstd ([N*C] each) are written for the backward pass. */
int tem_instance_norm(const tem_view *x, const float *scale, const float *offset, float eps,
                      const tem_view *y, float *mean, float *rstd, tem_stream_t stream);

/* Gradient of tem_instance_norm: dx (may alias dy), dscale[C], doffset[C] (either may be NULL).
 * workspace: 2*N*C doubles. */
int tem_instance_norm_bwd(const tem_view *x, const tem_view *dy, const float *scale, const float *mean,
                          const float *rstd, const tem_view *dx, float *dscale, float *doffset,
                          double *workspace, tem_stream_t stream);

/* ---- launch plans of the z-marching kernels: pin and read back (a test seam; off unless called)
 * The tile plan of wino_conv_k, wino_bww_k, conv_lds_k and conv3_bf16_k comes from a host-side cost model that searches the
 * feasible (tile block, z split) candidates of a geometry.  tem_plan_pin restricts that search, for the calling thread and one
 * family, to the candidates whose pinned fields match (a field of -1 is free; v4 == NULL clears the pin).  Every feasibility
 * condition of the planner applies unchanged, so a pin only selects among plans the planner could have chosen itself; where no
 * candidate matches, the family answers TEM_EUNSUPPORTED (and tem_conv / tem_conv_bf16 go on to their next kernel, as for
 * any geometry the family does not take).  While a pin is set the family's plan memo is neither read nor written.
 * tem_plan_last reports the plan of the calling thread's most recent successful decision of the family (dry query, slab-count
 * query or launch); TEM_EINVAL before any, or for an unknown family.
 *   family               pin v4                   last v8
 *   TEM_PLAN_WINO        {E, BY, BX, zsegs}       {E, BY, BX, zsegs, zper, nby, nbx, ndma}      (z in tiles of 2 planes)
 *   TEM_PLAN_WINO_BWW    {E, BY, BX, zsegs}       {E, BY, BX, zsegs, zper, nby, nbx, ndma}
 *   TEM_PLAN_CONV_LDS    {MTW, R, patch, zsegs}   {MTW, R, patch, zsegs, zper, nych, ntiles, 0}
 *   TEM_PLAN_CONV3_BF16  {nbx, TY, zsegs, -1}     {nbx, TY, zsegs, zper, nby, RD, ndma, 0}
 * The k4 s2 kernels take their launch geometry from closed-form rules, one number each; a pin replaces the number the rule
 * would have computed and every validity check of the host code applies unchanged.  Outside the range the kernel covers the
 * family answers TEM_EUNSUPPORTED (and tem_conv / tem_conv_transpose / tem_conv_bwd_weight go on to their next kernel); the
 * slab-count and *_is_tiled queries answer under a pin what the launch will do.  A pin takes precedence over the knob builds'
 * TEM_S2_WGS, TEM_BWW_S2_R and TEM_BWW_S2_TBR.
 *   family               pin v4            valid under a pin                          last v8
 *   TEM_PLAN_CONV_S2     {nblocks, -1..}   1 <= nblocks <= min(iters, resident)       {nblocks, ny, T, iters, total, tiles_pp, TB, resident}
 *   TEM_PLAN_CONVT_MFMA  {TY, -1..}        1 <= TY <= min(nQy, 32), the patch within  {TY, nband, nQz, nQy, nQx, NCLS, EPM, 0}
 *                                          the loader's registers and 56 KB of LDS
 *   TEM_PLAN_BWW_S2      {R, -1..}         1 <= R <= min(rows, max slabs)             {R, rows, tb (1: bww_s2tb_k), KS, OW, 0, 0, 0}
 * (conv_s2_k: workgroups along x, along y, tiles per iteration, iterations, tiles, tiles per plane, two-block form, resident
 * slots.  convT_mfma_k: Q_y rows per band, bands, Q extents, classes per patch, compiled epilogue.  bww_s2_k / bww_s2tb_k: row
 * ranges = slabs, output rows N OD OH, kernel extent, row length.)
 * The 3-D kernels of bf16 mode take their launch geometry from the host as well: conv_bf16_k an output patch from a score search
 * over TY 1..16 x nbx 1..8, convT_bf16_k the Q_y rows of a band and bww_bf16_k band rows, z-runs and column segments from closed
 * forms.  The same semantics: a pin replaces the searched or computed number, every validity check of the host code applies
 * unchanged, outside the valid range the family answers TEM_EUNSUPPORTED (the route goes on; these kernels are its last), and
 * tem_conv_bf16_describe / tem_conv_transpose_bf16_describe / tem_conv_bwd_weight_bf16_nslab answer under a pin what the launch
 * will do.  A pin takes precedence over the knob builds' TEM_BWWH_*.
 *   family               pin v4               valid under a pin                            last v8
 *   TEM_PLAN_CONV_BF16   {TY, nbx, -1, -1}    the search's own feasibility (loader chunks, {TY, nbx, TX, nby, rows, cols, tiles, LDS bytes}
 *                                             64 KB) and nbx == ceil(OW / TX): no empty
 *                                             last column
 *   TEM_PLAN_CONVT_BF16  {TY, -1..}           1 <= TY <= min(nQy, 32), the patch within    {TY, nband, nQz, nQy, nQx, NCLS, EPM, 0}
 *                                             the loader's registers and 56 KB of LDS
 *   TEM_PLAN_BWW_BF16    {TY, zsegs, seg, -1} TY: 1 .. the rule's own bound for the row;   {TY, nband, zsegs, zper, nseg, seg, NGRP, slabs}
 *                                             zsegs: 1 .. OD and canonical (zsegs ==
 *                                             ceil(OD / ceil(OD / zsegs))); seg: a multiple
 *                                             of 16 whose one-row band fits, pad 0 (seg >=
 *                                             OW: the single launch); workgroups <= nslab
 * (conv_bf16_k: patch rows, column blocks, patch columns, row blocks, input patch rows and columns, 16-voxel tiles of a full
 * patch, dynamic LDS.  bww_bf16_k: rows per band, bands, z-runs, planes per run, column segments, segment width (OW: one
 * launch), row groups = grid.y, slabs of the whole launch; TY, nband, zsegs, zper are the first segment's.) */
#define TEM_PLAN_WINO       1
#define TEM_PLAN_WINO_BWW   2
#define TEM_PLAN_CONV_LDS   3
#define TEM_PLAN_CONV3_BF16 4
#define TEM_PLAN_CONV_S2    5
#define TEM_PLAN_CONVT_MFMA 6
#define TEM_PLAN_BWW_S2     7
#define TEM_PLAN_CONV_BF16  8
#define TEM_PLAN_CONVT_BF16 9
#define TEM_PLAN_BWW_BF16   10
int tem_plan_pin(int32_t family, const int32_t *v4);
int tem_plan_last(int32_t family, int32_t *v8);

/* Library identification: returns TEM_ABI_VERSION; *arch (if non-NULL) receives a
 * static string naming the compiled offload target ("gfx950"). */
int tem_abi_version(const char **arch);

#ifdef __cplusplus
}
#endif
#endif /* TEM_HIP_H */
