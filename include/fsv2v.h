/* fsv2v.h - C ABI of libfsv2v_hip.so: the MI355X (gfx950) kernels behind the few-shot-vid2vid G/D training step.
 *
 * The reference (NVlabs/few-shot-vid2vid) has no FFI for this path - its operator seam is Python name binding
 * (SURVEY.md section 8b): models.networks.base_network.{batch_conv,resample}, normalization.SPADE,
 * architecture.SPADEResnetBlock, generator.{LabelEmbedder,FlowGenerator}, discriminator.NLayerDiscriminator, which in
 * turn call torch ATen (F.conv2d, F.grid_sample, BatchNorm, ...).  Its only native boundary is the pybind pattern of
 * the FlowNet2 extensions (models/networks/flownet2_pytorch/networks/resample2d_package/resample2d_cuda.cc:6-31:
 * plain tensors in, int status out, kernels enqueued on the caller's stream).  This header follows that convention:
 *
 *   - every function returns 0 (FSV_OK) or a negative fsv_status; nothing throws or aborts across the boundary;
 *   - all pointers are device pointers owned by the caller (PyTorch's caching allocator); the library allocates
 *     nothing and keeps no state between calls - no setter-style entry points, nothing "armed" for a later call; scratch
 *     buffers, optional workspaces and optional side outputs are explicit (nullable) arguments of the call that uses them;
 *   - work is only enqueued on `stream` (a hipStream_t); calls are re-entrant and graph-capturable
 *     (only kernels and hipMemsetAsync are issued);
 *   - activations are fp32 NHWC ("channels last"); convolution weights are fp32 OIHW at the boundary and are
 *     re-arranged K-major by fsv_prep_weight.
 *
 * Each entry point cites the reference code it replaces (paths relative to the reference root).
 */
#ifndef FSV2V_H
#define FSV2V_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef FSV_STREAM_T_DEFINED /* the kernel sources define it as hipStream_t before including this file; a pointer either way */
typedef void* fsv_stream_t; /* hipStream_t */
#endif

enum fsv_status { FSV_OK = 0, FSV_ERR_BAD_ARG = -1, FSV_ERR_UNSUPPORTED = -2, FSV_ERR_LAUNCH = -3 };
enum fsv_act { FSV_ACT_NONE = 0, FSV_ACT_LRELU = 1 /* leaky_relu(0.2), architecture.py:15-17 */, FSV_ACT_TANH = 2,
               FSV_ACT_SIGMOID = 3, FSV_ACT_RELU = 4 /* VGG19 stack */, FSV_ACT_LRELU01 = 5 /* leaky_relu(0.1), FlowNet2 */,
               /* gather-GEMM epilogue only: out = v * leaky_relu'(res) (res = the activated output of the layer below): the
                * activation-backward pass of a Linear + LeakyReLU chain (generator.py:103-110) folded into the data gradient */
               FSV_ACT_DLRELU = 6 };
/* objective of fsv_hinge_fwd / fsv_hinge_bwd: the reference's --gan_mode (GANLoss, models/networks/loss.py:17-104) */
enum fsv_gan_mode { FSV_GAN_HINGE = 0 /* loss.py:69-79 */, FSV_GAN_LS = 1 /* :57-61 */, FSV_GAN_ORIGINAL = 2 /* :50-53 */,
                    FSV_GAN_W = 3 /* :85-90 */ };

/* ---- convolution family (csrc/conv_igemm.hip) -----------------------------------------------------------------
 * Replaces F.conv2d at architecture.py:22-27,60,81-84; generator.py:112-131,479-504,541-572;
 * discriminator.py:67-88; nn.Linear at generator.py:103-110; batch_conv at base_network.py:56-71 and, through
 * autograd, their cudnn backward kernels.
 *
 * out[n, oy*osy+ooy, ox*osx+oox, co] = act(( sum_t sum_ci in[n, oy*sy+ty[t], ox*sx+tx[t], ci] * wt[t*Cin+ci][co]
 *                                            + bias[co] ) * scale) + res[...]
 * taps outside the input read as zero.  wt: K-major [Kpad][ldw] from fsv_prep_weight; per_sample != 0 selects one
 * weight matrix (stride w_bstride) and bias (stride b_bstride) per sample n.  accumulate != 0: `out` was zeroed by
 * the caller, results are added (used for the four parity classes of a stride-2 data gradient).
 * force_tile / force_split: -1 / 0 = automatic; a tile id is a row of the tile-variant table (csrc/conv_igemm.hip FSV_CONV_TILES,
 * readable through fsv_conv_tile_info): FSV_ERR_BAD_ARG for any other id.
 * Per-launch bounds: the INPUT tensor of one launch - all N samples together, also with per_sample != 0, whose kernels form a
 * sample's pixels as 32-bit byte offsets from the base of the batch - and one weight matrix may hold at most 2 GiB each:
 * FSV_ERR_UNSUPPORTED beyond, nothing launched.  `out` (and res / the split-K copies) is addressed with 64-bit element offsets and
 * has no bound of its own below 2^31 pixels per launch.  A caller with more (the attention of n_shot > 1, networks.py) issues
 * the launch in bands of samples / rows, each inside these bounds.  wscale: optional device scalar multiplying the accumulator before
 * the bias (the spectral-norm 1/sigma when wt holds un-normalised weights). */
/* split_ws / split_ws_floats (nullable; ordered split-K): when the call's plan splits K, split k stores its partial output into
 * the k-th copy inside split_ws (nsplit x N*outH*outW*Cout floats) and the copies are summed in ascending order: the same bits on
 * every run, no zero fill, no atomics (a finishing pass sums the copies).  A call that does not split, or whose copies do not fit into split_ws_floats,
 * ignores the workspace (and adds atomically into a zeroed output).
 * in_up != 0: nn.Upsample(scale_factor=2) in front of the convolution (generator.py:124,497-504,541-572) folded into the gather -
 * `in` is stored at H / 2 x W / 2 (H, W stay the size the convolution sees: even) and read at (y >> 1, x >> 1); the up-sampled
 * tensor is never written.  Float4-gather MFMA launches only (Cin % 4 == 0, Cout > 4, shared weights, no accumulate):
 * FSV_ERR_UNSUPPORTED otherwise - materialise with fsv_upsample2x_fwd then.  fsv_conv_wgrad takes the same flag. */
int fsv_conv_gather_fwd(const float* in, const float* wt, const float* bias, const float* res, float* out,
                        int N, int H, int W, int Cin, int OH, int OW, int Cout,
                        int ntaps, const int* ty, const int* tx, int sy, int sx,
                        int outH, int outW, int osy, int osx, int ooy, int oox,
                        int ldw, long long w_bstride, long long b_bstride, int per_sample,
                        int act, float scale, int force_tile, int force_split, int accumulate, const float* wscale,
                        float* split_ws, long long split_ws_floats, int in_up, fsv_stream_t stream);

/* ---- grouped launches: up to 64 INDEPENDENT problems in one grid --------------------------------------------------------
 * The reference issues the 16 weight-generator MLPs (generator.py:103-110,245-273: three nn.Linear each, per adaptive level
 * and per SPADE site) and the transposed-convolution data gradients of its stride-2 layers one cudnn call at a time; on this
 * device every such launch lasts as long as its longest workgroup while most of the 256 CUs idle.  A group puts the tiles of
 * all its problems into one grid (longest problems first).  fsv_conv_desc = the arguments of fsv_conv_gather_fwd;
 * accumulate != 0: `out` was zeroed by the caller and the problem may be K-split (atomic adds, no epilogue).  No problem of a
 * group may read what another one writes.  A problem with Cin % 4 != 0 sends the whole group to the scalar-gather kernel. */
typedef struct fsv_conv_desc {
  const float* in; const float* wt; const float* bias; const float* res; float* out; const float* wscale;
  int N, H, W, Cin, OH, OW, Cout, ntaps;
  int ty[16], tx[16];
  int sy, sx, outH, outW, osy, osx, ooy, oox, ldw;
  int per_sample, act, accumulate;
  float scale;
  long long w_bstride, b_bstride;
} fsv_conv_desc;
int fsv_conv_gather_group(const fsv_conv_desc* problems, int n, int force_tile, fsv_stream_t stream);
/* tile id the grouped launch uses for problems of these sizes (Mz = pixels per sample group, nchunks = ceil(taps * Cin / 32)) */
int fsv_conv_group_plan(const int* Mz, const int* Cout, const int* nchunks, const int* nsamp, int n, int* tile_out);
/* ---- conv3x3(nearest_x2(x)) forward of the deep layers as its four sub-pixel classes (generator.py:489-493, 559-563) ----------
 * out[n, 2y + ry, 2x + rx, :] = act((sum_{iy, ix in {0, 1}} x[n, y + ry - 1 + iy, x + rx - 1 + ix, :] @ wt[class (ry, rx)][tap (iy, ix)]
 *                                     * wscale + bias) * scale): 16 products per source pixel and channel pair instead of the 36 of the
 * gather through the up-sampling index.  x: NHWC fp32 [N][H][W][Cin] at SOURCE resolution; out: [N][2H][2W][Cout]; wt: the
 * class-major 16-tap K-major layout [16 Cin][ldw] (class c = 2 ry + rx owns rows [4 c Cin, 4 (c + 1) Cin), taps (iy, ix) row-major,
 * summed weights W0 | W1 + W2 resp. W0 + W1 | W2 per axis).  The four class problems run as ONE grouped launch with one tile shape
 * and one K-split factor, planned for the four together (fsv_conv_up_subpixel_plan; force_tile / force_split as in
 * fsv_conv_gather_fwd, a tile id counts for its shape).  nsplit > 1: split k of class c stores a dense copy into
 * workspace[c][k][N H W][Cout] and ONE finishing launch sums the copies in ascending k, applies wscale, bias, activation and scale
 * and stores to the placed positions - no atomics, the same bits on every run; workspace (16-byte aligned) must then hold
 * the plan's workspace_floats: FSV_ERR_BAD_ARG otherwise.  nsplit == 1 ignores the workspace.  Allocates nothing, keeps nothing.
 * Contract: (4 Cin) % 32 == 0, Cout % 4 == 0, fewer than 2^31 output elements, and no residual, statistics or per-sample weights -
 * res, stats non-null or per_sample != 0: FSV_ERR_UNSUPPORTED, nothing launched (the caller takes the single gather, in_up = 1). */
int fsv_conv_up_subpixel_plan(int N, int H, int W, int Cin, int Cout, int force_tile, int force_split, int* tile_out,
                              int* nsplit_out, long long* workspace_floats);
int fsv_conv_up_subpixel_fwd(const float* x, const float* wt, int ldw, const float* bias, const float* res, const float* wscale,
                             int act, float scale, float* out, double* stats, int N, int H, int W, int Cin, int Cout,
                             int per_sample, float* workspace, long long workspace_floats, int force_tile, int force_split,
                             fsv_stream_t stream);
/* grouped weight gradients (arguments of fsv_conv_wgrad): every dwt is a ZEROED [Kpad][ldw] matrix; float4-gather layers only
 * (Cin % 4 == 0), FSV_ERR_UNSUPPORTED with nothing launched otherwise - issue the problems one by one then */
typedef struct fsv_wgrad_desc {
  const float* in; const float* dout; float* dwt;
  int N, H, W, Cin, OH, OW, Cout, ntaps;
  int ty[16], tx[16];
  int sy, sx, ldw, Kpad;
  int per_sample, reserved;
  long long w_bstride;
} fsv_wgrad_desc;
int fsv_conv_wgrad_group(const fsv_wgrad_desc* problems, int n, fsv_stream_t stream);

/* fsv_conv_gather_fwd (dense output, shared weights) that also leaves the per-channel sums of its output for the
 * normalisation that follows - conv -> BatchNorm (architecture.py:57-69, generator.py:479-496) and conv -> InstanceNorm
 * (discriminator.py:67-88) read the convolution's output a second time only to reduce it; here the epilogue adds
 * (sum y, sum y^2) per channel into stats[group][slot][Cout][2] (doubles; zeroed by this call unless stats_prezeroed - a slice of
 * a per-pass arena the caller zeroes once; slot = pixel tile % stats_slots,
 * group = sample block: stats_groups = 1 for BatchNorm, N for InstanceNorm) and fsv_norm_stats_finish turns them into
 * mean / rstd.  *produced = 0: this launch could not (K-split plan, Cin % 4 != 0) - run fsv_norm_stats instead. */
int fsv_conv_gather_fwd_stats(const float* in, const float* wt, const float* bias, const float* res, float* out,
                              int N, int H, int W, int Cin, int OH, int OW, int Cout,
                              int ntaps, const int* ty, const int* tx, int sy, int sx,
                              int ldw, int act, float scale, const float* wscale,
                              double* stats, int stats_groups, int stats_slots, int stats_prezeroed, int* produced,
                              float* split_ws, long long split_ws_floats, int in_up, fsv_stream_t stream);
/* in place: x = act(x + bias[c]) over an NHWC tensor (finishing pass of operators that add several GEMM launches into one
 * output: convolutions with more than 16 taps, transposed convolutions); act codes as in the conv epilogue, 5 = leaky 0.1 */
int fsv_bias_act(float* x, const float* bias, long long total, int C, int act, fsv_stream_t stream);
/* dwt[t*Cin+ci][co] = sum_{n,oy,ox} in[n, oy*sy+ty[t], ox*sx+tx[t], ci] * dout[n, oy, ox, co]  (weight gradient)
 * prezeroed: dwt already holds zeros (a slice of the optimiser's per-pass arena), skip the split-K zero-fill;
 * force_tile: 0 = the launcher's plan, 1 / 2 / 3 / 4 = 64x64 / 128x64 / 64x128 / 128x128 rows x columns (float4-gather layers wide
 * enough for the tile, else ignored; for A/B runs) */
int fsv_conv_wgrad(const float* in, const float* dout, float* dwt,
                   int N, int H, int W, int Cin, int OH, int OW, int Cout,
                   int ntaps, const int* ty, const int* tx, int sy, int sx,
                   int ldw, int Kpad, long long w_bstride, int per_sample, int force_split, int prezeroed,
                   int force_tile, int in_up, fsv_stream_t stream);

/* ---- half-precision path (csrc/conv_h.hip): the reference's `--amp O1` arithmetic (options/base_options.py:127,
 * models/models.py:22-26, loss_collector.py:221-224; BASELINE.json configs[4] "fp16 MFMA path") with activations AND weights
 * 16-bit in HBM.  Contract of one convolution: operands are IEEE half in memory (whoever produced them rounded once), products are
 * exact, accumulation is fp32 (v_mfma_f32_32x32x16_f16), (acc * wscale + bias) * scale -> act -> + res in fp32, one rounding at
 * the store when out_h.  Activations NHWC half with Cin % 8 == 0; weights N-MAJOR half wt[z][nrows][Kpad] (K = taps * Cin
 * contiguous, Kpad % 64 == 0, zero padded) as written by fsv_hconv_prep_weight from the K-major fp32 layout of fsv_prep_weight.
 * fsv_hconv_desc = one problem; n == 1: a single launch that may split K (partial sums in fp32: `ws` when the output is half) and
 * may leave normalisation statistics (stats / *produced as fsv_conv_gather_fwd_stats); n > 1: ONE grid over independent
 * problems (fsv_conv_gather_group).  res / out are half when res_h / out_h, else fp32; act FSV_ACT_DLRELU reads res as the aux
 * tensor.  accumulate != 0: acc * wscale is ADDED into the fp32 `out` the caller zeroed (no bias, residual, activation, scale or
 * half output: FSV_ERR_BAD_ARG).  FSV_ERR_UNSUPPORTED (nothing launched) for geometries outside this contract: callers keep those on the fp32 path. */
typedef struct fsv_hconv_desc {
  const void* in; const void* wt; const float* bias; const void* res; void* out; const float* wscale;
  float* ws; double* stats;
  int N, H, W, Cin, OH, OW, Cout, ntaps;
  int ty[16], tx[16];
  int sy, sx, outH, outW, osy, osx, ooy, oox;
  int Kpad, nrows;
  int per_sample, act, accumulate;
  int out_h, res_h;
  int force_tile, force_split;
  int stats_groups, stats_slots, stats_prezeroed;
  float scale;
  long long w_bstride, b_bstride;
} fsv_hconv_desc;
int fsv_hconv_gather(const fsv_hconv_desc* problems, int n, int* produced, fsv_stream_t stream);
/* tile id (0 = 128x128, 1 = 128x64, 2 = 128x32, 4 = 64x64, 9 = 64x128; + 16: two LDS buffers instead of three) and K split the
 * single launch will use; nchunks = ceil(taps * Cin / 64) */
int fsv_hconv_plan(int Mz, int Cout, int nchunks, int nsamp, int force_tile, int force_split, int can_split, int* tile_out,
                   int* nsplit_out);
/* weight gradient from half activations `in` (NHWC, Cin % 8 == 0) and half output gradients `dout` ([pixels][Cout], Cout % 8 == 0)
 * into the fp32 K-major matrix dwt[Kpad][ldw] of fsv_conv_wgrad (same arguments); force_tile 1 / 2 / 3 / 4 / 5 = 64x64 / 128x64 /
 * 64x128 / 128x128 / 128x32 */
int fsv_hconv_wgrad(const void* in, const void* dout, float* dwt,
                    int N, int H, int W, int Cin, int OH, int OW, int Cout,
                    int ntaps, const int* ty, const int* tx, int sy, int sx,
                    int ldw, int Kpad, long long w_bstride, int per_sample, int force_split, int prezeroed,
                    int force_tile, fsv_stream_t stream);
/* K-major fp32 wt[z][Kpad32][ldw] -> N-major half wh[z][nrows][Kpad64], table-driven (one launch for a whole layout cache):
 * jobs[j] = {src, dst, Kpad32, ldw, nrows, Kpad64, nbatch, 0} as 64-bit words (device), tmap[b] = (job, 64-k tile, 64-n tile, z) */
int fsv_hconv_prep_weight(const long long* jobs, const int* tmap, int nblocks, fsv_stream_t stream);
/* the same for ONE layout with the geometry in the arguments (no device table: legal inside a graph capture) */
int fsv_hconv_prep_weight_one(const float* src, void* dst, int Kpad32, int ldw, int nrows, int Kpad64, int nbatch,
                              fsv_stream_t stream);
/* dense element conversion, dir 0: fp32 -> half (round to nearest even), 1: half -> fp32, 2: fp32 image in [-1, 1] -> uint8
 * (y = n bytes): (x + 1) / 2 * 255 in fp32, clipped to [0, 255], truncated - a generated NHWC frame as a video encoder takes it;
 * 3: uint8 (x = n bytes) -> fp32 in [-1, 1], the dataset's ToTensor + Normalize(0.5, 0.5): v / 255, then (t - 0.5) / 0.5, each step
 * rounded to fp32 on its own - a decoded frame as the model takes it; dir 3 needs x 4-byte and y 16-byte aligned (the bytes
 * are read as 32-bit words, the result is stored as float4): FSV_ERR_BAD_ARG otherwise */
int fsv_cast_half(const void* x, void* y, long long n, int dir, fsv_stream_t stream);

/* ---- narrow-operand GEMMs (csrc/conv_np.hip): the reference's `--amp` arithmetic (options/base_options.py:127,
 * models/models.py:22-26 `amp.initialize(..., opt_level=opt.amp, num_losses=2)`; BASELINE.json configs[4]).  Same
 * contracts and arguments as fsv_conv_gather_fwd / fsv_conv_wgrad plus `mode`: 1 = operands rounded to IEEE half while a
 * tile is staged through LDS, 2 = operands split into two bf16 terms (three MFMAs per tile pair); fp32 accumulation,
 * fp32 tensors in HBM.  Only float4-gather layers (Cin % 4 == 0) are implemented: FSV_ERR_UNSUPPORTED otherwise, callers
 * keep those on the fp32 entry points.  force_tile of the weight gradient: 1 / 2 / 3 / 4 = 64x64 / 128x64 / 64x128 /
 * 128x128. */
int fsv_conv_gather_fwd_np(const float* in, const float* wt, const float* bias, const float* res, float* out,
                           int N, int H, int W, int Cin, int OH, int OW, int Cout,
                           int ntaps, const int* ty, const int* tx, int sy, int sx,
                           int outH, int outW, int osy, int osx, int ooy, int oox,
                           int ldw, long long w_bstride, long long b_bstride, int per_sample,
                           int act, float scale, int force_tile, int force_split, int accumulate, const float* wscale,
                           int mode, fsv_stream_t stream);
int fsv_conv_wgrad_np(const float* in, const float* dout, float* dwt,
                      int N, int H, int W, int Cin, int OH, int OW, int Cout,
                      int ntaps, const int* ty, const int* tx, int sy, int sx,
                      int ldw, int Kpad, long long w_bstride, int per_sample, int force_split, int prezeroed,
                      int force_tile, int mode, fsv_stream_t stream);

/* ---- dynamic loss scale of the fp16 mode (csrc/amp.hip) - models/loss_collector.py:221-224 `amp.scale_loss(loss,
 * optimizer, loss_id)`; apex rule: skip the step and halve on inf / nan, double after `window` good steps.
 * scaler = {scale, good_steps, found_inf, window, max_scale, min_scale} on the device (no host read: graph-capturable).
 * fsv_amp_adam is fsv_adam_step with grad * gscale / scale, and does nothing when found_inf is set. */
int fsv_amp_check(const float* grad, long long n, float* scaler, fsv_stream_t stream);
int fsv_amp_adam(float* param, const float* grad, float* m, float* v, float* state, float* scaler, long long n,
                 float beta1, float beta2, float eps, float gscale, fsv_stream_t stream);
int fsv_amp_update(float* scaler, fsv_stream_t stream);

/* OIHW <-> K-major re-arrangement with an optional device scalar multiplier (the spectral-norm 1/sigma).
 * mode 0: wt[j*Cin+ci][co] = s*w[co][ci][kh_j][kw_j]; mode 1 (data gradient): wt[j*Cout+co][ci] = ...;
 * mode 2: inverse of mode 0 (gradients back to OIHW); mode 3: mode 2 accumulating into w.
 * col_scale (nullable, mode 0 without scale_ptr only; FSV_ERR_BAD_ARG otherwise): Cout per-output-channel factors shared by
 * every sample of a batch, wt[j*Cin+ci][co] = w[co][ci][kh_j][kw_j] * col_scale[co] - a frozen eval-mode BatchNorm (and
 * 1/sigma) folded into the layout. */
int fsv_prep_weight(const float* w, float* wt, const float* scale_ptr, int mode, int nbatch,
                    int Cout, int Cin, int KH, int KW, int ntaps, const int* kh, const int* kw,
                    int Kpad, int ldw, long long w_bstride, long long wt_bstride, const float* col_scale, fsv_stream_t stream);

/* every parameter weight of an optimiser re-arranged in one launch (un-scaled; used once per optimiser step).  dims[l] =
 * {Cout, Cin_pad, Cin_real, KH, KW, ntaps, Kpad, ldw, mode}; the layouts of one weight are consecutive in the tables and share
 * its source tile: tmap = (first layout of the weight, number of its layouts, 32-co tile, ci tile) quadruples (ci tile = 32
 * channels for KH*KW <= 8, else 16).  The layouts are pre-zeroed by their owner; a mode-1 layout gets its valid region written and
 * nothing else, a mode-0 layout is written in whole 32-column tiles, so its padding columns [Cout, ldw) receive zeros again
 * (rows beyond ntaps * Cin_pad are never written; the rows of padded input channels are written as zeros in both modes).
 * mode | 4: the two nibbles of a tap code are MASKS over kh / kw and the written weight is the sum of the selected source taps
 * (the summed-tap layouts of conv3x3(nearest_x2(x)): sub-pixel forward classes, one-launch data gradient) */
int fsv_prep_weight_grouped(const long long* src, const long long* dst, const int* dims, const unsigned long long* taps,
                            const int* tmap, int nblocks, fsv_stream_t stream);
/* grouped fixed-order sums: dst[j] = src[4 j] + src[4 j + 1] + ... (nsrc[j] in 1..4 terms, left to right) over count[j] floats,
 * njobs <= 8, one launch; pointers 16-byte aligned.  Adds the data gradients of the weight-generator MLPs that share their input
 * rows (generator.py:245-273: four FC stacks per level on the same encoded reference) without atomics. */
int fsv_sum_terms(float* const* dst, const float* const* src, const int* nsrc, const long long* count, int njobs,
                  fsv_stream_t stream);
/* Deferred weight-gradient finalisation (csrc/wgrad_finalize.hip): njobs K-major weight gradients -> OIHW, added into
 * their parameter-gradient slices, with torch.nn.utils.spectral_norm's backward correction where sig != 0.
 * ptrs[job][6] = {dwt, K-major W, sink, u, v, sig}; dims[job][8] = {Cout, CinP, CinR, KH, KW, ntaps, ldw, flags};
 * taps[job][2] packed (kh | kw << 4); dots: double[njobs] scratch; tmap_dot (job, 4096-element chunk) pairs over the
 * spectral jobs; tmap_apply (job, 32-co tile, ci tile) triples (ci tile = 32 channels for <= 8 taps, else 16). */
int fsv_wgrad_finalize(const long long* ptrs, const int* dims, const unsigned long long* taps, double* dots, int njobs,
                       const int* tmap_dot, int nblk_dot, const int* tmap_apply, int nblk_apply, fsv_stream_t stream);
/* dst += src over njobs small contiguous fp32 tensors in one launch: table[job][3] = {src, dst, n}, tmap (job, 4096-element
 * chunk) pairs.  Folds the separately accumulated gradients of small parameters into the flat gradient buffer. */
int fsv_gather_add(const long long* table, int njobs, const int* tmap, int nblk, fsv_stream_t stream);
/* n 64-bit words from host memory into a device array, carried in kernel arguments (legal inside a graph capture,
 * no staging buffer); used for the per-pass pointer table of fsv_wgrad_finalize */
int fsv_upload_i64(long long* dst, const long long* host_src, int n, fsv_stream_t stream);
/* tile / split-K plan the launcher will use (exported so host-side profilers label launches consistently) */
int fsv_conv_plan(int Mz, int Cout, int nchunks, int nsamp, int force_tile, int force_split, int* tile_out,
                  int* nsplit_out);
/* row `id` of the gather-GEMM's tile-variant table (csrc/conv_igemm.hip FSV_CONV_TILES): out = {BM pixels, BN channels, id of the
 * plan's tile of that shape, prefetch distance, in-place A fragments, mode (2 = loads straight into LDS)}; FSV_ERR_BAD_ARG when
 * no such row exists - for labels and tests, like fsv_conv_plan */
int fsv_conv_tile_info(int id, int* out /* bm, bn, shape, pf, af, mode */);
/* 1 when a Cout <= 4 layer of Mz pixels and K = taps * Cin takes the vector-ALU kernels (fsv_conv_thin_*), else 0 - NOT a status;
 * for profiler labels, like fsv_conv_plan */
int fsv_conv_thin_rule(int Mz, int K);

/* One-launch operand preparation of a SPADE (gamma, beta) 1x1 weight pair (normalization.py:37-52): wg / wb [B][C][Ch]
 * (sample strides swg / swb, 0 = shared), bg / bb [B][C] -> wcat_t [B][ceil32(Ch)][2C] (forward operand of map -> [gamma|beta]),
 * wcat_d [B][ceil32(2C)][ceil32(Ch)] (data-gradient operand, may be NULL), bcat [B][2C].  C % 16 == 0. */
int fsv_spade_prep(const float* wg, const float* wb, const float* bg, const float* bb, long long swg, long long swb,
                   long long sbg, long long sbb, float* wcat_t, float* wcat_d, float* bcat, int B, int C, int Ch,
                   fsv_stream_t stream);
/* ---- SPADE (csrc/spade.hip) - replaces SPADE.forward normalization.py:37-52 + actvn architecture.py:95-97 --------
 * h = act( (...((x - mean) * rstd) * (1 + g_0) + b_0 ...) * (1 + g_{n-1}) + b_{n-1} ),  g_k = map_k @ Wg_k + bg_k.
 * One launch; gamma/beta are MFMA accumulators and never reach HBM.
 * up != 0: x is the half-resolution tensor [N][H/2][W/2][C] (H = HW / W) and is read through the nearest x2 up-sampling
 * index - F.interpolate(scale_factor=2) of generator.py:124 folded into its consumer; W is only used then. */
int fsv_spade_mod_fwd(const float* x, const float* mean, const float* rstd, float* h,
                      int nmaps, const float* const* maps, const float* const* wg, const float* const* wb,
                      const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                      const long long* b_bstride, int N, int HW, int C, int ldw, long long stat_bstride, int act,
                      int W, int up, fsv_stream_t stream);
/* `--amp` forms of fsv_spade_mod_fwd.  flags bit 0: h written as IEEE half (h is only read by half-precision convolutions);
 * bit 2: gamma / beta GEMMs on the f16 matrix instructions - maps IEEE half ([N][HW][Ch], Ch % 8 == 0), wg / wb = gamma rows / beta
 * rows of the N-major half operand of fsv_spade_prep_h (row length ceil32(Ch) halves; ldw unused), w_bstride in halves */
int fsv_spade_mod_fwd_h(const float* x, const float* mean, const float* rstd, void* h,
                        int nmaps, const void* const* maps, const void* const* wg, const void* const* wb,
                        const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                        const long long* b_bstride, int N, int HW, int C, int ldw, long long stat_bstride, int act,
                        int W, int up, int flags, fsv_stream_t stream);
/* wcat_h [B][2C][Kh = ceil32(Ch)] halves, K contiguous, zero padded: rows [0, C) gamma weights, [C, 2C) beta weights */
int fsv_spade_prep_h(const float* wg, const float* wb, long long swg, long long swb, void* wcat_h, int B, int C, int Ch,
                     fsv_stream_t stream);
/* ---- bn_s modulation fused with conv_s (csrc/spade_conv.hip) - replaces `x_s = self.conv_s(self.bn_s(x, ...))`,
 * architecture.py:103-108 (SPADE.forward normalization.py:37-52 followed by the bias-free spectral-norm 1x1 convolution) ------
 * ONE launch: the gamma / beta GEMMs run with swapped operands (accumulators = [channel][pixel]), the modulated values are the A
 * fragments of a second chain of matrix instructions against the conv_s weight rows kept in registers; the modulated tensor
 * is written only when hs != NULL (a training forward: conv_s' weight gradient reads it).  Operands of the modulation as
 * fsv_spade_mod_fwd (no activation: bn_s has none); ws = K-major forward operand of the 1x1 weight ([>= C rows][ldws],
 * fsv_prep_weight mode 0), wscale = optional device scalar (1 / sigma) on the result; xs [N][HW][Cout].
 * fsv_spade_conv_s_supported: 1 when a kernel exists for (C, Cout, nmaps) - C in {64, 128}, Cout in {32, 64}, 1..3 maps;
 * fsv_spade_conv_s_fwd returns FSV_ERR_UNSUPPORTED otherwise (the caller runs the two launches). */
int fsv_spade_conv_s_supported(int C, int Cout, int nmaps);
int fsv_spade_conv_s_fwd(const float* x, const float* mean, const float* rstd, float* hs, float* xs,
                         int nmaps, const float* const* maps, const float* const* wg, const float* const* wb,
                         const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                         const long long* b_bstride, int N, int HW, int C, int ldw, long long stat_bstride, int W, int up,
                         const float* ws, int ldws, int Cout, const float* wscale, fsv_stream_t stream);
/* `--amp` form of fsv_spade_conv_s_fwd: f16 GEMMs - maps / wg / wb as fsv_spade_mod_fwd_h with flags bit 2 (IEEE half maps, N-major
 * half gamma | beta operand of fsv_spade_prep_h, Ch % 8 == 0), ws_h = N-major half operand of conv_s ([>= Cout rows][ldws halves],
 * K contiguous: fsv_hconv_prep_weight); the modulated value is rounded to half once (as the two-launch form does at its store),
 * hs_h (optional) receives it as half, xs is fp32 */
int fsv_spade_conv_s_fwd_h(const float* x, const float* mean, const float* rstd, void* hs_h, float* xs,
                           int nmaps, const void* const* maps, const void* const* wg, const void* const* wb,
                           const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                           const long long* b_bstride, int N, int HW, int C, long long stat_bstride, int W, int up,
                           const void* ws_h, int ldws, int Cout, const float* wscale, fsv_stream_t stream);
/* ---- SPADE modulation + activation fused with the 3x3 convolution that consumes it (csrc/spade_conv3.hip) - replaces
 * `dx = self.conv_0(actvn(self.bn_0(x, ...)))` / `self.conv_1(actvn(self.bn_1(dx, ...)))`, architecture.py:96-99 (SPADE.forward
 * normalization.py:37-52, leaky_relu(0.2) architecture.py:111-112, spectral-norm 3x3 convolution with padding 1) ------------
 * ONE launch: a workgroup computes the modulated values of its 8 x 16 output tile's one-pixel halo once into LDS (gamma / beta
 * GEMMs with swapped operands, operands straight from global memory) and runs the convolution from that patch; the modulated
 * tensor is written only when hs != NULL.  Operands of the modulation as fsv_spade_mod_fwd with the image as (H, W); wc = K-major
 * forward operand of the 3x3 weight ([9 C rows (tap, ci)][ldwc], fsv_prep_weight mode 0); out = acc * wscale + bias (+ res),
 * [N][H W][Cout]; stats (optional): fp64 partials [stats_groups][stats_slots][Cout][2] of the output's per-channel sums for the
 * normalisation that follows (as fsv_conv_gather_fwd_stats): stats_groups = 1 for a BatchNorm, = N (one group per sample) for an
 * InstanceNorm, anything else FSV_ERR_BAD_ARG.  mean / rstd are [C], or [N][C] with stat_bstride = C.  fsv_spade_conv3_supported: 1 when a kernel exists - C == 64, Cout in {32, 64}, 1..3 maps;
 * FSV_ERR_UNSUPPORTED otherwise.  Round 6: built and measured against the two-launch form (profiles/r06_notes.md section 8). */
int fsv_spade_conv3_supported(int C, int Cout, int nmaps);
int fsv_spade_conv3_fwd(const float* x, const float* mean, const float* rstd, float* hs, float* out,
                        int nmaps, const float* const* maps, const float* const* wg, const float* const* wb,
                        const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                        const long long* b_bstride, int N, int H, int W, int C, int ldw, long long stat_bstride, int up, int act,
                        const float* wc, int ldwc, int Cout, const float* bias, const float* res, const float* wscale,
                        double* stats, int stats_groups, int stats_slots, int stats_prezeroed, fsv_stream_t stream);
/* backward twin of fsv_spade_mod_fwd: the same operands plus the upstream gradient dh; gamma / beta are recomputed in
 * registers, outputs are dgb[k] = d(gamma | beta) of every map ([P][2C], gamma in columns [0, C)) and dxhat [P][C] (per
 * full-resolution pixel also when up != 0).  act: FSV_ACT_NONE or FSV_ACT_LRELU. */
int fsv_spade_mod_bwd(const float* x, const float* mean, const float* rstd, const float* dh,
                      int nmaps, const float* const* maps, const float* const* wg, const float* const* wb,
                      const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                      const long long* b_bstride, float* const* dgb, float* dxhat, int N, int HW, int C, int ldw,
                      long long stat_bstride, int act, int W, int up, fsv_stream_t stream);
/* general form of fsv_spade_mod_bwd.  flags bit 0: dh is IEEE half; bit 1: the d(gamma|beta) tensors are written as half; bit 2: f16
 * GEMMs (operands as fsv_spade_mod_fwd_h).  dbsum (optional): the bias gradients from this launch - per-channel sums of
 * d(gamma|beta) as doubles at dbsum + z * db_zstride[k] + k * 2C (zeroed by the call; db_zstride[k] = 0: summed over the batch);
 * db_slots > 1 (a power of two): pixel tile t adds into the copy at + (t % db_slots) * db_slot_stride, the caller sums the copies */
int fsv_spade_mod_bwd_h(const float* x, const float* mean, const float* rstd, const void* dh,
                        int nmaps, const void* const* maps, const void* const* wg, const void* const* wb,
                        const float* const* bg, const float* const* bb, const int* ch, const long long* w_bstride,
                        const long long* b_bstride, void* const* dgb, float* dxhat, int N, int HW, int C, int ldw,
                        long long stat_bstride, int act, int W, int up, int flags, double* dbsum, const long long* db_zstride,
                        int db_slots, long long db_slot_stride, fsv_stream_t stream);
/* element-wise part of the backward (general path, C % 16 != 0): from materialised gamma|beta ([P][2C] per map) to d(gamma|beta) and d(xhat) (dxhat is
 * written per full-resolution pixel also when up != 0: summing it over the 2x2 children gives the gradient of the
 * half-resolution normalised tensor) */
int fsv_spade_bwd_elem(const float* x, const float* mean, const float* rstd, const float* dh, const float* h,
                       int nmaps, const float* const* gb, float* const* dgb, float* dxhat,
                       int N, int HW, int C, long long stat_bstride, int act, int W, int up, fsv_stream_t stream);
/* ---- SPADE with 3x3 gamma / beta convolutions (csrc/spade_k3.hip) - normalization.py:18-52 with --spade_ks 3 -----------------
 * h = act( (...((x - mean) * rstd) * (1 + g_0) + b_0 ...) * (1 + g_{n-1}) + b_{n-1} ),  [g_k | b_k] = conv3x3(map_k, pad 1) + bcat_k,
 * one launch for 0..3 maps.  x [N][H W][C] (up != 0: [N][H/2 W/2][C], read through the nearest x2 index; H, W even), maps[k]
 * [N][H W][ch_k] (ch_k % 4 == 0), wt[k] = K-major forward operand of the combined weight [2C][ch_k][3][3] (fsv_prep_weight mode 0:
 * rows tap * ch_k + ci, ldw >= 2C columns, gamma in [0, C), beta in [C, 2C)) + z * w_bstride[k] (0: shared by the batch), bcat[k]
 * [2C] + z * b_bstride[k].  C % 4 == 0.  gb (optional, NULL or nmaps pointers): [N][H W][2C] gamma | beta of every map, the operand
 * of fsv_spade_bwd_elem. */
int fsv_spade_k3_fwd(const float* x, const float* mean, const float* rstd, float* h, int nmaps, const float* const* maps,
                     const float* const* wt, const float* const* bcat, const int* ch, const long long* w_bstride,
                     const long long* b_bstride, float* const* gb, int N, int H, int W, int C, int ldw, long long stat_bstride,
                     int act, int up, fsv_stream_t stream);

/* ---- measurement only (csrc/stamp.hip): device-side time stamps, graph-capturable brackets for bench.py's roofline object ----
 * fsv_stamp: *slot = the GPU's constant-rate wall clock when the stream reaches this point; fsv_stamp_rate_khz: its rate. */
int fsv_stamp(unsigned long long* slot, fsv_stream_t stream);
int fsv_stamp_rate_khz(void);

/* ---- normalisation (csrc/norm.hip) - BatchNorm (apex SyncBatchNorm) normalization.py:33,80; InstanceNorm :35,82 ----
 * tensors are [G][P][C]: BatchNorm G=1, P=N*H*W; InstanceNorm G=N, P=H*W.  workspace: fsv_norm_workspace_doubles(). */
int fsv_norm_workspace_doubles(int G, int P, int C);
int fsv_norm_stats(const float* x, double* workspace, float* mean, float* rstd, int G, int P, int C, float eps,
                   float* run_mean, float* run_var, float momentum, fsv_stream_t stream);
/* second stage alone: mean / rstd (+ running statistics) from partial sums part[g][slot][c][2] left by a producing kernel */
int fsv_norm_stats_finish(const double* part, float* mean, float* rstd, int G, int P, int C, int nslots, float eps,
                          float* run_mean, float* run_var, float momentum, int rep, fsv_stream_t stream);
/* statistics of a tensor that repeats every value of x `rep` times (nearest x2 up-sampling: rep = 4): mean / rstd are those
 * of x, the unbiased running-variance correction counts P * rep values */
int fsv_norm_stats_rep(const float* x, double* workspace, float* mean, float* rstd, int G, int P, int C, float eps,
                       float* run_mean, float* run_var, float momentum, int rep, fsv_stream_t stream);
/* y_half / dx_half (nullable): half side output, see fsv_act_bwd below */
int fsv_norm_apply(const float* x, const float* mean, const float* rstd, const float* w, const float* b, float* y,
                   int G, int P, int C, int act, void* y_half, fsv_stream_t stream);
int fsv_norm_bwd(const float* dy, const float* y, const float* x, const float* mean, const float* rstd, const float* w,
                 double* workspace, float* s1, float* s2, float* dx, float* dw, float* db, int G, int P, int C, int act,
                 int fixed_stats, void* dx_half, fsv_stream_t stream);   /* fixed_stats: eval mode, mean / rstd are constants */
int fsv_colsum(const float* x, double* workspace, float* out, int G, int P, int C, int accumulate, fsv_stream_t stream);
/* one-launch forms of the three reductions above: the workgroup that finishes last on a channel slab (a ticket per slab in
 * `counters`) sums that slab's partials and writes the final values, so the separate finalize launch disappears.  counters:
 * at least 64 ints, zero before the first use; every launch leaves them zero again (launches that may run concurrently need
 * different ranges).  counters == NULL, or a tensor above FSV_NORM_FUSE_MAX_MB (default 1 MB; one workgroup per slab reads all
 * partials, which only pays while the reduction is launch-bound): the two-launch path above. */
int fsv_norm_stats_fused(const float* x, double* workspace, float* mean, float* rstd, int G, int P, int C, float eps,
                         float* run_mean, float* run_var, float momentum, int rep, int* counters, fsv_stream_t stream);
/* fsv_norm_bwd_fused alone also runs WITHOUT y for act = LeakyReLU(0.2), LeakyReLU(0.1), ReLU: y == NULL and b = the bias the
 * forward applied (NULL exactly when w is NULL).  The slope then comes from the sign of the pre-activation
 * v = ((x - mean) * rstd) * w + b, recomputed per element by the expression fsv_norm_apply evaluates (y > 0 exactly when v > 0
 * for these three), so s1, s2, dw, db and dx carry the same bits as with y while both passes skip a tensor read.  With y given,
 * b is not read; y == NULL with tanh / sigmoid, or with only one of w and b, is FSV_ERR_BAD_ARG. */
int fsv_norm_bwd_fused(const float* dy, const float* y, const float* x, const float* mean, const float* rstd, const float* w,
                       const float* b, double* workspace, float* s1, float* s2, float* dx, float* dw, float* db, int G, int P,
                       int C, int act, int fixed_stats, int* counters, void* dx_half, fsv_stream_t stream);
int fsv_colsum_fused(const float* x, double* workspace, float* out, int G, int P, int C, int accumulate, int* counters,
                     fsv_stream_t stream);
/* cross-replica BatchNorm (opt-in; apex.parallel.SyncBatchNorm of the reference's multi-process path, normalization.py:15,33,80):
 * the device halves on either side of the host's all-reduce.  sums: doubles [2C] = {sum x, sum x^2} resp. {sum d, sum d*xhat};
 * count: values per channel over all ranks.  dw / db of an affine layer are the LOCAL sums (they travel with the gradients). */
int fsv_norm_sums(const float* x, double* workspace, double* sums, int P, int C, fsv_stream_t stream);
int fsv_norm_stats_from_sums(const double* sums, double count, float* mean, float* rstd, int C, float eps, float* run_mean,
                             float* run_var, float momentum, fsv_stream_t stream);
int fsv_norm_bwd_sums(const float* dy, const float* y, const float* x, const float* mean, const float* rstd,
                      double* workspace, double* sums, int P, int C, int act, fsv_stream_t stream);
int fsv_norm_bwd_apply(const float* dy, const float* y, const float* x, const float* mean, const float* rstd, const float* w,
                       const float* s1, const float* s2, float* dx, int P, int C, int count, int act, void* dx_half,
                       fsv_stream_t stream);
/* the bias gradients of a whole backward pass in two launches: table[job][8] = {src [P][C] rows, dst float[C] (added into),
 * offset of the job's partials in `part` (doubles), P, C, rows_per_blk, nchunks, V | shared << 8}; tmap1 (job, chunk, slab) triples,
 * tmap2 (job, 4-channel block) pairs; fsv_colsum_plan gives {V, TX, nslabs, rows_per_blk, nchunks} for one [P][C] */
int fsv_colsum_plan(int P, int C, int* out);
int fsv_colsum_grouped(const long long* table, int njobs, const int* tmap1, int nblk1, const int* tmap2, int nblk2,
                       double* part, fsv_stream_t stream);

/* ---- flow warp (csrc/warp.hip) - replaces resample/get_grid base_network.py:13-37 (F.grid_sample bilinear, border,
 * align_corners=True); tap indices are bit-identical to ATen's.  strides in elements: (batch, channel, y, x). ------ */
int fsv_warp_fwd(const float* img, const float* flow, const float* lin_x, const float* lin_y, float* out, int* taps,
                 int B, int C, int H, int W, const long long* img_strides, const long long* flow_strides,
                 const long long* out_strides, fsv_stream_t stream);
int fsv_warp_bwd(const float* img, const float* flow, const float* lin_x, const float* lin_y, const float* gout,
                 float* gimg, float* gflow, int B, int C, int H, int W, const long long* img_strides,
                 const long long* flow_strides, const long long* gout_strides, const long long* gimg_strides,
                 const long long* gflow_strides, fsv_stream_t stream);
/* warp + occlusion-mask compositing in one pass (generator.py:214-227, :441-443 on top of resample): writes the warped image
 * AND the composite.  mode 0 (--spade_combine): comp = dense NHWC [B][H*W][C+1] = (warp, mask), the input of the image
 * embedding; mode 1: comp = raw * mask + warp * (1 - mask) with the given strides.  mask: [B,1,H,W], mask_strides = (batch, y,
 * x); C <= 8; tap indices as fsv_warp_fwd.  Backward: g_warp / g_comp are the upstream gradients (either may be NULL), the
 * outputs gimg (scatter-add, zero-initialised, gimg_strides), gflow [B,2,H,W], gmask [B,H,W], graw [B,C,H,W] (dense) are
 * each optional. */
int fsv_warp_compose_fwd(const float* img, const float* flow, const float* lin_x, const float* lin_y, const float* mask,
                         const float* raw, float* warp, float* comp, int mode, int B, int C, int H, int W,
                         const long long* img_strides, const long long* flow_strides, const long long* mask_strides,
                         const long long* raw_strides, const long long* warp_strides, const long long* comp_strides,
                         fsv_stream_t stream);
int fsv_warp_compose_bwd(const float* img, const float* flow, const float* lin_x, const float* lin_y, const float* mask,
                         const float* raw, const float* g_warp, const float* g_comp, float* gimg, float* gflow, float* gmask,
                         float* graw, int mode, int B, int C, int H, int W, const long long* img_strides,
                         const long long* flow_strides, const long long* mask_strides, const long long* raw_strides,
                         const long long* g_warp_strides, const long long* g_comp_strides, const long long* gimg_strides,
                         fsv_stream_t stream);

/* ---- spectral norm (csrc/specnorm.hip) - torch.nn.utils.spectral_norm at architecture.py:60,81-84 etc. ----------- */
/* scratch: fsv_sn_scratch_floats(R, Cc) floats (t[Cc], s[R] and one partial row of W^T u per 64-row slab of W: the slabs are
 * summed in ascending order, no atomics - u, v and sigma are the same bits on every run) */
int fsv_sn_scratch_floats(int R, int Cc);
int fsv_sn_power_iter(const float* W, float* u, float* v, float* scratch, float* sig, int R, int Cc, float eps,
                      int training, fsv_stream_t stream);
/* every spectral-normalised layer of a network in four launches; W/u/v are arrays of device pointers (as 64-bit
 * integers), tmap_* map a flat block index to (layer, tile).  t_off[l]: the layer's t region in `scratch`,
 * cols * (1 + ceil(rows / 64)) floats (t, then the per-slab partials of W^T u); s_off[l]: rows floats */
int fsv_sn_power_iter_batched(const long long* W, const long long* u, const long long* v, const int* rows,
                              const int* cols, const int* t_off, const int* s_off, float* scratch,
                              long long scratch_floats, float* sig, float* snap, const int* u_off, const int* v_off,
                              int nlayers, const int* tmap_t, int nblk_t, const int* tmap_s, int nblk_s, float eps,
                              fsv_stream_t stream);
int fsv_sn_backward(const float* dWsn, const float* W, const float* u, const float* v, const float* sig, double* part,
                    float* dW, int R, int Cc, int accumulate, fsv_stream_t stream);

/* ---- element-wise helpers and the optimiser (csrc/elementwise.hip) ----------------------------------------------
 * nearest x2 up-sampling (generator.py:124, nn.Upsample), activations, Adam (base_model.py:39-48). */
int fsv_upsample2x_fwd(const float* x, float* y, int N, int H, int W, int C, fsv_stream_t stream);
int fsv_upsample2x_bwd(const float* dy, float* dx, int N, int H, int W, int C, fsv_stream_t stream);
int fsv_act_fwd(const float* x, float* y, long long total, int act, fsv_stream_t stream);
/* Half side output of the element-wise producers (`--amp`): fsv_norm_apply (y_half), fsv_norm_bwd / fsv_norm_bwd_fused /
 * fsv_norm_bwd_apply and fsv_act_bwd (dx_half) take a nullable pointer - when set, the call also stores its result as IEEE half
 * there, same element order, one rounding of the fp32 value: the consumer convolution reads that copy instead of converting the
 * fp32 tensor.  Contract: C % 4 == 0 and fewer than 2^31 elements (fsv_act_bwd: total % 4 == 0); FSV_ERR_UNSUPPORTED with nothing
 * launched otherwise. */
int fsv_act_bwd(const float* dy, const float* y, float* dx, long long total, int act, float scale, void* dx_half,
                fsv_stream_t stream);
/* channel concatenation into one NHWC tensor (one call per source) and its gradient slices; occlusion-mask
 * compositing out = a*m + b*(1-m) (generator.py:217,224,441-443,498,563) */
int fsv_cat_put(const float* src, float* out, long long N, int C, long long P, const long long* strides, int Ct, int coff,
                fsv_stream_t stream);
/* out [N][P][Ct] dense NHWC = the C channels of a (batch, channel, pixel)-strided source followed by Ct - C zero channels
 * (inputs whose channel count is not a multiple of 4 are padded once for the float4 gather of the convolutions) */
int fsv_pad_channels(const float* src, float* out, long long N, int C, long long P, const long long* strides, int Ct,
                     fsv_stream_t stream);
/* the same with `out` written as IEEE half ([N][P][Ct] halves; the `--amp` path: the padded tensor is a convolution input).
 * Pixel-contiguous source planes (strides[2] == 1) and Ct % 8 == 0 only: FSV_ERR_UNSUPPORTED otherwise */
int fsv_pad_channels_h(const float* src, void* out, long long N, int C, long long P, const long long* strides, int Ct,
                       fsv_stream_t stream);
int fsv_cat_get(const float* dout, float* dst, long long N, int C, long long P, int Ct, int coff, fsv_stream_t stream);
int fsv_blend_fwd(const float* a, const float* b, const float* m, float* out, int N, int C, long long P,
                  const long long* a_strides, const long long* b_strides, const long long* out_strides, fsv_stream_t stream);
int fsv_blend_bwd(const float* a, const float* b, const float* m, const float* g, float* da, float* db, float* dm, int N, int C,
                  long long P, const long long* a_strides, const long long* b_strides, const long long* g_strides,
                  fsv_stream_t stream);
/* 2x2 stride-2 max pooling of the VGG19 feature stack (models/networks/vgg.py:45-59), NHWC */
int fsv_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C, fsv_stream_t stream);
int fsv_maxpool2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, fsv_stream_t stream);
/* nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False) between the discriminators of a multi-scale pyramid
 * (reference models/networks/discriminator.py:28,56), NHWC; output (H - 1) / 2 + 1 by (W - 1) / 2 + 1 */
int fsv_avgpool3s2_fwd(const float* x, float* y, int N, int H, int W, int C, fsv_stream_t stream);
int fsv_avgpool3s2_bwd(const float* dy, float* dx, int N, int H, int W, int C, fsv_stream_t stream);
/* nn.AdaptiveAvgPool2d((OH, OW)) on NHWC tensors, any OH / OW - shrinking or growing (discriminator.py:146,153: AdaptiveDiscriminator.gen_conv_weights);
 * windows [floor(o in / out), ceil((o + 1) in / out)) as in ATen; the backward pass is a gather (no atomics) */
int fsv_adaptive_avgpool_fwd(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, fsv_stream_t stream);
int fsv_adaptive_avgpool_bwd(const float* dy, float* dx, int N, int H, int W, int C, int OH, int OW, fsv_stream_t stream);
/* csrc/pool_rows.hip - the same pooling straight into the operand of the weight generators under --use_label_ref concat
 * (generator.py:248,278 + reshape_embed_input): NHWC fp32 map x [N][H][W][C] -> channel-major rows [N * C][OH * OW], and the rows'
 * gradient back to the map's (a gather, no atomics, fixed summation order).  C a multiple of 4 (16-byte accesses), else
 * FSV_ERR_BAD_ARG; the backward pass returns FSV_ERR_UNSUPPORTED where 128 map pixels span more than 40 pooled columns (never for
 * OW <= 40) */
int fsv_pool_rows_fwd(const float* x, float* rows, int N, int H, int W, int C, int OH, int OW, fsv_stream_t stream);
int fsv_pool_rows_bwd(const float* drows, float* dx, int N, int H, int W, int C, int OH, int OW, fsv_stream_t stream);
/* csrc/roll_flip.hip - the adaptation target of test-time finetuning (vid2vid_model.py:207-237, util/util.py:157-168) for up to two
 * tensors (label and image) in one launch:
 *     dst[b][c][y][x] = src[b][idx][c][(y - ny) mod H][(x' - nx) mod W],   x' = flip ? W - 1 - x : x
 * src_t dense fp32 [B][N][C_t][H][W], dst_t dense NCHW fp32 [B][C_t][H][W]; src1 / dst1 are not read when C1 = 0.  params is a DEVICE
 * int32[4] = {idx, ny, nx, flip} read by the kernel (a captured launch follows the buffer): idx is clamped into [0, N), ny / nx are
 * reduced modulo H / W (negative values included), flip is read as != 0 - no value of the four integers takes an index outside the
 * tensors.  Pure data movement, bit-exact.  Null src0 / dst0 / params (src1 / dst1 with C1 > 0), non-positive B / N / H / W / C0,
 * negative C1: FSV_ERR_BAD_ARG; more than 2^31 - 1 workgroups (B (C0 + C1) H ceil(W / 256)): FSV_ERR_UNSUPPORTED; nothing is launched
 * in either case. */
int fsv_roll_flip(const float* src0, float* dst0, int C0, const float* src1, float* dst1, int C1, int B, int N, int H, int W,
                  const int* params, fsv_stream_t stream);
/* softmax over the contiguous channel dimension of [rows][C] (nn.Softmax(dim=1) at generator.py:384).  gsum != NULL: the launch
 * also writes gsum[rows][groups], gsum[row][g] = the sum of y[row][j] over the g-th contiguous slice of C / groups channels (the
 * attention mass per reference, generator.py:310,366), accumulated in fp32 in a fixed order, no atomics; y has the same bits with
 * and without gsum.  groups < 1 or C % groups != 0 with a non-null gsum: FSV_ERR_BAD_ARG (groups is not read when gsum is NULL).
 * Per-launch bounds (forward and backward): rows <= 4 * (2^24 - 1) = 67108860 (four rows per 256-thread workgroup, fewer than 2^32
 * work-items per launch): FSV_ERR_UNSUPPORTED beyond, nothing launched.  Rows are addressed as 64-bit element offsets, rows * C
 * is not bounded by 2^31.  The forward pass may run in place (y == x). */
int fsv_softmax_rows_fwd(const float* x, float* y, long long rows, int C, int groups, float* gsum, fsv_stream_t stream);
int fsv_softmax_rows_bwd(const float* dy, const float* y, float* dx, long long rows, int C, fsv_stream_t stream);

/* ---- streaming few-shot attention (csrc/attention.hip) - generator.py:298-316 without the [N P, P] attention tensor --------------
 * Forward only, exact fp32 on v_mfma_f32_32x32x2_f32, no atomics: the same bits on every run, whatever FSV_DETERMINISTIC says.
 *   q    [B][P][C]      query features (the NHWC memory of the atn_query encoder output, P = h w)
 *   k    [B][N P][C]    key features (the NHWC memory of the atn_key encoder output over the B N references)
 *   v0   [B][N P][C0]   reference features entering the attention;  v1 [B][N P][C1]: a second map, nullable (o1 / C1 are not read then)
 *   o0   [B][P][C0], o1 [B][P][C1]: o[b][p] = sum_key a[key] v[b][key], a = softmax over all N P keys of e[key] = <k[b][key], q[b][p]>
 *   mass [B][P][N], nullable: per query position the sum of a over each reference's P keys (the layout of fsv_softmax_rows_fwd's gsum)
 * A workgroup owns 128 query positions of one sample and walks tiles of 32 keys in ascending order with an online softmax (running
 * maximum, denominator and both output accumulators on chip); P is arbitrary (masked tails on both sides), every base is a 64-bit
 * element offset.  nsplit >= 1: the key tiles are divided over nsplit workgroups per query tile whose partial results a finishing
 * launch combines in ascending order; nsplit = 0: the library's choice, a function of the shape alone (fsv_attention_fused_plan).
 * One launch when nsplit is 1 and mass is NULL, one more (the finishing pass) otherwise.  A walk over the keys carries up to eight
 * 32-channel output tiles, both maps together (C0 = C1 = 128: one walk), and four where C > 128; more tiles than that
 * (ceil(C0 / 32) + ceil(C1 / 32)) take further walks, one launch each, with the same bits in the shared statistics.
 * Workspace (the caller's, 16-byte aligned; ws may be NULL when none is needed), in floats and in this order - the partial sums
 * first, they are read as 16-byte vectors:
 *     (nsplit > 1 ? nsplit B P (C0 + C1) : 0) + (nsplit > 1 || mass ? 2 nsplit B P : 0) + (mass ? 2 nsplit B P N : 0)
 * Contract: C, C0, C1 multiples of 4 and at most 256, N P < 2^31 - 64, B <= 65535: FSV_ERR_UNSUPPORTED beyond, nothing launched.
 * Null q / k / v0 / o0 (o1 with a v1), non-positive B / N / P / C / C0 (C1 with a v1): FSV_ERR_BAD_ARG, before anything else; then
 * the contract above; then nsplit above 8 or above the ceil(N P / 32) key tiles, or a workspace smaller than the formula:
 * FSV_ERR_BAD_ARG.  Nothing is launched in any of these cases.
 * fsv_attention_fused_plan: out[0] = the nsplit the launch would use (the given one when nsplit > 0), out[1] = the workspace in
 * floats; C1 = 0 for a single map; the same status codes. */
int fsv_attention_fused_fwd(const float* q, const float* k, const float* v0, const float* v1, float* o0, float* o1, float* mass,
                            int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws, long long ws_floats,
                            fsv_stream_t stream);
int fsv_attention_fused_plan(int B, int N, int P, int C, int C0, int C1, int want_mass, int nsplit, long long* out);
/* ---- the differentiable form (csrc/attention.hip, csrc/attention_bwd.hip): exact fp32 on v_mfma_f32_32x32x2_f32, no atomics, the
 * same bits on every run whatever FSV_DETERMINISTIC says; the same NHWC-in-place operands, 64-bit bases, masked tails for any P.
 * fsv_attention_fused_fwd_lse: fsv_attention_fused_fwd (one shared implementation: the same arguments, bounds, status codes,
 * workspace formula - fsv_attention_fused_plan - and launch counts; o0 / o1 / mass have the same bits) that also writes
 *   lse  [B][P], nullable: per query the running maximum plus the log of the softmax denominator
 * from the kernel's own epilogue when one workgroup walks all keys and no mass is wanted, from the finishing launch otherwise.
 * fsv_attention_fused_bwd: with p = exp(<k[key], q[query]> - lse[query]) recomputed tile by tile (never positive exponents) and the
 * cotangents do0 [B][P][C0], do1 [B][P][C1] of o0 / o1 (o1 / do1 are read only with a v1):
 *   delta[query] = sum_c do0 o0 + sum_c do1 o1,   dp = <do0[query], v0[key]> + <do1[query], v1[key]>,   ds = p (dp - delta[query])
 *   dq [B][P][C] = sum_key ds k[key]      dk [B][N P][C] = sum_query ds q[query]      dv_i [B][N P][Ci] = sum_query p do_i[query]
 * Each of dq / dk / dv0 / dv1 is nullable (a gradient the caller does not need; what is produced has the same bits whichever others
 * are asked for); at least one must be given, dv1 only with a v1.  Launches: delta (one wave per query, when dq or dk is wanted);
 * dq by a query-owning kernel (128 queries per workgroup, key tiles of 32 through LDS, the keys in nsplit ranges whose partial
 * sums one more launch adds in ascending order - nsplit as in the forward, 0: the library's choice); dv0 / dv1 and dk by two
 * key-owning launches (128 keys per workgroup, query tiles of 32 through LDS, every query in ascending order, no split).
 * Workspace (the caller's, 16-byte aligned), in floats: 4 ceil(B P / 4) + (nsplit > 1 ? nsplit B P C : 0) - a function of the shape
 * alone, whichever outputs are asked for (fsv_attention_fused_bwd_plan: out[0] = nsplit, out[1] = floats; C1 = 0: a single map).
 * Contract: C, C0, C1 multiples of 4 and at most 128 (the production shape), N P < 2^31 - 64, B <= 65535: FSV_ERR_UNSUPPORTED beyond,
 * nothing launched.  Null q / k / v0 / o0 / do0 / lse (o1 / do1 with a v1), a dv1 without a v1, all four outputs null, non-positive
 * B / N / P / C / C0 (C1 with a v1): FSV_ERR_BAD_ARG, before anything else; then the contract; then nsplit above 8 or above the
 * ceil(N P / 32) key tiles, a null or too small workspace: FSV_ERR_BAD_ARG. */
int fsv_attention_fused_fwd_lse(const float* q, const float* k, const float* v0, const float* v1, float* o0, float* o1, float* mass,
                                float* lse, int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws, long long ws_floats,
                                fsv_stream_t stream);
int fsv_attention_fused_bwd(const float* q, const float* k, const float* v0, const float* v1, const float* o0, const float* o1,
                            const float* do0, const float* do1, const float* lse, float* dq, float* dk, float* dv0, float* dv1,
                            int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws, long long ws_floats,
                            fsv_stream_t stream);
int fsv_attention_fused_bwd_plan(int B, int N, int P, int C, int C0, int C1, int nsplit, long long* out);
/* ---- the inference form on the f16 matrix cores (csrc/attention_h.hip): v_mfma_f32_32x32x16_f16, forward only, opt-in, no atomics,
 * the same bits on every run whatever FSV_DETERMINISTIC says.  With h(x) = round-to-nearest-even to IEEE half:
 *   split     for q and k: xh = h(x), xl = h((x - xh) * 2^11) (the remainder is exact in fp32; the scale keeps xl in half's normal
 *             range whenever xh is)
 *   energy    e = S_hh + 2^-11 * (S_hl + S_lh), S_hh = sum_c kh qh, S_hl + S_lh = sum_c (kh ql + kl qh): fp32 MFMA accumulations of
 *             exact products, the cross terms in an accumulator tile of their own; the kl ql term is dropped (about 22 bits)
 *   softmax   online, fp32 throughout: running maximum m, p = expf(e - m), l = sum p; the denominator and the masses from the
 *             unrounded p
 *   values    o = (sum_key h(p) h(v)) / l, accumulated in fp32 by the MFMA
 *   order     keys ascending, key ranges combined by fsv_attention_fused_fwd's finishing launch in ascending order
 *   range     operands must be finite and below 65504 in magnitude: a larger value becomes inf in h() and is the caller's error
 * fsv_attention_half_prep, once per reference set (one launch): k fp32 [B][N P][C] -> the half planes kh, kl [B][NPs][C];
 * v_i fp32 [B][N P][Ci] -> half v_it [B][Ci][NPs], key-contiguous (transposed through LDS tiles); NPs = N P rounded up to 32, the
 * tail zero-filled; v1 nullable (v1t / C1 are not read then).
 * fsv_attention_fused_fwd_h: q fp32 [B][P][C] as the query encoder left it (split in registers, once per workgroup), the prepared
 * operands, o0 / o1 / mass fp32 laid out as fsv_attention_fused_fwd writes them; its nsplit rules, workspace formula, finishing
 * launch, order of the checks and status codes (one launch when nsplit is 1 and mass is NULL, one more otherwise).
 * fsv_attention_fused_h_plan: out[0] = nsplit, out[1] = the workspace in floats, out[2] = NPs; C1 = 0 for a single map.
 * Contract: C, C0, C1 multiples of 8 and at most 128 (one instantiation: the production 128 / 128 / 128), N P < 2^31 - 64,
 * B <= 65535: FSV_ERR_UNSUPPORTED beyond, nothing launched.  Null pointers (v1 / v1t / o1 / mass nullable as above), non-positive
 * sizes: FSV_ERR_BAD_ARG, before anything else; then the contract; then nsplit above 8 or above the ceil(N P / 32) key tiles, or a
 * workspace smaller than the formula: FSV_ERR_BAD_ARG. */
int fsv_attention_half_prep(const float* k, const float* v0, const float* v1, void* kh, void* kl, void* v0t, void* v1t,
                            int B, int N, int P, int C, int C0, int C1, fsv_stream_t stream);
int fsv_attention_fused_fwd_h(const float* q, const void* kh, const void* kl, const void* v0t, const void* v1t, float* o0, float* o1,
                              float* mass, int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws, long long ws_floats,
                              fsv_stream_t stream);
int fsv_attention_fused_h_plan(int B, int N, int P, int C, int C0, int C1, int want_mass, int nsplit, long long* out);
/* state = {t, 1-beta1^t, 1-beta2^t, lr} on the device; gscale pre-multiplies the gradient (1/world_size) */
int fsv_adam_step(float* param, const float* grad, float* m, float* v, float* state, long long n, float beta1,
                  float beta2, float eps, float gscale, fsv_stream_t stream);
/* the same step issued in pieces (ranges of the flat buffers): tick != 0 advances the step count / bias corrections in `state`
 * (exactly one piece of a step), the other pieces - ordered behind it by the caller - only read them */
int fsv_adam_step_range(float* param, const float* grad, float* m, float* v, float* state, long long n, float beta1,
                        float beta2, float eps, float gscale, int tick, fsv_stream_t stream);

/* ---- losses, D-input packing, mask pooling (csrc/losses.hip) - models/networks/loss.py:17-104,130-138;
 * models/loss_collector.py:47-58,105-110,180; models/input_process.py:59 -------------------------------------------- */
int fsv_l1_fwd(const float* a, const float* b, float bconst, const float* m, int N, int C, long long P,
               const long long* a_strides, const long long* b_strides, double* part, float* loss, fsv_stream_t stream);
int fsv_l1_bwd(const float* a, const float* b, float bconst, const float* m, int N, int C, long long P,
               const long long* a_strides, const long long* b_strides, const float* gloss, float* da, float* db, float* dm,
               fsv_stream_t stream);
/* weighted sums of one-element loss tensors - `sum(lambda_i * term_i)` of loss_collector.py:60-67,85,161-162,204 and the sum of the
 * means of :218-219 - as one launch each way: out[0] = sum_i weights[i] * terms[i][0] (i ascending, fp32; terms: n <= 32 HOST-side
 * array of device pointers, weights: n host floats - both travel in the kernel argument); dterms[i] = weights[i] * g[0] */
int fsv_wsum_fwd(const float* const* terms, const float* weights, int n, float* out, fsv_stream_t stream);
int fsv_wsum_bwd(const float* weights, int n, const float* g, float* dterms, fsv_stream_t stream);
/* the GANLoss reduction (loss.py:17-104, called with for_discriminator=True in both steps) over the n values of one prediction
 * map, for all four objectives (mode: enum fsv_gan_mode; anything else: FSV_ERR_BAD_ARG, nothing launched).  sign = +1: the target
 * is real (t = 1), -1: fake (t = 0).  part: double[512] scratch.  gloss: the upstream scalar g.
 *   FSV_GAN_HINGE     loss.py:69-79   loss = -mean min(sign * x - 1, 0)                  dx_i = -g * sign * [sign * x_i < 1] / n
 *   FSV_GAN_LS        loss.py:57-61   loss = mean (x - t)^2                  (F.mse_loss) dx_i = 2 g (x_i - t) / n
 *   FSV_GAN_ORIGINAL  loss.py:50-53   loss = mean( max(x, 0) - x t + log1p(exp(-|x|)) )   dx_i = g (sigmoid(x_i) - t) / n
 *                                     (F.binary_cross_entropy_with_logits; no exp of a positive argument either way)
 *   FSV_GAN_W         loss.py:85-90   loss = -sign * mean x                               dx_i = -g * sign / n  (x is not read)
 * The per-element term is fp32, the sums are fp64 in a fixed order (no atomics): the same bits on every run. */
int fsv_hinge_fwd(const float* x, long long n, float sign, int mode, double* part, float* loss, fsv_stream_t stream);
int fsv_hinge_bwd(const float* x, long long n, float sign, int mode, const float* gloss, float* dx, fsv_stream_t stream);
int fsv_pack_d_input(const float* ref, const float* lab, const float* fake, const float* real, float* out,
                     int B, int Cr, int Cl, int Ci, long long P, const long long* ref_strides, const long long* lab_strides,
                     const long long* fake_strides, const long long* real_strides, fsv_stream_t stream);
/* the same for one image set only: out [B][P][Cr+Cl+Ci] = [ref | label | img] */
int fsv_pack_d_single(const float* ref, const float* lab, const float* img, float* out, int B, int Cr, int Cl, int Ci,
                      long long P, const long long* ref_strides, const long long* lab_strides, const long long* img_strides,
                      fsv_stream_t stream);
int fsv_unpack_d_grad(const float* dout, float* dfake, int B, int Ci, int Coff, int Ct, long long P, fsv_stream_t stream);
/* `--amp` forms: the packed discriminator input with Cto >= Cr + Cl + Ci channels (zero channels appended = the channel padding of
 * the first discriminator convolution) and, out_half != 0, as IEEE half; halves 2: [fake | real] on the batch axis (out [2B][P][Cto]),
 * 1: fake only (real may be NULL).  fsv_unpack_d_grad_h reads the half data gradient of that convolution. */
int fsv_pack_d_x(const float* ref, const float* lab, const float* fake, const float* real, void* out,
                 int B, int Cr, int Cl, int Ci, long long P, const long long* ref_strides, const long long* lab_strides,
                 const long long* fake_strides, const long long* real_strides, int halves, int Cto, int out_half,
                 fsv_stream_t stream);
int fsv_unpack_d_grad_h(const void* dout, float* dfake, int B, int Ci, int Coff, int Ct, long long P, fsv_stream_t stream);
/* DensePose part-group masks (models/input_process.py:64-94): x = pose channel [B, T, P] (strides sb, st, 1), N = B*T;
 * y[N][ngroups][P] = 1 where (x/2+0.5)*24 is within 0.1 of a member of group g0+g (9 groups; group 8 = face parts 23/24) */
int fsv_part_masks(const float* x, float* y, long long N, long long P, int T, long long sb, long long st, int g0, int ngroups,
                   fsv_stream_t stream);
int fsv_pool15(const float* x, float* y, int N, int H, int W, long long sn, long long sy, long long sx, int mode, float thresh,
               fsv_stream_t stream);

/* ---- face-region discriminator inputs (--add_face_D; models/face_refiner.py:32-39, 56-87), csrc/face.hip ----
 * boxes[n] = {ys, ye, xs, xe} of the face in label map n (pose [N][C][H][W], strides sn / sc, rows contiguous), computed
 * on the device; crop + F.interpolate(nearest, size S) of the last three channels of img for every sample in one launch,
 * and its gradient scattered into a zero-initialised dimg of img's layout. */
int fsv_face_boxes(const float* pose, long long sn, long long sc, int N, int C, int H, int W, int use_openpose,
                   int crop_smaller, int* boxes, fsv_stream_t stream);
int fsv_crop_resize_fwd(const float* img, long long sn, long long sc, long long sy, long long sx, int C, const int* boxes,
                        float* out, int N, int S, fsv_stream_t stream);
int fsv_crop_resize_bwd(const float* dout, const int* boxes, float* dimg, long long sn, long long sc, long long sy,
                        long long sx, int C, int N, int S, fsv_stream_t stream);
/* --refine_face (face_refiner.py:42-54 replace_face_region): out = img outside box n, clamp(bilinear resize of face[n]
 * [3][S][S] to the box size, -1, 1) inside (align_corners False); backward: dimg = dout outside the boxes, dface
 * (zero-initialised) receives the weighted dout where the clamp was inactive */
int fsv_paste_face_fwd(const float* img, const float* face, const int* boxes, float* out, int N, int H, int W, int S,
                       long long isn, long long isc, long long isy, long long isx, fsv_stream_t stream);
int fsv_paste_face_bwd(const float* dout, const float* out, const int* boxes, float* dimg, float* dface, int N, int H, int W,
                       int S, fsv_stream_t stream);

/* ---- the FlowNet2 teacher's three native operators, forward only (csrc/flownet_ops.hip) ----
 * correlation (correlation_cuda_kernel.cu:74-147; kernel_size 1): f1 / f2 NHWC [N][H][W][C] -> out NHWC
 *   [N][OH][OW][D*D], D = 2*(max_disp/stride2)+1, OH = ceil((H + 2*pad - 2*max_disp)/stride1), value = mean_c f1*f2.
 * resample2d (resample2d_kernel.cu:16-64): pixel-unit flow, clamped tap indices; strides = 4 x long long (n, c, y, x).
 * channelnorm (channelnorm_kernel.cu:18-60): out[n][p] = sqrt(sum_c x^2); x strides (sn, sc, sp). */
int fsv_correlation_fwd(const float* f1, const float* f2, float* out, int N, int H, int W, int C, int pad, int kernel_size,
                        int max_disp, int stride1, int stride2, fsv_stream_t stream);
int fsv_resample2d_fwd(const float* img, const float* flow, float* out, int N, int C, int H, int W,
                       const long long* img_strides, const long long* flow_strides, const long long* out_strides,
                       fsv_stream_t stream);
/* F.interpolate(mode='bilinear', align_corners=False) of the FlowNet2 teacher (flownet2_pytorch/models.py:119,137-142: x4 flow
 * up-sampling; models/flownet.py:66-77: resize to a multiple of 64 and back); element strides (n, c, y, x) */
int fsv_bilinear_resize_fwd(const float* in, float* out, int N, int C, int IH, int IW, int OH, int OW,
                            const long long* in_strides, const long long* out_strides, fsv_stream_t stream);
int fsv_channelnorm_fwd(const float* x, float* out, int N, int C, long long HW, long long sn, long long sc, long long sp,
                        fsv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FSV2V_H */
