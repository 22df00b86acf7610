// The adaptation target of test-time finetuning (vid2vid_model.py:207-237, util/util.py:157-168): a reference picked from the
// stack, rolled along H, rolled along W, then flipped along W - for the label and the image of the whole batch in ONE launch whose
// four draw parameters live in device memory, so that a captured launch gives a new target after the four integers were rewritten:
//
//     dst[b][c][y][x] = src[b][idx][c][(y - ny) mod H][(x' - nx) mod W],   x' = flip ? W - 1 - x : x
//
// which is `torch.flip(cat(cat(t[:, :, -ny:], t[:, :, :-ny], 2)[..., -nx:], ...[..., :-nx], 3), [3])` of t = src[:, idx]; ny = 0 and
// ny = H are both the identity, as with the slices.
//
// Memory: src is the dense [B][N][C][H][W] stack as ref_labels / ref_images arrive, dst is dense NCHW [B][C][H][W] - what the
// first consumers of forward_generator's tgt_label / tgt_image read as they are: fsv_part_masks and fsv_pool15 walk contiguous
// rows of single channel planes of the label (valid_labels, fg_mask_of), the image goes to fsv_pack_d_x / fsv_l1_fwd with explicit
// (batch, channel, pixel) strides; the channel-last copy the first convolution wants is made from there, as on the eager path.
//
// params = {idx, ny, nx, flip} cannot be validated at launch: the kernel clamps idx into [0, N), reduces ny / nx modulo H / W
// (negative values included) and reads flip as != 0, so every index stays inside the tensors whatever the four integers hold.
//
// Pure data movement, bit-exact.  A block owns 256 consecutive x of one output row: stores are coalesced, loads are one
// contiguous run per row (two where the roll wraps), read backwards under flip.
#include "fsv_common.h"

// grid: (rows0 + rows1) * xchunks blocks of 256, rows_t = B * C_t * H; the rows of tensor 0 come first
__global__ __launch_bounds__(256) void fsv_roll_flip_kernel(const float* __restrict__ src0, float* __restrict__ dst0, int C0,
                                                            const float* __restrict__ src1, float* __restrict__ dst1, int C1, int B,
                                                            int N, int H, int W, int xchunks, const int* __restrict__ params) {
  int idx = params[0], ny = params[1] % H, nx = params[2] % W;
  const bool flip = params[3] != 0;
  idx = idx < 0 ? 0 : (idx > N - 1 ? N - 1 : idx);
  if (ny < 0) ny += H;
  if (nx < 0) nx += W;
  long long row = blockIdx.x / xchunks;
  const int x = (int)(blockIdx.x % xchunks) * 256 + threadIdx.x;
  const long long rows0 = (long long)B * C0 * H;
  const float* src = src0;
  float* dst = dst0;
  int C = C0;
  if (row >= rows0) {
    row -= rows0; src = src1; dst = dst1; C = C1;
  }
  if (x >= W) return;
  const int y = (int)(row % H);
  const long long bc = row / H;
  const int c = (int)(bc % C);
  const long long b = bc / C;
  int sy = y - ny;
  if (sy < 0) sy += H;
  int sx = (flip ? W - 1 - x : x) - nx;
  if (sx < 0) sx += W;
  dst[row * W + x] = src[(((b * N + idx) * C + c) * H + sy) * (long long)W + sx];
}

extern "C" {
int fsv_roll_flip(const float* src0, float* dst0, int C0, const float* src1, float* dst1, int C1, int B, int N, int H, int W,
                  const int* params, hipStream_t stream) {
  if (!src0 || !dst0 || !params || C0 < 1 || B < 1 || N < 1 || H < 1 || W < 1) return FSV_ERR_BAD_ARG;
  if (C1 < 0 || (C1 > 0 && (!src1 || !dst1))) return FSV_ERR_BAD_ARG;
  const int xchunks = fsv_cdiv(W, 256);
  const long long blocks = (long long)B * ((long long)C0 + C1) * H * xchunks;
  if (blocks > 0x7fffffffLL) return FSV_ERR_UNSUPPORTED;
  FSV_LAUNCH(fsv_roll_flip_kernel, dim3((unsigned)blocks), dim3(256), stream, src0, dst0, C0, src1, dst1, C1, B, N, H, W, xchunks,
             params);
  return fsv_check_launch();
}
}  // extern "C"
