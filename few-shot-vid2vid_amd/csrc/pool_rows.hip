// The pooled-row operand of the weight generators under --use_label_ref concat (generator.py:248,278 + reshape_embed_input):
//
//     rows[b * C + c][oy * OW + ox] = mean of x[b][c][window(oy)][window(ox)]          nn.AdaptiveAvgPool2d((OH, OW)), OH = OW = 32
//
// x is an NHWC fp32 feature map of the reference encoder, rows is channel-major - what the first Linear of every fc_spade_* /
// fc_conv_* chain reads.  ATen's window rule, window(o) = [floor(o H / OH), ceil((o + 1) H / OH)), per axis: the map shrinks at the
// full-resolution levels (512 -> 32), is copied at 32 and GROWS below (16 -> 32), windows overlap when the sizes do not divide.
//
// Both kernels are bandwidth kernels.  The map is read (forward) / written (backward) once, 16 bytes per lane: eight lanes cover the
// 32 channels of a channel tile at one pixel (one 128-byte line), the other five bits of the work-item index walk pixels.  The
// channel <-> position transpose goes through LDS with an odd row pitch (33 dwords: ds_read_b32 / ds_write_b32 bank = dword mod 32,
// lanes of a 32-lane half then fall on 32 different banks), so the row side is read and written as runs of consecutive floats per
// channel.  No atomics and a summation order that depends on the shapes alone: results are bit-reproducible.
#include "fsv_common.h"

#define FSV_PR_PITCH 33        // LDS row pitch in dwords (32 channels + 1)
#define FSV_PR_MAXOX 40        // pooled columns one backward block can meet (host-checked)

__device__ __forceinline__ void fsv_pr_win(int o, int in, int out, int& s, int& e) {
  s = (int)(((long long)o * in) / out);
  e = (int)((((long long)(o + 1)) * in + out - 1) / out);
}

// grid: N * OH * nxc * ctiles blocks of 256.  A block owns one pooled row oy, OXB = 32 / S consecutive pooled columns and 32
// channels.  work-item = (slot p = tid / 8, lane = tid % 8): slot p works for pooled column p / S and sums every S-th element of its
// window (S = 1 where there are blocks enough, up to 32 at the full-resolution levels, where a 16 x 16 window of 32 channels would
// otherwise be one work-item's 256 dependent loads); the S partial sums are added in slot order.
__global__ __launch_bounds__(256) void fsv_pool_rows_fwd_kernel(const float* __restrict__ x, float* __restrict__ rows, int N, int H,
                                                                int W, int C, int OH, int OW, int S, int nxc, int ctiles) {
  __shared__ float part[32 * 32];                  // [slot][channel]
  __shared__ float fin[32 * FSV_PR_PITCH];         // [pooled column][channel]
  const int OXB = 32 / S;
  int bid = blockIdx.x;
  const int ct = bid % ctiles; bid /= ctiles;
  const int xc = bid % nxc; bid /= nxc;
  const int oy = bid % OH;
  const int n = bid / OH;
  const int tid = threadIdx.x, lane = tid & 7, p = tid >> 3;
  const int s = p % S;
  const int ox = xc * OXB + p / S;
  const int c = ct * 32 + lane * 4;
  int ys, ye;
  fsv_pr_win(oy, H, OH, ys, ye);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ox < OW && c < C) {
    int xs, xe;
    fsv_pr_win(ox, W, OW, xs, xe);
    const int ww = xe - xs, cnt = (ye - ys) * ww;
    const float* base = x + (((long long)n * H + ys) * W + xs) * C + c;
    for (int e = s; e < cnt; e += S) {
      const int wy = e / ww, wx = e - wy * ww;
      const float4 v = *(const float4*)(base + ((long long)wy * W + wx) * C);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  *(float4*)(part + p * 32 + lane * 4) = acc;
  __syncthreads();
  for (int o = tid; o < OXB * 32; o += 256) {
    const int cl = o & 31, ol = o >> 5;
    float sum = part[(ol * S) * 32 + cl];
    for (int k = 1; k < S; ++k) sum += part[(ol * S + k) * 32 + cl];
    const int oxo = xc * OXB + ol;
    float r = 0.f;
    if (oxo < OW) {
      int xs, xe;
      fsv_pr_win(oxo, W, OW, xs, xe);
      r = sum / (float)((ye - ys) * (xe - xs));
    }
    fin[ol * FSV_PR_PITCH + cl] = r;
  }
  __syncthreads();
  for (int o = tid; o < OXB * 32; o += 256) {       // consecutive work-items: consecutive pooled columns of one channel
    const int ol = o % OXB, cl = o / OXB;
    const int oxo = xc * OXB + ol, co = ct * 32 + cl;
    if (oxo < OW && co < C) rows[((long long)n * C + co) * OH * OW + (long long)oy * OW + oxo] = fin[ol * FSV_PR_PITCH + cl];
  }
}

// grid: N * H * nxc * ctiles blocks of 256.  A block owns one map row yy, 32 * PX consecutive pixels and 32 channels; work-item =
// (pixel slot, lane) holds PX pixels x 4 channels.  Every map element gathers drow / window size from the windows that contain it,
// pooled rows ascending, pooled columns ascending (the order in which ATen's scatter loop meets them).  Per pooled row the block
// stages the few pooled columns its pixels touch in LDS, read from the rows as runs of consecutive floats per channel.
template <int PX>
__global__ __launch_bounds__(256) void fsv_pool_rows_bwd_kernel(const float* __restrict__ drows, float* __restrict__ dx, int N, int H,
                                                                int W, int C, int OH, int OW, int nxc, int ctiles) {
  __shared__ float g[FSV_PR_MAXOX * FSV_PR_PITCH];        // [pooled column - ox_lo][channel]
  int bid = blockIdx.x;
  const int ct = bid % ctiles; bid /= ctiles;
  const int xc = bid % nxc; bid /= nxc;
  const int yy = bid % H;
  const int n = bid / H;
  const int tid = threadIdx.x, lane = tid & 7, p = tid >> 3;
  const int c = ct * 32 + lane * 4;
  const int x0 = xc * 32 * PX;
  const int x1 = (x0 + 32 * PX < W ? x0 + 32 * PX : W) - 1;
  const int oy_lo = (int)(((long long)yy * OH) / H);
  int oy_hi = (int)((((long long)yy + 1) * OH + H - 1) / H) - 1;
  if (oy_hi > OH - 1) oy_hi = OH - 1;
  const int ox_lo = (int)(((long long)x0 * OW) / W);
  int ox_hi = (int)((((long long)x1 + 1) * OW + W - 1) / W) - 1;
  if (ox_hi > OW - 1) ox_hi = OW - 1;
  const int nox = ox_hi - ox_lo + 1;
  float4 acc[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    int ys, ye;
    fsv_pr_win(oy, H, OH, ys, ye);
    if (yy < ys || yy >= ye) continue;               // (the same for every work-item of the block)
    const float kh = (float)(ye - ys);
    __syncthreads();                                 // the previous pooled row's tile has been consumed
    for (int o = tid; o < nox * 32; o += 256) {
      const int oxk = o % nox, cl = o / nox, co = ct * 32 + cl;
      g[oxk * FSV_PR_PITCH + cl] = co < C ? drows[((long long)n * C + co) * OH * OW + (long long)oy * OW + ox_lo + oxk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int xx = x0 + p + 32 * k;
      if (xx > x1 || c >= C) continue;
      const int oxa = (int)(((long long)xx * OW) / W);
      int oxb = (int)((((long long)xx + 1) * OW + W - 1) / W) - 1;
      if (oxb > ox_hi) oxb = ox_hi;
      for (int ox = oxa; ox <= oxb; ++ox) {
        int xs, xe;
        fsv_pr_win(ox, W, OW, xs, xe);
        if (xx < xs || xx >= xe) continue;
        const float kw = (float)(xe - xs);
        const float* gp = g + (ox - ox_lo) * FSV_PR_PITCH + lane * 4;
        acc[k].x += gp[0] / kh / kw;
        acc[k].y += gp[1] / kh / kw;
        acc[k].z += gp[2] / kh / kw;
        acc[k].w += gp[3] / kh / kw;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int xx = x0 + p + 32 * k;
    if (xx <= x1 && c < C) *(float4*)(dx + (((long long)n * H + yy) * W + xx) * C + c) = acc[k];
  }
}

extern "C" {
int fsv_pool_rows_fwd(const float* x, float* rows, int N, int H, int W, int C, int OH, int OW, hipStream_t stream) {
  if (!x || !rows || N < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || OH < 1 || OW < 1) return FSV_ERR_BAD_ARG;
  const int ctiles = fsv_cdiv(C, 32);
  const long win = (long)fsv_cdiv(H, OH) * fsv_cdiv(W, OW);          // window elements (1 where the map grows)
  int S = 1;
  while (S < 32 && 2 * S <= win && (long long)N * OH * ctiles * fsv_cdiv(OW, 32 / S) < 2048) S *= 2;
  const int nxc = fsv_cdiv(OW, 32 / S);
  const long long blocks = (long long)N * OH * nxc * ctiles;
  if (blocks > 0x7fffffffLL) return FSV_ERR_UNSUPPORTED;
  FSV_LAUNCH(fsv_pool_rows_fwd_kernel, dim3((unsigned)blocks), dim3(256), stream, x, rows, N, H, W, C, OH, OW, S, nxc, ctiles);
  return fsv_check_launch();
}

int fsv_pool_rows_bwd(const float* drows, float* dx, int N, int H, int W, int C, int OH, int OW, hipStream_t stream) {
  if (!drows || !dx || N < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || OH < 1 || OW < 1) return FSV_ERR_BAD_ARG;
  const int ctiles = fsv_cdiv(C, 32);
  const int PX = W >= 128 ? 4 : 1;
  const int nxc = fsv_cdiv(W, 32 * PX);
  const long span = fsv_cdiv((long)32 * PX * OW, W) + 2;            // pooled columns under one block's pixels
  if ((span < OW ? span : OW) > FSV_PR_MAXOX) return FSV_ERR_UNSUPPORTED;
  const long long blocks = (long long)N * H * nxc * ctiles;
  if (blocks > 0x7fffffffLL) return FSV_ERR_UNSUPPORTED;
  if (PX == 4)
    FSV_LAUNCH(fsv_pool_rows_bwd_kernel<4>, dim3((unsigned)blocks), dim3(256), stream, drows, dx, N, H, W, C, OH, OW, nxc, ctiles);
  else
    FSV_LAUNCH(fsv_pool_rows_bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), stream, drows, dx, N, H, W, C, OH, OW, nxc, ctiles);
  return fsv_check_launch();
}
}  // extern "C"
