// Fused SPADE modulation with 3x3 gamma / beta convolutions (--spade_ks 3) on the matrix cores.
//
// Reference semantics (models/networks/normalization.py:18-52 with ks = 3, SPADE.forward):
//     out = BN_noaffine(x)
//     for each non-None map k:   gamma_k = conv3x3(m_k; Wg_k, pad 1) + bg_k ;  beta_k = conv3x3(m_k; Wb_k, pad 1) + bb_k
//                                out = out * (1 + gamma_k) + beta_k
// followed by leaky_relu(0.2) for bn_0 / bn_1 (architecture.py:95-97).  Map 0 of the adaptive layers uses per-sample generated
// weights (batch_conv, base_network.py:56-71), the spade_combine maps fixed ones (mlp_gamma2/3).
//
// The structure of csrc/spade.hip (NHWC, grid.z = sample so that per-sample and shared weights mix - a batch stride of 0 means
// shared -, one K-chunk sequence across all maps, double-buffered LDS, an epilogue that applies the denormalisation, every map's
// modulation in order and the activation before the single write of h, the `up` mode that reads x through the nearest-x2 index).
// What differs is the A operand: K of map k is (tap, channel) = 9 * Ch_k deep, the order of the gather-GEMM's forward operand
// (fsv_prep_weight mode 0 of the combined [gamma | beta] weight [2C][Ch][3][3]: row tap * Ch + ci, gamma in columns [0, C), beta in
// [C, 2C)).  The row of output pixel (y, x) for tap (dy, dx) is the map's pixel (y + dy - 1, x + dx - 1), zero outside the image:
// the buffer descriptor's range check only covers the ends of the tensor, so every row carries its own predicate (the tap decoding
// of conv_igemm.hip, with the 3x3 / pad 1 table written out).  Ch % 4 == 0 keeps a quad of four k inside one tap.
//
// Optional side output gb[k] = gamma_k | beta_k ([N][HW][2C] fp32): the backward pass (ops._SpadeFn) then runs the element-wise
// chain fsv_spade_bwd_elem on it instead of recomputing the 9 * Ch-deep GEMMs (profiles/spade_k3_notes.md: measured choice).
#include "conv_igemm.h"

#define FSV_K3_BK 32
#define FSV_K3_MAXMAPS 3

struct SpadeK3P {
  const float* x;         // [N][HW][C], or [N][HW / 4][C] with up = 1
  const float* mean;      // [C] (+ z * stat_bstride)
  const float* rstd;
  float* h;               // [N][HW][C]
  const float* map[FSV_K3_MAXMAPS];     // [N][HW][Ch_k]
  const float* wt[FSV_K3_MAXMAPS];      // [kpad_k][ldw] (+ z * w_bstride_k)
  const float* bcat[FSV_K3_MAXMAPS];    // [2C] (+ z * b_bstride_k): gamma biases, then beta biases
  float* gb[FSV_K3_MAXMAPS];            // optional [N][HW][2C]
  int ch[FSV_K3_MAXMAPS], kdim[FSV_K3_MAXMAPS], kpad[FSV_K3_MAXMAPS];
  long long w_bstride[FSV_K3_MAXMAPS], b_bstride[FSV_K3_MAXMAPS];
  int nmaps, H, W, HW, C, ldw, act, up;
  long long stat_bstride;
};

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void fsv_spade_k3_kernel(SpadeK3P p) {
  constexpr int BK = FSV_K3_BK;
  constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
  constexpr int RPA = 256 / 8, NPA = BM / RPA;          // A: 8 work-items per row (one quad of 4 k each)
  constexpr int QB = BN / 4, RPB = 256 / QB, NPB = BK / RPB;
  constexpr int A_ST = BM * BK, B_ST = BK * BN;
  static_assert(WM * WN == 4, "4 waves");
  static_assert(NPA >= 1 && NPB >= 1 && NPA * RPA == BM && NPB * RPB == BK, "tile");
  __shared__ __attribute__((aligned(16))) float smem[2 * (A_ST + 2 * B_ST)];
  float* const As = smem;
  float* const Bs = smem + 2 * A_ST;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int z = blockIdx.z;
  const int bm0 = blockIdx.x * BM, bn0 = blockIdx.y * BN;
  const int lrow = lane & 31, lk = lane >> 5;
  const int kq = tid & 7, ar0 = tid >> 3;
  const int bq = tid % QB, br0 = tid / QB;
  const int bcol = bn0 + bq * 4;
  const bool bcol_ok = bcol < p.C;        // C % 4 == 0: the quad lies inside the gamma (and the beta) columns
  const long long pix0 = (long long)z * p.HW;

  // image coordinates of this work-item's A rows (fixed for the tile)
  int ay[NPA], ax[NPA];
  bool aok[NPA];
#pragma unroll
  for (int i = 0; i < NPA; ++i) {
    const int m = bm0 + ar0 + i * RPA;
    aok[i] = m < p.HW;
    ay[i] = m / p.W;
    ax[i] = m - ay[i] * p.W;
  }

  // ---- the flat chunk sequence over the maps -------------------------------------------------------------------------------------
  int nch[FSV_K3_MAXMAPS], total = 0;
#pragma unroll
  for (int k = 0; k < FSV_K3_MAXMAPS; ++k) { nch[k] = (k < p.nmaps) ? (p.kdim[k] + BK - 1) / BK : 0; total += nch[k]; }
  int ld_k = 0, ld_c = 0, ld_t = 0;       // (map, chunk) of the next chunk to load; ld_t counts the loaded chunks
  float4 areg[NPA], breg[2][NPB];
  auto issue_loads = [&]() {
    const int k = ld_k;                   // uniform
    const int Ch = p.ch[k];
    const fsv_buf abuf = fsv_make_buf(p.map[k] + pix0 * Ch, (long long)p.HW * Ch * 4);
    const int kk = ld_c * BK + kq * 4;
    const int tap = kk / Ch, ci = kk - tap * Ch;
    const int ty = tap / 3, dy = ty - 1, dx = tap - 3 * ty - 1;
    const bool kin = kk < p.kdim[k];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
      const int ys = ay[i] + dy, xs = ax[i] + dx;
      const bool ok = aok[i] & kin & (ys >= 0) & (ys < p.H) & (xs >= 0) & (xs < p.W);
      areg[i] = fsv_buf_load4(abuf, ok ? (unsigned)(((ys * p.W + xs) * Ch + ci) * 4) : FSV_BUF_OOB);
    }
    const fsv_buf wbuf = fsv_make_buf(p.wt[k] + z * p.w_bstride[k], (long long)p.kpad[k] * p.ldw * 4);
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
      const int kr = ld_c * BK + br0 + i * RPB;
      const bool ok = bcol_ok & (kr < p.kdim[k]);
      breg[0][i] = fsv_buf_load4(wbuf, ok ? (unsigned)((kr * p.ldw + bcol) * 4) : FSV_BUF_OOB);
      breg[1][i] = fsv_buf_load4(wbuf, ok ? (unsigned)((kr * p.ldw + p.C + bcol) * 4) : FSV_BUF_OOB);
    }
    ++ld_t;
    if (++ld_c >= nch[k == 0 ? 0 : (k == 1 ? 1 : 2)]) { ld_c = 0; ++ld_k; }
  };
  auto store_chunk = [&](int buf) {
    float* a_dst = As + buf * A_ST;
    float* b_dst = Bs + buf * (2 * B_ST);
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
      const int r = ar0 + i * RPA;
      // the A image of spade.hip: quad (k0 k1 k2 k3) stored as (k0 k2 | k1 k3), rows with bit 4 set as (k1 k3 | k0 k2), quad q of
      // row r in slot q ^ ((r >> 1) & 7)
      const bool hi = (r >> 4) & 1;
      float4 v;
      v.x = hi ? areg[i].y : areg[i].x; v.y = hi ? areg[i].w : areg[i].z;
      v.z = hi ? areg[i].x : areg[i].y; v.w = hi ? areg[i].z : areg[i].w;
      *reinterpret_cast<float4*>(&a_dst[r * BK + ((kq ^ ((r >> 1) & 7)) << 2)]) = v;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < NPB; ++i)
        *reinterpret_cast<float4*>(&b_dst[q * B_ST + (br0 + i * RPB) * BN + bq * 4]) = breg[q][i];
  };

  // ---- x of the tile (D layout), the per-channel statistics -------------------------------------------------------------------------
  float xv[TM][TN][16], mu[TN], rs[TN];
  {
    const long long xpix_n = p.up ? (p.HW >> 2) : p.HW;
    const fsv_buf xbuf = fsv_make_buf(p.x + (long long)z * xpix_n * p.C, xpix_n * p.C * 4);
    const float* mean = p.mean + z * p.stat_bstride;
    const float* rstd = p.rstd + z * p.stat_bstride;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = bn0 + wn * (TN * 32) + j * 32 + lrow;
      const bool cok = c < p.C;
      mu[j] = cok ? mean[c] : 0.f; rs[j] = cok ? rstd[c] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = bm0 + wm * (TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          int src = m;
          if (p.up) {
            const int y = m / p.W, xx = m - y * p.W;
            src = (y >> 1) * (p.W >> 1) + (xx >> 1);
          }
          xv[i][j][r] = fsv_buf_load1(xbuf, (cok & (m < p.HW)) ? (unsigned)((src * p.C + c) * 4) : FSV_BUF_OOB);
        }
    }
  }

  f32x16 acc[2][TM][TN], outv[TM][TN];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][i][j][r] = 0.f;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) outv[i][j][r] = (xv[i][j][r] - mu[j]) * rs[j];

  int a_off[TM], a_swz[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int r = wm * (TM * 32) + i * 32 + lrow;
    a_off[i] = r * BK + 2 * (lk ^ ((r >> 4) & 1));
    a_swz[i] = (r >> 1) & 7;
  }
  const int b_off = lk * BN + wn * (TN * 32) + lrow;
  auto read_group = [&](const float* a_src, const float* b_src, int g, float2 (&a4)[2][TM], float (&b)[4][2][TN]) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a4[q][i] = *reinterpret_cast<const float2*>(&a_src[a_off[i] + (((2 * g + q) ^ a_swz[i]) << 2)]);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < TN; ++j) b[s4][q][j] = b_src[q * B_ST + b_off + (8 * g + 2 * s4) * BN + j * 32];
  };
  auto mma_group = [&](const float2 (&a4)[2][TM], const float (&b)[4][2][TN]) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float2 v = a4[s4 >> 1][i];
        const float a = (s4 & 1) ? v.y : v.x;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[q][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[s4][q][j], acc[q][i][j], 0, 0, 0);
      }
  };

  int buf = 0;
  // one chunk: the next chunk's loads at the top, this chunk's MFMAs (fragments one k-group ahead), the loaded registers stored into
  // the other LDS buffer behind three quarters of them, one barrier
  auto chunk = [&]() {
    const bool more = ld_t < total;       // uniform
    if (more) issue_loads();
    const float* a_src = As + buf * A_ST;
    const float* b_src = Bs + buf * (2 * B_ST);
    float2 fa[2][2][TM];
    float fb[2][4][2][TN];
    read_group(a_src, b_src, 0, fa[0], fb[0]);
    FSV_SCHED_FENCE();
    read_group(a_src, b_src, 1, fa[1], fb[1]);
    FSV_SCHED_FENCE();
    mma_group(fa[0], fb[0]);
    FSV_SCHED_FENCE();
    read_group(a_src, b_src, 2, fa[0], fb[0]);
    FSV_SCHED_FENCE();
    mma_group(fa[1], fb[1]);
    FSV_SCHED_FENCE();
    read_group(a_src, b_src, 3, fa[1], fb[1]);
    FSV_SCHED_FENCE();
    mma_group(fa[0], fb[0]);
    FSV_SCHED_FENCE();
    if (more) store_chunk(buf ^ 1);
    FSV_SCHED_FENCE();
    mma_group(fa[1], fb[1]);
    __syncthreads();
    buf ^= 1;
  };

  // modulation of map k (registers only), with the optional gamma | beta side output
  auto modulate = [&](int k) {
    const float* bc = p.bcat[k] + z * p.b_bstride[k];
    float* gbk = p.gb[k] ? p.gb[k] + pix0 * 2 * p.C : nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = bn0 + wn * (TN * 32) + j * 32 + lrow;
      const bool cok = c < p.C;
      const float bg = cok ? bc[c] : 0.f, bb = cok ? bc[p.C + c] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = bm0 + wm * (TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          const float g = acc[0][i][j][r] + bg, b = acc[1][i][j][r] + bb;
          if (gbk && cok && m < p.HW) {
            gbk[(long long)m * 2 * p.C + c] = g;
            gbk[(long long)m * 2 * p.C + p.C + c] = b;
          }
          outv[i][j][r] = outv[i][j][r] * (1.f + g) + b;
          acc[0][i][j][r] = 0.f; acc[1][i][j][r] = 0.f;
        }
    }
  };

  if (total > 0) {
    issue_loads();
    store_chunk(0);
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < FSV_K3_MAXMAPS; ++k) {
    if (k < p.nmaps) {
#pragma unroll 1
      for (int c = 0; c < nch[k]; ++c) chunk();
      modulate(k);
    }
  }

  float* h_z = p.h + pix0 * p.C;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int c = bn0 + wn * (TN * 32) + j * 32 + lrow;
    const bool cok = c < p.C;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = bm0 + wm * (TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (cok && m < p.HW) h_z[(long long)m * p.C + c] = fsv_act(outv[i][j][r], p.act);
      }
  }
}

extern "C" {

int fsv_spade_k3_fwd(const float* x, const float* mean, const float* rstd, float* h, int nmaps, const float* const* maps,
                     const float* const* wt, const float* const* bcat, const int* ch, const long long* w_bstride,
                     const long long* b_bstride, float* const* gb, int N, int H, int W, int C, int ldw, long long stat_bstride,
                     int act, int up, hipStream_t stream) {
  if (!x || !mean || !rstd || !h || nmaps < 0 || nmaps > FSV_K3_MAXMAPS || N < 1 || H < 1 || W < 1) return FSV_ERR_BAD_ARG;
  if (nmaps > 0 && (!maps || !wt || !bcat || !ch || !w_bstride || !b_bstride)) return FSV_ERR_BAD_ARG;
  if (C < 4 || (C & 3) || ldw < 2 * C || (ldw & 3)) return FSV_ERR_UNSUPPORTED;
  if (up && ((H & 1) || (W & 1))) return FSV_ERR_BAD_ARG;
  const long long HW = (long long)H * W;
  if ((long long)N * HW * C * 4 > FSV_BUF_MAX_BYTES) return FSV_ERR_UNSUPPORTED;
  SpadeK3P p;
  p.x = x; p.mean = mean; p.rstd = rstd; p.h = h;
  for (int k = 0; k < FSV_K3_MAXMAPS; ++k) {
    const bool on = k < nmaps;
    p.map[k] = on ? maps[k] : nullptr; p.wt[k] = on ? wt[k] : nullptr; p.bcat[k] = on ? bcat[k] : nullptr;
    p.gb[k] = (on && gb) ? gb[k] : nullptr;
    p.ch[k] = on ? ch[k] : 0;
    p.kdim[k] = 9 * p.ch[k];
    p.kpad[k] = (p.kdim[k] + FSV_K3_BK - 1) / FSV_K3_BK * FSV_K3_BK;
    p.w_bstride[k] = on ? w_bstride[k] : 0; p.b_bstride[k] = on ? b_bstride[k] : 0;
    if (!on) continue;
    if (!maps[k] || !wt[k] || !bcat[k] || (gb && !gb[k])) return FSV_ERR_BAD_ARG;
    if (ch[k] < 4 || (ch[k] & 3)) return FSV_ERR_UNSUPPORTED;
    if (HW * ch[k] * 4 > FSV_BUF_MAX_BYTES || (long long)p.kpad[k] * ldw * 4 > FSV_BUF_MAX_BYTES) return FSV_ERR_UNSUPPORTED;
  }
  p.nmaps = nmaps; p.H = H; p.W = W; p.HW = (int)HW; p.C = C; p.ldw = ldw; p.act = act; p.up = up ? 1 : 0;
  p.stat_bstride = stat_bstride;
  if (C <= 32) {
    dim3 g(fsv_cdiv(HW, 128), 1, N);
    FSV_LAUNCH((fsv_spade_k3_kernel<128, 32, 4, 1>), g, dim3(256), stream, p);
  } else {
    dim3 g(fsv_cdiv(HW, 64), fsv_cdiv(C, 64), N);
    FSV_LAUNCH((fsv_spade_k3_kernel<64, 64, 2, 2>), g, dim3(256), stream, p);
  }
  return fsv_check_launch();
}

}  // extern "C"
