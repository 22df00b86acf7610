// The backward pass of the streaming few-shot attention (attention.hip): exact fp32, no atomics, fixed summation order, and like the
// forward pass no [N P, P] tensor - the probabilities are recomputed from the energies and the saved statistics
//     p[key][query] = exp(<k[key], q[query]> - lse[query]),    lse = running maximum + log(denominator)   (fsv_attention_fused_fwd_lse)
// (an exponent that is never positive: energies in the hundreds do not overflow).  With do_i the cotangents of the two outputs:
//     delta[query] = sum_c do0 o0 + sum_c do1 o1
//     dv_i[key]    = sum_query p do_i[query]
//     dp           = <do0[query], v0[key]> + <do1[query], v1[key]>,    ds = p (dp - delta[query])
//     dq[query]    = sum_key ds k[key],        dk[key] = sum_query ds q[query]
// Every sum is owned by ONE workgroup that walks its other axis in ascending order:
//   fsv_attn_bwd_delta_kernel   one wave per query row.
//   fsv_attn_bwd_q_kernel       the structure of the forward kernel: 128 queries per workgroup (32 per wave), q and do fragments in
//                               registers, K / V tiles of 32 keys through LDS.  Energies and dp come out as D[key][query] (lane = query),
//                               so register r of ds in the two half-waves IS the A fragment (row = query) of the dq product against rows
//                               of the K tile in LDS (the swapped-operand trick of attention.hip).  The keys may be split over nsplit
//                               workgroups per query tile; fsv_attn_bwd_sum_kernel adds their partial dq in ascending order.
//   fsv_attn_bwd_k_kernel<DK>   128 keys per workgroup (32 per wave), k (and for DK the v) fragments in registers, tiles of 32 queries
//                               (q, do, lse, delta) through LDS.  Energies come out as D[query][key] (lane = key): p is the A fragment
//                               (row = key) of the dv product against the do tile, ds that of the dk product against the q tile.
//                               DK = false writes dv0 / dv1 (no dp), DK = true writes dk: k, v0, v1 fragments and three accumulator sets
//                               at 128 channels each do not fit 512 registers, one more energy recomputation does.
// The energies are the fma chains of the forward kernel (the same products in the same channel order), so they have its bits.
#include "fsv_common.h"

#define FSV_AB_BT 128          // rows (queries or keys) a workgroup owns, 32 per wave
#define FSV_AB_BS 32           // rows per streamed tile
#define FSV_AB_LD 132          // LDS row of 128 channels + one 16-byte slot: conflict-free b128 fragment reads
#define FSV_AB_LD2 260         // LDS row of two 128-channel maps side by side
#define FSV_AB_MAX_SPLIT 8

struct AttnBwdP {
  const float* q;              // [B][P][C]
  const float* k;              // [B][N P][C]
  const float* v[2];           // [B][N P][cv[i]] (NULL: absent)
  const float* dout[2];        // [B][P][cv[i]]
  const float* lse;            // [B][P]
  const float* delta;          // [B][P]
  float* dq;                   // [B][P][C] (+ split * dq_split: the workspace copies when nsplit > 1)
  long long dq_split;
  float* dk;                   // [B][N P][C]
  float* dv[2];                // [B][N P][cv[i]] (NULL: not wanted)
  int cv[2];
  int B, N, P, C, nsplit, ntiles;
};

__host__ __device__ static inline int fsv_ab_tile0(int s, int nsplit, int ntiles) { return (int)((long long)s * ntiles / nsplit); }

__device__ static inline int fsv_ab_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

// rows [row0, row0 + 32) x 128 channels of src[nrows][C] -> dst[32][ld] from column col0, zero past the last row and the last channel
__device__ static inline void fsv_ab_stage(float* dst, int ld, int col0, const float* src, long long row0, long long nrows, int C, int tid) {
  const int c4 = (tid & 31) * 4, r0 = tid >> 5;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int r = r0 + 8 * u;
    const long long row = row0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src && c4 < C && row < nrows) v = *reinterpret_cast<const float4*>(src + row * C + c4);
    *reinterpret_cast<float4*>(&dst[r * ld + col0 + c4]) = v;
  }
}

// the fragments of row `row` of src[nrows][C] a lane keeps for a whole launch: lane (row, lk) holds channels 32 cq + 8 j + 4 lk + e
__device__ static inline void fsv_ab_fragment(float4 (&f)[4][4], const float* src, long long row, long long nrows, int C, int lk) {
  const bool ok = src && row < nrows;
  const float* p = src + (ok ? row : 0) * C;
#pragma unroll
  for (int cq = 0; cq < 4; ++cq)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 32 * cq + 8 * j + 4 * lk;
      f[cq][j] = (ok && c < C) ? *reinterpret_cast<const float4*>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// s[i][j] += sum_c a[i][c] b[j][c] over ncq 32-channel chunks: a = row (lane & 31) of an LDS tile (arow points at its channel 4 lk),
// b = the lane's register fragments
__device__ static inline f32x16 fsv_ab_dot(f32x16 s, const float* arow, const float4 (&bf)[4][4], int ncq) {
#pragma unroll
  for (int cq = 0; cq < 4; ++cq)
    if (cq < ncq) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(arow + 32 * cq + 8 * j);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bf[cq][j].x, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bf[cq][j].y, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bf[cq][j].z, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bf[cq][j].w, s, 0, 0, 0);
      }
    }
  return s;
}

// delta[row] = <do0[row], o0[row]> + <do1[row], o1[row]>: one wave per row, the lanes' channel quads in ascending order, then the
// xor tree - a fixed order
__global__ __launch_bounds__(256) void fsv_attn_bwd_delta_kernel(const float* o0, const float* do0, const float* o1, const float* do1,
                                                                 float* delta, long long rows, int c0, int c1) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float sum = 0.f;
  for (int c = 4 * lane; c < c0; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(o0 + row * c0 + c), g = *reinterpret_cast<const float4*>(do0 + row * c0 + c);
    sum += a.x * g.x; sum += a.y * g.y; sum += a.z * g.z; sum += a.w * g.w;
  }
  for (int c = 4 * lane; c < c1; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(o1 + row * c1 + c), g = *reinterpret_cast<const float4*>(do1 + row * c1 + c);
    sum += a.x * g.x; sum += a.y * g.y; sum += a.z * g.z; sum += a.w * g.w;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if (lane == 0) delta[row] = sum;
}

// ---- dq: the workgroup owns 128 queries and walks the key tiles [t0, t1) of its split ---------------------------------------------------
__global__ __launch_bounds__(256) void fsv_attn_bwd_q_kernel(AttnBwdP p) {
  __shared__ __attribute__((aligned(16))) float Ks[FSV_AB_BS * FSV_AB_LD];
  __shared__ __attribute__((aligned(16))) float Vs[FSV_AB_BS * FSV_AB_LD2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, split = blockIdx.y;
  const int P = p.P, C = p.C;
  const long long NP = (long long)p.N * P;
  const int q_wave = blockIdx.x * FSV_AB_BT + wave * 32;
  const int query = q_wave + lq;
  const bool wave_live = q_wave < P;
  const int t0 = fsv_ab_tile0(split, p.nsplit, p.ntiles), t1 = fsv_ab_tile0(split + 1, p.nsplit, p.ntiles);
  const int ncq = (C + 31) / 32, ncv0 = (p.cv[0] + 31) / 32, ncv1 = p.v[1] ? (p.cv[1] + 31) / 32 : 0;

  float4 qf[4][4], g0[4][4], g1[4][4];
  fsv_ab_fragment(qf, p.q + (long long)b * P * C, query, P, C, lk);
  fsv_ab_fragment(g0, p.dout[0] + (long long)b * P * p.cv[0], query, P, p.cv[0], lk);
  fsv_ab_fragment(g1, p.v[1] ? p.dout[1] + (long long)b * P * p.cv[1] : nullptr, query, P, p.cv[1], lk);
  const float lse = query < P ? p.lse[(long long)b * P + query] : 0.f;
  const float delta = query < P ? p.delta[(long long)b * P + query] : 0.f;

  const float* kbase = p.k + (long long)b * NP * C;
  const float* v0base = p.v[0] + (long long)b * NP * p.cv[0];
  const float* v1base = p.v[1] ? p.v[1] + (long long)b * NP * p.cv[1] : nullptr;

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int t = t0; t < t1; ++t) {
    const long long key0 = (long long)t * FSV_AB_BS;
    fsv_ab_stage(Ks, FSV_AB_LD, 0, kbase, key0, NP, C, tid);
    fsv_ab_stage(Vs, FSV_AB_LD2, 0, v0base, key0, NP, p.cv[0], tid);
    if (v1base) fsv_ab_stage(Vs, FSV_AB_LD2, 128, v1base, key0, NP, p.cv[1], tid);
    __syncthreads();
    if (wave_live) {
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
      s = fsv_ab_dot(s, &Ks[lq * FSV_AB_LD + 4 * lk], qf, ncq);                    // D[key][query]
      dp = fsv_ab_dot(dp, &Vs[lq * FSV_AB_LD2 + 4 * lk], g0, ncv0);
      dp = fsv_ab_dot(dp, &Vs[lq * FSV_AB_LD2 + 128 + 4 * lk], g1, ncv1);
      const int nkeys = (int)(NP - key0 < FSV_AB_BS ? NP - key0 : FSV_AB_BS);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pr = fsv_ab_row(r, lk) < nkeys ? expf(s[r] - lse) : 0.f;
        s[r] = pr * (dp[r] - delta);                                                // ds
      }
      // dq += ds K: register r of the half-waves is the A fragment over the keys (row(r, 0), row(r, 1))
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* krow = &Ks[fsv_ab_row(r, lk) * FSV_AB_LD + lq];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (ct < ncq) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], krow[32 * ct], acc[ct], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!wave_live) return;
  float* dst = p.dq + split * p.dq_split + (long long)b * P * C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = q_wave + fsv_ab_row(r, lk);
    if (qr >= P) continue;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
      if (32 * ct + lq < C) dst[(long long)qr * C + 32 * ct + lq] = acc[ct][r];
  }
}

// out[i] = sum over the splits' copies, in ascending split order (16-byte vectors)
__global__ __launch_bounds__(256) void fsv_attn_bwd_sum_kernel(const float* part, float* out, long long quads, int nsplit) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  float4 sum = *reinterpret_cast<const float4*>(part + 4 * i);
  for (int s = 1; s < nsplit; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(part + 4 * (s * quads + i));
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
  }
  *reinterpret_cast<float4*>(out + 4 * i) = sum;
}

// ---- dv (DK = false) or dk (DK = true): the workgroup owns 128 keys and walks every query tile in ascending order -------------------------
template <bool DK>
__global__ __launch_bounds__(256) void fsv_attn_bwd_k_kernel(AttnBwdP p) {
  __shared__ __attribute__((aligned(16))) float Qs[FSV_AB_BS * FSV_AB_LD];
  __shared__ __attribute__((aligned(16))) float Gs[FSV_AB_BS * FSV_AB_LD2];
  __shared__ float stat[2 * FSV_AB_BS];                                             // lse, delta of the tile's queries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z;
  const int P = p.P, C = p.C;
  const long long NP = (long long)p.N * P;
  const long long k_wave = (long long)blockIdx.x * FSV_AB_BT + wave * 32;
  const long long key = k_wave + lq;
  const bool wave_live = k_wave < NP;
  const int ncq = (C + 31) / 32;
  // the maps this launch reads: dv only where the gradient is wanted, dk every map there is
  const bool use0 = DK ? true : p.dv[0] != nullptr, use1 = DK ? p.v[1] != nullptr : p.dv[1] != nullptr;
  const int ncv0 = use0 ? (p.cv[0] + 31) / 32 : 0, ncv1 = use1 ? (p.cv[1] + 31) / 32 : 0;

  float4 kf[4][4];
  fsv_ab_fragment(kf, p.k + (long long)b * NP * C, key, NP, C, lk);
  float4 v0f[DK ? 4 : 1][4], v1f[DK ? 4 : 1][4];
  if constexpr (DK) {
    fsv_ab_fragment(v0f, p.v[0] + (long long)b * NP * p.cv[0], key, NP, p.cv[0], lk);
    fsv_ab_fragment(v1f, p.v[1] ? p.v[1] + (long long)b * NP * p.cv[1] : nullptr, key, NP, p.cv[1], lk);
  }
  const float* qbase = p.q + (long long)b * P * C;
  const float* g0base = use0 ? p.dout[0] + (long long)b * P * p.cv[0] : nullptr;
  const float* g1base = use1 ? p.dout[1] + (long long)b * P * p.cv[1] : nullptr;

  constexpr int NACC = DK ? 4 : 8;
  f32x16 acc[NACC];
#pragma unroll
  for (int t = 0; t < NACC; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int nqt = (P + FSV_AB_BS - 1) / FSV_AB_BS;
  for (int t = 0; t < nqt; ++t) {
    const long long q0 = (long long)t * FSV_AB_BS;
    fsv_ab_stage(Qs, FSV_AB_LD, 0, qbase, q0, P, C, tid);
    if (g0base) fsv_ab_stage(Gs, FSV_AB_LD2, 0, g0base, q0, P, p.cv[0], tid);
    if (g1base) fsv_ab_stage(Gs, FSV_AB_LD2, 128, g1base, q0, P, p.cv[1], tid);
    if (tid < 2 * FSV_AB_BS) {
      const long long qq = q0 + (tid & 31);
      // a query past the last one: exp(0 - inf) = 0 exactly
      stat[tid] = tid < 32 ? (qq < P ? p.lse[(long long)b * P + qq] : INFINITY) : (qq < P && DK ? p.delta[(long long)b * P + qq] : 0.f);
    }
    __syncthreads();
    if (wave_live) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      s = fsv_ab_dot(s, &Qs[lq * FSV_AB_LD + 4 * lk], kf, ncq);                    // D[query][key]
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = key < NP ? expf(s[r] - stat[fsv_ab_row(r, lk)]) : 0.f;
      if constexpr (DK) {
        f32x16 dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.f;
        dp = fsv_ab_dot(dp, &Gs[lq * FSV_AB_LD2 + 4 * lk], v0f, ncv0);
        dp = fsv_ab_dot(dp, &Gs[lq * FSV_AB_LD2 + 128 + 4 * lk], v1f, ncv1);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = s[r] * (dp[r] - stat[32 + fsv_ab_row(r, lk)]);
        // dk += ds^T Q: register r of the half-waves is the A fragment (row = key) over the queries (row(r, 0), row(r, 1))
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float* qrow = &Qs[fsv_ab_row(r, lk) * FSV_AB_LD + lq];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct)
            if (ct < ncq) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], qrow[32 * ct], acc[ct], 0, 0, 0);
        }
      } else {
        // dv += p^T dO
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float* grow = &Gs[fsv_ab_row(r, lk) * FSV_AB_LD2 + lq];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            if (ct < ncv0) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], grow[32 * ct], acc[ct], 0, 0, 0);
            if (ct < ncv1) acc[4 + ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], grow[128 + 32 * ct], acc[4 + ct], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!wave_live) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long kr = k_wave + fsv_ab_row(r, lk);
    if (kr >= NP) continue;
    if constexpr (DK) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (32 * ct + lq < C) p.dk[((long long)b * NP + kr) * C + 32 * ct + lq] = acc[ct][r];
    } else {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (p.dv[0] && 32 * ct + lq < p.cv[0]) p.dv[0][((long long)b * NP + kr) * p.cv[0] + 32 * ct + lq] = acc[ct][r];
        if (p.dv[1] && 32 * ct + lq < p.cv[1]) p.dv[1][((long long)b * NP + kr) * p.cv[1] + 32 * ct + lq] = acc[4 + ct][r];
      }
    }
  }
}

// argument errors, then the contract; C1 is 0 when there is no second map
static int fsv_ab_shape(int B, int N, int P, int C, int C0, int C1) {
  if (B <= 0 || N <= 0 || P <= 0 || C <= 0 || C0 <= 0 || C1 < 0) return FSV_ERR_BAD_ARG;
  if ((C | C0 | C1) & 3 || C > 128 || C0 > 128 || C1 > 128) return FSV_ERR_UNSUPPORTED;
  if (B > 65535 || (long long)N * P > (1ll << 31) - 64) return FSV_ERR_UNSUPPORTED;
  if ((long long)B * P / 4 >= 0x7fffffffll) return FSV_ERR_UNSUPPORTED;               // the delta launch's grid
  return FSV_OK;
}

// the key ranges of the dq launch (the forward's rule: fill 256 compute units, a function of the shape alone) and the workspace:
// delta [B][P], then the nsplit partial dq [nsplit][B][P][C] (16-byte vectors: B P is rounded up to a multiple of 4)
static int fsv_ab_plan(int B, int N, int P, int C, int nsplit, int* split_out, long long* ws_floats) {
  const int ntiles = (int)(((long long)N * P + FSV_AB_BS - 1) / FSV_AB_BS);
  if (nsplit <= 0) {
    const long long wgs = (long long)B * ((P + FSV_AB_BT - 1) / FSV_AB_BT);
    nsplit = (int)(256 / wgs);
    if (nsplit > FSV_AB_MAX_SPLIT) nsplit = FSV_AB_MAX_SPLIT;
    if (nsplit > ntiles) nsplit = ntiles;
    if (nsplit < 1) nsplit = 1;
  }
  if (nsplit > FSV_AB_MAX_SPLIT || nsplit > ntiles) return FSV_ERR_BAD_ARG;
  const long long rows = (long long)B * P;
  *split_out = nsplit;
  *ws_floats = (rows + 3) / 4 * 4 + (nsplit > 1 ? rows * nsplit * C : 0);
  return FSV_OK;
}

extern "C" int fsv_attention_fused_bwd_plan(int B, int N, int P, int C, int C0, int C1, int nsplit, long long* out) {
  if (!out) return FSV_ERR_BAD_ARG;
  int rc = fsv_ab_shape(B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  int split = 0;
  long long ws = 0;
  rc = fsv_ab_plan(B, N, P, C, nsplit, &split, &ws);
  if (rc != FSV_OK) return rc;
  out[0] = split; out[1] = ws;
  return FSV_OK;
}

extern "C" int fsv_attention_fused_bwd(const float* q, const float* k, const float* v0, const float* v1, const float* o0,
                                       const float* o1, const float* do0, const float* do1, const float* lse, float* dq, float* dk,
                                       float* dv0, float* dv1, int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws,
                                       long long ws_floats, hipStream_t stream) {
  if (!q || !k || !v0 || !o0 || !do0 || !lse || (v1 && (!o1 || !do1)) || (!v1 && dv1)) return FSV_ERR_BAD_ARG;
  if (!dq && !dk && !dv0 && !dv1) return FSV_ERR_BAD_ARG;
  if (v1 && C1 <= 0) return FSV_ERR_BAD_ARG;
  if (!v1) C1 = 0;
  int rc = fsv_ab_shape(B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  int split = 0;
  long long need = 0;
  rc = fsv_ab_plan(B, N, P, C, nsplit, &split, &need);
  if (rc != FSV_OK) return rc;
  if (!ws || ws_floats < need) return FSV_ERR_BAD_ARG;
  const long long rows = (long long)B * P, NP = (long long)N * P;
  if (rows * (C / 4) > 256ll * 0x7fffffff) return FSV_ERR_UNSUPPORTED;                // the dq sum's grid
  float* delta = ws;
  float* part = ws + (rows + 3) / 4 * 4;
  AttnBwdP p;
  p.q = q; p.k = k; p.v[0] = v0; p.v[1] = v1; p.dout[0] = do0; p.dout[1] = v1 ? do1 : nullptr; p.lse = lse; p.delta = delta;
  p.dq = split > 1 ? part : dq; p.dq_split = split > 1 ? rows * C : 0;
  p.dk = dk; p.dv[0] = dv0; p.dv[1] = dv1;
  p.cv[0] = C0; p.cv[1] = C1;
  p.B = B; p.N = N; p.P = P; p.C = C; p.nsplit = split;
  p.ntiles = (int)((NP + FSV_AB_BS - 1) / FSV_AB_BS);
  if (dq || dk)
    FSV_LAUNCH(fsv_attn_bwd_delta_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), stream, o0, do0, v1 ? o1 : nullptr,
               v1 ? do1 : nullptr, delta, rows, C0, C1);
  if (dq) {
    FSV_LAUNCH(fsv_attn_bwd_q_kernel, dim3((P + FSV_AB_BT - 1) / FSV_AB_BT, split, B), dim3(256), stream, p);
    if (split > 1) {
      const long long quads = rows * (C / 4);
      FSV_LAUNCH(fsv_attn_bwd_sum_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), stream, (const float*)part, dq, quads, split);
    }
  }
  const dim3 kgrid((unsigned)((NP + FSV_AB_BT - 1) / FSV_AB_BT), 1, B);
  if (dv0 || dv1) FSV_LAUNCH((fsv_attn_bwd_k_kernel<false>), kgrid, dim3(256), stream, p);
  if (dk) FSV_LAUNCH((fsv_attn_bwd_k_kernel<true>), kgrid, dim3(256), stream, p);
  return fsv_check_launch();
}
