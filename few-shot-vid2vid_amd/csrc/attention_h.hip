// Streaming few-shot attention (attention.hip) on the f16 matrix cores - v_mfma_f32_32x32x16_f16 - for INFERENCE: forward only,
// opt-in (FSV_ATTN_FUSED_HALF, InferenceSession(fused_attention='half')), no part of training or of the --amp definition.
//
// The arithmetic.  h(x) is round-to-nearest-even to IEEE half.
//   split     for q and k: xh = h(x), xl = h((x - xh) * 2^11).  The remainder is exact in fp32; the power-of-two scale keeps the low
//             part in half's normal range whenever the high part is.
//   energy    e = S_hh + 2^-11 * (S_hl + S_lh),  S_hh = sum_c kh qh,  S_hl + S_lh = sum_c (kh ql + kl qh): each an fp32 MFMA
//             accumulation of exact products, the cross terms in an accumulator tile of their own.  The kl ql term is dropped.
//             About 22 bits: the reference does not scale the energies by 1 / sqrt(c), they reach the hundreds, and an operand
//             error of 2^-11 in the exponent would be a per-cent error in the probabilities.
//   softmax   online, as attention.hip, fp32 throughout: running maximum m, p = expf(e - m), denominator l = sum p.  The
//             denominator and the per-reference masses come from the UNROUNDED p.
//   values    o = (sum_key h(p) h(v)) / l, accumulated in fp32 by the MFMA: here the error stays linear, so plain half is spent.
//   order     keys in ascending order, key ranges combined by attention.hip's finishing launch in ascending order, no atomics: the
//             same bits on every run.
//   range     operands must be finite and below 65504 in magnitude: a larger value becomes inf in h() and is the caller's error.
//
// fsv_attention_half_prep, once per reference set: k fp32 [B][N P][C] -> the planes kh, kl [B][NPs][C]; v_i fp32 [B][N P][Ci] ->
// half v_it [B][Ci][NPs], key-contiguous (the transpose goes through LDS tiles); NPs = N P rounded up to 32, the tail zero-filled,
// so the walk loads whole key tiles without a bounds test and a masked key adds exactly nothing.
//
// The walk keeps attention.hip's structure: a workgroup owns 128 queries of one sample (32 per wave), q is read as fp32 where the
// query encoder left it and split into registers once.  The energy tile is D[key][query] = MFMA(K fragment, Q fragment): lane l owns
// query (l & 31), its 16 registers are the keys (r & 3) + 8 (r >> 2) + 4 (l >> 5), so a query's statistics are one lane's registers
// and one __shfl_xor(.., 32).  The value product is D[channel][query] = MFMA(V^T fragment, P fragment): registers 8 t .. 8 t + 7 of
// a lane, rounded to half, ARE its B operand of the 16-key step t - over the keys 16 t + {0..3, 8..11} + 4 (l >> 5), so the V^T tile
// is stored to LDS in that key permutation and its A operand is one 16-byte read.  The output accumulators have the query on the
// lane: the rescale factor is the lane's own, and the epilogue stores four consecutive channels of its query at a time.
#include "attention_shared.h"

typedef _Float16 fsv_ah;
typedef _Float16 fsv_ah8 __attribute__((ext_vector_type(8)));
typedef _Float16 fsv_ah4 __attribute__((ext_vector_type(4)));

#define FSV_AH_CMAX 128        // channels of q / k and of each value map at most
#define FSV_AH_NCS 8           // 16-channel MFMA steps of the energy product at most
#define FSV_AH_NV 8            // 32-channel output tiles at most (both value maps together)
#define FSV_AH_LDK 136         // halves per key row of a K plane in LDS: 128 + one 16-byte slot (conflict-free b128 fragment reads)
#define FSV_AH_LDV 40          // halves per channel row of the V^T tile in LDS: 32 keys + one 16-byte slot

static inline long long fsv_ah_nps(int N, int P) { return ((long long)N * P + 31) / 32 * 32; }

// ---- the split of one fp32 value ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fsv_ah_split(float x, fsv_ah& hi, fsv_ah& lo) {
  hi = (fsv_ah)x;
  lo = (fsv_ah)((x - (float)hi) * 2048.f);
}

// A value that is the same in every lane of a wave (kernel arguments, blockIdx and the wave's index only) but that the compiler
// would keep in vector registers: pinned into scalar registers (the precedent is spade_conv3.hip's fsv_s3_uniform)
#ifdef FSV_EMU
template <typename T> static inline T* fsv_ah_uniform(T* q) { return q; }
static inline int fsv_ah_uniform_int(int v) { return v; }
#else
template <typename T> __device__ __forceinline__ T* fsv_ah_uniform(T* q) {
  const unsigned long long a = (unsigned long long)q;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return (T*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int fsv_ah_uniform_int(int v) { return __builtin_amdgcn_readfirstlane(v); }
#endif

// ---- prep: blockIdx.y = 0 splits 32 key rows of k; 1 + t transposes the 32-key x 32-channel tile t of v0, then of v1 --------------
struct AttnHalfPrepP {
  const float* k;              // [B][NP][C]
  const float* v[2];           // [B][NP][cv[i]]
  fsv_ah *kh, *kl;             // [B][NPs][C]
  fsv_ah* vt[2];               // [B][cv[i]][NPs]
  int cv[2], nv[2];
  int C;
  long long NP, NPs;
};

__global__ __launch_bounds__(256) void fsv_attn_half_prep_kernel(AttnHalfPrepP p) {
  __shared__ float tile[32 * 33];
  const int tid = threadIdx.x, b = blockIdx.z;
  const long long key0 = (long long)blockIdx.x * 32;
  if (blockIdx.y == 0) {
    const int cq = p.C / 4;                                  // channel quads per key row
    for (int i = tid; i < 32 * cq; i += 256) {
      const long long key = key0 + i / cq;
      const int c = 4 * (i % cq);
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (key < p.NP) x = *reinterpret_cast<const float4*>(p.k + ((long long)b * p.NP + key) * p.C + c);
      fsv_ah4 hi, lo;
      fsv_ah a, d;
      fsv_ah_split(x.x, a, d); hi[0] = a; lo[0] = d;
      fsv_ah_split(x.y, a, d); hi[1] = a; lo[1] = d;
      fsv_ah_split(x.z, a, d); hi[2] = a; lo[2] = d;
      fsv_ah_split(x.w, a, d); hi[3] = a; lo[3] = d;
      const long long dst = ((long long)b * p.NPs + key) * p.C + c;
      *reinterpret_cast<fsv_ah4*>(p.kh + dst) = hi;
      *reinterpret_cast<fsv_ah4*>(p.kl + dst) = lo;
    }
    return;
  }
  int t = blockIdx.y - 1;
  const int mp = t < p.nv[0] ? 0 : 1;
  if (mp) t -= p.nv[0];
  const int cv = p.cv[mp], c0 = 32 * t;
  {
    const long long key = key0 + (tid >> 3);
    const int c = c0 + 4 * (tid & 7);
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (key < p.NP && c < cv) x = *reinterpret_cast<const float4*>(p.v[mp] + ((long long)b * p.NP + key) * cv + c);
    float* dst = &tile[(4 * (tid & 7)) * 33 + (tid >> 3)];
    dst[0] = x.x; dst[33] = x.y; dst[66] = x.z; dst[99] = x.w;
  }
  __syncthreads();
  {
    const int c = tid >> 3, k4 = 4 * (tid & 7);
    if (c0 + c < cv) {
      fsv_ah4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = (fsv_ah)tile[c * 33 + k4 + e];
      *reinterpret_cast<fsv_ah4*>(p.vt[mp] + ((long long)b * cv + c0 + c) * p.NPs + key0 + k4) = h;
    }
  }
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
struct AttnHalfP {
  const float* q;              // [B][P][C]
  const fsv_ah *kh, *kl;       // [B][NPs][C]
  const fsv_ah* vt[2];         // [B][cv[i]][NPs]
  float* o[2];                 // [B][P][cv[i]] (+ split * osplit[i]: the workspace copies when nsplit > 1)
  long long osplit[2];
  float* ml;                   // workspace [nsplit][B][P][2]: maximum, denominator (NULL: not wanted)
  float* mp;                   // workspace [nsplit][B][P][N][2]: a reference's partial mass and the maximum it is relative to
  int cv[2], nv[2];            // channels of the two maps, 32-channel tiles of each (second: 0 when absent)
  int B, N, P, C, ncs, nsplit, ntiles;
  long long NPs;
};

__global__ __launch_bounds__(256) void fsv_attn_fused_h_kernel(AttnHalfP p) {
  __shared__ __attribute__((aligned(16))) fsv_ah Kh[FSV_AF_BK * FSV_AH_LDK];
  __shared__ __attribute__((aligned(16))) fsv_ah Kl[FSV_AF_BK * FSV_AH_LDK];
  __shared__ __attribute__((aligned(16))) fsv_ah Vs[32 * FSV_AH_NV * FSV_AH_LDV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, split = blockIdx.y;
  const int P = p.P, C = p.C;
  const long long NP = (long long)p.N * P, NPs = p.NPs;
  const int query = blockIdx.x * FSV_AF_BQ + wave * 32 + lq;
  const bool wave_live = blockIdx.x * FSV_AF_BQ + wave * 32 < P;
  const int t0 = fsv_af_tile0(split, p.nsplit, p.ntiles), t1 = fsv_af_tile0(split + 1, p.nsplit, p.ntiles);
  const int nvt = p.nv[0] + p.nv[1];

  // the K planes are zeroed once: the channels between C and the end of its last 16-channel step are read and never loaded
  for (int i = tid; i < FSV_AF_BK * FSV_AH_LDK / 8; i += 256) {
    fsv_ah8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (fsv_ah)0.f;
    reinterpret_cast<fsv_ah8*>(Kh)[i] = z;
    reinterpret_cast<fsv_ah8*>(Kl)[i] = z;
  }

  // ---- the wave's Q fragments: lane (query, lk) holds channels 16 cs + 8 lk + e, split into high and low halves -------------------
  fsv_ah8 qh[FSV_AH_NCS], ql[FSV_AH_NCS];
  {
    const float* qrow = p.q + ((long long)b * P + (query < P ? query : 0)) * C;
#pragma unroll
    for (int cs = 0; cs < FSV_AH_NCS; ++cs) {
      const int c = 16 * cs + 8 * lk;
      float x[8];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 v = (query < P && c + 4 * j < C) ? *reinterpret_cast<const float4*>(qrow + c + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        fsv_ah a, d;
        fsv_ah_split(x[e], a, d);
        qh[cs][e] = a; ql[cs][e] = d;
      }
    }
  }

  // ---- staging: 16-byte pieces.  A K tile is 32 key rows of C / 8 pieces of each plane; a work-item owns pieces (tid & 7) and
  // (tid & 7) + 8 of key row tid >> 3.  The V^T tile is 32 keys (four pieces) of every channel row; a work-item owns piece (tid & 3) of the rows
  // (tid >> 2) + 64 u ------------------------------------------------------------------------------------------------------------------
  const int kpr = C >> 3;                                     // pieces per key row
  const fsv_ah* khb = p.kh + (long long)b * NPs * C;
  const fsv_ah* klb = p.kl + (long long)b * NPs * C;
  const int krow = tid >> 3, kpiece = tid & 7;                // pieces kpiece and kpiece + 8 of key row krow
  const int ksrc = krow * C + 8 * kpiece, kdst = krow * FSV_AH_LDK + 8 * kpiece;
  // Row (tid >> 2) + 64 u is row vrow of the 32-channel tile 2 u + (tid >> 7) of both maps: the tile, hence the map, its base
  // address and the number of its rows that exist, are the same in every lane of a wave and are pinned into scalar registers
  const int vpiece = tid & 3, vrow = (tid >> 2) & 31;
  const long long voff = (long long)vrow * NPs + 8 * vpiece;
  const fsv_ah* vbase[4];
  int vrows[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int vtile = 2 * u + (tid >> 7);
    const int mpi = (vtile < p.nv[0] || vtile >= nvt) ? 0 : 1;          // (a tile past the last one: no rows, never loaded)
    const int c0 = 32 * (mpi ? vtile - p.nv[0] : vtile);
    vbase[u] = fsv_ah_uniform(p.vt[mpi] + ((long long)b * p.cv[mpi] + c0) * NPs);
    vrows[u] = fsv_ah_uniform_int(vtile < nvt ? p.cv[mpi] - c0 : 0);
  }
  // keys 8 vpiece .. + 7 of the row: the 16-key step vpiece >> 1, local keys 8 (vpiece & 1) + {0..3} (operand of lk = 0, elements
  // 4 (vpiece & 1) + {0..3}) and + {4..7} (the same elements of lk = 1)
  const int vdst = 16 * (vpiece >> 1) + 4 * (vpiece & 1);
  fsv_ah8 khreg[2], klreg[2], vreg[4];
  auto issue_loads = [&](int t) {
    const long long key0 = (long long)t * FSV_AF_BK;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (kpiece + 8 * u < kpr) {
        khreg[u] = *reinterpret_cast<const fsv_ah8*>(khb + key0 * C + ksrc + 64 * u);
        klreg[u] = *reinterpret_cast<const fsv_ah8*>(klb + key0 * C + ksrc + 64 * u);
      }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (vrow < vrows[u]) {
        vreg[u] = *reinterpret_cast<const fsv_ah8*>(vbase[u] + voff + key0);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) vreg[u][e] = (fsv_ah)0.f;
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (kpiece + 8 * u < kpr) {
        *reinterpret_cast<fsv_ah8*>(&Kh[kdst + 64 * u]) = khreg[u];
        *reinterpret_cast<fsv_ah8*>(&Kl[kdst + 64 * u]) = klreg[u];
      }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fsv_ah* dst = &Vs[((tid >> 2) + 64 * u) * FSV_AH_LDV + vdst];
      *reinterpret_cast<fsv_ah4*>(dst) = vreg[u].lo;
      *reinterpret_cast<fsv_ah4*>(dst + 8) = vreg[u].hi;
    }
  };

  f32x16 acc[FSV_AH_NV];
#pragma unroll
  for (int t = 0; t < FSV_AH_NV; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  // the mass of the reference the walk is in: its sum so far relative to m_run
  int g_cur = (int)((long long)t0 * FSV_AF_BK / P);
  float mass_cur = 0.f;
  const bool want_mass = p.mp != nullptr;
  const long long row0 = ((long long)split * p.B + b) * P;                 // row0 + query: this lane's row of the workspace arrays
  auto flush_mass = [&](int g, float sum, float mx) {
    if (want_mass && lk == 0 && query < P) {
      float* dst = p.mp + ((row0 + query) * p.N + g) * 2;
      dst[0] = sum; dst[1] = mx;
    }
  };

  issue_loads(t0);
  __syncthreads();                                                          // (the zeroed K planes)
  for (int t = t0; t < t1; ++t) {
    store_tile();
    __syncthreads();
    if (t + 1 < t1) issue_loads(t + 1);
    if (wave_live) {
      // ---- energies of 32 keys x 32 queries: D[key][query], the high product and the two cross products ------------------------------
      f32x16 s, x;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; x[r] = 0.f; }
#pragma unroll
      for (int cs = 0; cs < FSV_AH_NCS; ++cs)
        if (cs < p.ncs) {
          const fsv_ah8 ah = *reinterpret_cast<const fsv_ah8*>(&Kh[lq * FSV_AH_LDK + 16 * cs + 8 * lk]);
          const fsv_ah8 al = *reinterpret_cast<const fsv_ah8*>(&Kl[lq * FSV_AH_LDK + 16 * cs + 8 * lk]);
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, qh[cs], s, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ql[cs], x, 0, 0, 0);
          x = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qh[cs], x, 0, 0, 0);
        }
      // ---- online softmax of the lane's query -------------------------------------------------------------------------------------
      const long long key0 = (long long)t * FSV_AF_BK;
      const int nkeys = (int)(NP - key0 < FSV_AF_BK ? NP - key0 : FSV_AF_BK);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = (r & 3) + 8 * (r >> 2) + 4 * lk;
        s[r] = kk < nkeys ? s[r] + 0.00048828125f * x[r] : -INFINITY;
        mx = fmaxf(mx, s[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);                      // finite: every tile holds at least one key
      const float alpha = expf(m_run - m_new);                   // (first tile: exp(-inf) = 0)
      const int g_lo = (int)(key0 / P), g_hi = (int)((key0 + nkeys - 1) / P);
      if (g_lo != g_cur) { flush_mass(g_cur, mass_cur, m_run); g_cur = g_lo; mass_cur = 0.f; }
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = expf(s[r] - m_new); sum += s[r]; }
      sum += __shfl_xor(sum, 32);
      l_run = l_run * alpha + sum;
      mass_cur *= alpha;
      m_run = m_new;
      if (g_lo == g_hi) mass_cur += sum;
      else {
        for (int g = g_lo; g <= g_hi; ++g) {                     // reference boundaries inside the tile
          const long long lo = (long long)g * P - key0, hi = lo + P;
          float part = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kk = (r & 3) + 8 * (r >> 2) + 4 * lk;
            part += (kk >= lo && kk < hi) ? s[r] : 0.f;
          }
          part += __shfl_xor(part, 32);
          if (g != g_cur) { flush_mass(g_cur, mass_cur, m_run); g_cur = g; mass_cur = 0.f; }
          mass_cur += part;
        }
      }
      // ---- rescale the accumulators: the query is the lane's own (a factor of exactly 1 changes no bit) ----------------------------
      if (alpha != 1.f) {
#pragma unroll
        for (int vtile = 0; vtile < FSV_AH_NV; ++vtile)
          if (vtile < nvt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[vtile][r] *= alpha;
          }
      }
      // ---- o^T += V^T P: registers 8 st .. 8 st + 7, rounded to half, are the B operand of the 16-key step st ------------------------
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        fsv_ah8 ph;
#pragma unroll
        for (int e = 0; e < 8; ++e) ph[e] = (fsv_ah)s[8 * st + e];
#pragma unroll
        for (int vtile = 0; vtile < FSV_AH_NV; ++vtile)
          if (vtile < nvt) {
            const fsv_ah8 av = *reinterpret_cast<const fsv_ah8*>(&Vs[(32 * vtile + lq) * FSV_AH_LDV + 16 * st + 8 * lk]);
            acc[vtile] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, ph, acc[vtile], 0, 0, 0);
          }
      }
    }
    __syncthreads();
  }
  if (!wave_live) return;
  flush_mass(g_cur, mass_cur, m_run);
  if (p.ml && lk == 0 && query < P) { p.ml[(row0 + query) * 2] = m_run; p.ml[(row0 + query) * 2 + 1] = l_run; }
  if (query >= P) return;

  // ---- epilogue: normalised when this workgroup saw every key, the raw sums otherwise; register quad j of tile vtile is the
  // channels 32 vtile + 8 j + 4 lk + {0..3} of the lane's query -----------------------------------------------------------------------
  const float inv = p.nsplit == 1 ? 1.f / l_run : 1.f;
#pragma unroll
  for (int vtile = 0; vtile < FSV_AH_NV; ++vtile) {
    if (vtile >= nvt) continue;
    const int mpi = vtile < p.nv[0] ? 0 : 1;
    float* orow = p.o[mpi] + split * p.osplit[mpi] + ((long long)b * P + query) * p.cv[mpi];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = 32 * (mpi ? vtile - p.nv[0] : vtile) + 8 * j + 4 * lk;
      if (col < p.cv[mpi])
        *reinterpret_cast<float4*>(orow + col) = make_float4(acc[vtile][4 * j] * inv, acc[vtile][4 * j + 1] * inv,
                                                             acc[vtile][4 * j + 2] * inv, acc[vtile][4 * j + 3] * inv);
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
static int fsv_ah_shape(const void* v1, int B, int N, int P, int C, int C0, int C1) {
  if (B <= 0 || N <= 0 || P <= 0 || C <= 0 || C0 <= 0 || (v1 && C1 <= 0)) return FSV_ERR_BAD_ARG;
  if (!v1) C1 = 0;
  if ((C | C0 | C1) & 7 || C > FSV_AH_CMAX || C0 > FSV_AH_CMAX || C1 > FSV_AH_CMAX) return FSV_ERR_UNSUPPORTED;
  if (B > 65535 || (long long)N * P > (1ll << 31) - 64) return FSV_ERR_UNSUPPORTED;
  return FSV_OK;
}

extern "C" int fsv_attention_fused_h_plan(int B, int N, int P, int C, int C0, int C1, int want_mass, int nsplit, long long* out) {
  if (!out) return FSV_ERR_BAD_ARG;
  const int rc = fsv_ah_shape(C1 > 0 ? out : nullptr, B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  int split = 0;
  long long ws = 0;
  const int rc2 = fsv_af_plan(B, N, P, C0, C1 > 0 ? C1 : 0, want_mass, nsplit, &split, &ws);
  if (rc2 != FSV_OK) return rc2;
  out[0] = split; out[1] = ws; out[2] = fsv_ah_nps(N, P);
  return FSV_OK;
}

extern "C" int fsv_attention_half_prep(const float* k, const float* v0, const float* v1, void* kh, void* kl, void* v0t, void* v1t,
                                       int B, int N, int P, int C, int C0, int C1, hipStream_t stream) {
  if (!k || !v0 || !kh || !kl || !v0t || (v1 && !v1t)) return FSV_ERR_BAD_ARG;
  const int rc = fsv_ah_shape(v1, B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  if (!v1) C1 = 0;
  AttnHalfPrepP p;
  p.k = k; p.v[0] = v0; p.v[1] = v1;
  p.kh = (fsv_ah*)kh; p.kl = (fsv_ah*)kl; p.vt[0] = (fsv_ah*)v0t; p.vt[1] = (fsv_ah*)v1t;
  p.cv[0] = C0; p.cv[1] = C1; p.nv[0] = (C0 + 31) / 32; p.nv[1] = (C1 + 31) / 32;
  p.C = C; p.NP = (long long)N * P; p.NPs = fsv_ah_nps(N, P);
  FSV_LAUNCH(fsv_attn_half_prep_kernel, dim3((unsigned)(p.NPs / 32), 1 + p.nv[0] + p.nv[1], B), dim3(256), stream, p);
  return fsv_check_launch();
}

extern "C" int fsv_attention_fused_fwd_h(const float* q, const void* kh, const void* kl, const void* v0t, const void* v1t, float* o0,
                                         float* o1, float* mass, int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws,
                                         long long ws_floats, hipStream_t stream) {
  if (!q || !kh || !kl || !v0t || !o0 || (v1t && !o1)) return FSV_ERR_BAD_ARG;
  int rc = fsv_ah_shape(v1t, B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  if (!v1t) C1 = 0;
  int split = 0;
  long long need = 0;
  rc = fsv_af_plan(B, N, P, C0, C1, mass != nullptr, nsplit, &split, &need);
  if (rc != FSV_OK) return rc;
  if (need > 0 && (!ws || ws_floats < need)) return FSV_ERR_BAD_ARG;
  const long long rows = (long long)B * P, NP = (long long)N * P;
  if (rows * ((C0 + C1) / 4 + N) > 256ll * 0x7fffffff) return FSV_ERR_UNSUPPORTED;      // the finishing pass' grid
  // the workspace of attention.hip: the partial sums, then the (maximum, denominator) pairs, then the masses
  float* po0 = ws;
  float* po1 = po0 + (split > 1 ? rows * split * C0 : 0);
  float* ml = need ? po1 + (split > 1 ? rows * split * C1 : 0) : nullptr;
  float* mp = mass ? ml + 2 * rows * split : nullptr;
  AttnHalfP p;
  p.q = q; p.kh = (const fsv_ah*)kh; p.kl = (const fsv_ah*)kl; p.vt[0] = (const fsv_ah*)v0t; p.vt[1] = (const fsv_ah*)v1t;
  p.o[0] = split > 1 ? po0 : o0; p.o[1] = split > 1 ? po1 : o1;
  p.osplit[0] = split > 1 ? rows * C0 : 0; p.osplit[1] = split > 1 ? rows * C1 : 0;
  p.ml = ml; p.mp = mp;
  p.cv[0] = C0; p.cv[1] = C1; p.nv[0] = (C0 + 31) / 32; p.nv[1] = (C1 + 31) / 32;
  p.B = B; p.N = N; p.P = P; p.C = C; p.ncs = (C + 15) / 16; p.nsplit = split;
  p.ntiles = (int)((NP + FSV_AF_BK - 1) / FSV_AF_BK);
  p.NPs = fsv_ah_nps(N, P);
  FSV_LAUNCH(fsv_attn_fused_h_kernel, dim3((P + FSV_AF_BQ - 1) / FSV_AF_BQ, split, B), dim3(256), stream, p);
  rc = fsv_check_launch();
  if (rc != FSV_OK) return rc;
  if (split > 1 || mass) return fsv_af_finish(ml, mp, po0, po1, o0, o1, mass, nullptr, B, N, P, C0, C1, split, stream);
  return FSV_OK;
}
