// Few-shot attention (reference generator.py:298-316) as ONE streaming kernel: forward only, exact fp32, fixed summation order.
//     e[key][query] = <k[key], q[query]>,  a = softmax over all N P keys of a query,  o = sum_key a[key] v[key]
// The [N P, P] energy / attention matrix never exists: a workgroup owns 128 query positions of one sample (32 per wave), walks the
// key tiles (32 keys) in ascending order and keeps the running maximum, the running denominator and the output accumulators of
// both value maps in registers (online softmax).
//
// How the two GEMMs chain without a trip through LDS (the swapped-operand trick of spade_conv.hip).  The energy tile is computed as
// D[key][query] = v_mfma_f32_32x32x2_f32(K fragment, Q fragment): lane l then owns query (l & 31) and its 16 registers are the keys
// kk(r) = (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, so the softmax statistics of a query are a reduction over one lane's
// registers and one exchange between the half-waves.  Register r of the two half-waves IS the A fragment (row = query, k = l >> 5)
// of a 32x32x2 step of the second GEMM over the key pair (kk(r, 0), kk(r, 1)); its B fragment is row kk(r, l >> 5) of the value
// tile in LDS.  The accumulators of the second GEMM have the query on the REGISTER (row) axis: the per-query rescale factor is
// fetched from the lane that owns the query.
//
// The operands are read where the encoders left them: q [B][P][C], k [B][N P][C], v [B][N P][Cv] (NHWC memory), no K-major copies.
// The Q fragments of a wave stay in registers for the whole launch; K and V tiles go through LDS (zero-filled past the last key and
// past the last channel: a masked key adds exactly nothing), their global loads are issued one tile ahead.
//
// Keys may be split over `nsplit` workgroups per query tile (small P would leave the machine empty); every split writes its
// unnormalised sums, its maximum and its denominator to the caller's workspace and fsv_attn_fused_finish_kernel combines them in
// ascending split order - no atomics, the same bits on every run.  The per-reference masses come from the same walk: the sum of a
// reference's probabilities is kept relative to the running maximum and written, with that maximum, when the walk leaves the
// reference (a key tile may hold several reference boundaries); the finishing pass rescales it to the final maximum.
#include "attention_shared.h"   // FSV_AF_BQ / _BK / _MAX_SPLIT, fsv_af_tile0; fsv_af_plan and fsv_af_finish are defined here

#define FSV_AF_NV 8            // 32-channel output tiles per launch at most (both value maps together)

struct AttnFusedP {
  const float* q;              // [B][P][C]
  const float* k;              // [B][N P][C]
  // the output tiles of a launch: nv[0] 32-channel tiles of one value map from its column col0[0], then nv[1] of a second one
  const float* v[2];           // [B][N P][cv[i]]
  float* o[2];                 // [B][P][cv[i]] (+ split * osplit[i]: the workspace copies when nsplit > 1)
  long long osplit[2];
  int col0[2];
  float* ml;                   // workspace [nsplit][B][P][2]: maximum, denominator (NULL: not wanted)
  float* mp;                   // workspace [nsplit][B][P][N][2]: a reference's partial mass and the maximum it is relative to
  float* lse;                  // [B][P]: maximum + log(denominator), written here when nsplit == 1 and nothing is left to finish
  int cv[2], nv[2];            // channels of the two maps, tiles taken from each (second: 0 when absent)
  int B, N, P, C, ncq, nsplit, ntiles;
};

// PF: the global loads of tile t + 1 are in flight while tile t is computed (their registers live across the matrix work);
// the 256-channel form has no registers left for that: it loads a tile right before it stores it and carries NV = 4 output tiles
template <int CQ, bool PF, int NV>
__global__ __launch_bounds__(256) void fsv_attn_fused_kernel(AttnFusedP p) {
  constexpr int LDK = 32 * CQ + 4;                       // one 16-byte slot of padding: conflict-free b128 fragment reads
  constexpr int KQ = 8 * CQ, KRP = 256 / KQ;             // K staging: KQ quads per key row, KRP rows per pass, CQ passes
  __shared__ __attribute__((aligned(16))) float Ks[FSV_AF_BK * LDK];
  constexpr int LDV = 32 * NV, VQ = 8 * NV, VRP = 256 / VQ, VU = FSV_AF_BK / VRP;      // V staging like K's
  __shared__ __attribute__((aligned(16))) float Vs[FSV_AF_BK * LDV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, split = blockIdx.y;
  const int P = p.P, C = p.C;
  const long long NP = (long long)p.N * P;
  const int query = blockIdx.x * FSV_AF_BQ + wave * 32 + lq;
  const bool wave_live = blockIdx.x * FSV_AF_BQ + wave * 32 < P;
  const int t0 = fsv_af_tile0(split, p.nsplit, p.ntiles), t1 = fsv_af_tile0(split + 1, p.nsplit, p.ntiles);

  // ---- the wave's Q fragments: lane (query, lk) holds channels 32 cq + 8 j + 4 lk + e -------------------------------------------
  float4 qf[CQ][4];
  {
    const float* qrow = p.q + ((long long)b * P + (query < P ? query : 0)) * C;
#pragma unroll
    for (int cq = 0; cq < CQ; ++cq)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 32 * cq + 8 * j + 4 * lk;
        qf[cq][j] = (query < P && c < C) ? *reinterpret_cast<const float4*>(qrow + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }

  // ---- staging: every work-item owns one channel quad of the K rows and one of the V rows it loads -----------------------------
  const float* kbase = p.k + (long long)b * NP * C;
  const int kq4 = (tid % KQ) * 4, kr0 = tid / KQ;
  const bool kcol_ok = kq4 < C;
  const int vq = tid % VQ, vr0 = tid / VQ;
  const int vt = vq >> 3;
  const int vmap = vt < p.nv[0] ? 0 : 1;
  const int vcol = p.col0[vmap] + 32 * (vmap ? vt - p.nv[0] : vt) + (vq & 7) * 4;
  const int vC = p.cv[vmap];
  const bool vcol_ok = vt < p.nv[0] + p.nv[1] && vcol < vC;
  const float* vbase = p.v[vmap] ? p.v[vmap] + (long long)b * NP * vC + vcol : nullptr;
  float4 kreg[CQ], vreg[VU];
  auto issue_loads = [&](int t) {
    const long long key0 = (long long)t * FSV_AF_BK;
#pragma unroll
    for (int u = 0; u < CQ; ++u) {
      const long long key = key0 + kr0 + u * KRP;
      kreg[u] = (kcol_ok && key < NP) ? *reinterpret_cast<const float4*>(kbase + key * C + kq4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const long long key = key0 + vr0 + u * VRP;
      vreg[u] = (vcol_ok && key < NP) ? *reinterpret_cast<const float4*>(vbase + key * vC) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < CQ; ++u) *reinterpret_cast<float4*>(&Ks[(kr0 + u * KRP) * LDK + kq4]) = kreg[u];
#pragma unroll
    for (int u = 0; u < VU; ++u) *reinterpret_cast<float4*>(&Vs[(vr0 + u * VRP) * LDV + vq * 4]) = vreg[u];
  };

  f32x16 acc[NV];
#pragma unroll
  for (int t = 0; t < NV; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  // the mass of the reference the walk is in: its sum so far relative to m_run
  int g_cur = (int)((long long)t0 * FSV_AF_BK / P);
  float mass_cur = 0.f;
  const bool want_mass = p.mp != nullptr;
  const long long row = ((long long)split * p.B + b) * P + query;          // this lane's row of the workspace arrays
  auto flush_mass = [&](int g, float sum, float mx) {
    if (want_mass && lk == 0 && query < P) {
      float* dst = p.mp + (row * p.N + g) * 2;
      dst[0] = sum; dst[1] = mx;
    }
  };
  const int nvt = p.nv[0] + p.nv[1];

  if (PF) issue_loads(t0);
  for (int t = t0; t < t1; ++t) {
    if (!PF) issue_loads(t);
    store_tile();
    __syncthreads();
    if (PF && t + 1 < t1) issue_loads(t + 1);
    if (wave_live) {
      // ---- energies of 32 keys x 32 queries: D[key][query] -----------------------------------------------------------------------
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int cq = 0; cq < CQ; ++cq)
        if (cq < p.ncq) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 kv = *reinterpret_cast<const float4*>(&Ks[lq * LDK + 32 * cq + 8 * j + 4 * lk]);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qf[cq][j].x, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qf[cq][j].y, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, qf[cq][j].z, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, qf[cq][j].w, s, 0, 0, 0);
          }
        }
      // ---- online softmax of the lane's query -------------------------------------------------------------------------------------
      const long long key0 = (long long)t * FSV_AF_BK;
      const int nkeys = (int)(NP - key0 < FSV_AF_BK ? NP - key0 : FSV_AF_BK);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (kk >= nkeys) s[r] = -INFINITY;
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
      // ---- rescale the accumulators (rows = queries: the factor lives in the lane that owns the query) ------------------------------
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lk);
#pragma unroll
        for (int vtile = 0; vtile < NV; ++vtile)
          if (vtile < nvt) acc[vtile][r] *= ar;
      }
      // ---- o += P V: register r of the half-waves is the A fragment over keys (kk(r, 0), kk(r, 1)) ---------------------------------
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vrow = &Vs[((r & 3) + 8 * (r >> 2) + 4 * lk) * LDV + lq];
#pragma unroll
        for (int vtile = 0; vtile < NV; ++vtile)
          if (vtile < nvt) acc[vtile] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[r], vrow[32 * vtile], acc[vtile], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!wave_live) return;
  flush_mass(g_cur, mass_cur, m_run);
  if (p.ml && lk == 0 && query < P) { p.ml[row * 2] = m_run; p.ml[row * 2 + 1] = l_run; }
  if (p.lse && lk == 0 && query < P) p.lse[(long long)b * P + query] = m_run + logf(l_run);

  // ---- epilogue: normalised when this workgroup saw every key, the raw sums otherwise ------------------------------------------------
  const float inv = p.nsplit == 1 ? 1.f / l_run : 1.f;
  const int q_wave = blockIdx.x * FSV_AF_BQ + wave * 32;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * lk;
    const float ir = __shfl(inv, qr);
    if (q_wave + qr >= P) continue;
#pragma unroll
    for (int vtile = 0; vtile < NV; ++vtile) {
      if (vtile >= nvt) continue;
      const int mp = vtile < p.nv[0] ? 0 : 1;
      const int col = p.col0[mp] + 32 * (mp ? vtile - p.nv[0] : vtile) + lq;
      if (col < p.cv[mp])
        (p.o[mp] + split * p.osplit[mp])[((long long)b * P + q_wave + qr) * p.cv[mp] + col] = acc[vtile][r] * ir;
    }
  }
}

struct AttnFinishP {
  const float* ml;             // [nsplit][B][P][2]
  const float* mp;             // [nsplit][B][P][N][2] or NULL
  const float* po[2];          // [nsplit][B][P][cv[i]] (nsplit > 1)
  float* o[2];
  float* mass;                 // [B][P][N] or NULL
  float* lse;                  // [B][P] or NULL: the statistics a backward pass recomputes the probabilities from
  int cv[2];
  int B, N, P, nsplit, ntiles;
  long long rows;              // B P
  int per_row, nq0, nq1;       // work-items per (sample, query): channel quads of the two maps, then the references
};

// one work-item per output channel quad or per reference mass of a (sample, query); the splits in ascending order
__global__ __launch_bounds__(256) void fsv_attn_fused_finish_kernel(AttnFinishP p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.rows * p.per_row) return;
  const long long row = idx / p.per_row;
  const int item = (int)(idx - row * p.per_row);
  float m = -INFINITY;
  for (int s = 0; s < p.nsplit; ++s) m = fmaxf(m, p.ml[(s * p.rows + row) * 2]);
  float w[FSV_AF_MAX_SPLIT];
  float l = 0.f;
#pragma unroll
  for (int s = 0; s < FSV_AF_MAX_SPLIT; ++s) {
    w[s] = 0.f;
    if (s < p.nsplit) {
      w[s] = expf(p.ml[(s * p.rows + row) * 2] - m);
      l += w[s] * p.ml[(s * p.rows + row) * 2 + 1];
    }
  }
  if (p.lse && item == 0) p.lse[row] = m + logf(l);
  if (item < p.nq0 + p.nq1) {
    const int mpi = item < p.nq0 ? 0 : 1;
    const int c = 4 * (mpi ? item - p.nq0 : item);
    const int cv = p.cv[mpi];
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < FSV_AF_MAX_SPLIT; ++s)
      if (s < p.nsplit) {
        const float4 v = *reinterpret_cast<const float4*>(p.po[mpi] + (s * p.rows + row) * cv + c);
        sum.x += w[s] * v.x; sum.y += w[s] * v.y; sum.z += w[s] * v.z; sum.w += w[s] * v.w;
      }
    *reinterpret_cast<float4*>(p.o[mpi] + row * cv + c) = make_float4(sum.x / l, sum.y / l, sum.z / l, sum.w / l);
    return;
  }
  const int g = item - p.nq0 - p.nq1;
  const long long klo = (long long)g * p.P, khi = klo + p.P, NP = (long long)p.N * p.P;
  float sum = 0.f;
  for (int s = 0; s < p.nsplit; ++s) {
    // split s walked the keys [k0, k1): it wrote the mass of reference g only when it met one of g's keys
    const long long k0 = (long long)fsv_af_tile0(s, p.nsplit, p.ntiles) * FSV_AF_BK;
    long long k1 = (long long)fsv_af_tile0(s + 1, p.nsplit, p.ntiles) * FSV_AF_BK;
    if (k1 > NP) k1 = NP;
    if (k0 >= khi || k1 <= klo) continue;
    const float* src = p.mp + ((s * p.rows + row) * p.N + g) * 2;
    sum += src[0] * expf(src[1] - m);
  }
  p.mass[row * p.N + g] = sum / l;
}

int fsv_af_plan(int B, int N, int P, int C0, int C1, int want_mass, int nsplit, int* split_out, long long* ws_floats) {
  const long long NP = (long long)N * P;
  const int ntiles = (int)((NP + FSV_AF_BK - 1) / FSV_AF_BK);
  if (nsplit <= 0) {            // fill 256 compute units: a function of the shape alone
    const long long wgs = (long long)B * ((P + FSV_AF_BQ - 1) / FSV_AF_BQ);
    nsplit = (int)(256 / wgs);
    if (nsplit > FSV_AF_MAX_SPLIT) nsplit = FSV_AF_MAX_SPLIT;
    if (nsplit > ntiles) nsplit = ntiles;
    if (nsplit < 1) nsplit = 1;
  }
  if (nsplit > FSV_AF_MAX_SPLIT || nsplit > ntiles) return FSV_ERR_BAD_ARG;
  const long long rows = (long long)B * P;
  long long ws = 0;
  if (nsplit > 1 || want_mass) ws += 2 * rows * nsplit;
  if (want_mass) ws += 2 * rows * nsplit * N;
  if (nsplit > 1) ws += rows * nsplit * ((long long)C0 + C1);
  *split_out = nsplit;
  *ws_floats = ws;
  return FSV_OK;
}

// the finishing launch and the status of this file's launches since the last check (the half walk of attention_h.hip ends here too)
int fsv_af_finish(const float* ml, const float* mp, const float* po0, const float* po1, float* o0, float* o1, float* mass, float* lse,
                  int B, int N, int P, int C0, int C1, int nsplit, hipStream_t stream) {
  AttnFinishP f;
  f.ml = ml; f.mp = mp; f.po[0] = po0; f.po[1] = po1; f.o[0] = o0; f.o[1] = o1; f.mass = mass; f.lse = lse;
  f.cv[0] = C0; f.cv[1] = C1;
  f.B = B; f.N = N; f.P = P; f.nsplit = nsplit; f.ntiles = (int)(((long long)N * P + FSV_AF_BK - 1) / FSV_AF_BK);
  f.rows = (long long)B * P;
  f.nq0 = nsplit > 1 ? C0 / 4 : 0; f.nq1 = nsplit > 1 ? C1 / 4 : 0;
  f.per_row = f.nq0 + f.nq1 + (mass ? N : 0);
  const long long items = f.rows * f.per_row;
  FSV_LAUNCH(fsv_attn_fused_finish_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), stream, f);
  return fsv_check_launch();
}

static int fsv_af_shape(const void* v1, int B, int N, int P, int C, int C0, int C1) {
  if (B <= 0 || N <= 0 || P <= 0 || C <= 0 || C0 <= 0 || (v1 && C1 <= 0)) return FSV_ERR_BAD_ARG;
  if (!v1) C1 = 0;
  if ((C | C0 | C1) & 3 || C > 256 || C0 > 256 || C1 > 256) return FSV_ERR_UNSUPPORTED;
  if (B > 65535 || (long long)N * P > (1ll << 31) - 64) return FSV_ERR_UNSUPPORTED;
  return FSV_OK;
}

extern "C" int fsv_attention_fused_plan(int B, int N, int P, int C, int C0, int C1, int want_mass, int nsplit, long long* out) {
  if (!out) return FSV_ERR_BAD_ARG;
  const int rc = fsv_af_shape(C1 > 0 ? out : nullptr, B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  int split = 0;
  long long ws = 0;
  const int rc2 = fsv_af_plan(B, N, P, C0, C1 > 0 ? C1 : 0, want_mass, nsplit, &split, &ws);
  if (rc2 != FSV_OK) return rc2;
  out[0] = split; out[1] = ws;
  return FSV_OK;
}

// the one implementation of both forward entry points: lse == NULL is fsv_attention_fused_fwd
static int fsv_af_forward(const float* q, const float* k, const float* v0, const float* v1, float* o0, float* o1, float* mass,
                          float* lse, int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws, long long ws_floats,
                          hipStream_t stream) {
  if (!q || !k || !v0 || !o0 || (v1 && !o1)) return FSV_ERR_BAD_ARG;
  int rc = fsv_af_shape(v1, B, N, P, C, C0, C1);
  if (rc != FSV_OK) return rc;
  if (!v1) C1 = 0;
  int split = 0;
  long long need = 0;
  rc = fsv_af_plan(B, N, P, C0, C1, mass != nullptr, nsplit, &split, &need);
  if (rc != FSV_OK) return rc;
  if (need > 0 && (!ws || ws_floats < need)) return FSV_ERR_BAD_ARG;
  const long long rows = (long long)B * P, NP = (long long)N * P;
  if (rows * ((C0 + C1) / 4 + N) > 256ll * 0x7fffffff) return FSV_ERR_UNSUPPORTED;      // the finishing pass' grid
  // the workspace: the partial sums first (read as 16-byte vectors: C0 and C1 are multiples of 4, so both blocks keep the
  // alignment of ws), then the (maximum, denominator) pairs, then the masses
  float* po0 = ws;
  float* po1 = po0 + (split > 1 ? rows * split * C0 : 0);
  float* ml = need ? po1 + (split > 1 ? rows * split * C1 : 0) : nullptr;
  float* mp = mass ? ml + 2 * rows * split : nullptr;
  const int nv[2] = {(C0 + 31) / 32, (C1 + 31) / 32};
  const float* vs[2] = {v0, v1};
  float* os[2] = {split > 1 ? po0 : o0, split > 1 ? po1 : o1};
  const int cvs[2] = {C0, C1};
  // the 32-channel tiles of both maps, in order, as many per launch as the accumulators hold: both maps in ONE launch up to eight
  // tiles (C <= 128), four per launch for the 256-channel queries
  const int per = C <= 128 ? FSV_AF_NV : 4;
  const int total = nv[0] + nv[1];
  for (int first = 0; first < total; first += per) {
    AttnFusedP p;
    p.q = q; p.k = k;
    p.B = B; p.N = N; p.P = P; p.C = C; p.ncq = (C + 31) / 32; p.nsplit = split;
    p.ntiles = (int)((NP + FSV_AF_BK - 1) / FSV_AF_BK);
    const int last = first + per < total ? first + per : total;
    int seg = 0;
    for (int i = 0; i < 2; ++i) { p.v[i] = nullptr; p.o[i] = nullptr; p.osplit[i] = 0; p.col0[i] = 0; p.cv[i] = 0; p.nv[i] = 0; }
    for (int mpi = 0; mpi < 2; ++mpi) {
      const int lo = mpi ? nv[0] : 0, hi = lo + nv[mpi];
      const int a0 = first > lo ? first : lo, a1 = last < hi ? last : hi;
      if (a0 >= a1) continue;
      p.v[seg] = vs[mpi]; p.o[seg] = os[mpi]; p.osplit[seg] = split > 1 ? rows * cvs[mpi] : 0;
      p.col0[seg] = 32 * (a0 - lo); p.cv[seg] = cvs[mpi]; p.nv[seg] = a1 - a0;
      ++seg;
    }
    p.ml = first ? nullptr : ml;                       // (a later walk repeats the first one's statistics bit for bit)
    p.mp = first ? nullptr : mp;
    p.lse = (first || split > 1 || mass) ? nullptr : lse;      // (otherwise the finishing pass writes it)
    const dim3 grid((P + FSV_AF_BQ - 1) / FSV_AF_BQ, split, B);
    if (C <= 128) FSV_LAUNCH((fsv_attn_fused_kernel<4, true, FSV_AF_NV>), grid, dim3(256), stream, p);
    else FSV_LAUNCH((fsv_attn_fused_kernel<8, false, 4>), grid, dim3(256), stream, p);
  }
  if (split > 1 || mass) return fsv_af_finish(ml, mp, po0, po1, o0, o1, mass, lse, B, N, P, C0, C1, split, stream);
  return fsv_check_launch();
}

extern "C" int fsv_attention_fused_fwd(const float* q, const float* k, const float* v0, const float* v1, float* o0, float* o1,
                                       float* mass, int B, int N, int P, int C, int C0, int C1, int nsplit, float* ws,
                                       long long ws_floats, hipStream_t stream) {
  return fsv_af_forward(q, k, v0, v1, o0, o1, mass, nullptr, B, N, P, C, C0, C1, nsplit, ws, ws_floats, stream);
}

extern "C" int fsv_attention_fused_fwd_lse(const float* q, const float* k, const float* v0, const float* v1, float* o0, float* o1,
                                           float* mass, float* lse, int B, int N, int P, int C, int C0, int C1, int nsplit,
                                           float* ws, long long ws_floats, hipStream_t stream) {
  return fsv_af_forward(q, k, v0, v1, o0, o1, mass, lse, B, N, P, C, C0, C1, nsplit, ws, ws_floats, stream);
}
