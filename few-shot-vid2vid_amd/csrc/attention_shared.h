// What the streaming few-shot attention kernels share: csrc/attention.hip (exact fp32) defines the two functions below,
// csrc/attention_h.hip (half operands on the f16 matrix cores) calls them, so both walks divide the keys, size the workspace and
// combine their key ranges by the same code - fsv_attn_fused_finish_kernel, in ascending order, no atomics.
#pragma once
#include "fsv_common.h"

#define FSV_AF_BQ 128          // query positions per workgroup (32 per wave)
#define FSV_AF_BK 32           // keys per tile
#define FSV_AF_MAX_SPLIT 8

// the key tiles [t0, t1) of split s
__host__ __device__ static inline int fsv_af_tile0(int s, int nsplit, int ntiles) { return (int)((long long)s * ntiles / nsplit); }

// nsplit (<= 0: the library's choice, a function of the shape alone) and the workspace in floats of a forward walk; C1 = 0: one map.
// FSV_ERR_BAD_ARG: nsplit above FSV_AF_MAX_SPLIT or above the ceil(N P / 32) key tiles
int fsv_af_plan(int B, int N, int P, int C0, int C1, int want_mass, int nsplit, int* split_out, long long* ws_floats);

// the finishing launch over the workspace arrays of a walk (ml [nsplit][B][P][2], mp [nsplit][B][P][N][2] or NULL, po0 / po1
// [nsplit][B][P][Ci]: read when nsplit > 1) -> o0 / o1 (nsplit > 1), mass (non-null), lse (non-null); the status of that launch
int fsv_af_finish(const float* ml, const float* mp, const float* po0, const float* po1, float* o0, float* o1, float* mass, float* lse,
                  int B, int N, int P, int C0, int C1, int nsplit, hipStream_t stream);
