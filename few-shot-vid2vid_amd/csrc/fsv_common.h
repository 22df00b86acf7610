// Shared device/host helpers for the fsv2v HIP kernels (gfx950 / CDNA4 only).
//
// Every kernel in this directory is written for 64-wide wavefronts and the gfx950 MFMA lane layouts
// (see /opt/skills/guides/cdna_hip_programming.md section 3).  The only other compilation mode is the CPU
// SIMT emulator used by the `not gpu` tests (tests/emu/hip_emu.h), selected with -DFSV_EMU.
#pragma once
#ifdef FSV_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
// hipGetLastError() is per-thread state shared with everything else in the process (PyTorch's pinned-memory allocator
// leaves hipErrorNotReady there after polling an event): clear it before a launch and record only what the launch
// itself reports, so that fsv_check_launch() speaks for this library's launches alone.
static thread_local int fsv_launch_status = 0;
#define FSV_LAUNCH(kernel, grid, block, stream, ...)                                  \
  do {                                                                                \
    (void)hipGetLastError();                                                          \
    hipLaunchKernelGGL(kernel, (grid), (block), 0, (stream), __VA_ARGS__);            \
    if (hipGetLastError() != hipSuccess) fsv_launch_status = -3;                      \
  } while (0)
#endif
#include <stdint.h>
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// The C ABI itself: status codes (fsv_status), activation codes (fsv_act), descriptor structs and the declaration of every entry
// point.  Each definition in this directory is compiled against its declaration, so a parameter list that drifts from the
// header is a "conflicting types" error.  The definitions spell the stream as hipStream_t.
#define FSV_STREAM_T_DEFINED
typedef hipStream_t fsv_stream_t;
#include "fsv2v.h"

#ifdef FSV_EMU
static inline int fsv_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? FSV_OK : FSV_ERR_LAUNCH;
}
#else
static inline int fsv_check_launch() {        // status of the launches since the previous check (this thread, this file)
  const int s = fsv_launch_status;
  fsv_launch_status = FSV_OK;
  return s;
}
#endif

__device__ __forceinline__ float fsv_act(float v, int act) {
  if (act == FSV_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
  if (act == FSV_ACT_TANH) return tanhf(v);
  if (act == FSV_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
  if (act == FSV_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == FSV_ACT_LRELU01) return v > 0.f ? v : 0.1f * v;
  return v;
}

static inline int fsv_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// The one place the library reads its environment: the numeric value of switch `name`, `dflt` when it is unset.  WHEN a switch is
// read stays with its call site: once per process behind a function-local static, or at every call where tests toggle it at run
// time (FSV_DETERMINISTIC, FSV_CONV_THIN, FSV_SPADE_MAX_GX, FSV_SPLIT_FIN4, FSV_SPLIT_FIN_STATS, FSV_S3_RW).
static inline double fsv_env(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}
