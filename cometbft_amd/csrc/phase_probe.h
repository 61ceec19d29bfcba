// phase_probe.h -- the stamp macros of the helper-wave kernels' phase probes
// (tools/phase_probe.py, row_phase.py, keyed_phase.py). Built only into a
// separate library with -DCMTV_PHASE_PROBE; in the normal build every macro
// here expands to nothing. Lane 0 of every wave of a launch's first
// workgroups records the shader clock at fixed points of its kernel (the
// slots are named at each kernel) into its translation unit's buffer:
// kPhaseSlots words per wave, indexed by (block * waves + wave).
//
// A __device__ array cannot be shared between translation units without
// relocatable device code, so every .hip file that stamps places
// CMTV_PHASE_BUFFER(suffix) at file scope, before its kernels: the buffer and
// its accessor cmtv_debug_phase_times<suffix>(out, n), which copies the first
// n (<= 4096 * 4 * 8) words out after the device has drained.
#pragma once

#ifdef CMTV_PHASE_PROBE
#define CMTV_PHASE_BUFFER(suffix)                                                                          \
  namespace cmtv {                                                                                         \
  constexpr int kPhaseSlots = 8;                                                                           \
  static __device__ uint64_t g_phase[4096 * 4 * kPhaseSlots];                                              \
  }                                                                                                        \
  extern "C" int cmtv_debug_phase_times##suffix(uint64_t* out, size_t n) {                                 \
    const size_t cap = sizeof(cmtv::g_phase) / sizeof(uint64_t);                                           \
    if (n > cap) n = cap;                                                                                  \
    if (hipDeviceSynchronize() != hipSuccess) return -1;                                                   \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(cmtv::g_phase), n * sizeof(uint64_t), 0,                    \
                               hipMemcpyDeviceToHost) == hipSuccess                                        \
               ? 0                                                                                         \
               : -1;                                                                                       \
  }
// val into slot k of this wave, in a launch of `waves`-wave workgroups of
// which the first `cap` record (cap * waves <= 4096 * 4)
#define CMTV_PHASE_PUT(waves, cap, k, val)                                                                 \
  do {                                                                                                     \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < (cap))                                                     \
      g_phase[((size_t)blockIdx.x * (waves) + (threadIdx.x >> 6)) * kPhaseSlots + (k)] = (val);            \
  } while (0)
#define CMTV_CLOCK() __builtin_amdgcn_s_memtime()
#define CMTV_STAMP(k) CMTV_PHASE_PUT(4, 4096, k, CMTV_CLOCK())
// the 100 MHz constant clock, beside the shader clock (row4: slot 7 at entry,
// slot 6 at the lo wave's verdict): the launch's wall time and clock rate
#define CMTV_STAMP_RT(k) CMTV_PHASE_PUT(4, 4096, k, __builtin_amdgcn_s_memrealtime())
// a value of the wave's own (cycles summed over a loop's barriers)
#define CMTV_STAMP_VAL(k, val) CMTV_PHASE_PUT(4, 4096, k, val)
// five-wave workgroups (k_verify_keyed_quad_split, k_verify_quad_hs_fold)
#define CMTV_STAMP5(k) CMTV_PHASE_PUT(5, 3200, k, CMTV_CLOCK())
#define CMTV_STAMP5_VAL(k, val) CMTV_PHASE_PUT(5, 3200, k, val)
// slot 6 of a five-wave workgroup's wave: its HW_ID (bits 5:4 the SIMD, 11:8 the CU)
#define CMTV_HWID5()                                                                                       \
  do {                                                                                                     \
    uint32_t hwid_;                                                                                        \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid_));                                     \
    CMTV_PHASE_PUT(5, 3200, 6, hwid_);                                                                     \
  } while (0)
#else
#define CMTV_PHASE_BUFFER(suffix)
#define CMTV_STAMP(k) ((void)0)
#define CMTV_STAMP_RT(k) ((void)0)
#define CMTV_STAMP_VAL(k, val) ((void)0)
#define CMTV_STAMP5(k) ((void)0)
#define CMTV_STAMP5_VAL(k, val) ((void)0)
#define CMTV_HWID5() ((void)0)
#define CMTV_CLOCK() 0ull
#endif
