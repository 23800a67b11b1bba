// launch_util.hpp -- the small things every launcher of the library shares (included through stream_shape.hpp): the mapping of a HIP
// status to the C ABI's return codes, the pointer-alignment test of the vector paths, the device's CU count, and the one-element
// accessors Elem<T> of the streaming kernels (map_ops.hip, normal_ops.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pbr_hip.h"

namespace pbr {

// The C ABI's return code of a HIP status: PBR_OK, or 1000 + the hipError_t (include/pbr_hip.h).
inline int hip_code(hipError_t e) { return e == hipSuccess ? PBR_OK : 1000 + (int)e; }
// ... of the launches since the last query.
inline int launch_status() { return hip_code(hipGetLastError()); }
// ... of a runtime call that returns its own status (hipMemsetAsync, hipEventCreate): a failure is reported from that status, never as
// PBR_OK, and the runtime's record of it is cleared so that the next launcher's launch_status() does not find it.
inline int call_status(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
    return hip_code(e);
}

inline bool is_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }      // a: a power of two

// CUs of the current device, for the launches sized to what the chip holds at once (the streamed backward and loss kernels); 256,
// the MI355X's, when the query fails.
inline int resident_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    return cus;
}

// One element of a plane of T (float | __half) as fp32.
template <typename T> struct Elem;
template <> struct Elem<float> {
    static __device__ __forceinline__ float ld(const void *p, int64_t i) { return static_cast<const float *>(p)[i]; }
    static __device__ __forceinline__ void st(void *p, int64_t i, float v) { static_cast<float *>(p)[i] = v; }
};
template <> struct Elem<__half> {
    static __device__ __forceinline__ float ld(const void *p, int64_t i) { return (float)static_cast<const _Float16 *>(p)[i]; }
    static __device__ __forceinline__ void st(void *p, int64_t i, float v) { static_cast<_Float16 *>(p)[i] = (_Float16)v; }
};

}  // namespace pbr
