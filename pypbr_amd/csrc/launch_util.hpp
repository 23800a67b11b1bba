// launch_util.hpp -- the small things every launcher of the library shares (included through stream_shape.hpp): the mapping of a HIP
// status to the C ABI's return codes, the pointer-alignment tests of the vector paths (is_aligned, all_aligned, elem_bytes, quad_bytes),
// the device's CU count, the dispatch of a runtime dtype / vector flag to a type / width tag (with_dtype, with_width), and the plane
// accessors of the streaming kernels (map_ops.hip, blend.hip, normal_ops.hip, height_ops.hip): Elem<T>, one element, and
// Span<T, V>, V consecutive ones.  table_launch.hpp, host code only, adds what the launchers that carry a table of entries share.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

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
// ... of every pointer of a list; NULL (a plane that is absent or not wanted) passes
inline bool all_aligned(size_t a, std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!is_aligned(p, a)) return false;
    return true;
}
// bytes of one element of a checked dtype: 4 (PBR_F32) | 2 (PBR_F16)
inline size_t elem_bytes(int dtype) { return dtype == PBR_F32 ? 4 : 2; }
// bytes of four elements, the alignment Span<T, 4> needs: 16 (PBR_F32) | 8 (PBR_F16)
inline size_t quad_bytes(int dtype) { return 4 * elem_bytes(dtype); }

// A launcher names its kernel once, inside a generic lambda: with_dtype hands it the element type of a dtype the entry point has
// checked (PBR_F32 | PBR_F16), with_width the elements per lane of its vector test (4 | 1).
//   with_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type; ... kernel<T> ... });
//   with_width(vec, [&](auto w) { constexpr int V = decltype(w)::value; ... kernel<V> ... });
template <typename T> struct Type { using type = T; };
template <int V> struct Width { static constexpr int value = V; };
template <typename F> inline void with_dtype(int dtype, F &&f) {
    if (dtype == PBR_F32) f(Type<float>{}); else f(Type<__half>{});
}
template <typename F> inline void with_width(bool vec, F &&f) {
    if (vec) f(Width<4>{}); else f(Width<1>{});
}

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

// V consecutive elements of a plane of T at ELEMENT offset i, as fp32.  V = 1 is Elem<T>'s plain access in every form.  V = 4 is one
// 16-byte (fp32) / 8-byte (fp16) access -- the launcher checked the alignment (quad_bytes) -- plain (ld, st) or with the
// non-temporal hint (ld_nt, st_nt): which of the two a kernel uses is that kernel's measured choice.
template <typename T, int V> struct Span {
    static_assert(V == 1 || V == 4, "one element or one quad");
    using S = std::conditional_t<std::is_same<T, float>::value, float, _Float16>;
    typedef S v4 __attribute__((ext_vector_type(4)));
    using unit = std::conditional_t<V == 1, S, v4>;                   // what one access moves
    template <bool NT> static __device__ __forceinline__ void load(const void *p, int64_t i, float v[V]) {
        if constexpr (V == 1) {
            v[0] = Elem<T>::ld(p, i);
        } else {
            const v4 *q = reinterpret_cast<const v4 *>(static_cast<const S *>(p) + i);
            v4 t;
            if constexpr (NT) t = __builtin_nontemporal_load(q); else t = *q;
            v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
        }
    }
    template <bool NT> static __device__ __forceinline__ void store(void *p, int64_t i, const float v[V]) {
        if constexpr (V == 1) {
            Elem<T>::st(p, i, v[0]);
        } else {
            const v4 t = {(S)v[0], (S)v[1], (S)v[2], (S)v[3]};
            v4 *q = reinterpret_cast<v4 *>(static_cast<S *>(p) + i);
            if constexpr (NT) __builtin_nontemporal_store(t, q); else *q = t;
        }
    }
    static __device__ __forceinline__ void ld(const void *p, int64_t i, float v[V]) { load<false>(p, i, v); }
    static __device__ __forceinline__ void ld_nt(const void *p, int64_t i, float v[V]) { load<true>(p, i, v); }
    static __device__ __forceinline__ void st(void *p, int64_t i, const float v[V]) { store<false>(p, i, v); }
    static __device__ __forceinline__ void st_nt(void *p, int64_t i, const float v[V]) { store<true>(p, i, v); }
};

// Where unit u (V elements) of a plane starts, for the kernels that walk a plane in units: Span<T, V>::ld_nt(unit_at<T, V>(p, u), 0, v).
// The same address as element offset u V, formed as ONE index scaled by the unit's size; several kernels of map_ops.hip come out with
// fewer instructions or registers from this form than from the scaled offset (profiles/EXPERIMENTS.md).
template <typename T, int V> __device__ __forceinline__ const void *unit_at(const void *p, size_t u) { return static_cast<const typename Span<T, V>::unit *>(p) + u; }
template <typename T, int V> __device__ __forceinline__ void *unit_at(void *p, size_t u) { return static_cast<typename Span<T, V>::unit *>(p) + u; }

}  // namespace pbr
