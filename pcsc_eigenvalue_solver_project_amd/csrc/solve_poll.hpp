// Device-coherent loads and stores of the solve kernels that poll each other's results through memory: the
// triangular solve's value flags (sptrsv.hip) and the dense block-row substitution (dense_lu.hip).
#pragma once

#include "kernels_common.hpp"

namespace eigsol {
namespace dev {

__device__ __forceinline__ void st_coh(double* p, double v) { st_agent(p, v); }
__device__ __forceinline__ void st_coh(cplx* p, cplx v) {
    st_agent(&p->re, v.re);
    st_agent(&p->im, v.im);
}
__device__ __forceinline__ void st_coh(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_coh(cplxf* p, cplxf v) {
    st_coh(&p->re, v.re);
    st_coh(&p->im, v.im);
}
__device__ __forceinline__ float ld_coh(const float* p) {
    return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ cplxf ld_coh(const cplxf* p) { return cplxf{ld_coh(&p->re), ld_coh(&p->im)}; }
__device__ __forceinline__ double ld_coh(const double* p) { return ld_agent(p); }
__device__ __forceinline__ cplx ld_coh(const cplx* p) { return cplx{ld_agent(&p->re), ld_agent(&p->im)}; }

// Indexed coherent access to a solve buffer (uniform base, element index): complex values move as
// ONE device-coherent (sc1) buffer load / store of 16 (8) bytes instead of two 8 (4) byte atomics,
// which halves the dependency polls' memory requests.  A torn read (one half still the sentinel)
// is simply unready: both halves are checked.  Buffer offsets are 32-bit (solve buffers < 4 GiB).
constexpr int kBufSc1 = 16;   // buffer cache policy: sc1 (device scope), as the agent-scope atomics use
__device__ __forceinline__ __amdgpu_buffer_rsrc_t coh_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1, 0x00020000);
}
template <class S>
__device__ __forceinline__ S ld_cohi(const S* base, int j) {
    if constexpr (std::is_same_v<S, cplx>) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(coh_rsrc(base), (uint32_t)j * 16u, 0, kBufSc1);
        return __builtin_bit_cast(cplx, v);
    } else if constexpr (std::is_same_v<S, cplxf>) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(coh_rsrc(base), (uint32_t)j * 8u, 0, kBufSc1);
        return __builtin_bit_cast(cplxf, v);
    } else {
        return ld_coh(base + j);
    }
}
template <class S>
__device__ __forceinline__ void st_cohi(S* base, int i, S v) {
    if constexpr (std::is_same_v<S, cplx>) {
        typedef unsigned int u4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), coh_rsrc(base), (uint32_t)i * 16u, 0,
                                               kBufSc1);
    } else if constexpr (std::is_same_v<S, cplxf>) {
        typedef unsigned int u2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), coh_rsrc(base), (uint32_t)i * 8u, 0,
                                              kBufSc1);
    } else {
        st_coh(base + i, v);
    }
}

}  // namespace dev
}  // namespace eigsol
