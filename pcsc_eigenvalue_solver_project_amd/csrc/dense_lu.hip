// The dense partial-pivot LU of the shifted-solve family on gfx950 (Matrix::Dense, small non-triangular sparse
// matrices densified on the device, and the GMRES family's fallback): right-looking blocked LU (panels of 64 real /
// 32 complex columns, trailing update on the matrix cores; Eigen's PartialPivLU is blocked too), built for every
// scalar (single precision factors and solves in float, rank-NB updates on v_mfma_f32_16x16x4_f32), then per
// iteration a single-workgroup forward / back substitution with the vector in LDS, or from n > 64 a block-row
// substitution across the CUs.
//
// This file holds the factor kernels (lu_*), densify_kernel and shift_diag_kernel, the substitution kernels with
// their argument structs (DenseSolveArgs, DenseTriArgs) and the inverse / condition / premultiply kernels of the
// diagonal blocks, the factorisation (dense_lu_factor, dense_from_matrix, dense_from_csr) and the launch
// (dense_launch).  The factor object (DenseFactor) is in shift_factor.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "dense_lu.hpp"
#include "gemm.hpp"
#include "mfma_rankk.hpp"
#include "scratch.hpp"
#include "shift_factor.hpp"
#include "solve_poll.hpp"

namespace eigsol {
namespace dev {

// ------------------------------------------------------------------ dense LU (factor once)
__device__ __forceinline__ double score(double v) { return fabs(v); }
__device__ __forceinline__ double score(cplx v) { return hypot(v.re, v.im); }
__device__ __forceinline__ double score(float v) { return fabs((double)v); }
__device__ __forceinline__ double score(cplxf v) { return hypot((double)v.re, (double)v.im); }

// Column k: pivot = first row of largest modulus in rows k..n-1, swap full rows, record the
// transposition, scale the subdiagonal column by the pivot (skipped for a zero pivot, as Eigen's
// partial_lu_impl does; the first zero pivot is recorded).
template <class S>
__global__ __launch_bounds__(1024) void lu_pivot_kernel(S* a, int64_t n, int64_t k, int64_t c0, int64_t c1,
                                                        int32_t* piv, int32_t* zero_pivot) {
    __shared__ double sv[1024];
    __shared__ int si[1024];
    __shared__ int s_p;
    const int tid = threadIdx.x;
    double best = -1.0;
    int bi = (int)k;
    for (int64_t i = k + tid; i < n; i += 1024) {
        const double s = score(a[k * n + i]);
        if (s > best) { best = s; bi = (int)i; }
    }
    sv[tid] = best;
    si[tid] = bi;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (tid < off) {
            const double o = sv[tid + off];
            const int oi = si[tid + off];
            if (o > sv[tid] || (o == sv[tid] && oi < si[tid])) { sv[tid] = o; si[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        s_p = si[0];
        piv[k] = si[0];
        if (sv[0] == 0.0 && *zero_pivot < 0) *zero_pivot = (int)k;
    }
    __syncthreads();
    const int64_t p = s_p;
    if (p != k)
        for (int64_t j = c0 + tid; j < c1; j += 1024) {
            const S t = a[j * n + k];
            a[j * n + k] = a[j * n + p];
            a[j * n + p] = t;
        }
    __syncthreads();
    const S d = a[k * n + k];
    if (score(d) != 0.0)
        for (int64_t i = k + 1 + tid; i < n; i += 1024) a[k * n + i] = sdiv(a[k * n + i], d);
}

// panel update a_ij -= l_ik u_kj, i > k, k < j < c1 (one thread per element, column-major coalesced)
template <class S>
__global__ __launch_bounds__(256) void lu_update_kernel(S* a, int64_t n, int64_t k, int64_t c1) {
    const int64_t m = n - k - 1, w = c1 - k - 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * w) return;
    const int64_t i = k + 1 + idx % m;
    const int64_t j = k + 1 + idx / m;
    a[j * n + i] = sub(a[j * n + i], mul(a[k * n + i], a[j * n + k]));
}

// the panel's row interchanges (rows j <-> piv[j], j = k0 .. k0 + kb - 1, in order) applied to every
// column outside the panel; one thread per column
template <class S>
__global__ __launch_bounds__(256) void lu_laswp_kernel(S* a, int64_t n, int64_t k0, int kb, const int32_t* piv) {
    int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n - kb) return;
    if (c >= k0) c += kb;
    S* col = a + c * n;
    for (int j = 0; j < kb; ++j) {
        const int64_t r = k0 + j, p = piv[r];
        if (p != r) {
            const S t = col[r];
            col[r] = col[p];
            col[p] = t;
        }
    }
}

// U12 = L11^{-1} A12: L11 the panel's unit lower kb x kb block (LDS), one thread per column of A12
template <class S, int NB>
__global__ __launch_bounds__(256) void lu_trsm_kernel(S* a, int64_t n, int64_t k0, int kb) {
    __shared__ S l11[NB * NB];
    for (int e = threadIdx.x; e < kb * kb; e += 256) {
        const int i = e % kb, j = e / kb;
        l11[i + j * NB] = a[(k0 + i) + (k0 + j) * n];
    }
    __syncthreads();
    const int64_t c = k0 + kb + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    S* col = a + c * n + k0;
    S x[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) x[i] = i < kb ? col[i] : s_zero<S>();
#pragma unroll
    for (int j = 0; j < NB - 1; ++j) {
        if (j < kb) {   // kb < NB only for the last panel
#pragma unroll
            for (int i = j + 1; i < NB; ++i) x[i] = sub(x[i], mul(l11[i + j * NB], x[j]));
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
        if (i < kb) col[i] = x[i];
}

// ------------------------------------------------------------------ matrix right-hand sides (dense_getrs)
// all n interchanges (rows k <-> piv[k], k ascending) on the n x nrhs matrix B; one thread per column
template <class S>
__global__ __launch_bounds__(256) void getrs_laswp_kernel(S* B, int64_t ldb, int64_t nrhs, int64_t n, const int32_t* piv) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nrhs) return;
    S* col = B + c * ldb;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t p = piv[r];
        if (p != r) {
            const S t = col[r];
            col[r] = col[p];
            col[p] = t;
        }
    }
}

// B_k <- T^-1 B_k for the kb rows of B from k0: T the factor's diagonal block at k0 (LDS), its unit lower
// triangle (kUpper = false) or its upper triangle (kUpper = true); one thread per column of B, by substitution
// in the column order of lu_trsm_kernel: backward stable whatever the block holds
template <class S, int NB, bool kUpper>
__global__ __launch_bounds__(256) void getrs_trsm_kernel(const S* lu, int64_t n, int64_t k0, int kb, S* B, int64_t ldb,
                                                         int64_t nrhs) {
    __shared__ S t[NB * NB];
    for (int e = threadIdx.x; e < kb * kb; e += 256) {
        const int i = e % kb, j = e / kb;
        t[i + j * NB] = lu[(k0 + i) + (k0 + j) * n];
    }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nrhs) return;
    S* col = B + c * ldb + k0;
    S x[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) x[i] = i < kb ? col[i] : s_zero<S>();
    if constexpr (!kUpper) {
#pragma unroll
        for (int j = 0; j < NB - 1; ++j) {
            if (j < kb) {   // kb < NB only for the last block row
#pragma unroll
                for (int i = j + 1; i < NB; ++i) x[i] = sub(x[i], mul(t[i + j * NB], x[j]));
            }
        }
    } else {
#pragma unroll
        for (int j = NB - 1; j >= 0; --j) {
            if (j < kb) {
                x[j] = sdiv(x[j], t[j + j * NB]);
#pragma unroll
                for (int i = 0; i < j; ++i) x[i] = sub(x[i], mul(t[i + j * NB], x[j]));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
        if (i < kb) col[i] = x[i];
}

template <class S>
struct DenseSolveArgs {
    const S* lu;
    const int32_t* perm;
    int64_t n;
    const S* b_plain;
    S* y_plain;
    S* buf0;
    S* buf1;
    PowerCtl* ctl;
    const part4* rank_part;
    part4* my_part;
    S* trace;
    double sig_re, sig_im;
};

// One workgroup: z = P b (scaled by 1/||y_prev|| in iteration mode), L z = P b (unit lower),
// U y = z, all in LDS; column-oriented so every column access is coalesced.
template <class S, bool kIter>
__global__ __launch_bounds__(1024) void dense_lu_solve_kernel(DenseSolveArgs<S> a, int parity) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    S* z = reinterpret_cast<S*>(lds_raw);
    __shared__ Prologue pro;
    __shared__ double sm[3 * 16];
    const int tid = threadIdx.x;
    const int64_t n = a.n;
    const S* xin;
    S* yout;
    double nrm = 0.0;
    if constexpr (kIter) {
        shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) return;   // block-uniform exit
        nrm = pro.nrm;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    for (int64_t i = tid; i < n; i += 1024) {
        S v = xin[a.perm[i]];
        if constexpr (kIter) v = scale_in(v, nrm);
        z[i] = v;
    }
    __syncthreads();
    // forward: for each column j, z_i -= L_ij z_j (i > j)
    for (int64_t j = 0; j < n; ++j) {
        const S zj = z[j];
        const S* colj = a.lu + j * n;
        for (int64_t i = j + 1 + tid; i < n; i += 1024) z[i] = sub(z[i], mul(colj[i], zj));
        __syncthreads();
    }
    // backward: for each column j from the last, z_j /= U_jj, z_i -= U_ij z_j (i < j)
    for (int64_t j = n - 1; j >= 0; --j) {
        const S* colj = a.lu + j * n;
        const S zj = sdiv(z[j], colj[j]);
        __syncthreads();
        if (tid == 0) z[j] = zj;
        for (int64_t i = tid; i < j; i += 1024) z[i] = sub(z[i], mul(colj[i], zj));
        __syncthreads();
    }
    double n2 = 0.0, pr = 0.0, pi = 0.0;
    for (int64_t i = tid; i < n; i += 1024) {
        const S yi = z[i];
        yout[i] = yi;
        if constexpr (kIter) {
            S xi = xin[i];
            xi = scale_in(xi, nrm);
            n2 += sq_abs(yi);
            acc_dot(pr, pi, xi, yi);
        }
    }
    if constexpr (kIter) {
        // 1024 threads = 16 waves: wave sums then a fixed-order sum by thread 0
        n2 = wave_sum(n2);
        pr = wave_sum(pr);
        pi = wave_sum(pi);
        const int w = tid >> 6;
        if ((tid & 63) == 0) { sm[w] = n2; sm[16 + w] = pr; sm[32 + w] = pi; }
        __syncthreads();
        if (tid == 0) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < 16; ++i) { s0 += sm[i]; s1 += sm[16 + i]; s2 += sm[32 + i]; }
            a.my_part->a = s0;
            a.my_part->b = s1;
            a.my_part->c = s2;
            a.my_part->d = 0.0;
        }
    }
}

// ------------------------------------------------------------ multi-CU dense substitution
// L z = P b (L unit lower), then U y = z, for large dense factors: block rows of kDB rows, one
// persistent workgroup per resident slot taking block rows round-robin — all its forward rows in
// increasing order, then all its backward rows in decreasing order.  A block row accumulates the
// off-diagonal tiles L_rc z_c as the z_c it needs are published (epoch flags: no reset between
// launches), solves its kDB x kDB triangle in LDS, and publishes.  Forward rows wait only on
// smaller forward rows and backward rows only on forward rows and larger backward rows, and
// every workgroup finishes its forward list first, so with all workgroups resident the
// dependency graph always has a runnable item (bounded spins + an error word besides).
constexpr int kDB = 64;
__device__ __forceinline__ double readlane_s(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ cplx readlane_s(cplx v, int src) { return cplx{readlane_s(v.re, src), readlane_s(v.im, src)}; }
__device__ __forceinline__ float readlane_s(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ __forceinline__ cplxf readlane_s(cplxf v, int src) { return cplxf{readlane_s(v.re, src), readlane_s(v.im, src)}; }
template <class S>
struct DenseTriArgs {
    const S* lu;
    const int32_t* perm;
    int64_t n;
    int32_t nblk;
    int32_t epoch;
    int32_t* flag_f;     // [nblk] epoch when z of the block row is published
    int32_t* flag_b;     // [nblk] epoch when y of the block row is published
    const S* tinv;       // dense_trsv2_kernel: [nblk][2] inv(L_kk), inv(U_kk), 64 x 64 column-major
    const S* tmul;       // [nblk][2] inv(L_rr) L_{r,r-1}, inv(U_rr) U_{r,r+1} (dense_tmul_kernel)
    S* z;                // forward results (n)
    const S* b_plain;
    S* y_plain;
    S* buf0;
    S* buf1;
    PowerCtl* ctl;
    const part4* rank_part;
    part4* my_part;
    part4* wave_part;    // [grid] workgroup partials
    uint32_t* work;
    int32_t* err;
    S* trace;
    double sig_re, sig_im;
};

__device__ __forceinline__ void wait_flag(const int32_t* f, int32_t epoch, int32_t* err) {
    int spins = 0;
    while (__hip_atomic_load(const_cast<int32_t*>(f), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
        // back off: waves far ahead of the chain leave the memory system to the producers
        if (spins < 4) __builtin_amdgcn_s_sleep(2);
        else if (spins < 16) __builtin_amdgcn_s_sleep(8);
        else __builtin_amdgcn_s_sleep(32);
        if (++spins > (1 << 22)) { atomicOr(err, 1); break; }
    }
}

template <class S, bool kIter>
__global__ __launch_bounds__(256) void dense_trsv_kernel(DenseTriArgs<S> a, int parity) {
    __shared__ S tri[kDB * (kDB + 1)];     // the block row's diagonal tile (odd pitch)
    __shared__ S part[4][kDB];             // per-wave partial sums of the off-diagonal tiles
    __shared__ S zsh[4][kDB];              // per-wave copy of the block of z / y a tile multiplies
    __shared__ S vec[kDB];
    __shared__ Prologue pro;
    __shared__ int s_last;
    const S* xin;
    S* yout;
    double nrm = 0.0;
    if constexpr (kIter) {
        shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) return;   // epoch flags: nothing to reset
        nrm = pro.nrm;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = a.n;
    const int G = gridDim.x;
    double n2 = 0.0, pr = 0.0, pi = 0.0;
    for (int phase = 0; phase < 2; ++phase) {
        const bool fwd = phase == 0;
        // this workgroup's block rows: r = blockIdx.x + k G, forward increasing, backward decreasing
        const int cnt = a.nblk > (int)blockIdx.x ? (a.nblk - 1 - (int)blockIdx.x) / G + 1 : 0;
        for (int q = 0; q < cnt; ++q) {
            const int r = fwd ? (int)blockIdx.x + q * G : (int)blockIdx.x + (cnt - 1 - q) * G;
            const int64_t r0 = (int64_t)r * kDB;
            const int rn = (int)min<int64_t>(kDB, n - r0);
            // diagonal tile into LDS (column-major, pitch kDB + 1): all 16 loads of a thread first
            {
                constexpr int kPer = kDB * kDB / 256;
                S tv[kPer];
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    const int e = tid + 256 * q, i = e % kDB, j = e / kDB;
                    tv[q] = a.lu[(r0 + min(i, rn - 1)) + (r0 + min(j, rn - 1)) * n];
                }
#pragma unroll
                for (int q = 0; q < kPer; ++q) {
                    const int e = tid + 256 * q, i = e % kDB, j = e / kDB;
                    tri[i + j * (kDB + 1)] = (i < rn && j < rn) ? tv[q] : s_zero<S>();
                }
            }
            // off-diagonal tiles: forward c < r (L), backward c > r (U); wave wv takes every 4th
            S acc = s_zero<S>();
            const int c_beg = fwd ? 0 : r + 1, c_end = fwd ? r : a.nblk;
            for (int c = c_beg + wv; c < c_end; c += 4) {
                wait_flag(fwd ? a.flag_f + c : a.flag_b + c, a.epoch, a.err);
                const int64_t c0 = (int64_t)c * kDB;
                const int cn = (int)min<int64_t>(kDB, n - c0);
                const S* src = fwd ? a.z : yout;
                // the published block of z (or y): one coherent load per lane, broadcast from LDS
                zsh[wv][lane] = lane < cn ? ld_coh(src + c0 + lane) : s_zero<S>();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const S* tile = a.lu + c0 * n + r0 + min(lane, max(rn - 1, 0));
                if (cn == kDB) {
                    // 16 tile columns in flight per lane before the FMAs consume them
#pragma unroll
                    for (int j0 = 0; j0 < kDB; j0 += 16) {
                        S tv[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) tv[u] = tile[(int64_t)(j0 + u) * n];
#pragma unroll
                        for (int u = 0; u < 16; ++u) acc = add(acc, mul(tv[u], zsh[wv][j0 + u]));
                    }
                } else {
                    for (int j = 0; j < cn; ++j) acc = add(acc, mul(tile[(int64_t)j * n], zsh[wv][j]));
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            part[wv][lane] = lane < rn ? acc : s_zero<S>();
            __syncthreads();
            if (wv == 0) {
                // right-hand side of the block row
                S rhs = s_zero<S>();
                if (lane < rn) {
                    if (fwd) {
                        rhs = xin[a.perm[r0 + lane]];
                        if constexpr (kIter) rhs = scale_in(rhs, nrm);
                    } else {
                        rhs = ld_coh(a.z + r0 + lane);   // published by this wave, read past L1
                    }
                    rhs = sub(rhs, add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane])));
                }
                vec[lane] = rhs;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // triangle: forward unit lower (column order), backward upper (reverse column order)
                // the solved entry travels by v_readlane (wave-uniform j), the tile column from LDS
                S v = vec[lane];
                auto step = [&](const int j) {
                    S zj;
                    if (!fwd && lane == j) v = sdiv(v, tri[j + j * (kDB + 1)]);
                    zj = readlane_s(v, j);
                    const bool below = fwd ? (lane > j) : (lane < j);
                    const S lij = tri[lane + j * (kDB + 1)];
                    if (below) v = sub(v, mul(lij, zj));
                };
                if (rn == kDB) {
                    if (fwd) {
#pragma unroll
                        for (int j = 0; j < kDB; ++j) step(j);
                    } else {
#pragma unroll
                        for (int j = kDB - 1; j >= 0; --j) step(j);
                    }
                } else {
                    for (int jj = 0; jj < rn; ++jj) step(fwd ? jj : rn - 1 - jj);
                }
                if (lane < rn) {
                    if (fwd) {
                        st_coh(a.z + r0 + lane, v);
                    } else {
                        const S yi = v;
                        st_coh(yout + r0 + lane, yi);
                        if constexpr (kIter) {
                            S xi = xin[r0 + lane];
                            xi = scale_in(xi, nrm);
                            n2 += sq_abs(yi);
                            acc_dot(pr, pi, xi, yi);
                        }
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0)
                    __hip_atomic_store(fwd ? a.flag_f + r : a.flag_b + r, a.epoch, __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
        }
    }
    // workgroup partials (wave 0 holds them), then the last arriver sums them in workgroup order
    if (wv == 0) {
        n2 = wave_sum(n2);
        pr = wave_sum(pr);
        pi = wave_sum(pi);
        if (lane == 0) {
            part4* p = a.wave_part + blockIdx.x;
            st_agent(&p->a, n2);
            st_agent(&p->b, pr);
            st_agent(&p->c, pi);
        }
    }
    __syncthreads();
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t tk = __hip_atomic_fetch_add(&a.work[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    if constexpr (kIter) {
        if (tid == 0) {
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int i = 0; i < G; ++i) {
                sa += ld_agent(&a.wave_part[i].a);
                sb += ld_agent(&a.wave_part[i].b);
                sc += ld_agent(&a.wave_part[i].c);
            }
            a.my_part->a = sa;
            a.my_part->b = sb;
            a.my_part->c = sc;
            a.my_part->d = 0.0;
        }
    }
    if (tid == 0) __hip_atomic_store(&a.work[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Inverted diagonal blocks of a dense LU factor (after the factorization; one workgroup per block and
// triangle): tinv + 4096 (2 k) = inv(L_kk) (unit lower), tinv + 4096 (2 k + 1) = inv(U_kk), 64 x 64
// column-major, the identity past a partial last block.  Wave w solves for the 16 unit vectors
// e_{16 w} .. e_{16 w + 15} at once, lane = row, the solved entry broadcast by v_readlane.
template <class S>
__global__ __launch_bounds__(256) void dense_tinv_kernel(const S* lu, int64_t n, S* tinv) {
    __shared__ S tri[kDB * (kDB + 1)];
    const int k = blockIdx.x, upper = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t r0 = (int64_t)k * kDB;
    const int rn = (int)min<int64_t>(kDB, n - r0);
    for (int e = tid; e < kDB * kDB; e += 256) {
        const int i = e % kDB, j = e / kDB;
        S v = s_zero<S>();
        if (i < rn && j < rn) v = lu[(r0 + i) + (r0 + j) * n];
        else if (i == j) set_re_im(v, 1.0, 0.0);
        tri[i + j * (kDB + 1)] = v;
    }
    __syncthreads();
    S v[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        v[t] = s_zero<S>();
        if (lane == 16 * wv + t) set_re_im(v[t], 1.0, 0.0);
    }
    if (!upper) {
        for (int j = 0; j < kDB; ++j) {
            const S lij = tri[lane + j * (kDB + 1)];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const S zj = readlane_s(v[t], j);
                if (lane > j) v[t] = sub(v[t], mul(lij, zj));
            }
        }
    } else {
        for (int j = kDB - 1; j >= 0; --j) {
            const S ujj = tri[j + j * (kDB + 1)];
            const S uij = tri[lane + j * (kDB + 1)];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                if (lane == j) v[t] = sdiv(v[t], ujj);
                const S zj = readlane_s(v[t], j);
                if (lane < j) v[t] = sub(v[t], mul(uij, zj));
            }
        }
    }
    S* out = tinv + (int64_t)(2 * k + upper) * kDB * kDB;
#pragma unroll
    for (int t = 0; t < 16; ++t) out[(16 * wv + t) * kDB + lane] = v[t];
}

// Skeel condition number || |inv(T)| |T| ||_inf of every inverted diagonal block (T = L_kk with its unit
// diagonal, or U_kk; the identity past a partial last block), from dense_tinv_kernel's output: a product
// with inv(T) has a backward error of that many roundoffs where the substitution with T has one, so
// dense_lu_factor keeps dense_trsv2_kernel only while the largest stays small.  One wave per block and
// triangle, lane = row; a NaN (singular block) is kept as the result.
template <class S>
__global__ __launch_bounds__(64) void dense_tcond_kernel(const S* lu, const S* tinv, int64_t n, double* cond) {
    __shared__ double w[kDB];
    const int k = blockIdx.x, upper = blockIdx.y, lane = threadIdx.x;
    const int64_t r0 = (int64_t)k * kDB;
    const int rn = (int)min<int64_t>(kDB, n - r0);
    double s = 1.0;   // row sum of |T|: the unit diagonal of L_kk, or the identity's row
    if (lane < rn) {
        if (upper) s = 0.0;
        const int j0 = upper ? lane : 0, j1 = upper ? rn : lane;
        for (int j = j0; j < j1; ++j) s += score(lu[(r0 + lane) + (r0 + j) * n]);
    }
    w[lane] = s;
    __syncthreads();
    const S* ti = tinv + (int64_t)(2 * k + upper) * kDB * kDB;
    double c = 0.0;
    for (int j = 0; j < kDB; ++j) c += score(ti[lane + j * kDB]) * w[j];
    __syncthreads();
    w[lane] = c;
    __syncthreads();
    if (lane == 0) {
        double m = 0.0;
        for (int i = 0; i < kDB; ++i)
            if (w[i] > m || w[i] != w[i]) m = w[i];   // once NaN, m stays NaN
        cond[2 * k + upper] = m;
    }
}

// The premultiplied next-to-diagonal tiles of dense_trsv2_kernel's dense_pf 2: tmul + 4096 (2 r) =
// inv(L_rr) L_{r,r-1} (r >= 1), tmul + 4096 (2 r + 1) = inv(U_rr) U_{r,r+1} (r <= nblk - 2), 64 x 64
// column-major, rows past a partial last block and columns past a partial next block zero.  Thread =
// one column, 16 rows.
template <class S>
__global__ __launch_bounds__(256) void dense_tmul_kernel(const S* lu, const S* tinv, int64_t n, int nblk, S* tmul) {
    __shared__ S ti[kDB * (kDB + 1)];
    __shared__ S tl[kDB * (kDB + 1)];
    const int r = blockIdx.x, upper = blockIdx.y;
    const int tid = threadIdx.x;
    S* out = tmul + (int64_t)(2 * r + upper) * kDB * kDB;
    const int c = upper ? r + 1 : r - 1;
    if (c < 0 || c >= nblk) {
        for (int e = tid; e < kDB * kDB; e += 256) out[e] = s_zero<S>();
        return;
    }
    const int64_t r0 = (int64_t)r * kDB, c0 = (int64_t)c * kDB;
    const int rn = (int)min<int64_t>(kDB, n - r0), cn = (int)min<int64_t>(kDB, n - c0);
    const S* tv = tinv + (int64_t)(2 * r + upper) * kDB * kDB;
    for (int e = tid; e < kDB * kDB; e += 256) {
        const int i = e % kDB, j = e / kDB;
        ti[i + j * (kDB + 1)] = tv[e];
        tl[i + j * (kDB + 1)] = (i < rn && j < cn) ? lu[(r0 + i) + (c0 + j) * n] : s_zero<S>();
    }
    __syncthreads();
    const int j = tid & 63, i0 = (tid >> 6) * 16;
    S o[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] = s_zero<S>();
    for (int k = 0; k < kDB; ++k) {
        const S b = tl[k + j * (kDB + 1)];
#pragma unroll
        for (int t = 0; t < 16; ++t) o[t] = add(o[t], mul(ti[(i0 + t) + k * (kDB + 1)], b));
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) out[(i0 + t) + j * kDB] = o[t];
}

// The multi-CU substitution with the diagonal blocks applied as products with their inverses
// (dense_tinv_kernel) and every off-diagonal tile loaded before its block's flag is awaited (the
// multifrontal row-block solve's scheme, mf_big_fwd_kernel).  A block row: each wave takes 16 columns
// of every column block - forward c = 0 .. r - 1, backward c = nblk - 1 .. r + 1 - loads its 64 x 16
// piece of the tile, polls the block's 16 published values (value flags, below), and accumulates;
// then t = rhs - sum, y = inv(T_rr) t as four 64 x 16 products from registers, published by 64
// write-through stores.  The per-block hand-off is one store and one poll instead of the 64-step
// triangle of dense_trsv_kernel and its epoch flag.  Workgroups take block rows round-robin like it.
// value flags of dense_trsv2_kernel: an unsolved entry holds this NaN in every 8-byte word, a solved one
// never does (a NaN result is stored as the default quiet NaN), so a waiting wave polls the values
// themselves.  Two buffers alternate by the launch's epoch: a launch solves in one and resets its own
// rows of the other for the next launch (no reader of the other buffer is running).
constexpr unsigned long long kDnSent = 0x7FF4DEAD7FF4DEADull;
__device__ __forceinline__ bool dn_unready(double v) { return (unsigned long long)__double_as_longlong(v) == kDnSent; }
__device__ __forceinline__ bool dn_unready(cplx v) { return dn_unready(v.re) || dn_unready(v.im); }
__device__ __forceinline__ bool dn_unready(float v) { return (unsigned)__float_as_int(v) == (unsigned)(kDnSent & 0xffffffffu); }
__device__ __forceinline__ bool dn_unready(cplxf v) { return dn_unready(v.re) || dn_unready(v.im); }
template <class S>
__device__ __forceinline__ S dn_sent() {
    S v;
    if constexpr (std::is_same_v<S, double>) v = __longlong_as_double((long long)kDnSent);
    else if constexpr (std::is_same_v<S, cplx>) v = cplx{__longlong_as_double((long long)kDnSent), __longlong_as_double((long long)kDnSent)};
    else if constexpr (std::is_same_v<S, float>) v = __int_as_float((int)(kDnSent & 0xffffffffu));
    else v = cplxf{__int_as_float((int)(kDnSent & 0xffffffffu)), __int_as_float((int)(kDnSent & 0xffffffffu))};
    return v;
}
__device__ __forceinline__ double dn_clean(double v) { return v != v ? __longlong_as_double(0x7FF8000000000000ll) : v; }
__device__ __forceinline__ cplx dn_clean(cplx v) { return cplx{dn_clean(v.re), dn_clean(v.im)}; }
__device__ __forceinline__ float dn_clean(float v) { return v != v ? __int_as_float(0x7FC00000) : v; }
__device__ __forceinline__ cplxf dn_clean(cplxf v) { return cplxf{dn_clean(v.re), dn_clean(v.im)}; }
template <class S>
__device__ __forceinline__ S dn_poll(const S* p, int32_t* err) {
    S v = ld_coh(p);
    int spins = 0;
    while (dn_unready(v)) {
        __builtin_amdgcn_s_sleep(1);
        v = ld_coh(p);
        if (++spins > (1 << 24)) {
            atomicOr(err, 1);
            break;
        }
    }
    return v;
}

template <class S, bool kIter, int kPf>
__global__ __launch_bounds__(256) void dense_trsv2_kernel(DenseTriArgs<S> a, int parity) {
    __shared__ S part[4][kDB];
    __shared__ S part2[4][kDB];
    __shared__ S zsh[4][16];
    __shared__ S vec[kDB];
    __shared__ Prologue pro;
    __shared__ int s_last;
    const S* xin;
    S* yout;
    double nrm = 0.0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = a.n;
    const int G = gridDim.x;
    const int cnt = a.nblk > (int)blockIdx.x ? (a.nblk - 1 - (int)blockIdx.x) / G + 1 : 0;
    // a.z: [z | z' | y | y'] value buffers; this launch solves in (z, y) of its epoch's parity and
    // resets its own rows of the other pair for the next launch (also when the iteration has stopped)
    const int64_t pp = a.epoch & 1;
    S* zcur = a.z + pp * n;
    S* ycur = a.z + (2 + pp) * n;
    {
        S* znext = a.z + (1 - pp) * n;
        S* ynext = a.z + (3 - pp) * n;
        const S sent = dn_sent<S>();
        for (int q = 0; q < cnt; ++q) {
            const int64_t r0 = (int64_t)((int)blockIdx.x + q * G) * kDB;
            if (tid < kDB && r0 + tid < n) {
                st_coh(znext + r0 + tid, sent);
                st_coh(ynext + r0 + tid, sent);
            }
        }
    }
    if constexpr (kIter) {
        shift_prologue<S>(a.ctl, a.rank_part, parity, a.trace, a.sig_re, a.sig_im, &pro);
        if (!__builtin_amdgcn_readfirstlane(pro.go)) return;
        nrm = pro.nrm;
        xin = parity ? a.buf0 : a.buf1;
        yout = parity ? a.buf1 : a.buf0;
    } else {
        xin = a.b_plain;
        yout = a.y_plain;
    }
    double n2 = 0.0, pr = 0.0, pi = 0.0;
    for (int phase = 0; phase < 2; ++phase) {
        const bool fwd = phase == 0;
        for (int q = 0; q < cnt; ++q) {
            const int r = fwd ? (int)blockIdx.x + q * G : (int)blockIdx.x + (cnt - 1 - q) * G;
            const int64_t r0 = (int64_t)r * kDB;
            const int rn = (int)min<int64_t>(kDB, n - r0);
            const int64_t row = r0 + min(lane, rn - 1);
            // this wave's 16 columns of the inverted diagonal block, and the block row's right-hand side
            S iv[16];
            {
                const S* ti = a.tinv + (int64_t)(2 * r + (fwd ? 0 : 1)) * kDB * kDB + (16 * wv) * kDB + lane;
#pragma unroll
                for (int t = 0; t < 16; ++t) iv[t] = ti[t * kDB];
            }
            S rhs = s_zero<S>();
            if (wv == 0 && lane < rn) {
                if (fwd) {
                    rhs = xin[a.perm[r0 + lane]];
                    if constexpr (kIter) rhs = scale_in(rhs, nrm);
                } else {
                    rhs = dn_poll(zcur + r0 + lane, a.err);   // published by this workgroup in the forward phase
                }
            }
            S acc = s_zero<S>();
            const int nc = fwd ? r : a.nblk - 1 - r;
            // dense_pf 2: the block next to the diagonal enters as a product with the premultiplied tile
            // inv(T_rr) T_{r, r -/+ 1} (dense_tmul_kernel) after y' = inv(T_rr) (rhs - the other blocks)
            // is formed, so the chain's hand-off is followed by one 64 x 64 product instead of two
            const bool premul = kPf == 2 && nc > 0;
            const int nacc = premul ? nc - 1 : nc;
            const S* src = fwd ? zcur : ycur;
            const int j0 = 16 * wv;
            const S* tile = a.lu + row;
            // this wave's 64 x 16 piece of column block m's tile
            auto load_tile = [&](int m, S* tv) {
                const int c = fwd ? m : a.nblk - 1 - m;
                const int64_t c0 = (int64_t)c * kDB;
                const int cn = (int)min<int64_t>(kDB, n - c0);
#pragma unroll
                for (int t = 0; t < 16; ++t) tv[t] = tile[(c0 + min(j0 + t, cn - 1)) * n];
            };
            if constexpr (kPf >= 1) {
                // software-pipelined (default): the first poll of block m's values is issued before the
                // loads of tile m + 1, so the poll's wait leaves those in flight and a wave behind the
                // chain streams its tiles instead of paying one load latency per block; the same
                // products in the same order (bitwise the unpipelined loop)
                S tv[16], tn[16];
                if (nacc > 0) load_tile(0, tv);
                for (int m = 0; m < nacc; ++m) {
                    const int c = fwd ? m : a.nblk - 1 - m;
                    const int64_t c0 = (int64_t)c * kDB;
                    const int cn = (int)min<int64_t>(kDB, n - c0);
                    const bool mine = lane < 16 && j0 + lane < cn;
                    S zv = s_zero<S>();
                    if (mine) zv = ld_coh(src + c0 + j0 + lane);
                    if (m + 1 < nacc) load_tile(m + 1, tn);
                    if (mine) {
                        int spins = 0;
                        while (dn_unready(zv)) {
                            __builtin_amdgcn_s_sleep(1);
                            zv = ld_coh(src + c0 + j0 + lane);
                            if (++spins > (1 << 24)) {
                                atomicOr(a.err, 1);
                                break;
                            }
                        }
                    }
                    if (lane < 16) zsh[wv][lane] = zv;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int t = 0; t < 16; ++t) acc = add(acc, mul(tv[t], zsh[wv][t]));
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int t = 0; t < 16; ++t) tv[t] = tn[t];
                }
            } else {
                for (int m = 0; m < nc; ++m) {
                    const int c = fwd ? m : a.nblk - 1 - m;
                    const int64_t c0 = (int64_t)c * kDB;
                    const int cn = (int)min<int64_t>(kDB, n - c0);
                    S tv[16];
                    load_tile(m, tv);
                    if (lane < 16) zsh[wv][lane] = j0 + lane < cn ? dn_poll(src + c0 + j0 + lane, a.err) : s_zero<S>();
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int t = 0; t < 16; ++t) acc = add(acc, mul(tv[t], zsh[wv][t]));
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // premultiplied step: its tile piece and the first poll of its values issued now, under the
            // reductions below
            S tm[16];
            S zl = s_zero<S>();
            int64_t lc0 = 0;
            bool lmine = false;
            if (premul) {
                const int c = fwd ? r - 1 : r + 1;
                lc0 = (int64_t)c * kDB;
                const int cn = (int)min<int64_t>(kDB, n - lc0);
                lmine = lane < 16 && j0 + lane < cn;
                if (lmine) zl = ld_coh(src + lc0 + j0 + lane);
                const S* tmp = a.tmul + (int64_t)(2 * r + (fwd ? 0 : 1)) * kDB * kDB + j0 * kDB + lane;
#pragma unroll
                for (int t = 0; t < 16; ++t) tm[t] = tmp[t * kDB];
            }
            part[wv][lane] = acc;
            __syncthreads();
            if (wv == 0)
                vec[lane] = lane < rn ? sub(rhs, add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane])))
                                      : s_zero<S>();
            __syncthreads();
            S p = s_zero<S>();
#pragma unroll
            for (int t = 0; t < 16; ++t) p = add(p, mul(iv[t], vec[16 * wv + t]));
            part[wv][lane] = p;
            __syncthreads();
            S y = s_zero<S>();
            if (wv == 0) y = add(add(part[0][lane], part[1][lane]), add(part[2][lane], part[3][lane]));
            if (premul) {
                if (lmine) {
                    int spins = 0;
                    while (dn_unready(zl)) {
                        __builtin_amdgcn_s_sleep(1);
                        zl = ld_coh(src + lc0 + j0 + lane);
                        if (++spins > (1 << 24)) {
                            atomicOr(a.err, 1);
                            break;
                        }
                    }
                }
                if (lane < 16) zsh[wv][lane] = zl;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                S q = s_zero<S>();
#pragma unroll
                for (int t = 0; t < 16; ++t) q = add(q, mul(tm[t], zsh[wv][t]));
                part2[wv][lane] = q;
                __syncthreads();
                if (wv == 0) y = sub(y, add(add(part2[0][lane], part2[1][lane]), add(part2[2][lane], part2[3][lane])));
            }
            if (wv == 0) {
                if (lane < rn) {
                    // publish (the value is its own flag)
                    if (fwd) {
                        st_coh(zcur + r0 + lane, dn_clean(y));
                    } else {
                        st_coh(ycur + r0 + lane, dn_clean(y));
                        yout[r0 + lane] = y;
                        if constexpr (kIter) {
                            S xi = xin[r0 + lane];
                            xi = scale_in(xi, nrm);
                            n2 += sq_abs(y);
                            acc_dot(pr, pi, xi, y);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    // workgroup partials (wave 0 holds them), then the last arriver sums them in workgroup order
    if (wv == 0) {
        n2 = wave_sum(n2);
        pr = wave_sum(pr);
        pi = wave_sum(pi);
        if (lane == 0) {
            part4* pp = a.wave_part + blockIdx.x;
            st_agent(&pp->a, n2);
            st_agent(&pp->b, pr);
            st_agent(&pp->c, pi);
        }
    }
    __syncthreads();
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t tk = __hip_atomic_fetch_add(&a.work[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    if constexpr (kIter) {
        if (tid == 0) {
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int i = 0; i < G; ++i) {
                sa += ld_agent(&a.wave_part[i].a);
                sb += ld_agent(&a.wave_part[i].b);
                sc += ld_agent(&a.wave_part[i].c);
            }
            a.my_part->a = sa;
            a.my_part->b = sb;
            a.my_part->c = sc;
            a.my_part->d = 0.0;
        }
    }
    if (tid == 0) __hip_atomic_store(&a.work[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// CSR (device) -> dense column-major (device), for small non-triangular sparse matrices
template <class S>
__global__ void densify_kernel(const int32_t* rowptr, const int32_t* col, const S* val, int64_t n,
                               S* out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) out[(int64_t)col[e] * n + r] = val[e];
}

template <class S>
__global__ void shift_diag_kernel(S* a, int64_t n, S sigma) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i * n + i] = sub(a[i * n + i], sigma);
}

}  // namespace dev

// dense_trsv2_kernel's loop form (EIGSOL_DENSE_PF, read per call): 0 one tile load per block, 1 tile
// loads one block ahead, 2 (default) also the premultiplied next-to-diagonal block; each form is its own
// instantiation so the others' registers do not bound it
template <class S>
static const void* dense_trsv2_ptr(bool iter, int pf) {
    if (pf <= 0) return iter ? reinterpret_cast<const void*>(dev::dense_trsv2_kernel<S, true, 0>)
                             : reinterpret_cast<const void*>(dev::dense_trsv2_kernel<S, false, 0>);
    if (pf == 1) return iter ? reinterpret_cast<const void*>(dev::dense_trsv2_kernel<S, true, 1>)
                             : reinterpret_cast<const void*>(dev::dense_trsv2_kernel<S, false, 1>);
    return iter ? reinterpret_cast<const void*>(dev::dense_trsv2_kernel<S, true, 2>)
                : reinterpret_cast<const void*>(dev::dense_trsv2_kernel<S, false, 2>);
}
template <class S>
static int dense_pf_mode() {
    const char* e = std::getenv("EIGSOL_DENSE_PF");
    return e ? std::max(0, std::min(2, std::atoi(e))) : 2;
}

template <class S>
static int64_t kDenseSingleMax() {
    const char* e = std::getenv("EIGSOL_DENSE_TRSV_SINGLE_MAX");   // A/B: substitution crossover
    if (e) return std::atoll(e);
    // round 6 (profiles/r06_dense_small.log): the block-row substitution beats the one-workgroup one from
    // n = 128 on (0.080 -> 0.030 ms per iteration at 128, 0.332 -> 0.047 ms at 512)
    return 64;
}

// Largest Skeel condition number || |inv(T)| |T| ||_inf of a 64 x 64 diagonal block of L or U for which
// the factor keeps dense_trsv2_kernel: Gaussian, A / sqrt(n) + diag and planted-spectrum
// factors up to n = 16384 measure <= 9.4e2 in all four scalar types, the adversarial factors of
// tests/test_gpu_dense_lu_edges.py >= 5e8.
constexpr double kDenseBlockCondMax = 1e6;

template <class S>
void dense_getrf(hipStream_t st, S* a, int64_t n, int32_t* piv, int32_t* zero_pivot) {
    // right-looking blocked LU with partial pivoting (LAPACK getrf order): per panel of NB columns,
    // column-by-column pivoting and rank-1 updates inside the panel, the panel's interchanges on
    // the other columns, U12 = L11^-1 A12, and A22 -= L21 U12 on the fp64 matrix cores
    constexpr int NB = dev::RankKMax<S>::value;
    for (int64_t k0 = 0; k0 < n; k0 += NB) {
        const int kb = (int)std::min<int64_t>(NB, n - k0);
        const int64_t c1 = k0 + kb;
        for (int64_t k = k0; k < c1; ++k) {
            hipLaunchKernelGGL((dev::lu_pivot_kernel<S>), dim3(1), dim3(1024), 0, st, a, n, k, k0, c1, piv, zero_pivot);
            const int64_t m = n - k - 1, w = c1 - k - 1;
            if (m > 0 && w > 0)
                hipLaunchKernelGGL((dev::lu_update_kernel<S>), dim3((m * w + 255) / 256), dim3(256), 0, st, a, n, k, c1);
        }
        if (n - kb > 0)
            hipLaunchKernelGGL((dev::lu_laswp_kernel<S>), dim3((n - kb + 255) / 256), dim3(256), 0, st, a, n, k0, kb, piv);
        const int64_t rest = n - c1;
        if (rest > 0) {
            hipLaunchKernelGGL((dev::lu_trsm_kernel<S, NB>), dim3((rest + 255) / 256), dim3(256), 0, st, a, n, k0, kb);
            rankk_update<S, true>(st, (int)rest, (int)rest, kb, -1.0, a + c1 + k0 * n, n, a + k0 + c1 * n, n,
                                  a + c1 + c1 * n, n);
        }
    }
}

template <class S>
static int dense_lu_factor(const ShiftFactor* f, DenseFactor& d, bool from_sparse) {
    hipStream_t st = f->ctx->stream;
    const int64_t n = f->n;
    S* a = static_cast<S*>(d.lu);
    DevBuf pivots;
    EIGSOL_TRY(pivots.alloc(n * sizeof(int32_t)));
    int32_t* piv = pivots.as<int32_t>();
    EIGSOL_HIP(hipMalloc(&d.zero_pivot, sizeof(int32_t)));
    EIGSOL_HIP(hipMemsetAsync(d.zero_pivot, 0xff, sizeof(int32_t), st));
    hipLaunchKernelGGL((dev::shift_diag_kernel<S>), dim3((n + 255) / 256), dim3(256), 0, st, a, n,
                       make_sigma<S>(f->sig_re, f->sig_im));
    dense_getrf<S>(st, a, n, piv, d.zero_pivot);
    EIGSOL_HIP(hipGetLastError());
    std::vector<int32_t> hp(n);
    int32_t zp = -1;
    EIGSOL_HIP(hipMemcpyAsync(hp.data(), piv, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(&zp, d.zero_pivot, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    // a sparse matrix goes through SparseLU in the reference, which reports a singular matrix
    if (from_sparse && zp >= 0)
        return fail(EIGSOL_E_SOLVER, "solve_shifted: SparseLU factorization failed");
    // transpositions -> permutation: (P b)[i] = b[perm[i]]
    std::vector<int32_t> perm(n);
    for (int64_t i = 0; i < n; ++i) perm[i] = (int32_t)i;
    for (int64_t k = 0; k < n; ++k) std::swap(perm[k], perm[hp[k]]);
    EIGSOL_HIP(hipMalloc(&d.perm, n * sizeof(int32_t)));
    EIGSOL_HIP(hipMemcpyAsync(d.perm, perm.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    d.lds_bytes = (size_t)n * sizeof(S);
    if (n > kDenseSingleMax<S>()) {
        // multi-CU substitution: one persistent workgroup per CU at most (all resident)
        const int nblk = (int)((n + dev::kDB - 1) / dev::kDB);
        d.multi = 1;
        d.grid = std::max(1, std::min(nblk, 32));   // 16384^2 f64: 32 WGs 32 ms, 64: 37 ms, 256: 48 ms per solve
        if (const char* e = std::getenv("EIGSOL_DENSE_TRSV_GRID")) d.grid = std::max(1, std::min(nblk, std::atoi(e)));
        d.nblk = nblk;
        EIGSOL_HIP(hipMalloc(&d.flag_f, sizeof(int32_t) * nblk));
        EIGSOL_HIP(hipMalloc(&d.flag_b, sizeof(int32_t) * nblk));
        EIGSOL_HIP(hipMalloc(&d.zf, sizeof(S) * n));
        EIGSOL_HIP(hipMalloc(&d.work, 64));
        EIGSOL_HIP(hipMalloc(&d.err, 64));
        EIGSOL_HIP(hipMalloc(&d.wave_part, sizeof(dev::part4) * d.grid));
        EIGSOL_HIP(hipMemsetAsync(d.flag_f, 0, sizeof(int32_t) * nblk, st));
        EIGSOL_HIP(hipMemsetAsync(d.flag_b, 0, sizeof(int32_t) * nblk, st));
        EIGSOL_HIP(hipMemsetAsync(d.work, 0, 64, st));
        EIGSOL_HIP(hipMemsetAsync(d.err, 0, 64, st));
        // dense_trsv2_kernel applies the diagonal blocks as products with their inverses, which is backward
        // stable only while the blocks are well conditioned (partial pivoting bounds |l_ij| <= 1, not
        // inv(L_kk): entries near -1 give an inverse near 2^62).  So the blocks' Skeel condition numbers are
        // measured once here, and a factor with one above kDenseBlockCondMax (or singular: NaN) is solved by
        // the triangle substitution dense_trsv_kernel (64-step triangles on one wave, 32 workgroups), which
        // is backward stable whatever L and U hold, like PartialPivLU::solve.  EIGSOL_DENSE_TRSV=1 / 2 force
        // dense_trsv_kernel / dense_trsv2_kernel (A/B).
        const char* dv = std::getenv("EIGSOL_DENSE_TRSV");
        const int forced = dv ? std::atoi(dv) : 0;
        d.version = forced == 1 ? 1 : 2;
        if (d.version == 2) {
            EIGSOL_HIP(hipMalloc(&d.tinv, sizeof(S) * (size_t)nblk * 2 * dev::kDB * dev::kDB));
            hipLaunchKernelGGL((dev::dense_tinv_kernel<S>), dim3(nblk, 2), dim3(256), 0, st, static_cast<const S*>(d.lu),
                               n, static_cast<S*>(d.tinv));
            EIGSOL_HIP(hipGetLastError());
        }
        if (d.version == 2 && forced != 2) {
            DevBuf dcond;
            EIGSOL_TRY(dcond.alloc(sizeof(double) * 2 * nblk));
            hipLaunchKernelGGL((dev::dense_tcond_kernel<S>), dim3(nblk, 2), dim3(64), 0, st, static_cast<const S*>(d.lu),
                               static_cast<const S*>(d.tinv), n, dcond.as<double>());
            std::vector<double> hc(2 * (size_t)nblk);
            EIGSOL_HIP(hipMemcpyAsync(hc.data(), dcond.p, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, st));
            EIGSOL_HIP(hipStreamSynchronize(st));
            bool ok = true;
            for (double c : hc) ok = ok && c <= kDenseBlockCondMax;   // false for a NaN
            if (!ok) {
                d.version = 1;
                hipFree(d.tinv);
                d.tinv = nullptr;
            }
        }
        if (d.version == 2) {
            // value buffers [z | z' | y | y'] (dense_trsv2_kernel), all unsolved
            hipFree(d.zf);
            d.zf = nullptr;
            EIGSOL_HIP(hipMalloc(&d.zf, sizeof(S) * 4 * n));
            EIGSOL_HIP(hipMemsetD32Async(static_cast<hipDeviceptr_t>(d.zf), 0x7FF4DEADu, sizeof(S) * n, st));
            EIGSOL_HIP(hipMalloc(&d.tmul, sizeof(S) * (size_t)nblk * 2 * dev::kDB * dev::kDB));
            hipLaunchKernelGGL((dev::dense_tmul_kernel<S>), dim3(nblk, 2), dim3(256), 0, st, static_cast<const S*>(d.lu),
                               static_cast<const S*>(d.tinv), n, nblk, static_cast<S*>(d.tmul));
            EIGSOL_HIP(hipGetLastError());
            // one block row per workgroup while they all fit on the device at once (a cooperative launch)
            // (the fewest resident over the loop forms, so a later EIGSOL_DENSE_PF still fits the grid)
            int per_cu = 1 << 20;
            for (int pf = 0; pf < 3; ++pf)
                for (int it = 0; it < 2; ++it) {
                    int o = 1;
                    EIGSOL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, dense_trsv2_ptr<S>(it != 0, pf), 256, 0));
                    per_cu = std::min(per_cu, o);
                }
            d.grid = std::max(1, std::min(nblk, std::max(1, per_cu) * f->ctx->num_cus));
            if (const char* e = std::getenv("EIGSOL_DENSE_TRSV_GRID")) d.grid = std::max(1, std::min(nblk, std::atoi(e)));
            hipFree(d.wave_part);
            d.wave_part = nullptr;
            EIGSOL_HIP(hipMalloc(&d.wave_part, sizeof(dev::part4) * d.grid));
        }
        EIGSOL_HIP(hipStreamSynchronize(st));
    }
    return EIGSOL_OK;
}

// a dense factor must fit the device memory (288 GB of HBM); which substitution solves with it is kDenseSingleMax's
// and dense_lu_factor's choice
int dense_limits(int dtype, int64_t n, const char* who) {
    const double bytes = (double)n * (double)n * (double)scalar_bytes(dtype);
    if (n > INT32_MAX / 2 || bytes > 0.9 * 288e9)
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": dense factor of order " + std::to_string(n) +
                                              " does not fit the device memory");
    return EIGSOL_OK;
}

// factor d.lu (a copy of the matrix, or the densified A) in place
template <class S>
static int dense_from_t(const ShiftFactor* f, const void* a, const eigsol_csr* A, DenseFactor& d) {
    hipStream_t st = f->ctx->stream;
    const int64_t n = f->n;
    const size_t bytes = (size_t)n * n * sizeof(S);
    if (hipMalloc(&d.lu, bytes) != hipSuccess) return fail(EIGSOL_E_HIP, "hipMalloc(LU)");
    if (a) {
        EIGSOL_HIP(hipMemcpyAsync(d.lu, a, bytes, hipMemcpyDeviceToDevice, st));
    } else {
        // general sparse pattern: densify on the device and LU it (the reference's SparseLU)
        EIGSOL_HIP(hipMemsetAsync(d.lu, 0, bytes, st));
        hipLaunchKernelGGL((dev::densify_kernel<S>), dim3((n + 255) / 256), dim3(256), 0, st, A->rowptr, A->col,
                           static_cast<const S*>(A->val), n, static_cast<S*>(d.lu));
    }
    return dense_lu_factor<S>(f, d, A != nullptr);
}

int dense_from_matrix(const ShiftFactor* f, const void* a, DenseFactor& d) {
    return by_dtype(f->dtype, [&](auto tag) { return dense_from_t<decltype(tag)>(f, a, nullptr, d); });
}

int dense_from_csr(const ShiftFactor* f, const eigsol_csr* A, DenseFactor& d) {
    return by_dtype(f->dtype, [&](auto tag) { return dense_from_t<decltype(tag)>(f, nullptr, A, d); });
}

// the block-row substitution on d.grid persistent workgroups (large n), or the single-workgroup substitution
template <class S>
static int dense_launch_t(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it) {
    hipStream_t st = f->ctx->stream;
    DenseFactor& d = f->dense;
    int parity = it.parity;
    if (d.multi) {
        dev::DenseTriArgs<S> a{};
        fill_iter(a, f, b, y, it);
        a.lu = static_cast<const S*>(d.lu);
        a.perm = d.perm;
        a.nblk = d.nblk;
        a.epoch = ++d.epoch;
        a.flag_f = d.flag_f;
        a.flag_b = d.flag_b;
        a.tinv = static_cast<const S*>(d.tinv);
        a.tmul = static_cast<const S*>(d.tmul);
        a.z = static_cast<S*>(d.zf);
        a.wave_part = static_cast<dev::part4*>(d.wave_part);
        a.work = d.work;
        a.err = d.err;
        // cooperative: the persistent block-row workgroups wait on each other's epoch flags
        void* kargs[] = {&a, &parity};
        const void* dk = d.version == 2 ? dense_trsv2_ptr<S>(iter, dense_pf_mode<S>())
                                        : (iter ? reinterpret_cast<const void*>(dev::dense_trsv_kernel<S, true>)
                                                : reinterpret_cast<const void*>(dev::dense_trsv_kernel<S, false>));
        EIGSOL_HIP(hipLaunchCooperativeKernel(dk, dim3(d.grid), dim3(256), kargs, 0, st));
    } else {
        dev::DenseSolveArgs<S> a{};
        fill_iter(a, f, b, y, it);
        a.lu = static_cast<const S*>(d.lu);
        a.perm = d.perm;
        const void* k = iter ? reinterpret_cast<const void*>(dev::dense_lu_solve_kernel<S, true>)
                             : reinterpret_cast<const void*>(dev::dense_lu_solve_kernel<S, false>);
        EIGSOL_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)d.lds_bytes));
        if (iter) hipLaunchKernelGGL((dev::dense_lu_solve_kernel<S, true>), dim3(1), dim3(1024), d.lds_bytes, st, a, parity);
        else hipLaunchKernelGGL((dev::dense_lu_solve_kernel<S, false>), dim3(1), dim3(1024), d.lds_bytes, st, a, parity);
    }
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

int dense_launch(ShiftFactor* f, bool iter, const void* b, void* y, const ShiftIter& it) {
    return by_dtype(f->dtype, [&](auto tag) { return dense_launch_t<decltype(tag)>(f, iter, b, y, it); });
}

// ------------------------------------------------------------------ matrix right-hand sides
// The diagonal blocks are solved by substitution and not multiplied by their inverses (see dense_lu_factor on
// dense_trsv2_kernel: partial pivoting bounds |l_ij|, not inv(L_kk)), so the solve is backward stable whatever
// the factor holds.  2 ceil(n / NB) - 1 rank-NB updates on the matrix cores carry the n^2 nrhs flops.
template <class S>
void dense_getrs(hipStream_t st, const S* lu, int64_t n, const int32_t* piv, S* B, int64_t ldb, int64_t nrhs) {
    constexpr int NB = dev::RankKMax<S>::value;
    if (n <= 0 || nrhs <= 0) return;
    const dim3 cols((unsigned)((nrhs + 255) / 256));
    hipLaunchKernelGGL((dev::getrs_laswp_kernel<S>), cols, dim3(256), 0, st, B, ldb, nrhs, n, piv);
    for (int64_t k0 = 0; k0 < n; k0 += NB) {   // L Y = P B
        const int kb = (int)std::min<int64_t>(NB, n - k0);
        const int64_t c1 = k0 + kb;
        hipLaunchKernelGGL((dev::getrs_trsm_kernel<S, NB, false>), cols, dim3(256), 0, st, lu, n, k0, kb, B, ldb, nrhs);
        if (n - c1 > 0) rankk_update<S, true>(st, (int)(n - c1), (int)nrhs, kb, -1.0, lu + c1 + k0 * n, n, B + k0, ldb, B + c1, ldb);
    }
    for (int64_t k0 = ((n - 1) / NB) * NB; k0 >= 0; k0 -= NB) {   // U X = Y
        const int kb = (int)std::min<int64_t>(NB, n - k0);
        hipLaunchKernelGGL((dev::getrs_trsm_kernel<S, NB, true>), cols, dim3(256), 0, st, lu, n, k0, kb, B, ldb, nrhs);
        if (k0 > 0) rankk_update<S, true>(st, (int)k0, (int)nrhs, kb, -1.0, lu + k0 * n, n, B + k0, ldb, B, ldb);
    }
}

template void dense_getrf<double>(hipStream_t, double*, int64_t, int32_t*, int32_t*);
template void dense_getrf<cplx>(hipStream_t, cplx*, int64_t, int32_t*, int32_t*);
template void dense_getrs<double>(hipStream_t, const double*, int64_t, const int32_t*, double*, int64_t, int64_t);
template void dense_getrs<cplx>(hipStream_t, const cplx*, int64_t, const int32_t*, cplx*, int64_t, int64_t);

namespace {

template <class S>
int solve_host(eigsol_ctx* ctx, int64_t n, int64_t nrhs, const void* A_host, const void* B_host, void* X_out) {
    hipStream_t st = ctx->stream;
    DevBuf dA, dB, dpiv, dzp;
    EIGSOL_TRY(dA.alloc((size_t)n * n * sizeof(S)));
    EIGSOL_TRY(dB.alloc((size_t)n * nrhs * sizeof(S)));
    EIGSOL_TRY(dpiv.alloc((size_t)n * sizeof(int32_t)));
    EIGSOL_TRY(dzp.alloc(sizeof(int32_t)));
    EIGSOL_HIP(hipMemcpyAsync(dA.p, A_host, (size_t)n * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dB.p, B_host, (size_t)n * nrhs * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemsetAsync(dzp.p, 0xff, sizeof(int32_t), st));
    dense_getrf<S>(st, dA.as<S>(), n, dpiv.as<int32_t>(), dzp.as<int32_t>());
    EIGSOL_HIP(hipGetLastError());
    int32_t zp = -1;
    EIGSOL_HIP(hipMemcpyAsync(&zp, dzp.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    if (zp >= 0)
        return fail(EIGSOL_E_SOLVER, "eigsol_solve_dense: the matrix is singular: the pivot of column " + std::to_string(zp) + " is zero");
    dense_getrs<S>(st, dA.as<S>(), n, dpiv.as<int32_t>(), dB.as<S>(), n, nrhs);
    EIGSOL_HIP(hipGetLastError());
    EIGSOL_HIP(hipMemcpyAsync(X_out, dB.p, (size_t)n * nrhs * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" int eigsol_solve_dense(eigsol_ctx* ctx, int dtype, int64_t n, int64_t nrhs, const void* A_colmajor,
                                  const void* B_colmajor, void* X_out) {
    const char* who = "eigsol_solve_dense";
    if (n < 0 || nrhs < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative size");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    EIGSOL_TRY(dense_fn_check(who, ctx, dtype, std::max(n, nrhs)));
    if (n == 0 || nrhs == 0) return EIGSOL_OK;
    if (!A_colmajor || !B_colmajor || !X_out) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    return dtype == EIGSOL_C128 ? solve_host<cplx>(ctx, n, nrhs, A_colmajor, B_colmajor, X_out)
                                : solve_host<double>(ctx, n, nrhs, A_colmajor, B_colmajor, X_out);
}
