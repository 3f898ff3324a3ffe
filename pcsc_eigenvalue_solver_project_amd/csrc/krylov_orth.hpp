// The orthogonalisation and basis-rotation kernels the Krylov drivers share (krylov.hip: thick-restart
// Arnoldi; svds.hip: thick-restart Golub-Kahan-Lanczos), with their host launchers.  A basis is
// n x ncols, column-major; per step the host enqueues seven kernels and waits for nothing:
//   ks_dots_kernel     c = V_j^H w and w^H w in one pass: a thread owns rows, a chunk of kDotCols
//                      columns at a time is summed in registers (w is read again per chunk, from
//                      the caches: 1 / kDotCols of the pass), one ordered partial per workgroup.
//   ks_final_kernel    adds the partials in a fixed order (one wave per output); h (+)= c.
//   ks_update_kernel   w -= V_j c with c in LDS, and the workgroup's partial of ||w||^2 of the
//                      result, so that beta costs no pass of its own.
//   ks_norm_kernel     every workgroup adds the ||w||^2 partials in the same fixed order, then
//                      v_{j+1} = w / beta; workgroup 0 stores the column of S, beta and, for a step
//                      with beta <= floor_mult 2^-52 ||w before||, the breakdown word (w = 0 then).
// Per restart:
//   ks_mul_kernel      Out[:, :p] = V[:, :m] Q by row tiles: Q and the tile of V are staged in LDS,
//                      so the product runs in place (the rotation V[:, :p] <- V[:, :m] Q) and with
//                      a real V and a complex Q (the Ritz vectors of a real matrix).
// No floating-point atomics: every reduction is ordered workgroup partials plus a fixed-order final
// sum, so two runs give identical bits.  ncols = 0 is a supported step: h is empty and the step
// only takes the norm and scales.
#pragma once

#include <algorithm>

#include "kernels_common.hpp"
#include "scratch.hpp"

namespace eigsol {

namespace dev {
namespace ks {

constexpr int kMaxBasis = 64;   // most columns of V a step orthogonalises against
constexpr int kDotCols = 8;     // columns a thread sums at a time in ks_dots_kernel
constexpr int kOutCols = 4;     // output columns a thread sums at a time in ks_mul_kernel

__device__ __forceinline__ double conj_mul(double a, double b) { return a * b; }
__device__ __forceinline__ cplx conj_mul(cplx a, cplx b) {
    return cplx{a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
__device__ __forceinline__ double wave_sum_s(double v) { return wave_sum(v); }
__device__ __forceinline__ cplx wave_sum_s(cplx v) { return cplx{wave_sum(v.re), wave_sum(v.im)}; }
__device__ __forceinline__ double real_of(double v) { return v; }
__device__ __forceinline__ double real_of(cplx v) { return v.re; }

// s + c += x y without the rounding of the product or of the sum (Ogita, Rump and Oishi's Dot2): the
// product's error by one fma, the sum's by TwoSum; s + c at the end is the dot product as if it
// had been summed in twice the working precision and rounded once.
__device__ __forceinline__ void comp_mac(double& s, double& c, double x, double y) {
    const double p = x * y;
    const double ep = fma(x, y, -p);
    const double t = s + p;
    const double b = t - s;
    const double es = (s - (t - b)) + (p - b);
    s = t;
    c += ep + es;
}
// acc (sum s, compensation c, both of the output type) += v q
__device__ __forceinline__ void comp_acc(cplx& s, cplx& c, double v, cplx q) {
    comp_mac(s.re, c.re, v, q.re);
    comp_mac(s.im, c.im, v, q.im);
}
__device__ __forceinline__ void comp_acc(cplx& s, cplx& c, cplx v, cplx q) {
    comp_mac(s.re, c.re, v.re, q.re);
    comp_mac(s.re, c.re, -v.im, q.im);
    comp_mac(s.im, c.im, v.re, q.im);
    comp_mac(s.im, c.im, v.im, q.re);
}
__device__ __forceinline__ void comp_acc(double& s, double& c, double v, double q) { comp_mac(s, c, v, q); }

// sum of v over the workgroup in a fixed order (xor butterfly, then the waves in ascending order);
// valid in every thread
__device__ __forceinline__ double block_sum_all(double v, double* sm /*kWaves*/) {
    v = wave_sum(v);
    __syncthreads();   // sm may still be read from a previous call
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sm[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) s += sm[i];
    return s;
}

// ------------------------------------------------------------------ c = V^H w, w^H w
// part[blockIdx][0 .. ncols): this workgroup's partial of V[:, c]^H w; part[blockIdx][ncols]: of w^H w.
template <class S>
__global__ __launch_bounds__(kThreads) void ks_dots_kernel(const S* __restrict__ V, int64_t ldv, int ncols,
                                                           const S* __restrict__ w, int64_t n,
                                                           S* __restrict__ part) {
    __shared__ S red[kWaves * (kDotCols + 1)];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    S* mine = part + (size_t)blockIdx.x * (ncols + 1);
    const int64_t first = (int64_t)blockIdx.x * kThreads + t, stride = (int64_t)gridDim.x * kThreads;
    for (int c0 = 0; c0 == 0 || c0 < ncols; c0 += kDotCols) {
        const int nc = ncols - c0 < kDotCols ? ncols - c0 : kDotCols;   // workgroup-uniform
        S acc[kDotCols], accw = s_zero<S>();
#pragma unroll
        for (int i = 0; i < kDotCols; ++i) acc[i] = s_zero<S>();
        const S* base = V + (size_t)c0 * ldv;
        if (nc == kDotCols) {
            for (int64_t r = first; r < n; r += stride) {
                const S wr = w[r];
                S v[kDotCols];
#pragma unroll
                for (int i = 0; i < kDotCols; ++i) v[i] = base[(size_t)i * ldv + r];
#pragma unroll
                for (int i = 0; i < kDotCols; ++i) acc[i] = add(acc[i], conj_mul(v[i], wr));
                if (c0 == 0) accw = add(accw, conj_mul(wr, wr));
            }
        } else {
            for (int64_t r = first; r < n; r += stride) {
                const S wr = w[r];
#pragma unroll
                for (int i = 0; i < kDotCols; ++i)
                    if (i < nc) acc[i] = add(acc[i], conj_mul(base[(size_t)i * ldv + r], wr));
                if (c0 == 0) accw = add(accw, conj_mul(wr, wr));
            }
        }
        __syncthreads();   // red is free again
#pragma unroll
        for (int i = 0; i < kDotCols; ++i) {
            const S s = wave_sum_s(acc[i]);
            if (lane == 0) red[wv * (kDotCols + 1) + i] = s;
        }
        if (c0 == 0) {
            const S s = wave_sum_s(accw);
            if (lane == 0) red[wv * (kDotCols + 1) + kDotCols] = s;
        }
        __syncthreads();
        if (t < nc || (t == kDotCols && c0 == 0)) {
            S s = red[t];
#pragma unroll
            for (int q = 1; q < kWaves; ++q) s = add(s, red[q * (kDotCols + 1) + t]);
            mine[t == kDotCols ? ncols : c0 + t] = s;
        }
    }
}

// c[e] = the sum of part[g][e] over the workgroups g in a fixed order, e < ncols, and h (+)= c
// (pass 0 stores, pass 1 adds); e == ncols: scal[0] = w^H w (pass 0 only: the norm before the
// orthogonalisation).  One wave per output: lane l adds g = l, l + 64, ... ascending, then the butterfly.
template <class S>
__global__ __launch_bounds__(kThreads) void ks_final_kernel(const S* __restrict__ part, int nparts, int ncols, int pass,
                                                            S* __restrict__ c, S* __restrict__ h,
                                                            double* __restrict__ scal) {
    const int e = blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform
    if (e > ncols) return;
    const int lane = threadIdx.x & 63;
    S s = s_zero<S>();
    for (int g = lane; g < nparts; g += 64) s = add(s, part[(size_t)g * (ncols + 1) + e]);
    s = wave_sum_s(s);
    if (lane != 0) return;
    if (e == ncols) {
        if (pass == 0) scal[0] = real_of(s);
        return;
    }
    c[e] = s;
    h[e] = pass ? add(h[e], s) : s;
}

// w -= V c; npart[blockIdx] = this workgroup's partial of ||w||^2 of the result
template <class S>
__global__ __launch_bounds__(kThreads) void ks_update_kernel(const S* __restrict__ V, int64_t ldv, int ncols,
                                                             S* __restrict__ w, int64_t n, const S* __restrict__ c,
                                                             double* __restrict__ npart) {
    __shared__ S cs[kMaxBasis];
    __shared__ double sm[kWaves];
    const int t = threadIdx.x;
    if (t < ncols) cs[t] = c[t];
    __syncthreads();
    double a2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + t; r < n; r += stride) {
        S acc = w[r];
        const S* row = V + r;
        int i = 0;
        for (; i + 4 <= ncols; i += 4) {
            const S v0 = row[(size_t)i * ldv], v1 = row[(size_t)(i + 1) * ldv];
            const S v2 = row[(size_t)(i + 2) * ldv], v3 = row[(size_t)(i + 3) * ldv];
            acc = sub(acc, mul(v0, cs[i]));
            acc = sub(acc, mul(v1, cs[i + 1]));
            acc = sub(acc, mul(v2, cs[i + 2]));
            acc = sub(acc, mul(v3, cs[i + 3]));
        }
        for (; i < ncols; ++i) acc = sub(acc, mul(row[(size_t)i * ldv], cs[i]));
        w[r] = acc;
        a2 += sq_abs(acc);
    }
    a2 = block_sum_all(a2, sm);
    if (t == 0) npart[blockIdx.x] = a2;
}

// beta = sqrt(sum of npart) (every workgroup adds the partials in the same order); a breakdown is
// beta <= floor_mult 2^-52 sqrt(scal[0]) (or a beta that is not a number); w <- w / beta, or 0 on a
// breakdown.  Workgroup 0: scol[0 .. ncols) = h, scol[ncols] = beta (0 on a breakdown), when scol;
// scal[1] = beta; *bword = ncols on the first breakdown since the word was cleared.
template <class S>
__global__ __launch_bounds__(kThreads) void ks_norm_kernel(S* __restrict__ w, int64_t n, const double* __restrict__ npart,
                                                           int nparts, int ncols, double floor_mult,
                                                           const S* __restrict__ h, S* __restrict__ scol,
                                                           double* __restrict__ scal, int32_t* __restrict__ bword) {
    __shared__ double sm[kWaves];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int g = t; g < nparts; g += kThreads) s += npart[g];
    const double beta = sqrt(block_sum_all(s, sm));
    const double wn = sqrt(scal[0]);
    const bool broke = !(beta > floor_mult * 0x1p-52 * wn);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + t; r < n; r += stride)
        w[r] = broke ? s_zero<S>() : divr(w[r], beta);
    if (blockIdx.x != 0) return;
    if (scol && t < ncols) scol[t] = h[t];
    if (t == 0) {
        if (scol) set_re_im(scol[ncols], broke ? 0.0 : beta, 0.0);
        scal[1] = beta;
        if (broke && *bword == 0) *bword = ncols;
    }
}

// ------------------------------------------------------------------ Out[:, :p] = V[:, :m] Q
// V: n x m (SI, column-major, ldv), Q: m x p (SO, column-major), Out: n x p (SO, column-major, ldo);
// Out may be V (SI == SO): a workgroup stages its TR-row tile of V in LDS before it writes the
// tile's rows of Out, and tiles share no rows.  A thread owns a row of the tile and sums kOutCols
// output columns at a time over l ascending; the 256 / TR column groups split the p columns.
// The sums are compensated (comp_mac): the rotation is applied once per restart to a basis whose
// orthonormality every later step relies on, and its cost is LDS reads, not flops, so each entry
// is the product rounded once instead of carrying an error that grows with m.
// Dynamic LDS: [Q: m p SO | tile: TR m SI, column l of the tile at l * TR].
template <class SI, class SO, int TR>
__global__ __launch_bounds__(kThreads) void ks_mul_kernel(const SI* V, int64_t ldv, int64_t n, int m, int p,
                                                          const SO* __restrict__ Q, SO* Out, int64_t ldo) {
    extern __shared__ __align__(16) unsigned char ks_lds[];
    SO* qs = reinterpret_cast<SO*>(ks_lds);
    SI* tile = reinterpret_cast<SI*>(ks_lds + (((size_t)m * p * sizeof(SO) + 15) & ~(size_t)15));
    constexpr int kGroups = kThreads / TR;
    const int t = threadIdx.x, r = t % TR, g = t / TR;
    for (int i = t; i < m * p; i += kThreads) qs[i] = Q[i];
    for (int64_t r0 = (int64_t)blockIdx.x * TR; r0 < n; r0 += (int64_t)gridDim.x * TR) {
        __syncthreads();   // Q is staged; the previous tile has been read
        for (int idx = t; idx < TR * m; idx += kThreads) {
            const int rr = idx % TR, l = idx / TR;
            tile[idx] = r0 + rr < n ? V[(size_t)l * ldv + r0 + rr] : s_zero<SI>();
        }
        __syncthreads();
        for (int i0 = g * kOutCols; i0 < p; i0 += kGroups * kOutCols) {
            SO acc[kOutCols], cmp[kOutCols];
            const SO* qc[kOutCols];
#pragma unroll
            for (int u = 0; u < kOutCols; ++u) {
                acc[u] = cmp[u] = s_zero<SO>();
                qc[u] = qs + (size_t)(i0 + u < p ? i0 + u : p - 1) * m;   // past p: a copy that is not stored
            }
            for (int l = 0; l < m; ++l) {
                const SI v = tile[l * TR + r];
#pragma unroll
                for (int u = 0; u < kOutCols; ++u) comp_acc(acc[u], cmp[u], v, qc[u][l]);
            }
            if (r0 + r < n) {
#pragma unroll
                for (int u = 0; u < kOutCols; ++u)
                    if (i0 + u < p) Out[(size_t)(i0 + u) * ldo + r0 + r] = add(acc[u], cmp[u]);
            }
        }
    }
}

}  // namespace ks
}  // namespace dev

namespace ks = dev::ks;

inline int row_grid(int64_t n, int num_cus) {
    const int64_t want = (n + dev::kThreads - 1) / dev::kThreads;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, 4 * (int64_t)std::max(num_cus, 1)));
}

// device workspace of the orthogonalisation kernels
template <class S>
struct OrthWs {
    DevBuf part, c, h, npart, scal, bword;
    int grid = 1;
    int alloc(const eigsol_ctx* ctx, int64_t n, hipStream_t st) {
        grid = row_grid(n, ctx->num_cus);
        EIGSOL_TRY(part.alloc((size_t)grid * (ks::kMaxBasis + 1) * sizeof(S)));
        EIGSOL_TRY(c.alloc(ks::kMaxBasis * sizeof(S)));
        EIGSOL_TRY(h.alloc(ks::kMaxBasis * sizeof(S)));
        EIGSOL_TRY(npart.alloc((size_t)grid * sizeof(double)));
        EIGSOL_TRY(scal.alloc(4 * sizeof(double)));
        EIGSOL_TRY(bword.alloc(sizeof(int32_t)));
        EIGSOL_HIP(hipMemsetAsync(scal.p, 0, 4 * sizeof(double), st));
        EIGSOL_HIP(hipMemsetAsync(bword.p, 0, sizeof(int32_t), st));
        return EIGSOL_OK;
    }
};

// one step: w against the ncols columns of V (two passes), then normalised; scol: the column of S
template <class S>
int orth_step(OrthWs<S>& ws, const S* V, int64_t ldv, int ncols, S* w, int64_t n, S* scol, double floor_mult,
              hipStream_t st) {
    const dim3 blk(dev::kThreads), grid(ws.grid);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL((ks::ks_dots_kernel<S>), grid, blk, 0, st, V, ldv, ncols, (const S*)w, n, ws.part.template as<S>());
        EIGSOL_HIP(hipGetLastError());
        hipLaunchKernelGGL((ks::ks_final_kernel<S>), dim3((ncols + 1 + dev::kWaves - 1) / dev::kWaves), blk, 0, st,
                           (const S*)ws.part.template as<S>(), ws.grid, ncols, pass, ws.c.template as<S>(),
                           ws.h.template as<S>(), ws.scal.template as<double>());
        EIGSOL_HIP(hipGetLastError());
        hipLaunchKernelGGL((ks::ks_update_kernel<S>), grid, blk, 0, st, V, ldv, ncols, w, n,
                           (const S*)ws.c.template as<S>(), ws.npart.template as<double>());
        EIGSOL_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((ks::ks_norm_kernel<S>), grid, blk, 0, st, w, n, (const double*)ws.npart.template as<double>(),
                       ws.grid, ncols, floor_mult, (const S*)ws.h.template as<S>(), scol, ws.scal.template as<double>(),
                       ws.bword.template as<int32_t>());
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

// Out[:, :p] = V[:, :m] Q with Q (m x p, column-major) on the device
template <class SI, class SO>
int launch_mul(const eigsol_ctx* ctx, const SI* V, int64_t ldv, int64_t n, int m, int p, const SO* Q, SO* Out,
               int64_t ldo, hipStream_t st) {
    constexpr int TR = sizeof(SI) == 8 ? 64 : 32;   // 512-byte column segments of the tile
    const size_t lds = (((size_t)m * p * sizeof(SO) + 15) & ~(size_t)15) + (size_t)TR * m * sizeof(SI);
    auto kern = ks::ks_mul_kernel<SI, SO, TR>;
    if (lds > 65536)
        EIGSOL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
    const int64_t tiles = (n + TR - 1) / TR;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, 2 * (int64_t)std::max(ctx->num_cus, 1)));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(dev::kThreads), lds, st, V, ldv, n, m, p, Q, Out, ldo);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

}  // namespace eigsol
