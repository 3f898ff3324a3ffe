// Block subspace iteration (orthogonal iteration with Rayleigh-Ritz): the k dominant eigenpairs
// of a sparse or a dense matrix, plus the sparse block product Y = A X it is built on (the dense
// one: dense_block.hip).  The driver reaches the matrix through LinearOp (linear_op.hpp).
//
// Block vectors are n x m, row-major interleaved: X[i * m + j], the vector index fastest, so the m
// scalars one matrix entry needs are one contiguous segment.
//
// Kernels (double and complex double):
//   csr_spmm_kernel       Y = A X on the plain CSR arrays.  A group of MP lanes (m padded to a
//                         power of two) owns a row; lane j runs the row's ascending-column
//                         sequential sum for column j with the same mul / add as the SpMV kernels,
//                         so column j of Y is bitwise what eigsol_csr_spmv gives for column j of X.
//   gram_kernel           G = Z^H Z and B = Q^H Z (m x m) in one pass over Q and Z: every workgroup
//   gram_final_kernel     writes the partial of its row tiles, the final kernel adds the partials
//                         in a fixed order.  No floating-point atomics; two runs give equal bits.
//   chol_kernel           one workgroup: G = R^H R, then R^-1; a pivot that is not positive or
//                         below m 2^-52 max diag(G) writes 1 + its index to an error word.
//   block_mul_kernel      Out = In M (n x mi by mi x mo), optionally minus Xs diag(theta): the
//                         update Q <- Z R^-1, the Ritz vectors X = Q Y and the residual block
//                         Z Y - X Theta.
//
// Out of scope: single precision, double-double, row-sharded matrices and a
// session / step form (one call runs the whole iteration).
#include <algorithm>
#include <cmath>
#include <complex>

#include "kernels_common.hpp"
#include "linear_op.hpp"
#include "scratch.hpp"
#include "small_eig.hpp"

namespace eigsol {
namespace dev {

constexpr int kMaxBlock = 32;

template <class S> __device__ __forceinline__ S conj_mul(S a, S b);
template <> __device__ __forceinline__ double conj_mul<double>(double a, double b) { return a * b; }
template <> __device__ __forceinline__ cplx conj_mul<cplx>(cplx a, cplx b) {
    return cplx{a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
template <class D, class T> __device__ __forceinline__ D to_scalar(T v);
template <> __device__ __forceinline__ double to_scalar<double, double>(double v) { return v; }
template <> __device__ __forceinline__ cplx to_scalar<cplx, cplx>(cplx v) { return v; }
template <> __device__ __forceinline__ cplx to_scalar<cplx, double>(double v) { return cplx{v, 0.0}; }
__device__ __forceinline__ double real_of(double v) { return v; }
__device__ __forceinline__ double real_of(cplx v) { return v.re; }
__device__ __forceinline__ double scale_r(double v, double r) { return v * r; }
__device__ __forceinline__ cplx scale_r(cplx v, double r) { return cplx{v.re * r, v.im * r}; }
template <class S> __device__ __forceinline__ S from_real(double r);
template <> __device__ __forceinline__ double from_real<double>(double r) { return r; }
template <> __device__ __forceinline__ cplx from_real<cplx>(double r) { return cplx{r, 0.0}; }

// ------------------------------------------------------------------ Y = A X
// 256 / MP rows per workgroup.  The rows of a workgroup own one contiguous range of entries: the
// workgroup copies it (columns and values, coalesced) into LDS in windows of kSpmmCap entries, and
// the lanes of a row's group then read the same (column, value) pair from LDS and the contiguous
// segment X[c * m .. c * m + m) from memory.  That leaves one dependent memory round trip per four
// entries of a row instead of two (column, then x).  The sum of a row runs on across windows.
constexpr int kSpmmCap = 512;

template <class S, int MP>
__global__ __launch_bounds__(kThreads) void csr_spmm_kernel(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const S* __restrict__ val, int64_t nrows, int m,
                                                            const S* __restrict__ X, S* __restrict__ Y) {
    constexpr int kRows = kThreads / MP;
    __shared__ int32_t cs[kSpmmCap];
    __shared__ S vs[kSpmmCap];
    const int j = threadIdx.x % MP;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    const int64_t r1 = r0 + kRows < nrows ? r0 + kRows : nrows;
    const int64_t r = r0 + threadIdx.x / MP;
    const bool live = r < nrows && j < m;
    const int eb = rowptr[r0], ee = rowptr[r1];   // workgroup-uniform (r0 < nrows by the grid size)
    int rb = 0, re = 0;
    if (r < nrows) {
        rb = rowptr[r];
        re = rowptr[r + 1];
    }
    S acc = s_zero<S>();
    for (int base = eb; base < ee; base += kSpmmCap) {
        const int cnt = ee - base < kSpmmCap ? ee - base : kSpmmCap;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += kThreads) {
            cs[i] = col[base + i];
            vs[i] = val[base + i];
        }
        __syncthreads();
        if (!live) continue;
        int e = (rb > base ? rb : base) - base;
        const int e1 = (re < base + cnt ? re : base + cnt) - base;
        for (; e + 4 <= e1; e += 4) {
            const S x0 = X[(size_t)cs[e] * m + j], x1 = X[(size_t)cs[e + 1] * m + j];
            const S x2 = X[(size_t)cs[e + 2] * m + j], x3 = X[(size_t)cs[e + 3] * m + j];
            acc = add(acc, mul(vs[e], x0));
            acc = add(acc, mul(vs[e + 1], x1));
            acc = add(acc, mul(vs[e + 2], x2));
            acc = add(acc, mul(vs[e + 3], x3));
        }
        for (; e < e1; ++e) acc = add(acc, mul(vs[e], X[(size_t)cs[e] * m + j]));
    }
    if (live) Y[(size_t)r * m + j] = acc;
}

// ------------------------------------------------------------------ G = Z^H Z, B = Q^H Z
// Tiles of kTR rows are staged in LDS (a tile of a row-major block is one contiguous range).  A
// thread owns a kT x kT block of outputs (kT = 4; LDS reads per product drop with the block size),
// kNT threads cover the m x m outputs, and the 256 / kNT groups of such threads split a tile's rows
// into slots (row r of the tile goes to slot r % kSlots).  A workgroup walks its tiles in
// ascending order and adds its slots in ascending order at the end; its partial goes to
// part[blockIdx][G (m*m) | B (m*m)].
template <int MP> struct GramShape {
    static constexpr int kT = MP >= 4 ? 4 : MP;
    static constexpr int kNB = MP / kT;                  // output blocks per dimension
    static constexpr int kNT = kNB * kNB;                // threads that cover the outputs
    static constexpr int kSlots = kThreads / kNT;        // row slots
    static constexpr int kTR = kSlots > 32 ? kSlots : 32;   // rows per tile
};

template <class S, int MP>
__global__ __launch_bounds__(kThreads) void gram_kernel(const S* __restrict__ Q, const S* __restrict__ Z,
                                                        int64_t n, int m, int want_b, S* __restrict__ part) {
    using Sh = GramShape<MP>;
    constexpr int T = Sh::kT;
    __shared__ S zs[Sh::kTR * MP];
    __shared__ S qs[Sh::kTR * MP];
    __shared__ S red[kThreads];
    const int t = threadIdx.x;
    const int slot = t / Sh::kNT, w = t % Sh::kNT;
    const int a0 = (w / Sh::kNB) * T, b0 = (w % Sh::kNB) * T;
    S accg[T][T], accb[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int k = 0; k < T; ++k) accg[i][k] = accb[i][k] = s_zero<S>();
    const int64_t ntiles = (n + Sh::kTR - 1) / Sh::kTR;
    const int tile_elems = Sh::kTR * m;
    const size_t total = (size_t)n * m;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = (size_t)tile * Sh::kTR * m;
        __syncthreads();
        for (int i = t; i < tile_elems; i += kThreads) {
            const bool in = base + i < total;
            zs[i] = in ? Z[base + i] : s_zero<S>();
            if (want_b) qs[i] = in ? Q[base + i] : s_zero<S>();
        }
        __syncthreads();
        if (a0 >= m || b0 >= m) continue;   // no output of this thread is wanted (the barriers above are reached)
        for (int r = slot; r < Sh::kTR; r += Sh::kSlots) {
            S za[T], zb[T], qa[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                za[i] = a0 + i < m ? zs[r * m + a0 + i] : s_zero<S>();
                zb[i] = b0 + i < m ? zs[r * m + b0 + i] : s_zero<S>();
                qa[i] = (want_b && a0 + i < m) ? qs[r * m + a0 + i] : s_zero<S>();
            }
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int k = 0; k < T; ++k) {
                    accg[i][k] = add(accg[i][k], conj_mul<S>(za[i], zb[k]));
                    if (want_b) accb[i][k] = add(accb[i][k], conj_mul<S>(qa[i], zb[k]));
                }
        }
    }
    S* mine = part + (size_t)blockIdx.x * 2 * m * m;
    for (int which = 0; which < (want_b ? 2 : 1); ++which)
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int k = 0; k < T; ++k) {
                __syncthreads();
                red[t] = which ? accb[i][k] : accg[i][k];
                __syncthreads();
                if (slot == 0 && a0 + i < m && b0 + k < m) {
                    S s = red[w];
                    for (int q = 1; q < Sh::kSlots; ++q) s = add(s, red[q * Sh::kNT + w]);
                    mine[which * m * m + (a0 + i) * m + b0 + k] = s;
                }
            }
}

// out[e], e < count: the sum of part[g][e] over the workgroups g in a fixed order.  One wave per
// output: lane l adds the partials g = l, l + 64, ... in ascending order, then the xor butterfly.
__device__ __forceinline__ double wave_sum_s(double v) { return wave_sum(v); }
__device__ __forceinline__ cplx wave_sum_s(cplx v) { return cplx{wave_sum(v.re), wave_sum(v.im)}; }

template <class S>
__global__ __launch_bounds__(kThreads) void gram_final_kernel(const S* __restrict__ part, int nparts, int stride,
                                                              int count, S* __restrict__ out) {
    const int e = blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform
    if (e >= count) return;
    const int lane = threadIdx.x & 63;
    S s = s_zero<S>();
    for (int g = lane; g < nparts; g += 64) s = add(s, part[(size_t)g * stride + e]);
    s = wave_sum_s(s);
    if (lane == 0) out[e] = s;
}

// ------------------------------------------------------------------ G = R^H R, Rinv = R^-1
// One workgroup, right-looking.  *err = 0, or 1 + the index of the first pivot that is not positive
// or below m 2^-52 max diag(G); R^-1 is then the identity, so what follows stays finite until the
// host reads the word.
template <class S>
__global__ __launch_bounds__(kThreads) void chol_kernel(const S* __restrict__ G, int m, S* __restrict__ Rinv,
                                                        int32_t* __restrict__ err) {
    __shared__ S g[kMaxBlock * kMaxBlock];
    __shared__ double s_piv, s_thr;
    __shared__ int s_bad;
    const int t = threadIdx.x;
    for (int i = t; i < m * m; i += kThreads) g[i] = G[i];
    if (t == 0) s_bad = 0;
    __syncthreads();
    if (t == 0) {
        double mx = 0.0;
        for (int i = 0; i < m; ++i) mx = fmax(mx, real_of(g[i * m + i]));
        s_thr = (double)m * 0x1p-52 * mx;
    }
    __syncthreads();
    for (int k = 0; k < m; ++k) {
        if (t == 0) {
            const double d = real_of(g[k * m + k]);
            if (!(d > 0.0) || d < s_thr) s_bad = k + 1;
            else s_piv = sqrt(d);
        }
        __syncthreads();
        if (s_bad) break;   // block-uniform
        const double p = s_piv;
        if (t == k) g[k * m + k] = from_real<S>(p);
        if (t > k && t < m) g[k * m + t] = scale_r(g[k * m + t], 1.0 / p);
        __syncthreads();
        for (int idx = t; idx < m * m; idx += kThreads) {
            const int i = idx / m, j = idx % m;
            if (i > k && j >= i) g[idx] = sub(g[idx], conj_mul<S>(g[k * m + i], g[k * m + j]));
        }
        __syncthreads();
    }
    if (s_bad) {
        for (int i = t; i < m * m; i += kThreads) Rinv[i] = (i / m == i % m) ? from_real<S>(1.0) : s_zero<S>();
        if (t == 0) *err = s_bad;
        return;
    }
    // column j of R^-1 by back substitution (thread j); the diagonal of R is real and positive
    if (t < m) {
        const int j = t;
        S x[kMaxBlock];
#pragma unroll
        for (int i = 0; i < kMaxBlock; ++i) x[i] = s_zero<S>();
        for (int i = m - 1; i >= 0; --i) {
            if (i > j) continue;
            if (i == j) {
                x[i] = from_real<S>(1.0 / real_of(g[i * m + i]));
            } else {
                S s = s_zero<S>();
                for (int k = i + 1; k <= j; ++k) s = add(s, mul(g[i * m + k], x[k]));
                x[i] = scale_r(s, -1.0 / real_of(g[i * m + i]));
            }
        }
        for (int i = 0; i < m; ++i) Rinv[i * m + j] = x[i];
    }
    if (t == 0) *err = 0;
}

// ------------------------------------------------------------------ Out = In M [- Xs diag(theta)]
// In: n x mi (SI), M: mi x mo (SO, row-major, staged in LDS), Out / Xs: n x mo (SO).  MP >= mo lanes
// per row; each lane sums over the row's mi entries in ascending order.
template <class SI, class SO, int MP>
__global__ __launch_bounds__(kThreads) void block_mul_kernel(const SI* __restrict__ In, int64_t n, int mi, int mo,
                                                             const SO* __restrict__ M, const SO* __restrict__ Xs,
                                                             const SO* __restrict__ theta, SO* __restrict__ Out) {
    __shared__ SO ms[kMaxBlock * kMaxBlock];
    for (int i = threadIdx.x; i < mi * mo; i += kThreads) ms[i] = M[i];
    __syncthreads();
    constexpr int kRows = kThreads / MP;
    const int j = threadIdx.x % MP;
    if (j >= mo) return;
    for (int64_t r = (int64_t)blockIdx.x * kRows + threadIdx.x / MP; r < n; r += (int64_t)gridDim.x * kRows) {
        const SI* row = In + (size_t)r * mi;
        SO acc = s_zero<SO>();
        for (int l = 0; l < mi; ++l) acc = add(acc, mul(to_scalar<SO>(row[l]), ms[l * mo + j]));
        if (Xs) acc = sub(acc, mul(Xs[(size_t)r * mo + j], theta[j]));
        Out[(size_t)r * mo + j] = acc;
    }
}

}  // namespace dev

// ====================================================================================== host
namespace {

using cd = std::complex<double>;

inline int pad_width(int m) {
    int p = 1;
    while (p < m) p <<= 1;
    return p;
}

// calls f(std::integral_constant<int, MP>) for the padded width of m (1..32)
template <class F>
int with_width(int m, F&& f) {
    switch (pad_width(m)) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: return f(std::integral_constant<int, 32>{});
    }
}

template <class S>
int launch_spmm(const eigsol_csr* A, int m, const S* X, S* Y, hipStream_t st) {
    if (A->nrows == 0) return EIGSOL_OK;
    return with_width(m, [&](auto w) {
        constexpr int MP = decltype(w)::value;
        const int64_t rows_per = dev::kThreads / MP;
        const int64_t grid = (A->nrows + rows_per - 1) / rows_per;
        hipLaunchKernelGGL((dev::csr_spmm_kernel<S, MP>), dim3((unsigned)grid), dim3(dev::kThreads), 0, st, A->rowptr,
                           A->col, (const S*)A->val, A->nrows, m, X, Y);
        EIGSOL_HIP(hipGetLastError());
        return (int)EIGSOL_OK;
    });
}

// Z = A Q: the CSR kernel above, or the MFMA block product of the dense matrix
template <class S>
int launch_product(const LinearOp& A, int m, const S* X, S* Y, hipStream_t st) {
    if (A.csr) return launch_spmm<S>(A.csr, m, X, Y, st);
    return dense_gemm_launch(A.dense, m, X, Y);
}

inline int gram_grid(int64_t n, int m, int num_cus) {
    const int mp = pad_width(m);
    const int t = std::min(mp, 4), slots = dev::kThreads / ((mp / t) * (mp / t));
    const int tr = std::max(slots, 32);   // GramShape<mp>::kTR
    const int64_t ntiles = (n + tr - 1) / tr;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, 4 * (int64_t)std::max(num_cus, 1)));
}

// out = [G = Z^H Z | B = Q^H Z (when Q)], m x m each; part holds gram_grid() * 2 m^2 scalars
template <class S>
int launch_gram(const eigsol_ctx* ctx, const S* Q, const S* Z, int64_t n, int m, S* part, S* out, hipStream_t st) {
    const int grid = gram_grid(n, m, ctx->num_cus);
    const int want_b = Q ? 1 : 0;
    EIGSOL_TRY(with_width(m, [&](auto w) {
        constexpr int MP = decltype(w)::value;
        hipLaunchKernelGGL((dev::gram_kernel<S, MP>), dim3(grid), dim3(dev::kThreads), 0, st, Q ? Q : Z, Z, n, m,
                           want_b, part);
        EIGSOL_HIP(hipGetLastError());
        return (int)EIGSOL_OK;
    }));
    const int count = (want_b ? 2 : 1) * m * m;
    hipLaunchKernelGGL((dev::gram_final_kernel<S>), dim3((count + dev::kWaves - 1) / dev::kWaves),
                       dim3(dev::kThreads), 0, st, part, grid, 2 * m * m, count, out);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class SI, class SO>
int launch_mul(const eigsol_ctx* ctx, const SI* In, int64_t n, int mi, int mo, const SO* M, const SO* Xs,
               const SO* theta, SO* Out, hipStream_t st) {
    return with_width(mo, [&](auto w) {
        constexpr int MP = decltype(w)::value;
        const int64_t rows_per = dev::kThreads / MP;
        const int64_t want = (n + rows_per - 1) / rows_per;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, 16 * (int64_t)std::max(ctx->num_cus, 1)));
        hipLaunchKernelGGL((dev::block_mul_kernel<SI, SO, MP>), dim3(grid), dim3(dev::kThreads), 0, st, In, n, mi, mo,
                           M, Xs, theta, Out);
        EIGSOL_HIP(hipGetLastError());
        return (int)EIGSOL_OK;
    });
}

// small_eig, ritz_order and host_of: small_eig.hpp (shared with krylov.hip)
using smalleig::host_of;
using smalleig::ritz_order;
using smalleig::small_eig;

template <class S>
int subspace_run(const LinearOp& A, const eigsol_subspace_options* o, const void* X0v, double* eigenvalues,
                 double* eigenvectors, double* residuals, int32_t* iterations, int32_t* converged) {
    const int64_t n = A.nrows();
    const int m = o->block, k = o->nev;
    const eigsol_ctx* ctx = A.ctx();
    hipStream_t st = ctx->stream;
    EIGSOL_HIP(hipSetDevice(ctx->device));
    const size_t nm = (size_t)n * m;
    const int gparts = gram_grid(n, dev::kMaxBlock, ctx->num_cus);   // the most workgroups any width uses
    DevBuf q, z, t, part, gb, gk, rinv, err, xk, rk, small;
    EIGSOL_TRY(q.alloc(nm * sizeof(S)));
    EIGSOL_TRY(z.alloc(nm * sizeof(S)));
    EIGSOL_TRY(t.alloc(nm * sizeof(S)));
    EIGSOL_TRY(part.alloc((size_t)gparts * 2 * m * m * sizeof(cplx)));
    EIGSOL_TRY(gb.alloc((size_t)2 * m * m * sizeof(S)));
    EIGSOL_TRY(gk.alloc((size_t)k * k * sizeof(cplx)));   // Gram matrix of the Ritz / residual block (G of the iteration stays in gb)
    EIGSOL_TRY(rinv.alloc((size_t)m * m * sizeof(S)));
    EIGSOL_TRY(err.alloc(4 * sizeof(int32_t)));
    EIGSOL_TRY(small.alloc((size_t)(m * m + m) * sizeof(cplx)));   // Y (m x k) and theta (k) for the final products
    S *Q = q.as<S>(), *Z = z.as<S>(), *T = t.as<S>(), *GB = gb.as<S>(), *RI = rinv.as<S>();
    int32_t* ERR = err.as<int32_t>();
    EIGSOL_HIP(hipMemsetAsync(ERR, 0, 4 * sizeof(int32_t), st));

    // X0: column-major n x m on the host -> row-major interleaved on the device (in Z)
    {
        const S* x0 = static_cast<const S*>(X0v);
        std::vector<S> xr(nm);
        for (int j = 0; j < m; ++j)
            for (int64_t i = 0; i < n; ++i) xr[(size_t)i * m + j] = x0[(size_t)j * n + i];
        EIGSOL_HIP(hipMemcpyAsync(Z, xr.data(), nm * sizeof(S), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(stream_wait(st));
    }

    // Q <- cholqr2(Z): two passes of G = Z^H Z, R = chol(G), Z R^-1 (through T); the first G may be
    // there already.  Error words 0 / 1 (first / second factorisation) are read at the next wait.
    auto cholqr2 = [&](bool have_g) -> int {
        if (!have_g) EIGSOL_TRY(launch_gram<S>(ctx, nullptr, Z, n, m, part.as<S>(), GB, st));
        hipLaunchKernelGGL((dev::chol_kernel<S>), dim3(1), dim3(dev::kThreads), 0, st, GB, m, RI, ERR);
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY((launch_mul<S, S>(ctx, Z, n, m, m, RI, nullptr, nullptr, T, st)));
        EIGSOL_TRY(launch_gram<S>(ctx, nullptr, T, n, m, part.as<S>(), GB, st));
        hipLaunchKernelGGL((dev::chol_kernel<S>), dim3(1), dim3(dev::kThreads), 0, st, GB, m, RI, ERR + 1);
        EIGSOL_HIP(hipGetLastError());
        EIGSOL_TRY((launch_mul<S, S>(ctx, T, n, m, m, RI, nullptr, nullptr, Q, st)));
        return EIGSOL_OK;
    };
    EIGSOL_TRY(cholqr2(false));

    using HS = typename host_of<S>::type;
    std::vector<HS> hB((size_t)m * m);
    int32_t herr[4] = {0, 0, 0, 0};
    std::vector<cd> Bc((size_t)m * m), w, Y, theta(m), theta_old;
    std::vector<cd> Yk((size_t)m * k);     // wanted Ritz vectors of B, row-major m x k
    std::vector<int> order;
    std::vector<double> xn(k), rn(k);
    int it = 0;
    bool conv = false;

    // column 2-norms of the n x k complex block V (the diagonal of V^H V), one host wait
    auto col_norms = [&](const cplx* V, std::vector<double>& out) -> int {
        EIGSOL_TRY(launch_gram<cplx>(ctx, nullptr, V, n, k, part.as<cplx>(), gk.as<cplx>(), st));
        std::vector<cd> g((size_t)k * k);
        EIGSOL_HIP(hipMemcpyAsync(g.data(), gk.p, g.size() * sizeof(cd), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        for (int j = 0; j < k; ++j) out[j] = std::sqrt(std::max(g[(size_t)j * k + j].real(), 0.0));
        return EIGSOL_OK;
    };
    // X = Q Ys, R = Z Ys - X diag(theta) for the wanted pairs, Ys = Yk with column j scaled by
    // scale[j]; then the column norms of X and R
    auto ritz_pass = [&](const std::vector<double>& scale) -> int {
        if (!xk.p) {
            EIGSOL_TRY(xk.alloc((size_t)n * k * sizeof(cplx)));
            EIGSOL_TRY(rk.alloc((size_t)n * k * sizeof(cplx)));
        }
        std::vector<cd> h((size_t)m * k + k);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < k; ++j) h[(size_t)i * k + j] = Yk[(size_t)i * k + j] * scale[j];
        for (int j = 0; j < k; ++j) h[(size_t)m * k + j] = theta[j];
        cplx* ys = small.as<cplx>();
        EIGSOL_HIP(hipMemcpyAsync(ys, h.data(), h.size() * sizeof(cd), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(stream_wait(st));   // h leaves scope
        EIGSOL_TRY((launch_mul<S, cplx>(ctx, Q, n, m, k, ys, nullptr, nullptr, xk.as<cplx>(), st)));
        EIGSOL_TRY((launch_mul<S, cplx>(ctx, Z, n, m, k, ys, xk.as<cplx>(), ys + (size_t)m * k, rk.as<cplx>(), st)));
        EIGSOL_TRY(col_norms(xk.as<cplx>(), xn));
        EIGSOL_TRY(col_norms(rk.as<cplx>(), rn));
        return EIGSOL_OK;
    };
    const std::vector<double> ones(k, 1.0);

    for (it = 1; it <= o->max_iterations; ++it) {
        EIGSOL_TRY(launch_product<S>(A, m, Q, Z, st));
        EIGSOL_TRY(launch_gram<S>(ctx, Q, Z, n, m, part.as<S>(), GB, st));
        // the iteration's one host wait: B and the error words of the factorisations before it
        EIGSOL_HIP(hipMemcpyAsync(hB.data(), GB + (size_t)m * m, hB.size() * sizeof(S), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(herr, ERR, sizeof(herr), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        for (int e = 0; e < 2; ++e)
            if (herr[e])
                return fail(EIGSOL_E_SOLVER, "subspace_iteration: block lost rank at column " +
                                                 std::to_string(herr[e] - 1) + " (pass " + std::to_string(e + 1) +
                                                 " of the orthonormalisation before product " + std::to_string(it) +
                                                 ")");
        bool finite = true;
        for (size_t i = 0; i < hB.size(); ++i) {
            Bc[i] = cd(hB[i]);
            finite = finite && std::isfinite(Bc[i].real()) && std::isfinite(Bc[i].imag());
        }
        if (!finite) return fail(EIGSOL_E_SOLVER, "subspace_iteration: the projected matrix is not finite");
        if (!small_eig(m, Bc, w, Y))
            return fail(EIGSOL_E_SOLVER, "subspace_iteration: eig of the projected matrix did not converge");
        order = ritz_order(w);
        theta_old.assign(theta.begin(), theta.begin() + k);
        for (int j = 0; j < m; ++j) theta[j] = w[order[j]];
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < k; ++j) Yk[(size_t)i * k + j] = Y[(size_t)i * m + order[j]];
        if (it > 1) {
            bool close = true;
            std::vector<char> used(k, 0);
            for (int j = 0; j < k && close; ++j) {
                int best = -1;
                double bd = 0.0;
                for (int l = 0; l < k; ++l) {
                    if (used[l]) continue;
                    const double d = std::abs(theta[j] - theta_old[l]);
                    if (best < 0 || d < bd) {
                        best = l;
                        bd = d;
                    }
                }
                used[best] = 1;
                close = close_rel(theta[j].real(), theta[j].imag(), theta_old[best].real(), theta_old[best].imag(),
                                  o->tolerance, true);
            }
            if (close && o->residual_tolerance != 0.0) {
                EIGSOL_TRY(ritz_pass(ones));
                for (int j = 0; j < k && close; ++j)
                    close = xn[j] > 0.0 && rn[j] / xn[j] <= o->residual_tolerance * (1.0 + std::abs(theta[j]));
            }
            if (close) {
                conv = true;
                break;
            }
        }
        if (it == o->max_iterations) break;
        EIGSOL_TRY(cholqr2(true));
    }
    if (it > o->max_iterations) it = o->max_iterations;

    // Ritz pairs of the last product: unit vectors, explicit residuals
    EIGSOL_TRY(ritz_pass(ones));
    std::vector<double> scale(k);
    for (int j = 0; j < k; ++j) {
        if (!(xn[j] > 0.0) || !std::isfinite(xn[j]))
            return fail(EIGSOL_E_SOLVER, "subspace_iteration: Ritz vector " + std::to_string(j) + " has no finite norm");
        scale[j] = 1.0 / xn[j];
    }
    EIGSOL_TRY(ritz_pass(scale));
    for (int j = 0; j < k; ++j) {
        eigenvalues[2 * j] = theta[j].real();
        eigenvalues[2 * j + 1] = theta[j].imag();
        if (residuals) residuals[j] = rn[j];
    }
    if (eigenvectors) {
        std::vector<cd> xr((size_t)n * k);
        EIGSOL_HIP(hipMemcpyAsync(xr.data(), xk.p, xr.size() * sizeof(cd), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(stream_wait(st));
        cd* ev = reinterpret_cast<cd*>(eigenvectors);
        for (int j = 0; j < k; ++j)
            for (int64_t i = 0; i < n; ++i) ev[(size_t)j * n + i] = xr[(size_t)i * k + j];
    }
    if (iterations) *iterations = it;
    if (converged) *converged = conv ? 1 : 0;
    return EIGSOL_OK;
}

// the checks every matrix kind shares, then the run
int subspace_entry(const LinearOp& A, int64_t ncols, const eigsol_subspace_options* opts, const void* X0,
                   double* eigenvalues, double* eigenvectors, double* residuals, int32_t* iterations,
                   int32_t* converged) {
    if (A.dtype() != EIGSOL_F64 && A.dtype() != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "subspace_iteration: only double and complex double matrices are supported");
    if (A.nrows() != ncols) return fail(EIGSOL_E_NOT_SQUARE, "subspace_iteration: matrix must be square");
    if (A.nrows() == 0) return fail(EIGSOL_E_ZERO_SIZE, "subspace_iteration: matrix has zero size");
    if (opts->nev < 1) return fail(EIGSOL_E_INVALID, "subspace_iteration: nev must be at least 1");
    if (opts->block < opts->nev) return fail(EIGSOL_E_INVALID, "subspace_iteration: block must be at least nev");
    if (opts->block > dev::kMaxBlock) return fail(EIGSOL_E_INVALID, "subspace_iteration: block must be at most 32");
    if (opts->block > A.nrows()) return fail(EIGSOL_E_INVALID, "subspace_iteration: block exceeds the matrix order");
    if (opts->max_iterations < 1) return fail(EIGSOL_E_INVALID, "subspace_iteration: max_iterations must be at least 1");
    if (A.dtype() == EIGSOL_C128)
        return subspace_run<cplx>(A, opts, X0, eigenvalues, eigenvectors, residuals, iterations, converged);
    return subspace_run<double>(A, opts, X0, eigenvalues, eigenvectors, residuals, iterations, converged);
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_csr_spmm(eigsol_csr* A, int32_t m, const void* X_dev, void* Y_dev) {
    if (!A || (!X_dev && A->ncols) || (!Y_dev && A->nrows))
        return fail(EIGSOL_E_INVALID, "eigsol_csr_spmm: null pointer");
    if (m < 1 || m > dev::kMaxBlock)
        return fail(EIGSOL_E_INVALID, "eigsol_csr_spmm: m must be in 1..32");
    if (A->dist) return fail(EIGSOL_E_UNSUPPORTED, "eigsol_csr_spmm: row-sharded matrix");
    if (A->dtype != EIGSOL_F64 && A->dtype != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_csr_spmm: only double and complex double matrices are supported");
    if (A->nrows == 0) return EIGSOL_OK;
    EIGSOL_HIP(hipSetDevice(A->ctx->device));
    if (A->dtype == EIGSOL_C128)
        return launch_spmm<cplx>(A, m, (const cplx*)X_dev, (cplx*)Y_dev, A->ctx->stream);
    return launch_spmm<double>(A, m, (const double*)X_dev, (double*)Y_dev, A->ctx->stream);
}

int eigsol_subspace_csr(eigsol_csr* A, const eigsol_subspace_options* opts, const void* X0,
                        double* eigenvalues, double* eigenvectors, double* residuals,
                        int32_t* iterations, int32_t* converged) {
    if (!A || !opts || !X0 || !eigenvalues)
        return fail(EIGSOL_E_INVALID, "eigsol_subspace_csr: null pointer");
    if (A->dist) return fail(EIGSOL_E_UNSUPPORTED, "subspace_iteration: row-sharded matrix");
    return subspace_entry(LinearOp(A), A->ncols, opts, X0, eigenvalues, eigenvectors, residuals, iterations,
                          converged);
}

int eigsol_subspace_dense(eigsol_dense* A, const eigsol_subspace_options* opts, const void* X0,
                          double* eigenvalues, double* eigenvectors, double* residuals,
                          int32_t* iterations, int32_t* converged) {
    if (!A || !opts || !X0 || !eigenvalues)
        return fail(EIGSOL_E_INVALID, "eigsol_subspace_dense: null pointer");
    return subspace_entry(LinearOp(A), A->ncols, opts, X0, eigenvalues, eigenvectors, residuals, iterations,
                          converged);
}

}  // extern "C"
