// C = A B on the fp64 matrix cores with both operands staged through LDS (gfx950; double and cplx; DESIGN.md
// section 28), and the plain kernels the matrix exponential runs around it (expm.hip): a linear combination of
// matrices plus a multiple of I, the scaling by 2^-s and the 1-norm.
//
// gemm_kernel.  A workgroup of four waves owns one TM x TN tile of C: 128 x 128 (double) or 128 x 64 (cplx), the
// waves 2 x 2, each with a 64 x 64 (64 x 32) piece as 4 x 4 (4 x 2) accumulator tiles of v_mfma_f64_16x16x4_f64.
// That is 128 accumulator registers per lane in both types, kept for the whole K loop; C is stored once and never
// read.  K advances in slices of BK = 16:
//   - every thread fetches its share of the next slice of A (TM x BK) and of B (BK x TN) from global memory into
//     registers (entries past an edge of A or B are fetched as zeros: edges are masked, nothing is padded in memory);
//   - the slice in LDS is consumed: four k-steps of 4, each 8 (6) ds_read_b64 and 16 (32) MFMAs per wave;
//   - barrier, the registers go to LDS, barrier.
// The global loads of slice s + 1 are in flight while slice s is multiplied, so one LDS buffer serves: 36 KB
// (double) or 54 KB (cplx, real and imaginary planes apart, so that both types read one double per lane and
// operand), two workgroups per CU.  A second LDS buffer would save one of the two barriers per 64 (128) MFMAs
// of a wave and cost the second workgroup.
//
// Operand fragments (mfma_rankk.hpp): the MFMA's A operand, lane l = B(k0 + (l >> 4), c0 + (l & 15)); its B
// operand, lane l = A(r0 + (l & 15), k0 + (l >> 4)); D lane l register r = C(r0 + (l & 15), c0 + (l >> 4) + 4 r), so 16
// lanes store 128 contiguous bytes of a column of C.  A complex product is four real MFMAs,
//   re += Bre Are - Bim Aim,   im += Bre Aim + Bim Are.
//
// LDS layout and banks (ds_read_b64: 64 banks of 4 bytes, conflicts within each half of 32 lanes, that is two
// values of l >> 4 and sixteen of l & 15):
//   A slice as sA[k][row], pitch TM + 16 = 144 doubles: 16 lanes read 32 consecutive banks and the next k lies
//     288 banks = 32 (mod 64) further: conflict-free.  It is global memory's own order, written 128 rows at a time.
//   B slice as sB[col][k], pitch BK + 2 = 18 doubles, which is also global memory's order (no transposition on the
//     way in): lane (l & 15, l >> 4) reads bank 36 (l & 15) + 2 (l >> 4) (mod 64); 36 j (mod 64) runs through 16
//     different multiples of 4, so the 32 lanes hit 32 different bank pairs: conflict-free.  The pitch 16 would put
//     all sixteen columns of one k on banks 0 (mod 32): 8-way.
// One output entry is summed by one lane in ascending k: no split-K, no atomics, the same bits on every run.
#include <algorithm>
#include <string>
#include <vector>

#include "gemm.hpp"
#include "mfma_rankk.hpp"
#include "scratch.hpp"

namespace eigsol {
namespace dev {

template <class S>
struct GemmShape {
    static constexpr bool kC = std::is_same_v<S, cplx>;
    static constexpr int WM = 4, WN = kC ? 2 : 4;      // accumulator tiles of a wave
    static constexpr int TM = 32 * WM, TN = 32 * WN;   // the workgroup's tile of C
    static constexpr int BK = 16;
    static constexpr int LDA = TM + 16, LDB = BK + 2;
    static constexpr int P = kC ? 2 : 1;               // planes: re, im
    static constexpr int NA = TM * BK / 256, NBL = BK * TN / 256;   // entries of a slice per thread
};

template <class S>
__global__ __launch_bounds__(256, 2) void gemm_kernel(int m, int n, int k, const S* __restrict__ A, int64_t lda,
                                                      const S* __restrict__ B, int64_t ldb, S* __restrict__ C, int64_t ldc) {
    using G = GemmShape<S>;
    constexpr bool kC = G::kC;
    __shared__ double sA[G::P][G::BK * G::LDA];
    __shared__ double sB[G::P][G::TN * G::LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int bm = blockIdx.x * G::TM, bn = blockIdx.y * G::TN;
    const int wr = 16 * G::WM * (wave & 1), wc = 16 * G::WN * (wave >> 1);
    S pa[G::NA], pb[G::NBL];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < G::NA; ++j) {
            const int row = bm + (tid & (G::TM - 1)), kk = k0 + (tid >> 7) + 2 * j;
            pa[j] = (row < m && kk < k) ? A[row + (int64_t)kk * lda] : s_zero<S>();
        }
#pragma unroll
        for (int j = 0; j < G::NBL; ++j) {
            const int e = tid + 256 * j, kk = k0 + (e & (G::BK - 1)), col = bn + (e >> 4);
            pb[j] = (col < n && kk < k) ? B[kk + (int64_t)col * ldb] : s_zero<S>();
        }
    };
    mfma_d4 are[G::WM][G::WN], aim[kC ? G::WM : 1][kC ? G::WN : 1];
#pragma unroll
    for (int ti = 0; ti < G::WM; ++ti)
#pragma unroll
        for (int tj = 0; tj < G::WN; ++tj) {
            are[ti][tj] = mfma_d4{0, 0, 0, 0};
            if constexpr (kC) aim[ti][tj] = mfma_d4{0, 0, 0, 0};
        }
    fetch(0);
    for (int k0 = 0; k0 < k; k0 += G::BK) {
        __syncthreads();   // the slice in LDS has been consumed
#pragma unroll
        for (int j = 0; j < G::NA; ++j) {
            const int at = ((tid >> 7) + 2 * j) * G::LDA + (tid & (G::TM - 1));
            sA[0][at] = re_of(pa[j]);
            if constexpr (kC) sA[1][at] = im_of(pa[j]);
        }
#pragma unroll
        for (int j = 0; j < G::NBL; ++j) {
            const int e = tid + 256 * j, at = (e >> 4) * G::LDB + (e & (G::BK - 1));
            sB[0][at] = re_of(pb[j]);
            if constexpr (kC) sB[1][at] = im_of(pb[j]);
        }
        __syncthreads();
        if (k0 + G::BK < k) fetch(k0 + G::BK);
#pragma unroll
        for (int kq = 0; kq < G::BK / 4; ++kq) {
            const int kk = 4 * kq + lk;
            double ar[G::WM], ai[kC ? G::WM : 1], br[G::WN], bi[kC ? G::WN : 1];
#pragma unroll
            for (int ti = 0; ti < G::WM; ++ti) {
                ar[ti] = sA[0][kk * G::LDA + wr + 16 * ti + li];
                if constexpr (kC) ai[ti] = sA[1][kk * G::LDA + wr + 16 * ti + li];
            }
#pragma unroll
            for (int tj = 0; tj < G::WN; ++tj) {
                br[tj] = sB[0][(wc + 16 * tj + li) * G::LDB + kk];
                if constexpr (kC) bi[tj] = sB[1][(wc + 16 * tj + li) * G::LDB + kk];
            }
#pragma unroll
            for (int ti = 0; ti < G::WM; ++ti)
#pragma unroll
                for (int tj = 0; tj < G::WN; ++tj) {
                    are[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[tj], ar[ti], are[ti][tj], 0, 0, 0);
                    if constexpr (kC) {
                        are[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(-bi[tj], ai[ti], are[ti][tj], 0, 0, 0);
                        aim[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[tj], ai[ti], aim[ti][tj], 0, 0, 0);
                        aim[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bi[tj], ar[ti], aim[ti][tj], 0, 0, 0);
                    }
                }
        }
    }
#pragma unroll
    for (int ti = 0; ti < G::WM; ++ti)
#pragma unroll
        for (int tj = 0; tj < G::WN; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bm + wr + 16 * ti + li, col = bn + wc + 16 * tj + lk + 4 * r;
                if (row < m && col < n) {
                    if constexpr (kC) C[row + (int64_t)col * ldc] = cplx{are[ti][tj][r], aim[ti][tj][r]};
                    else C[row + (int64_t)col * ldc] = are[ti][tj][r];
                }
            }
}

template <class S>
struct LinArgs {
    const S* M[4];
    double c[4];
    double d;
    int cnt;
};

__device__ __forceinline__ double scale_by(double v, double c) { return c * v; }
__device__ __forceinline__ cplx scale_by(cplx v, double c) { return cplx{c * v.re, c * v.im}; }
__device__ __forceinline__ double add_re(double v, double d) { return v + d; }
__device__ __forceinline__ cplx add_re(cplx v, double d) { return cplx{v.re + d, v.im}; }

// Out = c0 M0 + c1 M1 + .. + d I, each product and each sum rounded on its own, in that order
template <class S>
__global__ __launch_bounds__(256) void lincomb_kernel(LinArgs<S> a, int64_t n, S* Out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    S v = s_zero<S>();
    for (int q = 0; q < a.cnt; ++q) {
        const S t = scale_by(a.M[q][idx], a.c[q]);
        v = q == 0 ? t : add(v, t);
    }
    if (a.d != 0.0 && idx % (n + 1) == 0) v = add_re(v, a.d);
    Out[idx] = v;
}

template <class S>
__global__ __launch_bounds__(256) void scale_pow2_kernel(const S* A, int64_t cnt, int s, S* Out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= cnt) return;
    const S v = A[idx];
    if constexpr (std::is_same_v<S, cplx>) Out[idx] = cplx{ldexp(v.re, -s), ldexp(v.im, -s)};
    else Out[idx] = ldexp(v, -s);
}

__device__ __forceinline__ bool finite_s(double v) { return fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ bool finite_s(cplx v) { return finite_s(v.re) && finite_s(v.im); }

// colsum[j] = sum_i |A(i, j)| (kCheck: 1 where the column holds a non-finite entry, else 0), j = blockIdx.x: the
// threads' strided partial sums, then a tree over the 256 partials, both in a fixed order
template <class S, bool kCheck>
__global__ __launch_bounds__(256) void colsum_kernel(const S* A, int64_t n, double* colsum) {
    __shared__ double part[256];
    const S* col = A + (int64_t)blockIdx.x * n;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        if constexpr (kCheck) s = (s != 0.0 || !finite_s(col[i])) ? 1.0 : 0.0;
        else s += mod_abs(col[i]);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            if constexpr (kCheck) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + w]);
            else part[threadIdx.x] += part[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) colsum[blockIdx.x] = part[0];
}

// the larger of two column sums; a NaN wins
__device__ __forceinline__ double max_nan(double a, double b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }

__global__ __launch_bounds__(256) void colmax_kernel(const double* colsum, int64_t n, double* out) {
    __shared__ double part[256];
    double m = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) m = max_nan(m, colsum[j]);
    part[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] = max_nan(part[threadIdx.x], part[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

}  // namespace dev

template <class S>
int gemm_device(hipStream_t st, int64_t m, int64_t n, int64_t k, const S* A, int64_t lda, const S* B, int64_t ldb, S* C,
                int64_t ldc) {
    using G = dev::GemmShape<S>;
    if (m < 1 || n < 1 || k < 1) return fail(EIGSOL_E_INVALID, "gemm_device: an empty operand");
    const int64_t gx = (m + G::TM - 1) / G::TM, gy = (n + G::TN - 1) / G::TN;
    if (std::max(std::max(m, n), k) > INT32_MAX / 2 || gy > 65535)
        return fail(EIGSOL_E_UNSUPPORTED, "gemm_device: an order above the kernel's index range");
    hipLaunchKernelGGL(dev::gemm_kernel<S>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, (int)m, (int)n, (int)k, A, lda, B,
                       ldb, C, ldc);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class S>
int mat_lincomb(hipStream_t st, int64_t n, int cnt, const double* c, const S* const* M, double d, S* Out) {
    if (cnt < 0 || cnt > 4) return fail(EIGSOL_E_INVALID, "mat_lincomb: at most four matrices");
    dev::LinArgs<S> a{};
    for (int q = 0; q < cnt; ++q) {
        a.M[q] = M[q];
        a.c[q] = c[q];
    }
    a.d = d;
    a.cnt = cnt;
    hipLaunchKernelGGL(dev::lincomb_kernel<S>, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, a, n, Out);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class S>
int mat_scale_pow2(hipStream_t st, int64_t cnt, int s, const S* A, S* Out) {
    hipLaunchKernelGGL(dev::scale_pow2_kernel<S>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, A, cnt, s, Out);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

template <class S>
int mat_norm1(hipStream_t st, int64_t n, const S* A, bool check, double* colsum, double* out) {
    if (check) hipLaunchKernelGGL((dev::colsum_kernel<S, true>), dim3((unsigned)n), dim3(256), 0, st, A, n, colsum);
    else hipLaunchKernelGGL((dev::colsum_kernel<S, false>), dim3((unsigned)n), dim3(256), 0, st, A, n, colsum);
    hipLaunchKernelGGL(dev::colmax_kernel, dim3(1), dim3(256), 0, st, colsum, n, out);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

#define EIGSOL_GEMM_INSTANCES(S)                                                                                            \
    template int gemm_device<S>(hipStream_t, int64_t, int64_t, int64_t, const S*, int64_t, const S*, int64_t, S*, int64_t); \
    template int mat_lincomb<S>(hipStream_t, int64_t, int, const double*, const S* const*, double, S*);                     \
    template int mat_scale_pow2<S>(hipStream_t, int64_t, int, const S*, S*);                                                \
    template int mat_norm1<S>(hipStream_t, int64_t, const S*, bool, double*, double*);
EIGSOL_GEMM_INSTANCES(double)
EIGSOL_GEMM_INSTANCES(cplx)
#undef EIGSOL_GEMM_INSTANCES

namespace {

template <class S>
int gemm_host(eigsol_ctx* ctx, int64_t m, int64_t n, int64_t k, const void* A, const void* B, void* C) {
    hipStream_t st = ctx->stream;
    DevBuf dA, dB, dC;
    EIGSOL_TRY(dA.alloc((size_t)m * k * sizeof(S)));
    EIGSOL_TRY(dB.alloc((size_t)k * n * sizeof(S)));
    EIGSOL_TRY(dC.alloc((size_t)m * n * sizeof(S)));
    EIGSOL_HIP(hipMemcpyAsync(dA.p, A, (size_t)m * k * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(dB.p, B, (size_t)k * n * sizeof(S), hipMemcpyHostToDevice, st));
    EIGSOL_TRY(gemm_device<S>(st, m, n, k, dA.as<S>(), m, dB.as<S>(), k, dC.as<S>(), m));
    EIGSOL_HIP(hipMemcpyAsync(C, dC.p, (size_t)m * n * sizeof(S), hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    return EIGSOL_OK;
}

}  // namespace

int dense_fn_check(const char* who, eigsol_ctx* ctx, int dtype, int64_t order) {
    if (dtype_wide(dtype) || dtype_single(dtype))
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": double and complex double matrices only");
    if (!dtype_valid(dtype)) return fail(EIGSOL_E_INVALID, std::string(who) + ": unknown dtype");
    const double bytes = (double)order * (double)order * (double)scalar_bytes(dtype);
    if (order > INT32_MAX / 2 || bytes > 0.05 * 288e9)   // the drivers hold up to a dozen matrices of the order
        return fail(EIGSOL_E_UNSUPPORTED, std::string(who) + ": order " + std::to_string(order) + " does not fit the device memory");
    EIGSOL_HIP(hipSetDevice(ctx->device));
    return EIGSOL_OK;
}

}  // namespace eigsol

using namespace eigsol;

extern "C" int eigsol_gemm_dense(eigsol_ctx* ctx, int dtype, int64_t m, int64_t n, int64_t k, const void* A_colmajor,
                                 const void* B_colmajor, void* C_out) {
    const char* who = "eigsol_gemm_dense";
    if (m < 0 || n < 0 || k < 0) return fail(EIGSOL_E_INVALID, std::string(who) + ": negative size");
    if (!ctx) return fail(EIGSOL_E_INVALID, std::string(who) + ": null context");
    EIGSOL_TRY(dense_fn_check(who, ctx, dtype, std::max(std::max(m, n), k)));
    if (m == 0 || n == 0) return EIGSOL_OK;
    if (!C_out || (k > 0 && (!A_colmajor || !B_colmajor))) return fail(EIGSOL_E_INVALID, std::string(who) + ": null pointer");
    if (k == 0) {   // the empty sum
        std::fill_n(static_cast<char*>(C_out), (size_t)m * n * scalar_bytes(dtype), 0);
        return EIGSOL_OK;
    }
    return dtype == EIGSOL_C128 ? gemm_host<cplx>(ctx, m, n, k, A_colmajor, B_colmajor, C_out)
                                : gemm_host<double>(ctx, m, n, k, A_colmajor, B_colmajor, C_out);
}
