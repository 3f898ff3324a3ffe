// Tall-skinny block product Y = A X of a device-resident dense (column-major) matrix on the fp64
// matrix cores (gfx950, v_mfma_f64_16x16x4_f64): the operator of the dense subspace iteration.
//
// A is nrows x ncols, column-major; X (ncols x m) and Y (nrows x m) are row-major interleaved
// blocks, X[i * m + j], 1 <= m <= 32, padded to NT = 1 or 2 tiles of 16 block columns.
//
//   dense_gemm_kernel   grid = row tiles of 256 rows x column chunks.  A wave owns 64 rows (four
//                       16-row fragments) and walks its chunk's columns four at a time.  With the
//                       fragment layout of mfma_rankk.hpp, X rides on the A operand (lane l holds
//                       X[k + (l >> 4)][l & 15]) and the matrix on the B operand (lane l holds
//                       A[row + (l & 15)][k + (l >> 4)]): 16 lanes read 128 (c128: 256) contiguous
//                       bytes of one column of A, a wave 512 of each of four columns, and the four
//                       waves of a workgroup read the same rows of X, which the caches serve.  A is
//                       read once per product, non-temporal.  Block columns >= m, rows >= nrows and
//                       columns >= ncols are masked on load (never loaded).  A complex product
//                       takes four real MFMAs.  No LDS and no barrier.  The chunk's partial of Y
//                       goes to part[chunk][nrows * m].
//   dense_gemm_final    Y[e] = the sum of part[chunk][e] over the chunks in ascending order.
// No floating-point atomics and no workgroup waits for another: two runs give identical bits.
//
// The workspace of partials is allocated on first use and kept on the eigsol_dense (gpart).
#include <algorithm>

#include "linear_op.hpp"
#include "mfma_rankk.hpp"

namespace eigsol {
namespace dev {

constexpr int kGemmRows = 256;      // rows of A per workgroup (64 per wave)
constexpr int kGemmColStep = 16;    // columns of A a wave loads before its MFMAs (4 k-steps)
constexpr int kGemmMinChunk = 256;  // fewest columns per chunk (a multiple of kGemmColStep)

__device__ __forceinline__ double gemm_ld_a(const double* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ cplx gemm_ld_a(const cplx* p) {
    typedef double d2v __attribute__((ext_vector_type(2)));
    const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
    return cplx{t.x, t.y};
}

// 16 columns of the chunk from column j: the loads, then the MFMAs in ascending column order.
// kFull: all 64 rows and all 16 columns are inside the matrix (only the block columns are masked).
template <class S, int NT, bool kFull>
__device__ __forceinline__ void gemm_cols(const S* __restrict__ A, int64_t nrows, int64_t r0, int64_t j, int64_t c1,
                                          int m, const S* __restrict__ X, int li, int lk, mfma_d4 (&are)[4][NT],
                                          mfma_d4 (&aim)[4][NT]) {
    constexpr bool kC = std::is_same_v<S, cplx>;
    constexpr int kU = kGemmColStep / 4;
    S x[kU][NT], a[kU][4];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const int64_t k = j + 4 * u + lk;
        const bool kv = kFull || k < c1;
#pragma unroll
        for (int t = 0; t < NT; ++t) x[u][t] = (kv && 16 * t + li < m) ? X[k * m + 16 * t + li] : s_zero<S>();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t row = r0 + 16 * s + li;
            a[u][s] = (kv && (kFull || row < nrows)) ? gemm_ld_a(A + k * nrows + row) : s_zero<S>();
        }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double xr = re_of(x[u][t]), ar = re_of(a[u][s]);
                are[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, ar, are[s][t], 0, 0, 0);
                if constexpr (kC) {
                    const double xi = im_of(x[u][t]), ai = im_of(a[u][s]);
                    are[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xi, ai, are[s][t], 0, 0, 0);
                    aim[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, ai, aim[s][t], 0, 0, 0);
                    aim[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xi, ar, aim[s][t], 0, 0, 0);
                }
            }
}

template <class S, int NT>
__global__ __launch_bounds__(256) void dense_gemm_kernel(const S* __restrict__ A, int64_t nrows, int64_t ncols, int m,
                                                         int64_t cw, const S* __restrict__ X, S* __restrict__ part) {
    constexpr bool kC = std::is_same_v<S, cplx>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * kGemmRows + 64 * wave;
    if (r0 >= nrows) return;   // wave-uniform; the kernel has no barrier
    const int64_t c0 = (int64_t)blockIdx.y * cw;
    const int64_t c1 = min(ncols, c0 + cw);
    mfma_d4 are[4][NT], aim[4][NT];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) are[s][t] = aim[s][t] = mfma_d4{0, 0, 0, 0};
    int64_t j = c0;
    if (r0 + 64 <= nrows)
        for (; j + kGemmColStep <= c1; j += kGemmColStep)
            gemm_cols<S, NT, true>(A, nrows, r0, j, c1, m, X, li, lk, are, aim);
    for (; j < c1; j += kGemmColStep) gemm_cols<S, NT, false>(A, nrows, r0, j, c1, m, X, li, lk, are, aim);
    // D lane l register r: block column (l >> 4) + 4 r of the tile, row l & 15 of the fragment
    S* mine = part + (size_t)blockIdx.y * (size_t)nrows * m;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = r0 + 16 * s + li;
                const int col = 16 * t + lk + 4 * r;
                if (row < nrows && col < m) {
                    if constexpr (kC) mine[row * m + col] = cplx{are[s][t][r], aim[s][t][r]};
                    else mine[row * m + col] = are[s][t][r];
                }
            }
}

template <class S>
__global__ __launch_bounds__(256) void dense_gemm_final(const S* __restrict__ part, int nchunk, int64_t count,
                                                        S* __restrict__ Y) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    S s = part[e];
    for (int q = 1; q < nchunk; ++q) s = add(s, part[(int64_t)q * count + e]);
    Y[e] = s;
}

}  // namespace dev

namespace {

// chunks of a product: about 4 workgroups per CU, at least kGemmMinChunk columns each
void gemm_layout(const eigsol_dense* A, int64_t& ntr, int64_t& nchunk, int64_t& cw) {
    ntr = (A->nrows + dev::kGemmRows - 1) / dev::kGemmRows;
    const int64_t want = std::max<int64_t>(1, 4 * (int64_t)std::max(A->ctx->num_cus, 1) / std::max<int64_t>(ntr, 1));
    const int64_t most = std::max<int64_t>(1, (A->ncols + dev::kGemmMinChunk - 1) / dev::kGemmMinChunk);
    nchunk = std::min(want, most);
    cw = (A->ncols + nchunk - 1) / nchunk;
    cw = std::max<int64_t>(dev::kGemmColStep, (cw + dev::kGemmColStep - 1) / dev::kGemmColStep * dev::kGemmColStep);
    nchunk = std::max<int64_t>(1, (A->ncols + cw - 1) / cw);
}

template <class S>
int gemm_launch_t(eigsol_dense* A, int m, const S* X, S* Y) {
    int64_t ntr, nchunk, cw;
    gemm_layout(A, ntr, nchunk, cw);
    const int64_t count = A->nrows * m;
    const size_t need = (size_t)nchunk * (size_t)count * sizeof(S);
    hipStream_t st = A->ctx->stream;
    if (need > A->gpart_bytes) {
        if (A->gpart) {
            EIGSOL_HIP(stream_wait(st));   // an earlier product may still read the old workspace
            EIGSOL_HIP(hipFree(A->gpart));
            A->gpart = nullptr;
            A->gpart_bytes = 0;
        }
        EIGSOL_HIP(hipMalloc(&A->gpart, need));
        A->gpart_bytes = need;
    }
    S* part = static_cast<S*>(A->gpart);
    const dim3 grid((unsigned)ntr, (unsigned)nchunk);
    if (m <= 16)
        hipLaunchKernelGGL((dev::dense_gemm_kernel<S, 1>), grid, dim3(256), 0, st, (const S*)A->a, A->nrows, A->ncols,
                           m, cw, X, part);
    else
        hipLaunchKernelGGL((dev::dense_gemm_kernel<S, 2>), grid, dim3(256), 0, st, (const S*)A->a, A->nrows, A->ncols,
                           m, cw, X, part);
    EIGSOL_HIP(hipGetLastError());
    hipLaunchKernelGGL((dev::dense_gemm_final<S>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st,
                       (const S*)part, (int)nchunk, count, Y);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

}  // namespace

int dense_gemm_launch(eigsol_dense* A, int m, const void* X, void* Y) {
    if (A->nrows == 0) return EIGSOL_OK;
    if (A->dtype == EIGSOL_C128) return gemm_launch_t<cplx>(A, m, (const cplx*)X, (cplx*)Y);
    return gemm_launch_t<double>(A, m, (const double*)X, (double*)Y);
}

}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_dense_gemm(eigsol_dense* A, int32_t m, const void* X_dev, void* Y_dev) {
    if (!A || (!X_dev && A->ncols) || (!Y_dev && A->nrows))
        return fail(EIGSOL_E_INVALID, "eigsol_dense_gemm: null pointer");
    if (m < 1 || m > 32) return fail(EIGSOL_E_INVALID, "eigsol_dense_gemm: m must be in 1..32");
    if (A->dtype != EIGSOL_F64 && A->dtype != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_dense_gemm: only double and complex double matrices are supported");
    if (A->nrows == 0) return EIGSOL_OK;
    EIGSOL_HIP(hipSetDevice(A->ctx->device));
    return dense_gemm_launch(A, m, X_dev, Y_dev);
}

}  // extern "C"
