// y = A^H x for a device-resident column-major dense matrix (eigsol_dense_gemv_h), gfx950.
//
// Every output is a dot product down one contiguous column, so A streams exactly once (HBM-bound,
// as the forward product of dense_power.hip):
//
//   grid = row chunks x column groups.  A workgroup takes kAdjCols columns per wave (4 waves: 32
//   columns) over the rows of its chunk.  Lane l owns 16 bytes of every 64-lane row segment (2 rows
//   f64, 1 row c128), so a wave-load is one contiguous 1 KiB piece of a column, non-temporal; the
//   kAdjCols loads of a segment are issued before their products and the wave keeps one accumulator
//   per column in registers over all its segments: one wave reduction per column per chunk.
//   adj_final_kernel adds the chunk partials part[chunk][ncols] in ascending chunk order.
//
// Columns that are not 16-byte aligned (odd nrows for f64) and the ragged last segment of a chunk
// take the scalar loads with a row guard; a ragged last column group reads its last column again
// in the lanes past it and stores nothing for them.  For complex matrices the conjugate is taken
// on A.  No floating-point atomics: the order of every sum depends on the shape alone, so two
// calls return the same bits.
#include <algorithm>

#include "kernels_common.hpp"

namespace eigsol {
namespace dev {

constexpr int kAdjCols = 8;   // columns a wave sums at a time: 8 x 1 KiB loads in flight per wave

__device__ __forceinline__ double adj_mul(double a, double x) { return a * x; }
__device__ __forceinline__ cplx adj_mul(cplx a, cplx x) {   // conj(a) x
    return cplx{a.re * x.re + a.im * x.im, a.re * x.im - a.im * x.re};
}
__device__ __forceinline__ double adj_wave_sum(double v) { return wave_sum(v); }
__device__ __forceinline__ cplx adj_wave_sum(cplx v) { return cplx{wave_sum(v.re), wave_sum(v.im)}; }

// part[chunk][c] = sum over the chunk's rows of conj(A[r, c]) x[r].  chunk_rows is a multiple of the
// 64-lane segment.  blockIdx.x: column group (32 columns), blockIdx.y: row chunk.
template <class S>
__global__ __launch_bounds__(kThreads) void adj_kernel(const S* __restrict__ A, int64_t nrows, int64_t ncols,
                                                       int64_t chunk_rows, const S* __restrict__ x,
                                                       S* __restrict__ part) {
    constexpr int PL = 16 / (int)sizeof(S);   // rows per lane and segment
    constexpr int R = 64 * PL;                // rows per segment
    typedef double d2v __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = ((int64_t)blockIdx.x * kWaves + w) * kAdjCols;   // wave-uniform
    if (c0 >= ncols) return;
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r1 = min(nrows, r0 + chunk_rows);
    const S* col[kAdjCols];
#pragma unroll
    for (int u = 0; u < kAdjCols; ++u) col[u] = A + min(c0 + u, ncols - 1) * nrows;
    S acc[kAdjCols];
#pragma unroll
    for (int u = 0; u < kAdjCols; ++u) acc[u] = s_zero<S>();

    int64_t seg = r0;
    if (nrows % PL == 0) {   // 16-byte aligned columns: whole segments by 16-byte loads
        for (; seg + R <= r1; seg += R) {
            const int64_t r = seg + (int64_t)lane * PL;
            S xv[PL], v[kAdjCols][PL];
#pragma unroll
            for (int p = 0; p < PL; ++p) xv[p] = x[r + p];
#pragma unroll
            for (int u = 0; u < kAdjCols; ++u) {
                const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(col[u] + r));
                __builtin_memcpy(&v[u][0], &t, 16);
            }
#pragma unroll
            for (int u = 0; u < kAdjCols; ++u)
#pragma unroll
                for (int p = 0; p < PL; ++p) acc[u] = add(acc[u], adj_mul(v[u][p], xv[p]));
        }
    }
    for (; seg < r1; seg += R) {   // unaligned columns, and the ragged last segment
        const int64_t r = seg + (int64_t)lane * PL;
#pragma unroll
        for (int p = 0; p < PL; ++p) {
            if (r + p < r1) {
                const S xv = x[r + p];
#pragma unroll
                for (int u = 0; u < kAdjCols; ++u) acc[u] = add(acc[u], adj_mul(col[u][r + p], xv));
            }
        }
    }
    S* mine = part + (size_t)blockIdx.y * ncols;
#pragma unroll
    for (int u = 0; u < kAdjCols; ++u) {
        const S s = adj_wave_sum(acc[u]);
        if (lane == 0 && c0 + u < ncols) mine[c0 + u] = s;
    }
}

// y[c] = part[0][c] + part[1][c] + ... in ascending chunk order
template <class S>
__global__ __launch_bounds__(kThreads) void adj_final_kernel(const S* __restrict__ part, int nchunk, int64_t ncols,
                                                             S* __restrict__ y) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= ncols) return;
    S s = part[c];
    for (int q = 1; q < nchunk; ++q) s = add(s, part[(size_t)q * ncols + c]);
    y[c] = s;
}

// y = 0 (a matrix without rows)
template <class S>
__global__ __launch_bounds__(kThreads) void adj_zero_kernel(S* __restrict__ y, int64_t ncols) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c < ncols) y[c] = s_zero<S>();
}

}  // namespace dev

namespace {

// row chunks: about 1024 workgroups (4 per CU, as the forward product), a chunk a whole number of segments
void adj_layout(const eigsol_dense* A, int& nchunk, int64_t& chunk_rows, int& ngroups) {
    const int64_t R = 64 * (16 / (int64_t)scalar_bytes(A->dtype));
    const int64_t gcols = (int64_t)dev::kWaves * dev::kAdjCols;
    ngroups = (int)((A->ncols + gcols - 1) / gcols);
    const int64_t nseg = std::max<int64_t>(1, (A->nrows + R - 1) / R);
    constexpr int64_t kAdjTargetBlocks = 1024;
    int64_t nch = std::max<int64_t>(1, kAdjTargetBlocks / std::max(1, ngroups));
    nch = std::min<int64_t>(std::min<int64_t>(nch, nseg), 65535);
    chunk_rows = (nseg + nch - 1) / nch * R;
    nchunk = (int)((A->nrows + chunk_rows - 1) / chunk_rows);
}

template <class S>
int adj_launch(eigsol_dense* A, const void* x, void* y) {
    hipStream_t st = A->ctx->stream;
    const dim3 blk(dev::kThreads);
    const unsigned gy = (unsigned)((A->ncols + dev::kThreads - 1) / dev::kThreads);
    if (A->nrows == 0) {
        hipLaunchKernelGGL((dev::adj_zero_kernel<S>), dim3(gy), blk, 0, st, (S*)y, A->ncols);
        EIGSOL_HIP(hipGetLastError());
        return EIGSOL_OK;
    }
    int nchunk, ngroups;
    int64_t chunk_rows;
    adj_layout(A, nchunk, chunk_rows, ngroups);
    if (!A->hpart) EIGSOL_HIP(hipMalloc(&A->hpart, (size_t)nchunk * A->ncols * sizeof(S)));
    hipLaunchKernelGGL((dev::adj_kernel<S>), dim3(ngroups, nchunk), blk, 0, st, (const S*)A->a, A->nrows, A->ncols,
                       chunk_rows, (const S*)x, (S*)A->hpart);
    EIGSOL_HIP(hipGetLastError());
    hipLaunchKernelGGL((dev::adj_final_kernel<S>), dim3(gy), blk, 0, st, (const S*)A->hpart, nchunk, A->ncols, (S*)y);
    EIGSOL_HIP(hipGetLastError());
    return EIGSOL_OK;
}

}  // namespace
}  // namespace eigsol

using namespace eigsol;

extern "C" {

int eigsol_dense_gemv_h(eigsol_dense* A, const void* x_dev, void* y_dev) {
    if (!A || (!x_dev && A->nrows) || (!y_dev && A->ncols))
        return fail(EIGSOL_E_INVALID, "eigsol_dense_gemv_h: null pointer");
    if (A->dtype != EIGSOL_F64 && A->dtype != EIGSOL_C128)
        return fail(EIGSOL_E_UNSUPPORTED, "eigsol_dense_gemv_h: only double and complex double matrices are supported");
    if (A->ncols == 0) return EIGSOL_OK;
    EIGSOL_HIP(hipSetDevice(A->ctx->device));
    return A->dtype == EIGSOL_C128 ? adj_launch<cplx>(A, x_dev, y_dev) : adj_launch<double>(A, x_dev, y_dev);
}

}  // extern "C"
