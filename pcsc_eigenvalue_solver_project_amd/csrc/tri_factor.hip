// The level-ordered triangular factor of the shifted solves: analysis and layout.
//
// A triangular A (config 5), the L and U of the general-sparse family (gmres.hip) and the shift-invert
// mode of the Krylov-Schur solver all solve with the same factor: pivots d_i - sigma, rows ordered by
// dependency level, a head of narrow levels solved from LDS and a tail spread over the GPU (the solve
// kernels and their launch paths: sptrsv.hip).  The factor is built on the device (factor_tri_device)
// or on the host (factor_tri_host); both take every head / tail decision and every layout knob from
// one plan (tri_plan), so the device build gives the host build's layout bit for bit.  tri_build is
// the one way in.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "shift_factor.hpp"

namespace eigsol {

namespace dev {

// ---- on-device analysis of a triangular CSR (factor_tri_device): the same level order and the same
// position-indexed chunk layout the host build produces, without moving the matrix off the device.

// Per row: pivot d_i - sigma (the diagonal entries summed in stored order, 0 where there is none),
// off-diagonal count, and the triangularity / zero-pivot flags (flags[0]: an entry left of the
// diagonal, [1]: right of it, [2]: a zero pivot), one atomic per wave.
template <class S>
__global__ __launch_bounds__(256) void tri_rows_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                       const S* __restrict__ val, int64_t n, S sig,
                                                       S* __restrict__ pv, int32_t* __restrict__ offlen,
                                                       int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool lo = false, hi = false, zp = false;
    if (i < n) {
        S d = s_zero<S>();
        int32_t off = 0;
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e) {
            const int32_t c = ci[e];
            if (c == i) d = add(d, val[e]);
            else {
                ++off;
                lo |= c < i;
                hi |= c > i;
            }
        }
        const S p = sub(d, sig);
        pv[i] = p;
        offlen[i] = off;
        if constexpr (std::is_same_v<S, double> || std::is_same_v<S, float>) zp = p == 0;
        else zp = p.re == 0 && p.im == 0;
    }
    const uint64_t bl = __ballot(lo), bh = __ballot(hi), bz = __ballot(zp);
    if ((threadIdx.x & 63) == 0) {
        if (bl) atomicOr(flags + 0, 1);
        if (bh) atomicOr(flags + 1, 1);
        if (bz) atomicOr(flags + 2, 1);
    }
}

// Dependency levels, sync-free: level(i) = 1 + max level of the rows row i reads (0 for none).
// Rows are claimed in dependency order through a ticket (upper: row n-1 first), four rows per wave
// (16 lanes per row); a row's dependencies always hold smaller tickets, claimed by waves that are
// already running, so every wait ends.  A wave re-polls its unfinished rows' dependencies
// (agent-scope loads, -1 = not yet known) and publishes a row as soon as all of them are known,
// inside the loop (a divergent group must never wait on a row its own wave publishes after the
// loop).  Per level: row count and longest row (atomics); maxlev = the deepest level.  A wait past
// ~2 s of the 100 MHz constant clock sets err and publishes level 0, so a broken analysis ends
// (the host then builds on the CPU).
__global__ __launch_bounds__(256) void tri_level_kernel(const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                        const int32_t* __restrict__ offlen, int64_t n, int upper,
                                                        int32_t* lev, uint32_t* ticket, int32_t* lcnt,
                                                        int32_t* lmax, int32_t* maxlev, int32_t* err) {
    const int lane = threadIdx.x & (kRowLanes - 1);
    const int grp = (threadIdx.x & 63) / kRowLanes;
    for (;;) {
        uint32_t t0 = 0;
        if ((threadIdx.x & 63) == 0) t0 = atomicAdd(ticket, (uint32_t)kWaveRows);
        t0 = __shfl(t0, 0, 64);
        if ((int64_t)t0 >= n) return;
        const int64_t t = (int64_t)t0 + grp;
        const bool live = t < n;
        const int64_t i = live ? (upper ? n - 1 - t : t) : 0;
        const int32_t e0 = live ? rp[i] : 0, e1 = live ? rp[i + 1] : 0;
        bool done = !live;
        const long long t_start = wall_clock64();
        for (;;) {
            int32_t m = -1;
            bool ready = true;
            if (!done)
                for (int32_t e = e0 + lane; e < e1; e += kRowLanes) {
                    const int32_t c = ci[e];
                    if (c == i) continue;
                    const int32_t l = __hip_atomic_load(lev + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (l < 0) ready = false;
                    m = max(m, l);
                }
            // the row's 16 lanes: all ready (ballot), and the largest dependency level (every lane
            // shuffles: a shuffle under a divergent mask would read inactive lanes' stale registers)
#pragma unroll
            for (int off = kRowLanes / 2; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
            const uint64_t unready = __ballot(!ready);
            ready = ((unready >> (grp * kRowLanes)) & ((1ull << kRowLanes) - 1)) == 0;
            bool timeout = false;
            if (!done && !ready && wall_clock64() - t_start > 200000000ll) {
                timeout = true;
                ready = true;
                m = -1;
            }
            if (!done && ready) {
                if (lane == 0) {
                    if (timeout) atomicOr(err, 1);
                    const int32_t l = m + 1;
                    __hip_atomic_store(lev + i, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    atomicAdd(lcnt + l, 1);
                    atomicMax(lmax + l, offlen[i]);
                    atomicMax(maxlev, l);
                }
                done = true;
            }
            if (__ballot(!done) == 0) break;
            __builtin_amdgcn_s_sleep(1);
        }
    }
}

// position -> row: the rows sorted by level (stable: ascending row inside a level) placed at their
// level's padded start; padding positions stay -1
__global__ __launch_bounds__(256) void tri_order_kernel(const int32_t* __restrict__ lev_sorted,
                                                        const int32_t* __restrict__ rows_sorted, int64_t n,
                                                        const int32_t* __restrict__ ustart,
                                                        const int32_t* __restrict__ pstart, int32_t* __restrict__ order) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int32_t l = lev_sorted[k];
    order[pstart[l] + (k - ustart[l])] = rows_sorted[k];
}

// per position: its row's off-diagonal count (plen[npos] = 0 closes the scan) and its pivot
template <class S>
__global__ __launch_bounds__(256) void tri_poslen_kernel(const int32_t* __restrict__ order, int64_t npos,
                                                         const int32_t* __restrict__ offlen, const S* __restrict__ pv,
                                                         S one, int32_t* __restrict__ plen, S* __restrict__ ppiv) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > npos) return;
    if (p == npos) {
        plen[p] = 0;
        return;
    }
    const int32_t i = order[p];
    plen[p] = i >= 0 ? offlen[i] : 0;
    ppiv[p] = i >= 0 ? pv[i] : one;
}

// the position-ordered off-diagonal CSR: 16 lanes per position copy its row's entries (diagonal
// skipped, stored order kept) to pptr[p]
template <class S>
__global__ __launch_bounds__(256) void tri_gather_kernel(const int32_t* __restrict__ order, int64_t npos,
                                                         const int32_t* __restrict__ pptr,
                                                         const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                         const S* __restrict__ val, const int32_t* __restrict__ offlen,
                                                         int32_t* __restrict__ pcol, S* __restrict__ pval) {
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kRowLanes;
    const int lane = threadIdx.x & (kRowLanes - 1);
    if (p >= npos) return;
    const int32_t i = order[p];
    if (i < 0) return;
    const int32_t e0 = rp[i], len = rp[i + 1] - e0, nd = len - offlen[i], base = pptr[p];
    for (int32_t k = lane; k < len; k += kRowLanes) {
        const int32_t c = ci[e0 + k];
        if (c == i) continue;
        const int32_t o = base + (c < i ? k : k - nd);
        pcol[o] = c;
        pval[o] = val[e0 + k];
    }
}

// head rows: row -> head position (their columns become LDS positions)
__global__ __launch_bounds__(256) void tri_rowpos_kernel(const int32_t* __restrict__ order, int32_t hpos,
                                                         int32_t* __restrict__ rowpos) {
    const int32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hpos) return;
    const int32_t i = order[p];
    if (i >= 0) rowpos[i] = p;
}

// 1 / pivot as the host build forms it (complex: in double, no contraction), for bitwise-equal heads
__device__ __forceinline__ double head_recip(double p) { return 1.0 / p; }
__device__ __forceinline__ float head_recip(float p) { return 1.0f / p; }
__device__ __forceinline__ cplx head_recip(cplx p) {
#pragma clang fp contract(off)
    const double d = p.re * p.re + p.im * p.im;
    return cplx{p.re / d, -p.im / d};
}
__device__ __forceinline__ cplxf head_recip(cplxf p) {
#pragma clang fp contract(off)
    const double re = p.re, im = p.im;
    const double d = re * re + im * im;
    return cplxf{(float)(re / d), (float)(-im / d)};
}

// one-wave head, pass-major (see sptrsv_whead_kernel): thread (q, u) fills row u of pass q; the
// arrays arrive pre-filled with the padding (values 0, columns hpos, pivots 1, targets -1)
template <class S>
__global__ __launch_bounds__(256) void tri_whead_kernel(const int2* __restrict__ ptab, int32_t nreal,
                                                        const int32_t* __restrict__ order, const int32_t* __restrict__ rp,
                                                        const int32_t* __restrict__ ci, const S* __restrict__ val,
                                                        const S* __restrict__ pv, const int32_t* __restrict__ rowpos,
                                                        S* __restrict__ wval, int32_t* __restrict__ wcol,
                                                        S* __restrict__ wrp, int32_t* __restrict__ wdst) {
    const int32_t g = blockIdx.x * 256 + threadIdx.x;
    const int32_t q = g / kWHeadRows, u = g % kWHeadRows;
    if (q >= nreal) return;
    const int2 pt = ptab[q];   // {first position, rows}
    if (u >= pt.y) return;
    const int32_t p = pt.x + u;
    const int32_t i = order[p];
    wrp[(size_t)q * kWHeadRows + u] = head_recip(pv[i]);
    wdst[(size_t)q * kWHeadRows + u] = p;
    int32_t idx = 0;
    for (int32_t e = rp[i]; e < rp[i + 1]; ++e) {
        const int32_t c = ci[e];
        if (c == i) continue;
        const size_t slot = ((size_t)q * 4 + (size_t)(idx % 4)) * 64 + (size_t)(4 * u + idx / 4);
        wcol[slot] = rowpos[c];
        wval[slot] = val[e];
        ++idx;
    }
}

template <class T>
__global__ __launch_bounds__(256) void fill_kernel(T* __restrict__ a, int64_t n, T v) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) a[k] = v;
}

}  // namespace dev

// Level analysis of a triangular pattern (host, once per matrix): level(i) = 1 + max level of
// the rows it reads; positions sorted by level, each level padded to a multiple of kWaveRows.
static void level_order(const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int64_t n,
                        bool upper, std::vector<int32_t>& order, int32_t& nlevels,
                        std::vector<int64_t>& lstart, std::vector<int64_t>& lcount) {
    std::vector<int32_t> lev(n, 0);
    int32_t maxl = 0;
    auto visit = [&](int64_t i) {
        int32_t l = 0;
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e) l = std::max(l, lev[ci[e]] + 1);
        lev[i] = l;
        maxl = std::max(maxl, l);
    };
    if (upper) for (int64_t i = n - 1; i >= 0; --i) visit(i);
    else for (int64_t i = 0; i < n; ++i) visit(i);
    nlevels = maxl + 1;
    std::vector<int64_t> cnt(nlevels + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++cnt[lev[i] + 1];
    std::vector<int64_t> start(nlevels + 1, 0);
    constexpr int64_t W = dev::kWaveRows;
    for (int32_t l = 0; l < nlevels; ++l) start[l + 1] = start[l] + ((cnt[l + 1] + W - 1) / W) * W;
    order.assign(start[nlevels], -1);
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n; ++i) order[fill[lev[i]]++] = (int32_t)i;
    lstart = start;
    lcount.assign(cnt.begin() + 1, cnt.end());
}

// Head of the level order solved by one workgroup from LDS: the longest prefix of levels whose
// positions fit the LDS budget and whose levels are narrow (a wide level is cheaper spread over
// the whole GPU).
template <class S>
static int32_t head_levels(const std::vector<int64_t>& lstart, const std::vector<int64_t>& lcount,
                           const std::vector<int32_t>& lmaxlen, int32_t nlevels, bool wave_head) {
    constexpr int64_t cap = (int64_t)(150 * 1024) / (int64_t)sizeof(S);
    // widest head level.  One-workgroup head: config 5 256 -> 0.861 ms, 1024 -> 0.872 ms per solve.
    // One-wave head (16 rows per pass, ~0.26 us a pass): 64 -> 0.833 ms, 256 -> 0.879 ms (a wider
    // level is cheaper in the tail, ~1.7 us a level)
    const int64_t width = wave_head ? 64 : 256;
    int32_t h = 0;
    int64_t npass = 0;   // the pass table shares the LDS budget (8 bytes a pass)
    while (h < nlevels && lcount[h] <= width && lmaxlen[h] <= dev::kRowLanes) {
        const int64_t np = npass + (lcount[h] + dev::kHeadRows - 1) / dev::kHeadRows;
        if ((lstart[h + 1] + 1) * (int64_t)sizeof(S) + (np + dev::kHeadDepth) * 8 > cap * (int64_t)sizeof(S)) break;
        npass = np;
        ++h;
    }
    return h;
}

// What both builds decide from the per-level tables: the pass tables of the two heads and the slices
// of the slice tail.  The scalar decisions go straight into the factor (see tri_plan).
struct TriPlan {
    std::vector<int2> passes;      // one-workgroup head: {first position, end | barrier}, padded to kHeadDepth
    std::vector<int2> wpass;       // one-wave head: {first position, rows}, padded to kWHeadDepth (empty passes:
    int32_t nwreal = 0;            // the ring loop is straight-line code); nwreal: the passes that hold rows
    std::vector<int64_t> sfirst;   // tail slices (see sptrsv_slice_kernel): 64 rows of one level each;
    std::vector<int32_t> scount;   // first position, rows,
    std::vector<int32_t> slen;     // longest row
    bool device_buildable = false;   // a layout factor_tri_device produces: chunk tail, one-wave head or none
};

// The layout of a level-ordered factor, decided once for both builds from the per-level tables (padded
// start, rows, longest off-diagonal row); f holds nlevels and npos.  Sets f's wave_head, poll_fast,
// poll_mode, hlevels, hpos, tail_chunks, chunk0, nchunks, chunk_two, nwpass, nslices and slice_b.
// plen (the host build has it): the off-diagonal entries of every position, which the slices and
// slice_b's percentile need; without it there are no slices and slice_b is 4 unless the knob says
// otherwise.  Every EIGSOL_TRSV_* layout knob is read here or in head_levels, on every build (the
// tests switch them inside one process).
template <class S>
static TriPlan tri_plan(ShiftFactor* f, const std::vector<int64_t>& lstart, const std::vector<int64_t>& lcount,
                        const std::vector<int32_t>& lmaxlen, const std::vector<int32_t>* plen) {
    TriPlan pl;
    if (const char* e = std::getenv("EIGSOL_TRSV_HEAD")) f->tri.wave_head = std::strcmp(e, "block") ? 1 : 0;
    f->tri.hlevels = head_levels<S>(lstart, lcount, lmaxlen, f->tri.nlevels, f->tri.wave_head != 0);
    if (const char* e = std::getenv("EIGSOL_TRSV_POLL_FAST"))
        f->tri.poll_fast = (f->tri.poll_fast & ~0xffff) | std::min(0xffff, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("EIGSOL_TRSV_POLL_SLOW"))
        f->tri.poll_fast = (f->tri.poll_fast & 0xffff) | (std::min(7, std::max(0, std::atoi(e))) << 16);
    if (const char* e = std::getenv("EIGSOL_TRSV_POLL_MODE")) f->tri.poll_mode = std::atoi(e);
    f->tri.hpos = (int32_t)lstart[f->tri.hlevels];
    for (int32_t l = 0; l < f->tri.hlevels; ++l) {
        const int32_t p0 = (int32_t)lstart[l], p1 = (int32_t)(lstart[l] + lcount[l]);
        for (int32_t p = p0; p < p1; p += dev::kHeadRows) {
            const int32_t e = std::min(p1, p + dev::kHeadRows);
            pl.passes.push_back(make_int2(p, e | (e == p1 ? dev::kPassBarrier : 0)));
        }
        // one-wave head: passes of <= 16 rows inside a level
        for (int32_t p = p0; p < p1; p += dev::kWHeadRows) pl.wpass.push_back(make_int2(p, std::min(dev::kWHeadRows, p1 - p)));
    }
    while (!pl.passes.empty() && pl.passes.size() % dev::kHeadDepth) pl.passes.push_back(make_int2(0, 0));   // empty
    pl.nwreal = (int32_t)pl.wpass.size();
    while (pl.wpass.size() % dev::kWHeadDepth) pl.wpass.push_back(make_int2(0, 0));
    f->tri.nwpass = (int32_t)pl.wpass.size();
    // tail variant: slices (row per lane) for few, very wide levels; chunks (16 lanes per row)
    // otherwise.  EIGSOL_TRSV_TAIL=slice|chunk overrides.
    {
        // slices when most tail rows sit in levels of >= 64k rows (a wave's 64 rows then rarely
        // wait); measured: one 1M-row level 74 vs 195 us, config 5 (widest level 21k) 1.3 vs 0.86 ms
        int64_t trows = 0, wide = 0;
        for (int32_t l = f->tri.hlevels; l < f->tri.nlevels; ++l) {
            trows += lcount[l];
            if (lcount[l] >= 65536) wide += lcount[l];
        }
        f->tri.tail_chunks = (trows > 0 && 2 * wide < trows) ? 1 : 0;
        if (const char* e = std::getenv("EIGSOL_TRSV_TAIL")) f->tri.tail_chunks = std::strcmp(e, "slice") ? 1 : 0;
    }
    if (f->tri.tail_chunks) {
        f->tri.chunk0 = f->tri.hpos / dev::kWaveRows;
        f->tri.nchunks = f->tri.npos / dev::kWaveRows;
        int32_t longest = 0;
        for (int32_t l = f->tri.hlevels; l < f->tri.nlevels; ++l) longest = std::max(longest, lmaxlen[l]);
        // rows past 16 entries: the second entry of every lane is polled with the first
        // (EIGSOL_TRSV_TWO=0|1 overrides; round 4, the exact LU's U of config 5 made general)
        f->tri.chunk_two = longest > dev::kRowLanes ? 1 : 0;
        if (const char* e = std::getenv("EIGSOL_TRSV_TWO")) f->tri.chunk_two = std::atoi(e) != 0;
    }
    // tail slices (see sptrsv_slice_kernel): 64 rows of one level each; B = the smallest of
    // 4 / 8 / 16 that holds the entries of at least 95 % of the slices (longer slices loop)
    if (plen)
        for (int32_t l = f->tri.tail_chunks ? f->tri.nlevels : f->tri.hlevels; l < f->tri.nlevels; ++l)
            for (int64_t p = lstart[l]; p < lstart[l] + lcount[l]; p += 64) {
                const int32_t c = (int32_t)std::min<int64_t>(64, lstart[l] + lcount[l] - p);
                int32_t K = 0;
                for (int32_t u = 0; u < c; ++u) K = std::max(K, (*plen)[p + u]);
                pl.sfirst.push_back(p);
                pl.scount.push_back(c);
                pl.slen.push_back(K);
            }
    f->tri.nslices = (int32_t)pl.slen.size();
    {
        std::vector<int32_t> sorted(pl.slen);
        std::sort(sorted.begin(), sorted.end());
        const int32_t q95 = sorted.empty() ? 0 : sorted[(size_t)(0.95 * (double)(sorted.size() - 1))];
        f->tri.slice_b = q95 <= 4 ? 4 : (q95 <= 8 ? 8 : 16);
    }
    pl.device_buildable = f->tri.tail_chunks && (f->tri.hpos == 0 || f->tri.wave_head);
    return pl;
}

static int dev_upload(hipStream_t st, void** dst, const void* src, size_t bytes) {
    EIGSOL_HIP(hipMalloc(dst, std::max<size_t>(bytes, 16)));
    if (bytes && src) EIGSOL_HIP(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
    return EIGSOL_OK;
}

// Solve state of a triangular factor: the two polled value buffers (every row unsolved: the
// sentinel; the zero slot z[n] stays 0 for good), the ticket / error words and the wave partials.
template <class S>
static int tri_state_alloc(ShiftFactor* f) {
    hipStream_t st = f->ctx->stream;
    const int64_t n = f->n;
    EIGSOL_TRY(dev_upload(st, &f->tri.z[0], nullptr, (n + 1) * sizeof(S)));
    EIGSOL_TRY(dev_upload(st, &f->tri.z[1], nullptr, (n + 1) * sizeof(S)));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.work, nullptr, 64));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.err, nullptr, 64));
    EIGSOL_TRY(dev_upload(st, &f->tri.wave_part, nullptr, (size_t)f->tri.grid * dev::kWaves * sizeof(dev::part4)));
    const uint32_t sent = (uint32_t)(dev::kSent & 0xffffffffu);
    for (void* zb : f->tri.z) {
        hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(zb), (int)sent, n * sizeof(S) / 4, st);
        hipMemsetAsync(static_cast<char*>(zb) + n * sizeof(S), 0, sizeof(S), st);
    }
    hipMemsetAsync(f->tri.work, 0, 64, st);
    hipMemsetAsync(f->tri.err, 0, 64, st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(EIGSOL_E_HIP, "factor upload");
    return EIGSOL_OK;
}

// No slice tail (nslices = 0): the kernel prefetches "slice 0" for a wave past the last slice, so
// slice 0 always exists (an empty one here)
template <class S>
static int tri_empty_slice0(ShiftFactor* f) {
    hipStream_t st = f->ctx->stream;
    const int32_t Bs = f->tri.slice_b;
    const std::vector<int2> smeta(1, make_int2(0, Bs));
    const std::vector<int32_t> trow(64, -1), tcol((size_t)64 * Bs, (int32_t)f->n);   // padding: the zero slot z[n]
    const std::vector<S> tpiv(64, make_sigma<S>(1.0, 0.0)), tval((size_t)64 * Bs, s_zero<S>());
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.smeta, smeta.data(), smeta.size() * sizeof(int2)));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.trow, trow.data(), trow.size() * 4));
    EIGSOL_TRY(dev_upload(st, &f->tri.tpiv, tpiv.data(), tpiv.size() * sizeof(S)));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.tcol, tcol.data(), tcol.size() * 4));
    EIGSOL_TRY(dev_upload(st, &f->tri.tval, tval.data(), tval.size() * sizeof(S)));
    EIGSOL_HIP(hipStreamSynchronize(st));   // the small host vectors above go out of scope
    return EIGSOL_OK;
}

// EIGSOL_TRSV_DUMP=prefix (debugging): the built factor's position-indexed arrays, downloaded and
// written to prefix_<name>.bin (host and device builds compare byte for byte)
template <class S>
static void tri_dump(const ShiftFactor* f) {
    const char* pre = std::getenv("EIGSOL_TRSV_DUMP");
    if (!pre || f->kind != FactorKind::Tri) return;
    hipStreamSynchronize(f->ctx->stream);
    auto put = [&](const char* name, const void* d, size_t bytes) {
        std::vector<unsigned char> h(bytes);
        if (bytes && hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost) != hipSuccess) return;
        const std::string path = std::string(pre) + "_" + name + ".bin";
        if (FILE* fp = std::fopen(path.c_str(), "wb")) {
            std::fwrite(h.data(), 1, bytes, fp);
            std::fclose(fp);
        }
    };
    const int32_t meta[21] = {f->tri.nlevels, f->tri.npos, f->tri.hpos, f->tri.hlevels, f->tri.nwpass, f->tri.chunk0, f->tri.nchunks, f->tri.chunk_two,
                              f->tri.tail_chunks, f->tri.grid, f->tri.multi, (int32_t)f->tri.nnz_off,
                              f->tri.npass, f->tri.nslices, f->tri.slice_b, f->tri.wave_head, f->tri.poll_fast, f->tri.poll_mode, f->tri.grid_multi,
                              f->tri.hconc, f->tri.red_grid};
    if (FILE* fp = std::fopen((std::string(pre) + "_meta.bin").c_str(), "wb")) {
        std::fwrite(meta, sizeof(meta), 1, fp);
        std::fclose(fp);
    }
    // the position-indexed chunk arrays exist with the chunk tail only
    const size_t cpos = f->tri.tail_chunks ? (size_t)f->tri.npos : 0, cnnz = f->tri.tail_chunks ? (size_t)f->tri.nnz_off : 0;
    put("porder", f->tri.porder, cpos * 4);
    put("pptr", f->tri.pptr, f->tri.tail_chunks ? (cpos + 1) * 4 : 0);
    put("pcol", f->tri.pcol, cnnz * 4);
    put("pval", f->tri.pval, cnnz * sizeof(S));
    put("ppiv", f->tri.ppiv, cpos * sizeof(S));
    put("order", f->tri.order, (size_t)f->tri.hpos * 4);
    put("wval", f->tri.wval, (size_t)f->tri.nwpass * 256 * sizeof(S));
    put("wcol", f->tri.wcol, (size_t)f->tri.nwpass * 256 * 4);
    put("wrp", f->tri.wrp, (size_t)f->tri.nwpass * 16 * sizeof(S));
    put("wdst", f->tri.wdst, (size_t)f->tri.nwpass * 16 * 4);
    // slice tail (slice 0 always exists; the entry streams end with one more slice_b-deep slice, the
    // prefetch past the last slice) and one-workgroup head
    const size_t ns = (size_t)std::max(1, f->tri.nslices);
    int2 last = make_int2(0, 0);
    if (f->tri.nslices > 0 &&
        hipMemcpy(&last, f->tri.smeta + (f->tri.nslices - 1), sizeof(int2), hipMemcpyDeviceToHost) != hipSuccess)
        return;
    const size_t tent = (f->tri.nslices > 0 ? (size_t)last.x + 64 * (size_t)last.y : 0) + 64 * (size_t)f->tri.slice_b;
    put("smeta", f->tri.smeta, ns * sizeof(int2));
    put("trow", f->tri.trow, ns * 64 * 4);
    put("tpiv", f->tri.tpiv, ns * 64 * sizeof(S));
    put("tcol", f->tri.tcol, tent * 4);
    put("tval", f->tri.tval, tent * sizeof(S));
    put("hcol", f->tri.hcol, (size_t)f->tri.npass * dev::kHeadThreads * 4);
    put("hval", f->tri.hval, (size_t)f->tri.npass * dev::kHeadThreads * sizeof(S));
    put("hpiv", f->tri.hpiv, (size_t)f->tri.npass * dev::kHeadRows * sizeof(S));
    put("passes", f->tri.passes, (size_t)f->tri.npass * sizeof(int2));
}

// Triangular CSR (host arrays, columns ascending per row) -> level-ordered factor of A - sigma I.
template <class S>
static int factor_tri_host(eigsol_ctx* ctx, int dtype, int64_t n, const int32_t* rp, const int32_t* ci, const S* v,
                           bool up, double sre, double sim, ShiftFactor** out) {
    hipStream_t st = ctx->stream;
    const int64_t nnz = rp[n];
    ShiftFactor* f = shift_factor_new(ctx, dtype, n, sre, sim, nnz);
    int rc = EIGSOL_OK;
    f->tri.upper = up ? 1 : 0;
    // split diagonal / off-diagonal; pivots d_i - sigma (missing diagonal: 0 - sigma)
    const S sig = make_sigma<S>(sre, sim);
    std::vector<int32_t> orp(n + 1, 0), oci;
    std::vector<S> ov, pv(n);
    oci.reserve(nnz);
    ov.reserve(nnz);
    for (int64_t i = 0; i < n; ++i) {
        S d = s_zero<S>();
        for (int32_t e = rp[i]; e < rp[i + 1]; ++e) {
            if (ci[e] == i) {
                d = h_add(d, v[e]);
            } else {
                oci.push_back(ci[e]);
                ov.push_back(v[e]);
            }
        }
        pv[i] = h_sub(d, sig);
        if (h_zero(pv[i])) {
            shift_factor_free(f);
            return fail(EIGSOL_E_SOLVER, "solve_shifted: SparseLU factorization failed");
        }
        orp[i + 1] = (int32_t)oci.size();
    }
    f->tri.nnz_off = (int64_t)oci.size();
    std::vector<int32_t> order;
    std::vector<int64_t> lstart, lcount;
    level_order(orp, oci, n, up, order, f->tri.nlevels, lstart, lcount);
    f->tri.npos = (int32_t)order.size();
    std::vector<int32_t> plen(f->tri.npos, 0);         // off-diagonal entries per position
    std::vector<int32_t> lmaxlen(f->tri.nlevels, 0);   // longest row (off-diagonal entries) per level
    for (int32_t l = 0; l < f->tri.nlevels; ++l)
        for (int64_t p = lstart[l]; p < lstart[l] + lcount[l]; ++p) {
            plen[p] = orp[order[p] + 1] - orp[order[p]];
            lmaxlen[l] = std::max(lmaxlen[l], plen[p]);
        }
    const TriPlan pl = tri_plan<S>(f, lstart, lcount, lmaxlen, &plen);
    const std::vector<int2>& passes = pl.passes;
    f->tri.npass = (int32_t)passes.size();
    std::vector<int32_t> rowpos;
    if (f->tri.hpos > 0) {
        rowpos.assign(n, -1);
        for (int32_t p = 0; p < f->tri.hpos; ++p)
            if (order[p] >= 0) rowpos[order[p]] = p;
    }
    // head, pass-major (see sptrsv_head_kernel): columns are LDS positions of earlier head rows
    const size_t hslots = (size_t)f->tri.npass * dev::kHeadThreads;
    std::vector<int32_t> hcol(hslots, f->tri.hpos);   // padding: the zero slot
    std::vector<S> hval(hslots, s_zero<S>()), hpiv((size_t)f->tri.npass * dev::kHeadRows, make_sigma<S>(1.0, 0.0));
    for (int32_t q = 0; q < f->tri.npass; ++q) {
        const int32_t p0 = passes[q].x, p1 = passes[q].y & ~dev::kPassBarrier;
        for (int32_t p = p0; p < p1; ++p) {
            const size_t g = (size_t)q * dev::kHeadRows + (p - p0);
            const int32_t i = order[p];
            hpiv[g] = pv[i];
            for (int32_t e = orp[i]; e < orp[i + 1]; ++e) {
                hcol[g * dev::kRowLanes + (e - orp[i])] = rowpos[oci[e]];
                hval[g * dev::kRowLanes + (e - orp[i])] = ov[e];
            }
        }
    }
    // one-wave head (see sptrsv_whead_kernel): passes of <= 16 rows inside a level, 4 lanes per row,
    // entry idx of a row at lane 4 g + idx / 4, slot idx % 4; reciprocal pivots.
    // EIGSOL_TRSV_HEAD=block selects the one-workgroup head.
    std::vector<S> wval, wrp;
    std::vector<int32_t> wcol, wdst;
    {
        auto recip = [](S p) -> S {
            if constexpr (is_real_v<S>) return (S)1 / p;
            else {
                const double d = (double)p.re * (double)p.re + (double)p.im * (double)p.im;
                S r;
                r.re = (decltype(p.re))((double)p.re / d);
                r.im = (decltype(p.im))(-(double)p.im / d);
                return r;
            }
        };
        wval.assign((size_t)f->tri.nwpass * 256, s_zero<S>());
        wcol.assign((size_t)f->tri.nwpass * 256, f->tri.hpos);
        wrp.assign((size_t)f->tri.nwpass * dev::kWHeadRows, make_sigma<S>(1.0, 0.0));
        wdst.assign((size_t)f->tri.nwpass * dev::kWHeadRows, -1);
        for (int32_t q = 0; q < pl.nwreal; ++q) {
            const int32_t p = pl.wpass[q].x;
            for (int32_t u = 0; u < pl.wpass[q].y; ++u) {
                const int32_t i = order[p + u];
                wrp[(size_t)q * dev::kWHeadRows + u] = recip(pv[i]);
                wdst[(size_t)q * dev::kWHeadRows + u] = p + u;
                for (int32_t e = orp[i]; e < orp[i + 1]; ++e) {
                    const int32_t idx = e - orp[i];
                    const size_t slot = ((size_t)q * 4 + (size_t)(idx % 4)) * 64 + (size_t)(4 * u + idx / 4);
                    wcol[slot] = rowpos[oci[e]];
                    wval[slot] = ov[e];
                }
            }
        }
    }
    std::vector<int32_t> porder, pptr, pcol;
    std::vector<S> pval, ppiv;
    if (f->tri.tail_chunks) {   // position-indexed copies: no dependent metadata loads in the kernel
        porder = order;
        pptr.assign((size_t)f->tri.npos + 1, 0);
        ppiv.assign((size_t)f->tri.npos, make_sigma<S>(1.0, 0.0));
        pcol.reserve(oci.size());
        pval.reserve(oci.size());
        for (int32_t p = 0; p < f->tri.npos; ++p) {
            const int32_t i = order[p];
            if (i >= 0) {
                for (int32_t e = orp[i]; e < orp[i + 1]; ++e) {
                    pcol.push_back(oci[e]);
                    pval.push_back(ov[e]);
                }
                ppiv[p] = pv[i];
            }
            pptr[p + 1] = (int32_t)pcol.size();
        }
    }
    // the tail slices of the plan (none: nothing here, tri_empty_slice0 below)
    const std::vector<int32_t>&slen = pl.slen, &scount = pl.scount;
    const std::vector<int64_t>& sfirst = pl.sfirst;
    const int32_t Bs = f->tri.slice_b;
    std::vector<int2> smeta(f->tri.nslices, make_int2(0, Bs));
    std::vector<int32_t> trow((size_t)f->tri.nslices * 64, -1);
    std::vector<S> tpiv((size_t)f->tri.nslices * 64, make_sigma<S>(1.0, 0.0));
    int64_t tent = 0;
    for (int32_t sl = 0; sl < f->tri.nslices; ++sl) tent += 64 * (int64_t)std::max(slen[sl], Bs);
    if (f->tri.nslices > 0) tent += 64 * (int64_t)Bs;   // the prefetch of "slice ns" reads slice 0's range: keep it in bounds
    if (tent * (int64_t)sizeof(S) >= (int64_t)1 << 32) {
        shift_factor_free(f);
        return fail(EIGSOL_E_UNSUPPORTED, "triangular solve: factor streams exceed 4 GiB");
    }
    std::vector<int32_t> tcol((size_t)tent, (int32_t)n);   // padding: the zero slot z[n]
    std::vector<S> tval((size_t)tent, s_zero<S>());
    {
        int64_t off = 0;
        for (int32_t sl = 0; sl < f->tri.nslices; ++sl) {
            const int32_t Kp = std::max(slen[sl], Bs);
            smeta[sl] = make_int2((int32_t)off, Kp);
            for (int32_t u = 0; u < scount[sl]; ++u) {
                const int32_t i = order[sfirst[sl] + u];
                trow[(size_t)sl * 64 + u] = i;
                tpiv[(size_t)sl * 64 + u] = pv[i];
                for (int32_t e = orp[i]; e < orp[i + 1]; ++e) {
                    tcol[(size_t)(off + 64 * (e - orp[i]) + u)] = oci[e];
                    tval[(size_t)(off + 64 * (e - orp[i]) + u)] = ov[e];
                }
            }
            off += 64 * (int64_t)Kp;
        }
    }
    std::vector<int32_t>().swap(oci);
    std::vector<S>().swap(ov);
    auto up_ = [&](void** dst, const void* src, size_t bytes) -> int { return dev_upload(st, dst, src, bytes); };
    if (rc == EIGSOL_OK) rc = tri_launch_setup(f);
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.order, order.data(), (size_t)f->tri.hpos * 4);
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.hcol, hcol.data(), hcol.size() * 4);
    if (rc == EIGSOL_OK) rc = up_(&f->tri.hval, hval.data(), hval.size() * sizeof(S));
    if (rc == EIGSOL_OK) rc = up_(&f->tri.hpiv, hpiv.data(), hpiv.size() * sizeof(S));
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.passes, passes.data(), passes.size() * sizeof(int2));
    if (rc == EIGSOL_OK) rc = up_(&f->tri.wval, wval.data(), wval.size() * sizeof(S));
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.wcol, wcol.data(), wcol.size() * 4);
    if (rc == EIGSOL_OK) rc = up_(&f->tri.wrp, wrp.data(), wrp.size() * sizeof(S));
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.wdst, wdst.data(), wdst.size() * 4);
    if (rc == EIGSOL_OK && f->tri.nslices == 0) rc = tri_empty_slice0<S>(f);
    if (f->tri.nslices > 0) {
        if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.smeta, smeta.data(), smeta.size() * sizeof(int2));
        if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.trow, trow.data(), trow.size() * 4);
        if (rc == EIGSOL_OK) rc = up_(&f->tri.tpiv, tpiv.data(), tpiv.size() * sizeof(S));
        if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.tcol, tcol.data(), tcol.size() * 4);
        if (rc == EIGSOL_OK) rc = up_(&f->tri.tval, tval.data(), tval.size() * sizeof(S));
    }
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.porder, porder.data(), porder.size() * 4);
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.pptr, pptr.data(), pptr.size() * 4);
    if (rc == EIGSOL_OK) rc = up_((void**)&f->tri.pcol, pcol.data(), pcol.size() * 4);
    if (rc == EIGSOL_OK) rc = up_(&f->tri.pval, pval.data(), pval.size() * sizeof(S));
    if (rc == EIGSOL_OK) rc = up_(&f->tri.ppiv, ppiv.data(), ppiv.size() * sizeof(S));
    if (rc == EIGSOL_OK) rc = tri_state_alloc<S>(f);
    if (rc != EIGSOL_OK) { shift_factor_free(f); return rc; }
    f->kind = FactorKind::Tri;
    tri_dump<S>(f);
    *out = f;
    return EIGSOL_OK;
}

// What the device build holds while it runs: its device scratch, the pinned read-back words and the
// factor under construction.  The destructor gives all of it back, so every way out of the build
// cleans up; a finished build takes its factor out first (release).
struct TriDeviceBuild {
    hipStream_t st;
    std::vector<void*> scratch;
    int32_t* hostw = nullptr;
    ShiftFactor* f = nullptr;
    explicit TriDeviceBuild(hipStream_t s) : st(s) {}
    TriDeviceBuild(const TriDeviceBuild&) = delete;
    TriDeviceBuild& operator=(const TriDeviceBuild&) = delete;
    ~TriDeviceBuild() {
        hipStreamSynchronize(st);
        for (void* p : scratch) hipFree(p);
        if (hostw) hipHostFree(hostw);
        if (f) shift_factor_free(f);
    }
    ShiftFactor* release() {
        ShiftFactor* built = f;
        f = nullptr;
        return built;
    }
};

// Triangular CSR already on the device -> the level-ordered factor of A - sigma I, built on the device
// (round 5; the host build of config 5's 1M-row factor took 0.37 s, most of it moving 320 MB of
// matrix down and the layout back up).  The result is the host build's layout bit for bit: the
// same levels, positions sorted by level with ascending rows inside a level (stable radix sort),
// the same padding, the same position-indexed chunk CSR and the same one-wave head.  Only the small
// per-level tables (counts, longest rows) travel to the host, where tri_plan takes the head / tail
// decisions of both builds.  declined = true (nothing built) for a matrix that is not
// triangular or a layout this build does not produce (slice tail, one-workgroup head): the caller
// then takes the host path.
template <class S>
static int factor_tri_device(const TriCsrView& A, double sre, double sim, ShiftFactor** out, bool& declined) {
    declined = false;
    eigsol_ctx* ctx = A.ctx;
    hipStream_t st = ctx->stream;
    const int64_t n = A.n, nnz = A.nnz;
    const S* val = static_cast<const S*>(A.val);
    TriDeviceBuild own{st};   // every return below, the macros' included, leaves through its destructor
    std::vector<void*>& scratch = own.scratch;
    auto dalloc = [&](void** p, size_t bytes) -> int {
        EIGSOL_HIP(hipMalloc(p, std::max<size_t>(bytes, 16)));
        scratch.push_back(*p);
        return EIGSOL_OK;
    };
    int32_t*& hostw = own.hostw;   // pinned: flags[0..2], maxlev, err, nnz_off
    ShiftFactor*& f = own.f;
    constexpr int64_t W = dev::kWaveRows;
    S* pv = nullptr;
    int32_t *offlen = nullptr, *lev = nullptr, *lcnt = nullptr, *lmax = nullptr, *words = nullptr;
    int rc = EIGSOL_OK;
    if ((rc = dalloc((void**)&pv, n * sizeof(S))) || (rc = dalloc((void**)&offlen, n * 4)) ||
        (rc = dalloc((void**)&lev, n * 4)) || (rc = dalloc((void**)&lcnt, (n + 1) * 4)) ||
        (rc = dalloc((void**)&lmax, (n + 1) * 4)) || (rc = dalloc((void**)&words, 64)))
        return rc;
    if (hipHostMalloc(&hostw, 64, hipHostMallocDefault) != hipSuccess) return fail(EIGSOL_E_HIP, "hipHostMalloc");
    // words: [0..2] flags, [3] deepest level, [4] err, [5] ticket
    hipMemsetAsync(words, 0, 64, st);
    hipMemsetAsync(lev, 0xFF, n * 4, st);
    hipMemsetAsync(lcnt, 0, (n + 1) * 4, st);
    hipMemsetAsync(lmax, 0, (n + 1) * 4, st);
    const unsigned gb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((dev::tri_rows_kernel<S>), dim3(gb), dim3(256), 0, st, A.rowptr, A.col, val, n,
                       make_sigma<S>(sre, sim), pv, offlen, words);
    EIGSOL_HIP(hipMemcpyAsync(hostw, words, 64, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(EIGSOL_E_HIP, "triangular analysis: row scan");
    const bool up = !hostw[0], lo = !hostw[1];
    if (!up && !lo) {
        declined = true;
        return EIGSOL_OK;
    }
    if (hostw[2]) return fail(EIGSOL_E_SOLVER, "solve_shifted: SparseLU factorization failed");
    hipLaunchKernelGGL(dev::tri_level_kernel, dim3(std::max(1, 4 * ctx->num_cus)), dim3(256), 0, st, A.rowptr, A.col,
                       offlen, n, up ? 1 : 0, lev, reinterpret_cast<uint32_t*>(words + 5), lcnt, lmax, words + 3,
                       words + 4);
    EIGSOL_HIP(hipMemcpyAsync(hostw, words, 64, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(EIGSOL_E_HIP, "triangular analysis: levels");
    if (hostw[4]) {   // a dependency wait ran out of time: build on the host instead
        declined = true;
        return EIGSOL_OK;
    }
    const int32_t nlevels = hostw[3] + 1;
    std::vector<int32_t> hcnt(nlevels), hmax(nlevels);
    EIGSOL_HIP(hipMemcpyAsync(hcnt.data(), lcnt, nlevels * 4, hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipMemcpyAsync(hmax.data(), lmax, nlevels * 4, hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> lstart(nlevels + 1, 0), lcount(hcnt.begin(), hcnt.end());
    for (int32_t l = 0; l < nlevels; ++l) lstart[l + 1] = lstart[l] + ((lcount[l] + W - 1) / W) * W;
    f = shift_factor_new(ctx, A.dtype, n, sre, sim, nnz);
    f->tri.upper = up ? 1 : 0;
    f->tri.nlevels = nlevels;
    f->tri.npos = (int32_t)lstart[nlevels];
    const TriPlan pl = tri_plan<S>(f, lstart, lcount, hmax, nullptr);
    if (!pl.device_buildable) {
        declined = true;
        return EIGSOL_OK;
    }
    // positions: rows sorted by level, at each level's padded start
    int bits = 1;
    while (bits < 31 && (int64_t(1) << bits) <= (int64_t)(nlevels - 1)) ++bits;
    int32_t *lev_s = nullptr, *rows_s = nullptr, *ustart = nullptr, *pstart = nullptr, *plen = nullptr;
    if ((rc = dalloc((void**)&lev_s, n * 4)) || (rc = dalloc((void**)&rows_s, n * 4)) ||
        (rc = dalloc((void**)&ustart, (size_t)nlevels * 4)) || (rc = dalloc((void**)&pstart, (size_t)nlevels * 4)) ||
        (rc = dalloc((void**)&plen, ((size_t)f->tri.npos + 1) * 4)))
        return rc;
    if (tri_sort_rows_by_level(st, lev, lev_s, rows_s, n, bits) != hipSuccess)
        return fail(EIGSOL_E_HIP, "triangular analysis: level sort");
    std::vector<int32_t> hu(nlevels), hp(nlevels);
    {
        int64_t u = 0;
        for (int32_t l = 0; l < nlevels; ++l) {
            hu[l] = (int32_t)u;
            hp[l] = (int32_t)lstart[l];
            u += lcount[l];
        }
    }
    EIGSOL_HIP(hipMemcpyAsync(ustart, hu.data(), (size_t)nlevels * 4, hipMemcpyHostToDevice, st));
    EIGSOL_HIP(hipMemcpyAsync(pstart, hp.data(), (size_t)nlevels * 4, hipMemcpyHostToDevice, st));
    const int64_t npos = f->tri.npos;
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.porder, nullptr, (size_t)npos * 4));
    EIGSOL_HIP(hipMemsetAsync(f->tri.porder, 0xFF, (size_t)npos * 4, st));
    hipLaunchKernelGGL(dev::tri_order_kernel, dim3(gb), dim3(256), 0, st, lev_s, rows_s, n, ustart, pstart, f->tri.porder);
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.order, nullptr, (size_t)f->tri.hpos * 4));
    if (f->tri.hpos > 0)
        EIGSOL_HIP(hipMemcpyAsync(f->tri.order, f->tri.porder, (size_t)f->tri.hpos * 4, hipMemcpyDeviceToDevice, st));
    // position-indexed chunk CSR: pivots, row pointers (scan of the off-diagonal counts), entries
    const S one = make_sigma<S>(1.0, 0.0);
    EIGSOL_TRY(dev_upload(st, &f->tri.ppiv, nullptr, (size_t)npos * sizeof(S)));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.pptr, nullptr, ((size_t)npos + 1) * 4));
    hipLaunchKernelGGL((dev::tri_poslen_kernel<S>), dim3((unsigned)((npos + 256) / 256)), dim3(256), 0, st, f->tri.porder,
                       npos, offlen, pv, one, plen, static_cast<S*>(f->tri.ppiv));
    if (tri_exclusive_scan(st, plen, f->tri.pptr, npos) != hipSuccess)
        return fail(EIGSOL_E_HIP, "triangular analysis: row pointer scan");
    EIGSOL_HIP(hipMemcpyAsync(hostw + 5, f->tri.pptr + npos, 4, hipMemcpyDeviceToHost, st));
    EIGSOL_HIP(hipStreamSynchronize(st));
    f->tri.nnz_off = hostw[5];
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.pcol, nullptr, (size_t)f->tri.nnz_off * 4));
    EIGSOL_TRY(dev_upload(st, &f->tri.pval, nullptr, (size_t)f->tri.nnz_off * sizeof(S)));
    hipLaunchKernelGGL((dev::tri_gather_kernel<S>), dim3((unsigned)((npos * dev::kRowLanes + 255) / 256)), dim3(256), 0,
                       st, f->tri.porder, npos, f->tri.pptr, A.rowptr, A.col, val, offlen, f->tri.pcol, static_cast<S*>(f->tri.pval));
    // one-wave head: the plan's passes (the padding passes keep the arrays' pre-fill)
    const std::vector<int2>& ptab = pl.wpass;
    const int32_t nreal = pl.nwreal;
    const size_t wslots = (size_t)f->tri.nwpass * 256, wrows = (size_t)f->tri.nwpass * dev::kWHeadRows;
    EIGSOL_TRY(dev_upload(st, &f->tri.wval, nullptr, wslots * sizeof(S)));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.wcol, nullptr, wslots * 4));
    EIGSOL_TRY(dev_upload(st, &f->tri.wrp, nullptr, wrows * sizeof(S)));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.wdst, nullptr, wrows * 4));
    if (f->tri.nwpass > 0) {
        int32_t* rowpos = nullptr;
        int2* dtab = nullptr;
        if ((rc = dalloc((void**)&rowpos, n * 4)) || (rc = dalloc((void**)&dtab, (size_t)nreal * sizeof(int2))))
            return rc;
        EIGSOL_HIP(hipMemcpyAsync(dtab, ptab.data(), (size_t)nreal * sizeof(int2), hipMemcpyHostToDevice, st));
        EIGSOL_HIP(hipMemsetAsync(rowpos, 0xFF, n * 4, st));
        EIGSOL_HIP(hipMemsetAsync(f->tri.wval, 0, wslots * sizeof(S), st));
        EIGSOL_HIP(hipMemsetAsync(f->tri.wdst, 0xFF, wrows * 4, st));
        hipLaunchKernelGGL((dev::fill_kernel<int32_t>), dim3(256), dim3(256), 0, st, f->tri.wcol, (int64_t)wslots, f->tri.hpos);
        hipLaunchKernelGGL((dev::fill_kernel<S>), dim3(64), dim3(256), 0, st, static_cast<S*>(f->tri.wrp), (int64_t)wrows, one);
        hipLaunchKernelGGL(dev::tri_rowpos_kernel, dim3((unsigned)((f->tri.hpos + 255) / 256)), dim3(256), 0, st, f->tri.porder,
                           f->tri.hpos, rowpos);
        hipLaunchKernelGGL((dev::tri_whead_kernel<S>), dim3((unsigned)((nreal * dev::kWHeadRows + 255) / 256)), dim3(256),
                           0, st, dtab, nreal, f->tri.porder, A.rowptr, A.col, val, pv, rowpos, static_cast<S*>(f->tri.wval),
                           f->tri.wcol, static_cast<S*>(f->tri.wrp), f->tri.wdst);
    }
    // the one-workgroup head's tables stay empty (npass = 0: that head is not built here)
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.hcol, nullptr, 0));
    EIGSOL_TRY(dev_upload(st, &f->tri.hval, nullptr, 0));
    EIGSOL_TRY(dev_upload(st, &f->tri.hpiv, nullptr, 0));
    EIGSOL_TRY(dev_upload(st, (void**)&f->tri.passes, nullptr, 0));
    // slice tail: none (nslices = 0)
    EIGSOL_TRY(tri_empty_slice0<S>(f));
    if (hipGetLastError() != hipSuccess) return fail(EIGSOL_E_HIP, "triangular analysis: launch");
    if ((rc = tri_launch_setup(f)) != EIGSOL_OK) return rc;
    if ((rc = tri_state_alloc<S>(f)) != EIGSOL_OK) return rc;
    f->kind = FactorKind::Tri;
    tri_dump<S>(f);
    *out = own.release();
    return EIGSOL_OK;
}

// the host build is forced, whatever the device build could do (read per call)
static bool tri_host_forced() {
    const char* e = std::getenv("EIGSOL_TRSV_HOST");
    return e && std::atoi(e);
}

template <class S>
int tri_build(const TriCsrView& A, double sre, double sim, int up, TriHostCsr<S>& h, ShiftFactor** out) {
    *out = nullptr;
    if (A.n > 0 && !tri_host_forced()) {
        bool declined = false;
        const int rc = factor_tri_device<S>(A, sre, sim, out, declined);
        if (!declined) return rc;
    }
    if (!h.rp) {
        hipStream_t st = A.ctx->stream;
        h.rp_own.resize(A.n + 1);
        h.ci_own.resize(A.nnz);
        h.v_own.resize(A.nnz);
        EIGSOL_HIP(hipMemcpyAsync(h.rp_own.data(), A.rowptr, (A.n + 1) * 4, hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(h.ci_own.data(), A.col, A.nnz * 4, hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipMemcpyAsync(h.v_own.data(), A.val, A.nnz * sizeof(S), hipMemcpyDeviceToHost, st));
        EIGSOL_HIP(hipStreamSynchronize(st));
        h.rp = h.rp_own.data();
        h.ci = h.ci_own.data();
        h.v = h.v_own.data();
    }
    if (up < 0) {
        bool upper = true, lower = true;
        for (int64_t i = 0; i < A.n && (upper || lower); ++i)
            for (int32_t e = h.rp[i]; e < h.rp[i + 1]; ++e) {
                if (h.ci[e] < i) upper = false;
                if (h.ci[e] > i) lower = false;
            }
        if (!upper && !lower) return EIGSOL_OK;
        up = upper ? 1 : 0;
    }
    return factor_tri_host<S>(A.ctx, A.dtype, A.n, h.rp, h.ci, h.v, up != 0, sre, sim, out);
}
template int tri_build<double>(const TriCsrView&, double, double, int, TriHostCsr<double>&, ShiftFactor**);
template int tri_build<float>(const TriCsrView&, double, double, int, TriHostCsr<float>&, ShiftFactor**);
template int tri_build<cplx>(const TriCsrView&, double, double, int, TriHostCsr<cplx>&, ShiftFactor**);
template int tri_build<cplxf>(const TriCsrView&, double, double, int, TriHostCsr<cplxf>&, ShiftFactor**);

// triangular factor from host CSR arrays (the ILU(0) factors of the GMRES path, gmres.hip)
int shift_factor_tri(eigsol_ctx* ctx, int dtype, int64_t n, std::vector<int32_t>& rp, std::vector<int32_t>& ci,
                     const void* vals, bool up, ShiftFactor** out) {
    // the GMRES path's L / U (host arrays): uploaded once and analysed and laid out on the device
    // like a triangular A (round 5: the 1M general-sparse factor's two host layouts took ~0.8 s);
    // a forced host build (tri_host_forced) or a declined device analysis keeps the host build (the same bytes), which
    // reads the caller's arrays
    return by_dtype(dtype, [&](auto tag) {
        using S = decltype(tag);
        TriHostCsr<S> h;
        h.rp = rp.data();
        h.ci = ci.data();
        h.v = static_cast<const S*>(vals);
        TriCsrView A{ctx, dtype, n, rp[n], nullptr, nullptr, nullptr};
        void* d[3] = {nullptr, nullptr, nullptr};   // row pointers, columns, values: all the device analysis reads
        int rc = EIGSOL_OK;
        if (n > 0 && !tri_host_forced()) {
            hipStream_t st = ctx->stream;
            if (hipMalloc(&d[0], (n + 1) * 4) != hipSuccess || hipMalloc(&d[1], std::max<int64_t>(1, A.nnz) * 4) != hipSuccess ||
                hipMalloc(&d[2], std::max<int64_t>(1, A.nnz) * sizeof(S)) != hipSuccess)
                rc = fail(EIGSOL_E_HIP, "solve_shifted: triangular factor upload");
            if (rc == EIGSOL_OK) {
                hipMemcpyAsync(d[0], rp.data(), (n + 1) * 4, hipMemcpyHostToDevice, st);
                hipMemcpyAsync(d[1], ci.data(), A.nnz * 4, hipMemcpyHostToDevice, st);
                hipMemcpyAsync(d[2], vals, A.nnz * sizeof(S), hipMemcpyHostToDevice, st);
            }
            A.rowptr = static_cast<const int32_t*>(d[0]);
            A.col = static_cast<const int32_t*>(d[1]);
            A.val = d[2];
        }
        if (rc == EIGSOL_OK) rc = tri_build<S>(A, 0.0, 0.0, up ? 1 : 0, h, out);
        hipStreamSynchronize(ctx->stream);
        for (void* p : d)
            if (p) hipFree(p);
        return rc;
    });
}

// A triangular factor given as device CSR arrays (the GMRES path's L / U, split on the device):
// analysed and laid out on the device; a declined analysis or a forced host build takes the host
// build on a downloaded copy (the same bytes).  The arrays stay the caller's.
int shift_factor_tri_dev(eigsol_ctx* ctx, int dtype, int64_t n, int32_t* rp, int32_t* ci, void* vals, int64_t nnz,
                         bool up, ShiftFactor** out) {
    return by_dtype(dtype, [&](auto tag) {
        using S = decltype(tag);
        TriHostCsr<S> h;
        return tri_build<S>(TriCsrView{ctx, dtype, n, nnz, rp, ci, vals}, 0.0, 0.0, up ? 1 : 0, h, out);
    });
}

}  // namespace eigsol
