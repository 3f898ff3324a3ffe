// Call-local scratch of the host drivers: owning device and pinned buffers and a per-call stage timer.
// Everything here is released by its destructor, so a driver may return from any point.  Buffers that
// outlive a call (members of a matrix, session or factor handle) are freed by their handle instead.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "internal.hpp"

namespace eigsol {

// Device memory.  alloc() takes at least 64 bytes (a zero-size request still yields a pointer) and first
// releases what the buffer holds; hipFree waits for the device, so kernels still queued on a stream when a
// driver returns have finished before their scratch goes.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    int alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 64));
        if (e == hipSuccess) return EIGSOL_OK;
        p = nullptr;
        return fail(EIGSOL_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Pinned host memory (staging of small device results read every sweep)
struct PinBuf {
    void* p = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    int alloc(size_t bytes) {
        release();
        const hipError_t e = hipHostMalloc(&p, std::max<size_t>(bytes, 64), hipHostMallocDefault);
        if (e == hipSuccess) return EIGSOL_OK;
        p = nullptr;
        return fail(EIGSOL_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Stage times of one driver call: stage q runs from event q to event q + 1.  The driver marks the
// boundaries it passes and, once the stream has been waited for, reads the stages between two marks.
struct StageClock {
    std::vector<hipEvent_t> ev;
    std::vector<char> marked;
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock() {
        for (hipEvent_t x : ev) (void)hipEventDestroy(x);
    }
    int start(int stages) {
        while ((int)ev.size() <= stages) {   // stages + 1 boundaries
            hipEvent_t x = nullptr;
            const hipError_t e = hipEventCreate(&x);
            if (e != hipSuccess) return fail(EIGSOL_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
            ev.push_back(x);
            marked.push_back(0);
        }
        return EIGSOL_OK;
    }
    int mark(int i, hipStream_t st) {
        if (i < 0 || i >= (int)ev.size()) return fail(EIGSOL_E_INVALID, "StageClock: mark outside the stages started");
        EIGSOL_HIP(hipEventRecord(ev[i], st));
        marked[i] = 1;
        return EIGSOL_OK;
    }
    // ms[q] for q < count: the time of stage q where both of its marks were recorded, else 0
    void read(double* ms, int count) const {
        for (int q = 0; q < count; ++q) {
            float t = 0.0f;
            if (q + 1 < (int)ev.size() && marked[q] && marked[q + 1] && hipEventElapsedTime(&t, ev[q], ev[q + 1]) != hipSuccess)
                t = 0.0f;
            ms[q] = t;
        }
    }
};

}  // namespace eigsol
