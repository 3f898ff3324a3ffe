// The failure contract of csrc/scratch.hpp (DevBuf, PinBuf, StageClock), run with no visible device so that
// every allocation and every event creation fails: the status returned, the state left behind, and
// that releasing and destroying empty objects does nothing.  Built with the host sanitizers by
// tests/test_scratch_cpu.py; stands alone (eigsol::fail is defined here, as runtime.cpp defines it).
#include <cstdio>
#include <string>
#include <type_traits>

#include "scratch.hpp"

namespace {
std::string g_last_error;
int g_failed = 0;
}  // namespace

namespace eigsol {
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int status, const std::string& msg) {
    g_last_error = msg;
    return status;
}
}  // namespace eigsol

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("test_scratch: FAILED %s (line %d)\n", #cond, __LINE__); \
            ++g_failed;                                                        \
        }                                                                      \
    } while (0)

using eigsol::DevBuf;
using eigsol::PinBuf;
using eigsol::StageClock;

static_assert(!std::is_copy_constructible_v<DevBuf> && !std::is_copy_assignable_v<DevBuf>);
static_assert(!std::is_copy_constructible_v<PinBuf> && !std::is_copy_assignable_v<PinBuf>);
static_assert(!std::is_copy_constructible_v<StageClock> && !std::is_copy_assignable_v<StageClock>);

template <class Buf>
static void failed_alloc(const char* what) {
    Buf never;   // destroyed without ever holding memory
    Buf b;
    g_last_error.clear();
    const int rc = b.alloc(1024);
    CHECK(rc == EIGSOL_E_HIP);
    CHECK(b.p == nullptr);
    CHECK(b.template as<double>() == nullptr);
    CHECK(!g_last_error.empty());
    CHECK(g_last_error.find(what) != std::string::npos);
    g_last_error.clear();
    CHECK(b.alloc(0) == EIGSOL_E_HIP && b.p == nullptr && !g_last_error.empty());   // a second attempt, the same
    b.release();
    b.release();
    CHECK(b.p == nullptr);
}

// what a driver does: the first failure returns, and everything declared so far is destroyed
static int driver_shape() {
    DevBuf a, b;
    PinBuf h;
    StageClock clock;
    EIGSOL_TRY(clock.start(4));
    EIGSOL_TRY(a.alloc(64));
    EIGSOL_TRY(b.alloc(64));
    EIGSOL_TRY(h.alloc(64));
    return EIGSOL_OK;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        std::printf("test_scratch: a device is visible; run with HIP_VISIBLE_DEVICES= (empty)\n");
        return 2;
    }
    failed_alloc<DevBuf>("hipMalloc");
    failed_alloc<PinBuf>("hipHostMalloc");
    {
        StageClock never;
        double ms[3] = {1.0, 2.0, 3.0};
        never.read(ms, 3);   // nothing started: zeros
        CHECK(ms[0] == 0.0 && ms[1] == 0.0 && ms[2] == 0.0);
    }
    {
        StageClock clock;
        g_last_error.clear();
        CHECK(clock.start(4) == EIGSOL_E_HIP);
        CHECK(!g_last_error.empty());
        CHECK(clock.ev.empty());              // no event exists, so read below cannot touch one
        CHECK(clock.mark(0, nullptr) != EIGSOL_OK);
        double ms[4] = {1.0, 2.0, 3.0, 4.0};
        clock.read(ms, 4);
        CHECK(ms[0] == 0.0 && ms[1] == 0.0 && ms[2] == 0.0 && ms[3] == 0.0);
    }
    CHECK(driver_shape() == EIGSOL_E_HIP);
    if (g_failed) return 1;
    std::printf("test_scratch: ok\n");
    return 0;
}
