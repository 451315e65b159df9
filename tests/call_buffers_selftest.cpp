// Stand-alone check of CallBuffers (cuda-slam_amd/csrc/call_buffers.hpp) on the host: the header alone, with a malloc-backed, counting stand-in
// for the allocator devbuf.h declares and a stand-in hipMemcpyAsync that records each copy and does it with memcpy.  No HIP runtime is linked.
// tests/test_call_buffers.py builds it plain and under the address and undefined-behaviour sanitizers and runs both.
#include "../cuda-slam_amd/csrc/call_buffers.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

static int g_allocs = 0, g_errors = 0;
static bool g_fail_next = false;
struct Copy { void* dst; const void* src; size_t bytes; };
static std::vector<Copy> g_copies;

extern "C" const char* hipGetErrorString(hipError_t) { return "stand-in"; }
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t)
{
    g_copies.push_back(Copy{dst, src, bytes});
    memcpy(dst, src, bytes);
    return hipSuccess;
}

namespace mislam {
void set_error(const char*, ...) { g_errors++; }
hipError_t device_alloc(void** p, size_t bytes)
{
    if (g_fail_next) { g_fail_next = false; return hipErrorOutOfMemory; }
    *p = calloc(bytes ? bytes : 1, 1);
    g_allocs++;
    return hipSuccess;
}
void device_free(void* p) { free(p); }
void retire_later(void* p) { free(p); }
double& alloc_ms_counter() { static double ms = 0.0; return ms; }
double wall_ms() { static double t = 0.0; return t += 1.0; }
}  // namespace mislam

using mislam::CallBuffers;
using mislam::DevBuf;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

int main()
{
    {   // need reserves and records; result with a null host pointer does neither; fits() holds after the reserves
        DevBuf<float> a, skipped;
        DevBuf<int> b;
        DevBuf<unsigned char> d;
        CallBuffers l;
        float* none = nullptr;
        int host_b[7];
        unsigned char host_d[5];
        CHECK(l.need(a, 100) == MI_OK && a.p && a.cap == 100 && l.used == 1 && g_allocs == 1);
        CHECK(l.result(skipped, 50, none) == MI_OK && skipped.p == nullptr && skipped.cap == 0 && l.used == 1 && g_allocs == 1);
        CHECK(l.result(b, 7, host_b) == MI_OK && b.cap == 7 && l.used == 2);
        CHECK(l.need(d, 5, host_d) == MI_OK && d.cap == 5 && l.used == 3 && g_allocs == 3);
        CHECK(l.fits());

        // download: exactly the recorded copies, in the order recorded, count * sizeof(T) bytes each; what stays on the device is not copied
        for (int i = 0; i < 7; i++) b.p[i] = 10 + i;
        for (int i = 0; i < 5; i++) d.p[i] = (unsigned char)(200 + i);
        CHECK(l.download(nullptr) == MI_OK && g_copies.size() == 2);
        CHECK(g_copies[0].dst == host_b && g_copies[0].src == b.p && g_copies[0].bytes == 7 * sizeof(int));
        CHECK(g_copies[1].dst == host_d && g_copies[1].src == d.p && g_copies[1].bytes == 5);
        CHECK(host_b[6] == 16 && host_d[4] == 204);
        g_copies.clear();

        // recorded twice: one entry, the larger length holds, in either order; a host pointer given later stands
        float host_a[120];
        CHECK(l.need(a, 120, host_a) == MI_OK && l.used == 3 && a.cap >= 120 && l.fits());
        CHECK(l.need(a, 60) == MI_OK && l.used == 3);
        CHECK(l.download(nullptr) == MI_OK && g_copies.size() == 3 && g_copies[0].dst == host_a && g_copies[0].bytes == 120 * sizeof(float));
        g_copies.clear();

        // fits() reads the buffers again: a recorded buffer that was move-assigned a shorter one, or an empty one, no longer fits
        DevBuf<int> shorter, longer;
        CHECK(shorter.reserve(6) == MI_OK && longer.reserve(9) == MI_OK);
        b = std::move(longer);
        CHECK(l.fits());
        b = std::move(shorter);
        CHECK(!l.fits());
        b = DevBuf<int>();
        CHECK(b.p == nullptr && !l.fits());
        CHECK(b.reserve(7) == MI_OK && l.fits());
    }
    {   // watch records another owner's buffer and reserves nothing: it fits once that owner has made it long enough, and no sooner
        DevBuf<float> theirs;
        CallBuffers l;
        const int allocs = g_allocs;
        CHECK(l.watch(theirs, 30) == MI_OK && l.used == 1 && theirs.p == nullptr && g_allocs == allocs && !l.fits());
        CHECK(theirs.reserve(20) == MI_OK && !l.fits());
        CHECK(theirs.reserve(30) == MI_OK && l.fits());
        CHECK(l.need(theirs, 10) == MI_OK && l.used == 1 && l.fits());                  // the same entry; the larger length holds
        CHECK(l.download(nullptr) == MI_OK && g_copies.empty());
    }
    {   // a failing allocation: need returns the error, records nothing, and the list still speaks for the others
        DevBuf<float> a, f;
        CallBuffers l;
        float host_f[4];
        CHECK(l.need(a, 8) == MI_OK);
        g_fail_next = true;
        const int errors = g_errors;
        CHECK(l.need(f, 4, host_f) == MI_ERR_HIP && g_errors == errors + 1 && l.used == 1 && f.p == nullptr && l.fits());
        CHECK(l.download(nullptr) == MI_OK && g_copies.empty());
        // ... and one that fails while a recorded buffer grows leaves that entry, which no longer fits
        g_fail_next = true;
        CHECK(l.need(a, 800) == MI_ERR_HIP && l.used == 1 && a.p == nullptr && !l.fits());
    }
    {   // one entry more than the capacity is refused: nothing allocated, nothing written (the sanitized build watches the guards on either side)
        struct { unsigned char before[64]; CallBuffers l; unsigned char after[64]; } s;
        memset(s.before, 0xa5, sizeof s.before); memset(s.after, 0x5a, sizeof s.after);
        std::vector<DevBuf<int>> bufs(CallBuffers::CAPACITY + 1);
        for (int i = 0; i < CallBuffers::CAPACITY; i++) CHECK(s.l.need(bufs[i], 3) == MI_OK);
        const int allocs = g_allocs, errors = g_errors;
        DevBuf<int>& extra = bufs[CallBuffers::CAPACITY];
        CHECK(s.l.need(extra, 3) == MI_ERR_STATE && s.l.used == CallBuffers::CAPACITY && g_allocs == allocs && g_errors == errors + 1 && extra.p == nullptr);
        CHECK(s.l.need(bufs[0], 9) == MI_OK && s.l.used == CallBuffers::CAPACITY && s.l.fits());      // a buffer already listed is still taken
        bool intact = true;
        for (unsigned char v : s.before) intact = intact && v == 0xa5;
        for (unsigned char v : s.after) intact = intact && v == 0x5a;
        CHECK(intact);
    }

    if (g_failed) { printf("call buffers selftest: %d checks FAILED\n", g_failed); return 1; }
    printf("call buffers selftest ok\n");
    return 0;
}
