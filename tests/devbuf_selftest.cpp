// Stand-alone check of DevBuf's ownership rules (cuda-slam_amd/csrc/devbuf.h) on the host: the header alone, with malloc-backed, counting
// stand-ins for the allocator it declares.  No HIP runtime is linked.  tests/test_devbuf.py builds it plain and under the address and
// undefined-behaviour sanitizers and runs both.
#include "../cuda-slam_amd/csrc/devbuf.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <utility>

static std::set<void*> g_live;          // what device_alloc handed out and nobody has freed
static int g_allocs = 0, g_frees = 0, g_retired = 0, g_double_frees = 0, g_errors = 0;
static bool g_fail_next = false;
static size_t g_last_bytes = 0;
static void* g_last_retired = nullptr;

static void give_back(void* p)
{
    if (g_live.erase(p) != 1) { g_double_frees++; return; }
    free(p);
}

extern "C" const char* hipGetErrorString(hipError_t) { return "stand-in"; }

namespace mislam {
void set_error(const char*, ...) { g_errors++; }
hipError_t device_alloc(void** p, size_t bytes)
{
    if (g_fail_next) { g_fail_next = false; return hipErrorOutOfMemory; }      // (*p is left as it was)
    *p = malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    g_allocs++;
    g_last_bytes = bytes;
    return hipSuccess;
}
void device_free(void* p) { g_frees++; give_back(p); }
void retire_later(void* p) { g_retired++; g_last_retired = p; give_back(p); }
double& alloc_ms_counter() { static double ms = 0.0; return ms; }
double wall_ms() { static double t = 0.0; return t += 1.0; }
}  // namespace mislam

using mislam::DevBuf;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

struct Several {
    DevBuf<float> a, b;
    DevBuf<int> c;
    struct Inner { DevBuf<unsigned char> d; } inner;
};

int main()
{
    {   // a scope exit frees the buffer
        DevBuf<float> b;
        CHECK(b.reserve(100) == MI_OK && b.p != nullptr && b.cap == 100 && g_last_bytes == 100 * sizeof(float));
        CHECK(g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_allocs == 1 && g_frees == 1 && g_retired == 0);
    {   // an empty one frees nothing
        DevBuf<int> e;
    }
    CHECK(g_frees == 1);

    {   // a struct of several buffers frees all of them by its implicit destructor
        Several s;
        CHECK(s.a.reserve(3) == MI_OK && s.b.reserve(5) == MI_OK && s.c.reserve(7) == MI_OK && s.inner.d.reserve(9) == MI_OK);
        CHECK(g_live.size() == 4);
    }
    CHECK(g_live.empty() && g_frees == 5);

    {   // moves leave the source empty and free nothing twice
        DevBuf<float> a;
        CHECK(a.reserve(10) == MI_OK);
        float* pa = a.p;
        DevBuf<float> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 10 && g_frees == 5);
        DevBuf<float> c;
        CHECK(c.reserve(20) == MI_OK);
        float* pc = c.p;
        b = std::move(c);                                  // b's own buffer goes, c's moves in
        CHECK(g_frees == 6 && g_live.count(pa) == 0 && c.p == nullptr && c.cap == 0 && b.p == pc && b.cap == 20);
        DevBuf<float>& self = b;
        b = std::move(self);                               // onto itself: nothing happens
        CHECK(g_frees == 6 && b.p == pc && b.cap == 20);
        Several s, t;
        CHECK(s.a.reserve(4) == MI_OK && t.a.reserve(6) == MI_OK);
        s = std::move(t);                                  // member-wise, by the implicit move assignment
        CHECK(g_frees == 7 && s.a.cap == 6 && t.a.p == nullptr);
    }
    CHECK(g_live.empty() && g_double_frees == 0 && g_frees == 9 && g_retired == 0);

    {   // growth: the outgrown pointer goes to retire_later, once, and never to device_free; at least half again
        DevBuf<int> b;
        CHECK(b.reserve(100) == MI_OK);
        int* p0 = b.p;
        const int allocs = g_allocs;
        CHECK(b.reserve(100) == MI_OK && b.reserve(1) == MI_OK && b.p == p0 && g_allocs == allocs);      // fits: untouched
        CHECK(b.reserve(101) == MI_OK && b.cap == 150 && g_last_bytes == 150 * sizeof(int));
        CHECK(g_retired == 1 && g_last_retired == p0 && g_frees == 9);
        CHECK(b.reserve(1000) == MI_OK && b.cap == 1000 && g_retired == 2);
    }
    CHECK(g_live.empty() && g_frees == 10 && g_double_frees == 0);

    {   // a failed allocation leaves the buffer empty (the outgrown pointer is retired all the same); the destructor then frees nothing
        DevBuf<double> b;
        g_fail_next = true;
        CHECK(b.reserve(8) == MI_ERR_HIP && b.p == nullptr && b.cap == 0 && g_errors == 1);
        CHECK(b.reserve(8) == MI_OK && b.cap == 8);
        g_fail_next = true;
        CHECK(b.reserve(9) == MI_ERR_HIP && b.p == nullptr && b.cap == 0 && g_retired == 3);
    }
    CHECK(g_live.empty() && g_frees == 10 && g_double_frees == 0);
    static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "DevBuf does not copy");

    if (g_failed) { printf("devbuf selftest: %d checks FAILED\n", g_failed); return 1; }
    printf("devbuf selftest ok\n");
    return 0;
}
