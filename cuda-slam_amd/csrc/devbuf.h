// DevBuf: the grow-only device buffer behind every allocation of the library.  It owns its memory.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "../../include/mi_slam.h"

namespace mislam {

void set_error(const char* fmt, ...);

#define MI_HIP(call)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            mislam::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);  \
            return MI_ERR_HIP;                                                                             \
        }                                                                                                  \
    } while (0)

// Device buffers that were outgrown: work already enqueued may still read them, so they are released at the next point where the
// host has drained the stream anyway (retire_buffers, called behind the loads' and runs' own synchronisations) -- not behind a
// device-wide synchronisation per buffer, which is what a load of forty buffers used to pay when a size was new.
// The list is the CONTEXT's (mi_ctx::retired): a buffer outgrown inside a call on context A is released only behind a drain of A's own
// stream, with A's device current -- never by another host thread's context, never on another device (round 3 kept one process-wide list).
void retire_later(void* p);                        // into the list of the context whose call is running on this thread (CtxScope)
// Device memory comes out of the runtime's stream-ordered pool, kept whole (release threshold: never): hipFree of a plain
// allocation costs ~0.2 ms on this machine (tools/alloc_probe.cpp) -- forty buffers outgrown by a new size were 8 ms -- the pool's
// free is ~1 us and its memory is handed out again.  MISLAM_POOL=0 (or a runtime without the pool) falls back to hipMalloc / hipFree.
hipError_t device_alloc(void** p, size_t bytes);
void device_free(void* p);
double& alloc_ms_counter();        // host ms this thread has spent in hipMalloc through DevBuf::reserve (mi_icp_load_times)
double wall_ms();

// grow-only device buffer; grows by at least half (a sweep over slowly rising sizes reallocates a few times, not every call).
// It frees its memory when it goes out of scope, so an owner of buffers -- the context, a workspace struct, a call's locals -- lists them as
// members and nothing else; it moves, and does not copy.  The destructor frees at once (device_free, never retire_later: no call is running
// then), so the owner drains the streams that used the buffer first: mi_ctx_destroy does, a call's locals go behind the call's last
// synchronisation.  No DevBuf may have static storage duration: its destructor would run after the HIP runtime has shut down.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    ~DevBuf() { if (p) device_free(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            if (p) device_free(p);
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    int reserve(size_t count)
    {
        if (count <= cap) return MI_OK;
        if (p) retire_later(p);
        p = nullptr;
        const size_t grown = cap + cap / 2;
        if (cap != 0 && count < grown) count = grown;
        cap = 0;
        const double t0 = wall_ms();
        MI_HIP(device_alloc((void**)&p, count * sizeof(T)));
        alloc_ms_counter() += wall_ms() - t0;
        cap = count;
        return MI_OK;
    }
};

}  // namespace mislam
