// CallBuffers: the device buffers of one call, each stated once with the length the call's launches assume.  A driver fills the list before its
// first upload, asks fits() in front of its first hand-written kernel, and ends in download(stream).  Which of the three to record with:
//   need(buf, count [, host])   a buffer the call's kernels use whatever was asked for: reserved and recorded; with a host pointer it is also
//                               copied there at the end (a null one: it stays on the device);
//   result(buf, count, host)    an output only: a null host pointer means it was not asked for -- nothing reserved, checked or copied;
//   watch(buf, count)           a buffer another owner reserves (the search front end, the voxel front end): recorded, never reserved here.
// fits() reads every recorded buffer's p and cap again, so it also catches a buffer that another reserve replaced or another owner sized
// differently.  No heap: a fixed list, and one entry too many is refused (MI_ERR_STATE).
#pragma once
#include <cstring>

#include "devbuf.h"

namespace mislam {

struct CallBuffers {
    static constexpr int CAPACITY = 40;                  // the longest driver (pose_graph_api.hip) records 35
    struct Entry {
        const void* p;                                   // the DevBuf's own fields, read again by fits() and download(): &buf.p ...
        const size_t* cap;                               // ... and &buf.cap
        size_t count, elem_bytes;                        // what the call assumes, in elements
        void* host;                                      // null: stays on the device
    };
    Entry entries[CAPACITY];
    int used = 0;

    // recorded twice: the larger length holds, and a host pointer given later stands
    template <typename T>
    int watch(DevBuf<T>& b, size_t count, T* host = nullptr)
    {
        Entry* e = find(&b.p);
        if (!e) {
            if (used == CAPACITY) { set_error("internal: a call records more than %d device buffers", CAPACITY); return MI_ERR_STATE; }
            e = &entries[used++];
            *e = Entry{&b.p, &b.cap, 0, sizeof(T), nullptr};
        }
        if (count > e->count) e->count = count;
        if (host) e->host = host;
        return MI_OK;
    }
    template <typename T>
    int need(DevBuf<T>& b, size_t count, T* host = nullptr)
    {
        if (used == CAPACITY && !find(&b.p)) return watch(b, count, host);       // (the refusal, before anything is reserved)
        const int rc = b.reserve(count);
        return rc != MI_OK ? rc : watch(b, count, host);                          // (a failed reserve records nothing)
    }
    template <typename T>
    int result(DevBuf<T>& b, size_t count, T* host) { return host ? need(b, count, host) : MI_OK; }

    bool fits() const
    {
        for (int i = 0; i < used; i++)
            if (entries[i].count != 0 && (device(entries[i]) == nullptr || *entries[i].cap < entries[i].count)) return false;
        return true;
    }
    // the recorded copies, in the order their buffers were first recorded
    int download(hipStream_t s) const
    {
        for (int i = 0; i < used; i++) {
            const Entry& e = entries[i];
            if (e.host && e.count != 0) MI_HIP(hipMemcpyAsync(e.host, device(e), e.count * e.elem_bytes, hipMemcpyDeviceToHost, s));
        }
        return MI_OK;
    }

private:
    // the buffer's pointer as it is now: its bytes copied out (a T* is not read through a void* lvalue)
    static void* device(const Entry& e) { void* p; std::memcpy(&p, e.p, sizeof p); return p; }
    Entry* find(const void* p)
    {
        for (int i = 0; i < used; i++)
            if (entries[i].p == p) return &entries[i];
        return nullptr;
    }
};

}  // namespace mislam
