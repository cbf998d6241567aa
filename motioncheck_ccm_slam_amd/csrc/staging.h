// staging.h -- the per-call staging area of the host entry points that move their data in one block: a page-locked host block and
// its device twin `io` with the same layout, 64-byte segments, [ results | inputs ].  A call reserves the block, fills the inputs,
// uploads one range, launches on pointers into io, queues one download (or two ranges) and waits once.  An upload is asynchronous:
// the host block stays busy until the copy has run, which the next reserve() or wait() sees to.
#pragma once
#include "ccm_internal.h"

// The offset of the next segment of `bytes` in a layout that has reached `off`
static inline size_t seg(size_t& off, size_t bytes) { const size_t o = off; off += (bytes + 63) & ~(size_t)63; return o; }

struct Staging {
    DevBuf io;                                   // device twin
    uint8_t* block = nullptr; size_t cap = 0;    // page-locked, same layout as io
    bool pending = false;                        // an upload from `block` may still be queued
    // detached: entry points may return with an upload still queued (the setters of the frame handles and of the map-point table).
    // Every upload is then followed by an event, and the next reserve() waits for that copy alone.  Where every call ends in wait()
    // no event is recorded: only an error return leaves an upload pending, and the next reserve() waits for the whole stream.
    const bool detached; hipEvent_t host_free = nullptr;
    explicit Staging(bool detached_uploads) : detached(detached_uploads) {}

    // At least `bytes` in both blocks, the host one free to write (the last upload from it has completed).
    int reserve(ccm_ctx* c, size_t bytes)
    {
        if (detached && !host_free) CCM_HIP(c, hipEventCreateWithFlags(&host_free, hipEventDisableTiming));
        if (pending) { CCM_HIP(c, detached ? hipEventSynchronize(host_free) : hipStreamSynchronize(c->stream)); pending = false; }
        if (bytes > cap) {
            if (block) (void)hipHostFree(block);
            block = nullptr; cap = 0;
            const size_t want = bytes + bytes / 4 + 4096;
            if (hipHostMalloc((void**)&block, want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); block = nullptr;
                return ccm_fail(c, CCM_E_NOMEM, "page-locked staging of %zu bytes failed", want);
            }
            cap = want;
        }
        CCM_RESERVE(c, io, bytes);
        return CCM_OK;
    }
    // host [a, b) -> dst (default: io at the same offsets), asynchronous; the host block stays busy until the copy has run
    int upload(ccm_ctx* c, size_t a, size_t b, void* dst = nullptr)
    {
        if (b <= a) return CCM_OK;
        CCM_HIP(c, hipMemcpyAsync(dst ? dst : io.as<uint8_t>() + a, block + a, b - a, hipMemcpyHostToDevice, c->stream));
        if (detached) CCM_HIP(c, hipEventRecord(host_free, c->stream));
        pending = true;
        return CCM_OK;
    }
    // io [a, b) -> host [a, b), queued; wait() before reading it
    int download(ccm_ctx* c, size_t a, size_t b)
    {
        if (b <= a) return CCM_OK;
        CCM_HIP(c, hipMemcpyAsync(block + a, io.as<uint8_t>() + a, b - a, hipMemcpyDeviceToHost, c->stream));
        return CCM_OK;
    }
    // Everything queued on the context's stream has run: the downloads have landed and the host block is free
    int wait(ccm_ctx* c)
    {
        CCM_HIP(c, hipStreamSynchronize(c->stream));
        pending = false;
        return CCM_OK;
    }
    template <class T> T* host(size_t off) const { return reinterpret_cast<T*>(block + off); }
    template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(io.as<uint8_t>() + off); }
    // Copies into and out of the host block that do nothing for a null pointer or zero bytes (optional arrays of the C ABI)
    void put(size_t off, const void* src, size_t bytes) { if (src && bytes) std::memcpy(block + off, src, bytes); }
    void get(void* dst, size_t off, size_t bytes) const { if (dst && bytes) std::memcpy(dst, block + off, bytes); }
    void release()
    {
        if (block) (void)hipHostFree(block);
        if (host_free) (void)hipEventDestroy(host_free);
        block = nullptr; cap = 0; host_free = nullptr; pending = false;
        io.release();
    }
};
