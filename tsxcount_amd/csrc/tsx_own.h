// tsx_own.h -- the owners of the host library's GPU resources (host-only C++17).
// Every device buffer, pinned buffer, event and stream the library creates lives in one of these four move-only
// types: empty by default, released by the destructor (errors ignored, as a `(void)hipFree` would).  Nothing else
// under csrc/ calls the create / destroy functions of the HIP runtime.  Sizes are BYTES throughout, as the call
// sites compute them.  A caller's stream is never owned.
#pragma once
#include "../../include/tsxcount_hip.h"

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>

namespace tsx {

// Sets the text of tsx_hip_last_error ("<what>: <HIP's message>") and returns ENOMEM for hipErrorOutOfMemory,
// else EHIP: what HIP_TRY does (tsxcount_hip.hip).
int own_fail(const char *what, hipError_t e);

// live owners of the process (tsx_hip_debug_counters, words 0-2): device buffers, pinned buffers, events + streams
inline std::atomic<long> g_live_dev{0}, g_live_pin{0}, g_live_sync{0};

template <typename T, bool PINNED>
class Buf {
    T *p_ = nullptr;
    size_t cap_ = 0;
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Buf() { reset(); }
    T *get() const { return p_; }
    size_t cap() const { return cap_; }   // bytes
    void reset() {
        if (p_) { (void)(PINNED ? hipHostFree(p_) : hipFree(p_)); --(PINNED ? g_live_pin : g_live_dev); }
        p_ = nullptr; cap_ = 0;
    }
    int alloc(size_t bytes) {   // exactly `bytes`; what was held is released first
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return own_fail(PINNED ? "hipHostMalloc" : "hipMalloc", e); }
        if (p_) { cap_ = bytes; ++(PINNED ? g_live_pin : g_live_dev); }
        return TSX_HIP_OK;
    }
    // Room for `need` bytes: nothing when they are there.  Else waits for *st when a buffer is held (st == nullptr: the
    // caller has waited already), frees it -- the owner is empty from here on -- and allocates `want` bytes.
    int reserve(const hipStream_t *st, size_t need, size_t want) {
        if (need <= cap_) return TSX_HIP_OK;
        if (p_ && st) {
            const hipError_t e = hipStreamSynchronize(*st);
            if (e != hipSuccess) return own_fail("hipStreamSynchronize", e);
        }
        return alloc(want);
    }
};
template <typename T> using DevBuf = Buf<T, false>;   // hipMalloc
template <typename T> using PinBuf = Buf<T, true>;    // hipHostMalloc(hipHostMallocDefault)

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~Event() { reset(); }
    hipEvent_t get() const { return e_; }
    void reset() { if (e_) { (void)hipEventDestroy(e_); --g_live_sync; } e_ = nullptr; }
    int create(unsigned flags = hipEventDisableTiming) {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) { e_ = nullptr; return own_fail("hipEventCreate", e); }
        ++g_live_sync;
        return TSX_HIP_OK;
    }
};

class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~Stream() { reset(); }
    hipStream_t get() const { return s_; }
    void reset() { if (s_) { (void)hipStreamDestroy(s_); --g_live_sync; } s_ = nullptr; }
    int create() {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) { s_ = nullptr; return own_fail("hipStreamCreate", e); }
        ++g_live_sync;
        return TSX_HIP_OK;
    }
};

// "Nothing queued may outlive the buffers": waits for the stream when the scope ends.  Declare it BEHIND the owners it
// guards, so that it runs before they release.
struct SyncAtExit {
    hipStream_t st;
    explicit SyncAtExit(hipStream_t s) : st(s) {}
    SyncAtExit(const SyncAtExit &) = delete;
    SyncAtExit &operator=(const SyncAtExit &) = delete;
    ~SyncAtExit() { (void)hipStreamSynchronize(st); }
};

}  // namespace tsx
