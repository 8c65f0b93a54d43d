#pragma once
// mcq_cli_buffers.hpp -- what mcq_query_cli and mcq_query_mpi hold of the GPU, each behind a move-only owner whose destructor
// gives it back (so every way out of a function frees): pinned host memory, device memory, a stream, an event.
#include <cstdint>
#include <cstdio>
#include <utility>

#include <hip/hip_runtime_api.h>

// The HIP check of both programs: reports the call and the error under the program's prefix, then leaves as `on_fail` says --
// "FAIL" and `return false` / `return 1` in mcq_query_cli (MCQ_HIP), "ABORT" and MPI_Abort in mcq_query_mpi.
#define MCQ_HIP_AS(prefix, call, on_fail) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    std::fprintf(stderr, prefix ": %s: %s\n", #call, hipGetErrorString(e_)); on_fail; } } while (0)
#define MCQ_HIP(call, on_fail) MCQ_HIP_AS("FAIL", call, on_fail)

static inline hipError_t pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
static inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }

// cap elements of T at p.  grow(need) does not keep the contents: whoever still needs them moves the buffer aside first
// (`old = std::move(buf); buf.grow(need);`) and lets `old` live for as long as they are read.
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)> struct Buf {
    T* p = nullptr; uint64_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { if (p) (void)Free(p); }
    bool grow(uint64_t need) {
        if (cap >= need) return true;
        if (p) MCQ_HIP(Free(p), return false);
        p = nullptr; cap = 0;
        MCQ_HIP(Alloc((void**)&p, (need ? need : 1) * sizeof(T)), return false);
        cap = need;
        return true;
    }
};
template <class T> using PinnedBuf = Buf<T, pinned_alloc, hipHostFree>;
template <class T> using DeviceBuf = Buf<T, device_alloc, hipFree>;

template <class H, hipError_t (*Destroy)(H)> struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> { bool create() { MCQ_HIP(hipStreamCreateWithFlags(&h, hipStreamNonBlocking), return false); return true; } };
struct Event : Handle<hipEvent_t, hipEventDestroy> { bool create() { MCQ_HIP(hipEventCreateWithFlags(&h, hipEventDisableTiming), return false); return true; } };
