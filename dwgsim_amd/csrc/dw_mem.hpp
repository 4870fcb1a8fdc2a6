// dw_mem.hpp -- owners of device and page-locked host memory, events and streams for the host code (dw_host.cpp, dw_eval.cpp; no kernel includes it).
//
// DevMem / HostMem own one hipMalloc / hipHostMalloc allocation each: move-only, freed by the destructor.  reserve(need, want) keeps the
// allocation when it holds `need` bytes, else frees it and allocates `want` bytes -- every site keeps its own growth rule and exact sizes --
// and records the new capacity only once the allocation succeeded.  An allocation function may be passed (dw_host.cpp: dev_malloc, which
// retries when the device is out of memory).  DevEvent and DevStream own a hipEvent_t / hipStream_t the same way: create() makes the handle once, the
// destructor gives it back.  Destroying a stream does not wait for its work: whoever owns one synchronises it before the owner goes.  These are the
// only places in the host code that create or destroy an event or a stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dw {

template <class Kind> class Mem {
public:
    Mem() = default;
    Mem(const Mem &) = delete;
    Mem &operator=(const Mem &) = delete;
    Mem(Mem &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Mem &operator=(Mem &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Mem() { reset(); }

    template <class Alloc> hipError_t reserve(size_t need, size_t want, Alloc alloc)
    {
        if (need <= cap_) return hipSuccess;      // (need 0: nothing, not even a first allocation)
        reset();
        void *p = nullptr;
        const hipError_t e = alloc(&p, want);
        if (e != hipSuccess) return e;
        p_ = p; cap_ = want;
        return hipSuccess;
    }
    hipError_t reserve(size_t need, size_t want) { return reserve(need, want, Kind::alloc); }
    void reset()
    {
        if (p_) Kind::release(p_);
        p_ = nullptr; cap_ = 0;
    }

    template <class T = uint8_t> T *get() const { return static_cast<T *>(p_); }      // (bytes unless a type is given)
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};

struct DevKind {
    static hipError_t alloc(void **p, size_t n) { return hipMalloc(p, n); }
    static void release(void *p) { (void)hipFree(p); }
};
struct HostKind {
    static hipError_t alloc(void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static void release(void *p) { (void)hipHostFree(p); }
};
using DevMem = Mem<DevKind>;
using HostMem = Mem<HostKind>;

class DevEvent {
public:
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    DevEvent(DevEvent &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept
    {
        if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    ~DevEvent() { reset(); }

    hipError_t create() { return e_ ? hipSuccess : hipEventCreate(&e_); }      // (once: an event that exists is kept)
    void reset()
    {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }

private:
    hipEvent_t e_ = nullptr;
};

class DevStream {
public:
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    DevStream(DevStream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    DevStream &operator=(DevStream &&o) noexcept
    {
        if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; }
        return *this;
    }
    ~DevStream() { reset(); }

    hipError_t create() { return s_ ? hipSuccess : hipStreamCreate(&s_); }      // (once: a stream that exists is kept, whatever its priority)
    hipError_t create(int priority) { return s_ ? hipSuccess : hipStreamCreateWithPriority(&s_, hipStreamDefault, priority); }
    void reset()
    {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }

private:
    hipStream_t s_ = nullptr;
};

} // namespace dw
