// swe2d_devmem.h - who owns ordinary device memory: one funnel, one owner type.  Host-only; it names hipError_t / hipSuccess and
// leaves their declaration to whoever includes it (the library: the HIP runtime; tests/devmem_main.cpp: a stand-in over malloc).
#pragma once
#include <cstddef>

// The only callers of hipMalloc / hipFree for ordinary device memory (defined once, swe2d_api.hip).  They count live bytes and
// live allocations process-wide (swe2d_debug_live_device_memory) and, in the SWE_RANGE_CHECK build, record every range.
int swe_dev_alloc(void **p, size_t bytes);              // a hipError_t as int; *p is null after a failure
void swe_dev_free(void *p);                             // null: nothing

// n elements of T on the device, freed with their owner.  Move-only: a struct that holds one is move-only too, and resetting a
// slot by assignment (s = Handle::Slide()) frees what the slot held.  Launch-argument structs are views, filled from get().
template <class T> class DevArray {
    T *p_ = nullptr;
    size_t n_ = 0;
public:
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    DevArray(DevArray &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevArray &operator=(DevArray &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevArray() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    size_t size() const { return n_; }                  // elements

    void reset() { swe_dev_free(p_); p_ = nullptr; n_ = 0; }
    // exactly n elements: keeps what it holds when that is n already, else frees it first; empty after a failure
    hipError_t alloc(size_t n)
    {
        if (p_ && n_ == n) return hipSuccess;
        reset();
        void *q = nullptr;
        const hipError_t e = (hipError_t)swe_dev_alloc(&q, n*sizeof(T));
        if (e == hipSuccess) { p_ = static_cast<T *>(q); n_ = n; }
        return e;
    }
    // n elements unless it holds some already (a buffer whose size never changes, allocated at first use)
    hipError_t ensure(size_t n) { return p_ ? hipSuccess : alloc(n); }
};
