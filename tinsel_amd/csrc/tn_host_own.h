// tn_host_own.h -- the owners of the host side: every device buffer, stream, event and page-locked registration has exactly one
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
//
// The only file that allocates or frees.  Each owner is a handle with a destructor, move-only; a destructor frees and never waits (what has
// to be waited for first is the caller's business, as before).  Failures are reported through fail() and an int, like HIP_TRY.  A resource of
// several parts is made in a local and moved into long-lived state when it is complete, so a failed call leaves no half-made one behind.
#pragma once

namespace {

// one hipMalloc; count() elements (an allocation of 0 elements is one element large, so that get() is never null after alloc)
template <class T>
struct DevBuf
{
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { DevBuf t(std::move(o)); swap(t); return *this; }
    ~DevBuf() { reset(); }

    int alloc(size_t count)
    {
        reset();
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(T)*(count ? count : 1)));
        p = (T*)d;
        n = count;
        return 0;
    }
    int grow(size_t count) { return p && n >= count ? 0 : alloc(count); }      // contents are not kept
    int upload(const T* host, size_t count)
    {
        if (alloc(count))
            return -1;
        if (count)
            HIP_TRY(hipMemcpy(p, host, sizeof(T)*count, hipMemcpyHostToDevice));
        return 0;
    }
    T* get() const { return p; }
    size_t count() const { return n; }
    explicit operator bool() const { return p != nullptr; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }

private:
    T* p = nullptr;
    size_t n = 0;
};

// many allocations of one lifetime, handed out as raw pointers (the kernel-facing records keep those): the scene's uploads, a batch's path
// state, one generation of device-built trees
struct DevPool
{
    DevPool() = default;
    DevPool(DevPool&& o) noexcept { allocs.swap(o.allocs); }
    DevPool& operator=(DevPool&& o) noexcept { DevPool t(std::move(o)); allocs.swap(t.allocs); return *this; }
    ~DevPool() { release(); }

    template <class T>
    int alloc(T** out, size_t count)
    {
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(T)*(count ? count : 1)));
        allocs.push_back(d);
        *out = (T*)d;
        return 0;
    }
    // nullptr: nothing to upload, or a failure (the caller names what could not be uploaded)
    template <class T>
    T* upload(const T* host, size_t count)
    {
        T* d = nullptr;
        if (count == 0 || alloc(&d, count) || hipMemcpy(d, host, sizeof(T)*count, hipMemcpyHostToDevice) != hipSuccess)
            return nullptr;
        return d;
    }
    void release()
    {
        for (void* p : allocs)
            (void)hipFree(p);
        allocs.clear();
    }

private:
    std::vector<void*> allocs;
};

template <class H, hipError_t (*Destroy)(H)>
struct DevHandle
{
    DevHandle() = default;
    DevHandle(DevHandle&& o) noexcept { std::swap(h, o.h); }
    DevHandle& operator=(DevHandle&& o) noexcept { DevHandle t(std::move(o)); std::swap(h, t.h); return *this; }
    ~DevHandle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }

protected:
    H h = nullptr;
};

// a non-blocking stream
struct Stream : DevHandle<hipStream_t, hipStreamDestroy>
{
    int create()
    {
        if (!h)
            HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
        return 0;
    }
};

// an event: for ordering (the default) or for timing
struct Event : DevHandle<hipEvent_t, hipEventDestroy>
{
    int create(bool timing = false)
    {
        if (!h)
            HIP_TRY(hipEventCreateWithFlags(&h, timing ? hipEventDefault : hipEventDisableTiming));
        return 0;
    }
};

// a code object loaded at run time (a baked instance, tn_host_bake.h); its functions live as long as it does
struct Module : DevHandle<hipModule_t, hipModuleUnload>
{
    int load(const void* image)
    {
        Module fresh;
        HIP_TRY(hipModuleLoadData(&fresh.h, image));
        std::swap(h, fresh.h);
        return 0;
    }
};

// The caller's output array page-locked in place for the read-back DMA (TINSEL_LOOKAHEAD_PIN_OUTPUT: the caller guarantees the array outlives
// the renderer or the next Init).  A registration must not outlive the memory it names, so it is dropped as soon as it is not asked for.
struct PinnedOutput
{
    PinnedOutput() = default;
    PinnedOutput(const PinnedOutput&) = delete;
    PinnedOutput& operator=(const PinnedOutput&) = delete;
    ~PinnedOutput() { release(nullptr); }

    // true: [p, p + bytes) is page-locked now.  A registration of something else is dropped (after the copies on `copies`); a refusal to
    // register is swallowed: the pageable copy is still correct.
    bool want(void* p, size_t bytes, bool pin, hipStream_t copies)
    {
        if (ptr && (!pin || ptr != p || size != bytes))
            release(copies);
        if (pin && !ptr)
        {
            if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess)
            {
                ptr = p;
                size = bytes;
            }
            else
                (void)hipGetLastError();
        }
        return ptr != nullptr;
    }
    bool held() const { return ptr != nullptr; }
    void release(hipStream_t copies)
    {
        if (!ptr)
            return;
        if (copies)
            (void)hipStreamSynchronize(copies);
        (void)hipHostUnregister(ptr);
        ptr = nullptr;
        size = 0;
    }

private:
    void* ptr = nullptr;
    size_t size = 0;
};

} // namespace
