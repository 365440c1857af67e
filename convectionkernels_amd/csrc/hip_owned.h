// Move-only owners of what the host side of the C ABI allocates through the HIP runtime: a device buffer, a page-locked buffer,
// an event, a stream.  Each frees what it holds in its destructor, so a struct of them that is destroyed half-built frees what
// exists and nothing else.  No reference counts, no pools.  None of them synchronises: whoever lets go of a buffer, an event or
// a stream that the device may still use waits for that use first.
//
// The header takes hipError_t, hipSuccess, hipEvent_t, hipStream_t and the hip* calls below from the translation unit that
// includes it (after <hip/hip_runtime.h>, or after stand-ins: tests/hip_owned_harness.cpp) and includes nothing of the runtime.
#ifndef CVTTMI_HIP_OWNED_H
#define CVTTMI_HIP_OWNED_H

#include <stddef.h>

namespace cvtt_owned __attribute__((visibility("hidden")))
{
    struct DeviceMemory
    {
        static hipError_t allocate(void **p, size_t bytes) { return hipMalloc(p, bytes); }
        static void release(void *p) { (void)hipFree(p); }
    };
    struct PinnedMemory
    {
        static hipError_t allocate(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
        static void release(void *p) { (void)hipHostFree(p); }
    };

    template <class Memory>
    class Buffer
    {
        void *p_ = nullptr;
        size_t bytes_ = 0;

    public:
        Buffer() = default;
        Buffer(const Buffer &) = delete;
        Buffer &operator=(const Buffer &) = delete;
        Buffer(Buffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
        Buffer &operator=(Buffer &&o) noexcept
        {
            if (this != &o)
            {
                reset();
                p_ = o.p_, bytes_ = o.bytes_;
                o.p_ = nullptr, o.bytes_ = 0;
            }
            return *this;
        }
        ~Buffer() { reset(); }

        // At least `bytes`: grows (what it held is freed first, its contents are not kept) and never shrinks.  A failed
        // allocation leaves the owner empty.
        hipError_t reserve(size_t bytes)
        {
            if (p_ && bytes <= bytes_)
                return hipSuccess;
            reset();
            const hipError_t e = Memory::allocate(&p_, bytes);
            if (e != hipSuccess)
                p_ = nullptr;
            else
                bytes_ = bytes;
            return e;
        }
        void reset()
        {
            if (p_)
                Memory::release(p_);
            p_ = nullptr, bytes_ = 0;
        }
        void *get() const { return p_; }
        template <class T>
        T *as() const { return static_cast<T *>(p_); }
        size_t bytes() const { return bytes_; }
        explicit operator bool() const { return p_ != nullptr; }
    };
    typedef Buffer<DeviceMemory> DeviceBuffer;
    typedef Buffer<PinnedMemory> PinnedBuffer;

    class Event
    {
        hipEvent_t ev_ = nullptr;

    public:
        Event() = default;
        Event(const Event &) = delete;
        Event &operator=(const Event &) = delete;
        Event(Event &&o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
        Event &operator=(Event &&o) noexcept
        {
            if (this != &o)
            {
                reset();
                ev_ = o.ev_;
                o.ev_ = nullptr;
            }
            return *this;
        }
        ~Event() { reset(); }

        // created by the first call (at set-up, or lazily where the event is first needed); later calls keep it
        hipError_t create(unsigned flags)
        {
            if (ev_)
                return hipSuccess;
            const hipError_t e = hipEventCreateWithFlags(&ev_, flags);
            if (e != hipSuccess)
                ev_ = nullptr;
            return e;
        }
        void reset()
        {
            if (ev_)
                (void)hipEventDestroy(ev_);
            ev_ = nullptr;
        }
        hipEvent_t get() const { return ev_; }
        operator hipEvent_t() const { return ev_; }
    };

    class Stream
    {
        hipStream_t s_ = nullptr;

    public:
        Stream() = default;
        Stream(const Stream &) = delete;
        Stream &operator=(const Stream &) = delete;
        Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
        Stream &operator=(Stream &&o) noexcept
        {
            if (this != &o)
            {
                reset();
                s_ = o.s_;
                o.s_ = nullptr;
            }
            return *this;
        }
        ~Stream() { reset(); }

        hipError_t create()
        {
            if (s_)
                return hipSuccess;
            const hipError_t e = hipStreamCreate(&s_);
            if (e != hipSuccess)
                s_ = nullptr;
            return e;
        }
        void reset()
        {
            if (s_)
                (void)hipStreamDestroy(s_);
            s_ = nullptr;
        }
        hipStream_t get() const { return s_; }
        operator hipStream_t() const { return s_; }
    };
}

#endif
