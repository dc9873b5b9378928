// device_stage.h -- what owns device memory for the length of one call on g.stream, for the point-cloud, the triangle-mesh and
// the volume units alike: Staged, the scratch of a work function and the device copies of a host form's arrays, with the one rule of
// when queueing stops, when the stream is waited for and which error is reported; read_back, a device value the host needs on the
// way; copy_out, the front of a compacted device array into the caller's; ProfCount, the 64-bit device words that a launch's lanes
// count into.  hipcc only.
#pragma once
#include "lib_internal.h"

#include <type_traits>
#include <vector>

// `bytes` of device memory into the host's, synchronised
inline hipError_t read_back(void* host, const void* dev, size_t bytes)
{
    hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    return e;
}

// the first `count` values of a device array into the caller's (nothing when either is null); queued, not waited for
template <class T>
hipError_t copy_out(T* host, const T* dev, size_t count)
{
    if (!host || !dev || !count) return hipSuccess;
    return hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, g.stream);
}

// The device buffers of one call on g.stream: scratch, buffers a handle adopts when the call succeeds, and the device copies of
// a host form's arrays.  Nothing more is allocated or queued after the first failure.  finish() copies the outputs back,
// synchronises -- always after a failure, so that nothing is freed under a queued kernel's feet -- frees what it owns, and
// reports: an SDFK_ERR_* of an allocation or of a step first, else the HIP error of the queueing, else that of the synchronise,
// as "<who>: <error string>".  After a finish() that returned SDFK_OK the object may be used for a further phase of the call.
class Staged {
    struct Buf { void* p; bool kept; };
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<Buf> bufs;
    std::vector<Out> outs;
    int r = SDFK_OK;
    hipError_t e = hipSuccess;

    void* alloc(size_t bytes, bool kept)
    {
        void* p = nullptr;
        if (ok()) r = dev_alloc(&p, bytes);
        if (p) bufs.push_back({p, kept});
        return p;
    }

public:
    Staged() = default;
    Staged(const Staged&) = delete;
    bool ok() const { return !r && e == hipSuccess; }
    template <class T>
    T* scratch(size_t count)
    {
        return (T*)alloc(count * sizeof(T), false);
    }
    template <class T>
    T* kept(size_t count)   // for the handle: freed by a finish() that fails, left to the caller by one that succeeds
    {
        return (T*)alloc(count * sizeof(T), true);
    }
    template <class T>
    T* in(const T* host, size_t count)   // (a null or empty array: null, nothing done)
    {
        T* d = host && count ? scratch<T>(count) : nullptr;
        if (d) e = hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, g.stream);
        return d;
    }
    template <class T>
    T* out(T* host, size_t count)   // (an output the caller left null: null, nothing done)
    {
        T* d = host ? scratch<T>(count) : nullptr;
        if (d) outs.push_back({host, d, count * sizeof(T)});
        return d;
    }
    template <class T>
    T* inout(T* host, size_t count)
    {
        T* d = in(host, count);
        if (d) outs.push_back({host, d, count * sizeof(T)});
        return d;
    }
    // One step, skipped once something has failed.  step() returns SDFK_OK or an SDFK_ERR_* (a launch function, a scan, a
    // refusal), or a hipError_t (a copy, a memset), or nothing: it launched kernels, and hipGetLastError is taken.
    template <class F>
    void run(F&& step)
    {
        if (!ok()) return;
        using R = decltype(step());
        if constexpr (std::is_void<R>::value) {
            step();
            e = hipGetLastError();
        } else if constexpr (std::is_same<R, hipError_t>::value) {
            e = step();
        } else {
            r = step();
        }
    }
    void read(void* host, const void* dev, size_t bytes)   // read_back as a step: synchronises
    {
        if (ok()) e = read_back(host, dev, bytes);
    }
    // wait = false: the end of a work function on device memory.  What it queued may still run; its scratch goes back to the
    // stream-ordered pool, and only a failure is waited for.
    int finish(const char* who, bool wait = true)
    {
        for (const Out& o : outs)
            if (ok()) e = hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, g.stream);
        const hipError_t es = wait || !ok() ? hipStreamSynchronize(g.stream) : hipSuccess;
        const bool failed = !ok() || es != hipSuccess;
        for (const Buf& b : bufs)
            if (!b.kept || failed) dev_free(b.p);
        bufs.clear();
        outs.clear();
        if (r) return r;
        if (failed) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
        return SDFK_OK;
    }
};

// The N 64-bit device words one launch counts into (with wave_add of device_wave.h), as steps of the call's Staged: begin() before
// the launch -- when `on`, scratch and its zeroing; otherwise dev stays null and the kernel counts nothing -- and end() after it,
// which reads the words back (synchronises).  Putting them on a handle is the caller's business.
template <int N>
struct ProfCount {
    unsigned long long* dev = nullptr;
    void begin(Staged& st, bool on = g.prof_on)
    {
        if (!on) return;
        dev = st.scratch<unsigned long long>(N);
        st.run([&] { return hipMemsetAsync(dev, 0, N * sizeof(unsigned long long), g.stream); });
    }
    bool end(Staged& st, unsigned long long (&host)[N])   // true: host[] holds the counts
    {
        if (!dev) return false;
        st.read(host, dev, sizeof host);
        return st.ok();
    }
};
