// points_set.h -- the handle behind sdfk_points_* (KdTree): the static points and their search grid, built by lib_points.hip and
// read by every query of the family (lib_points.hip, lib_points_knn.hip, lib_pointcloud.hip, lib_orient.hip, lib_points_filter.hip) through the walk of
// points_walk.h; and what owns the copies between host and device on g.stream: Staged, the device copies of the arrays of a query's
// host form, and read_back, a device value the host needs on the way.
#pragma once
#include "lib_internal.h"
#include "points_grid.h"

#include <vector>

struct sdfk_points {
    DeviceState* owner = &cur_state();
    int64_t n = 0;
    float* xyz = nullptr;          // n x 3, insertion order (the source of every rebuild)
    float4* sorted = nullptr;      // n, cell order: (x, y, z, bits(index))
    uint32_t* starts = nullptr;    // cells + 1
    int64_t cells = 0;
    sdfk_points_grid::Grid G{};
    float first[3] = {0, 0, 0};
    int64_t last_candidates = 0, last_queries = 0;   // of the last profiled query call, whichever kind
};

// `bytes` of device memory into the host's, synchronised
inline hipError_t read_back(void* host, const void* dev, size_t bytes)
{
    hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    return e;
}

// The device copies of a host form's arrays on g.stream.  Nothing more is queued after the first failure; finish() copies the
// outputs back, synchronises -- on failure too -- before any buffer is freed, and reports: an SDFK_ERR_* of an allocation or of
// the launch function first, else the HIP error of the queueing, else that of the synchronise, as "<who>: <error string>".
class Staged {
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<void*> bufs;
    std::vector<Out> outs;
    int r = SDFK_OK;
    hipError_t e = hipSuccess;
    bool ok() const { return !r && e == hipSuccess; }

public:
    Staged() = default;
    Staged(const Staged&) = delete;
    template <class T>
    T* scratch(size_t count)
    {
        void* p = nullptr;
        if (ok()) r = dev_alloc(&p, count * sizeof(T));
        if (p) bufs.push_back(p);
        return (T*)p;
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
    template <class F>
    void run(F&& launch)   // launch() queues the work and returns SDFK_OK or an SDFK_ERR_*
    {
        if (ok()) r = launch();
    }
    int finish(const char* who)
    {
        for (const Out& o : outs)
            if (ok()) e = hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, g.stream);
        const hipError_t es = hipStreamSynchronize(g.stream);
        for (void* p : bufs) dev_free(p);
        bufs.clear();
        outs.clear();
        if (r) return r;
        if (e != hipSuccess || es != hipSuccess) return fail(SDFK_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
        return SDFK_OK;
    }
};
