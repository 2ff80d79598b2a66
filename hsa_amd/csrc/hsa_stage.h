// hsa_stage.h -- the host plumbing of a device stage of the 64-bit path (hsa_sa64.hip,
// hsa_refine.hip, hsa_choose.hip, hsa_sam.hip, hsa_reads.hip), stated once: the events
// around a stage's launches, its scratch layout, the scan's sizing call, the stream and
// grid rules, and the row -> read search of the kernels that run one lane per row.
// Included by hsa_internal.h (after HSA_HIP), whose hsa_index holds the timers.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

#define HSA_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)

// The events around the launches of a stage's last call, for its hsa_*_timing /
// hsa_*_launch_times pair: n + 1 events, created at the first timed call.
struct StageTimer {
    static constexpr int MAX_LAUNCHES = 8;
    const int n;                               // the stage's launches
    hipEvent_t ev[MAX_LAUNCHES + 1] = {};
    bool on = false;                           // the call in progress records
    bool timed = false;                        // the last call recorded every event
    explicit StageTimer(int launches) : n(launches) {}

    int begin(bool want)
    {
        timed = false;
        on = want;
        for (int i = 0; on && i <= n; ++i)
            if (!ev[i]) HSA_HIP(hipEventCreate(&ev[i]));
        return 0;
    }
    int mark(int i, hipStream_t st)
    {
        if (on) HSA_HIP(hipEventRecord(ev[i], st));
        return 0;
    }
    void end() { timed = on; }
    // ms[i]: launch i of the last call; what: "hsa_choose" for hsa_choose_launch_times
    int times(float *ms, const char *what)
    {
        if (!timed) { hsa_set_error("%s_launch_times: the last call was not timed (%s_timing)", what, what); return HSA_E_ARG; }
        HSA_HIP(hipEventSynchronize(ev[n]));
        for (int i = 0; i < n; ++i) HSA_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
        return 0;
    }
    void destroy()
    {
        for (hipEvent_t &e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
    }
};

// A stage's scratch layout, written once as a sequence of take() calls and run twice:
// on Carver() to measure what hsa_grow must hold, on Carver(base) to place the pointers.
// Every array starts on a 256-byte boundary; bytes() keeps 256 bytes of slack.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *b = nullptr) : base((char *)b) {}
    template <class T> T *take(size_t count)
    {
        T *p = base ? (T *)(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
    size_t bytes() const { return off + 256; }
};

// The temporary storage rocPRIM's exclusive scan of n items wants.
template <class T, class Op> static int hsa_scan_bytes(size_t &bytes, T init, size_t n, Op op, hipStream_t st)
{
    bytes = 0;
    HSA_HIP(rocprim::exclusive_scan(nullptr, bytes, (T *)nullptr, (T *)nullptr, init, n, op, st));
    return 0;
}

// A call's stream: the caller's, or the index's own.
static inline hipStream_t hsa_stage_stream(void *stream, hipStream_t own) { return stream ? (hipStream_t)stream : own; }

// Blocks of a kernel whose lane 0 always writes the counters: at least one.
static inline unsigned hsa_stage_blocks(uint64_t items, uint64_t per_block)
{
    return items ? (unsigned)((items + per_block - 1) / per_block) : 1u;
}

// Row t belongs to the last read j with pos_off[j] <= t (reads without rows share their
// successor's offset); pos_off[0] <= t < pos_off[n_jobs].
__device__ __forceinline__ uint32_t hsa_row_read(const uint64_t *pos_off, uint32_t n_jobs, uint64_t t)
{
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (pos_off[m] <= t) lo = m; else hi = m;
    }
    return lo;
}
