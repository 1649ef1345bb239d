/*
 * rt_host.h -- the host-side plumbing that every unit but rt_capi.hip and rt_multi.hip shares, one copy per rule: how an error
 * is reported, the small address helpers, the body of a host-memory entry point, and what a unit that composes rt_capi.hip's
 * launches keeps in the handle.  It is a header of its own and not a part of rt_internal.h, because rt_internal.h is the contract
 * ACROSS object files and is included by rt_capi.hip as well, which owns the error text and so has a fail() and a HIP_TRY of
 * its own; everything here has internal linkage (each unit compiles its own copy, none of it is a symbol of the library) and
 * reaches rt_capi.hip only through rt_internal.h.
 */
#ifndef RT_HOST_H_
#define RT_HOST_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "rt_internal.h"

namespace {

inline int fail(int code, const std::string &msg) { return rt_internal_set_error(code, msg.c_str()); }

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorNoDevice ? RT_ERR_NO_DEVICE : RT_ERR_HIP,               \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

/* two buffers, both given, share a byte */
inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

/* ---- THE HOST-MEMORY ENTRY POINTS ---- */

/* a buffer of the caller's in host memory.  host == NULL: the buffer is absent -- nothing is allocated or copied for it, and the
 * launch sees a NULL device pointer.  pitch > 0 (an output): rows of row_bytes, pitch bytes apart in host memory and dense on
 * the device */
struct HostIn {
    const void *host;
    size_t bytes;
};
struct HostOut {
    void *host;
    size_t bytes, row_bytes = 0, pitch = 0;
};

struct StagedBuffers {       /* a staged call's allocations, freed on every way out */
    std::vector<void *> p;
    hipEvent_t start = nullptr, stop = nullptr;
    ~StagedBuffers() {
        if (start) (void)hipEventDestroy(start);
        if (stop) (void)hipEventDestroy(stop);
        for (void *q : p) (void)hipFree(q);
    }
};

/* The body of a host-memory entry point, its arguments checked: on `device`, device copies of the n_in inputs, room for the n_out
 * outputs and scratch_bytes of scratch; enqueue(d_in, d_out, d_scratch) -- int(void *const *, void *const *, void *) -- puts
 * the work on the null stream; the outputs come back, and *kernel_ms (if not NULL) is the time between two events that
 * bracket exactly what enqueue put there, never the copies. */
template <class Enqueue>
int staged_call(int device, const HostIn *in, int n_in, const HostOut *out, int n_out, size_t scratch_bytes, double *kernel_ms,
                Enqueue enqueue) {
    StagedBuffers d;
    d.p.assign((size_t)(n_in + n_out + 1), nullptr);
    void **d_in = d.p.data(), **d_out = d_in + n_in, **d_scratch = d_out + n_out;
    HIP_TRY(hipSetDevice(device));
    for (int k = 0; k < n_in; ++k)
        if (in[k].host) HIP_TRY(hipMalloc(&d_in[k], in[k].bytes));
    for (int k = 0; k < n_out; ++k)
        if (out[k].host) HIP_TRY(hipMalloc(&d_out[k], out[k].bytes));
    if (scratch_bytes) HIP_TRY(hipMalloc(d_scratch, scratch_bytes));
    HIP_TRY(hipEventCreate(&d.start));
    HIP_TRY(hipEventCreate(&d.stop));
    for (int k = 0; k < n_in; ++k)
        if (in[k].host) HIP_TRY(hipMemcpy(d_in[k], in[k].host, in[k].bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(d.start, nullptr));
    const int rc = enqueue(d_in, d_out, *d_scratch);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(d.stop, nullptr));
    HIP_TRY(hipEventSynchronize(d.stop));
    for (int k = 0; k < n_out; ++k) {
        const HostOut &o = out[k];
        if (!o.host) continue;
        if (o.pitch == 0 || o.pitch == o.row_bytes) {
            HIP_TRY(hipMemcpy(o.host, d_out[k], o.bytes, hipMemcpyDeviceToHost));
        } else {
            HIP_TRY(hipMemcpy2D(o.host, o.pitch, d_out[k], o.row_bytes, o.row_bytes, o.bytes / o.row_bytes, hipMemcpyDeviceToHost));
        }
    }
    if (kernel_ms) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, d.start, d.stop));
        *kernel_ms = ms;
    }
    return RT_OK;
}

/* ---- THE COMPOSING UNITS (rt_adaptive.hip, rt_lens.hip, rt_indirect.hip, rt_mirror.hip) ---- */

struct Unlock {              /* the handle's lock, given back on every way out */
    rt_scene *s;
    ~Unlock() { rt_internal_unlock(s); }
};

/* a piece of the handle's scratch: it only grows, and goes with the unit's state */
struct Buffer {
    void *p = nullptr;
    size_t bytes = 0;
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { if (p) (void)hipFree(p); }
    int grow(size_t need) { return rt_internal_grow(&p, &bytes, need); }
};

/* The events of a unit's last call: mark() records the call's next one, and the time between two consecutive ones is a stage's.
 * A call starts with n_events = 0 -- the events of the call before are recorded anew without being waited for: its stage times,
 * if nobody asked for them, are lost -- and ends with collected = false and seq = the handle's launch number; the unit reads
 * intervals() at most once a call (collected), and maps them to its rt_*_info itself. */
struct StageClock {
    std::vector<hipEvent_t> events;
    int n_events = 0;
    bool collected = true;
    uint64_t seq = 0;

    int mark(hipStream_t stream) {
        if ((size_t)n_events == events.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            events.push_back(e);
        }
        HIP_TRY(hipEventRecord(events[n_events], stream));
        n_events += 1;
        return RT_OK;
    }

    /* the n_events - 1 times, in ms, after one wait for the last event; the call is then collected */
    int intervals(std::vector<float> *ms) {
        ms->assign(n_events > 0 ? (size_t)(n_events - 1) : 0, 0.0f);
        if (n_events > 0) HIP_TRY(hipEventSynchronize(events[n_events - 1]));
        for (int i = 0; i + 1 < n_events; ++i) HIP_TRY(hipEventElapsedTime(&(*ms)[i], events[i], events[i + 1]));
        collected = true;
        return RT_OK;
    }

    void release() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        events.clear();
        n_events = 0;
    }
};

/* a unit's state in its place in the handle (RT_INTERNAL_UNIT_*), made on the unit's first call and registered with how
 * rt_scene_destroy frees it and what rt_get_timing reports of it (rt_internal.h) */
template <class State>
State *unit_state(rt_scene *s, int unit, void (*free_state)(void *), double (*stage_ms)(void *, uint64_t)) {
    rt_internal_unit *slot = rt_internal_unit_slot(s, unit);
    if (!slot->state) {
        slot->state = new State();
        slot->free_state = free_state;
        slot->stage_ms = stage_ms;
    }
    return static_cast<State *>(slot->state);
}

} // namespace

#endif /* RT_HOST_H_ */
