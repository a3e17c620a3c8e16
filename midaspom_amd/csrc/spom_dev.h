// midaspom_amd/csrc/spom_dev.h -- what the five HIP units share of their host
// side: the check of a HIP call, the owning device buffer, the switch over a
// kernel template's width, and a handle's device, stream and timing events.
#ifndef SPOM_DEV_H
#define SPOM_DEV_H
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "mdp_internal.h"

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return mdp_set_error(MDP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                 __FILE__, __LINE__);                                        \
    } while (0)

// bytes held by every live DevBuf of the process (mdp_dev_live_bytes)
inline std::atomic<unsigned long long> g_dev_live_bytes{0};

// One device allocation and its capacity in elements; the destructor frees it.
// Move-only: a launch that takes its arguments by value (hipExtLaunchKernelGGL
// packs them into a tuple) cannot be handed a buffer by mistake, the sites
// pass get().
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { return swap(o), *this; }  // (o frees what this held)
    ~DevBuf() { reset(); }

    void swap(DevBuf &o) noexcept { std::swap(p_, o.p_), std::swap(cap_, o.cap_); }
    T *get() const { return p_; }
    size_t cap() const { return cap_; }  // elements
    bool empty() const { return !p_; }
    void reset()
    {
        if (!p_) return;
        (void)hipFree(p_);
        g_dev_live_bytes.fetch_sub(cap_ * sizeof(T), std::memory_order_relaxed);
        p_ = nullptr, cap_ = 0;
    }
    // grow-only: `need` elements (one at the least), kept while the allocation
    // holds them, reallocated -- the contents dropped -- when it does not.
    // After a failed hipMalloc (MDP_ENOMEM) the buffer is null and empty.
    int grow(size_t need)
    {
        if (p_ && need <= cap_) return MDP_OK;
        reset();
        if (need == 0) need = 1;
        const hipError_t e = hipMalloc((void **)&p_, need * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return mdp_set_error(MDP_ENOMEM, "hipMalloc(%zu bytes) failed: %s", need * sizeof(T), hipGetErrorString(e));
        }
        cap_ = need;
        g_dev_live_bytes.fetch_add(cap_ * sizeof(T), std::memory_order_relaxed);
        return MDP_OK;
    }
    // grow, then copy h[n] in
    int assign(const T *h, size_t n)
    {
        if (int rc = grow(n)) return rc;
        if (n) HIP_TRY(hipMemcpy(p_, h, n * sizeof(T), hipMemcpyHostToDevice));
        return MDP_OK;
    }
    int assign(const std::vector<T> &h) { return assign(h.data(), h.size()); }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// The stream rule of a handle (include/midaspom.h, "Streams"): a call gives the
// result it would give alone, whatever earlier device-form calls on the handle
// are still pending on any stream.  A device form launches on the caller's
// stream and returns; its kernels read -- and write -- device state the handle
// owns (the grid's axes and tables, scratch, the look-back flag) until that
// stream gets to them.  So:
//   * a device form ends with launched_on(st): a flag and the stream's handle,
//     no HIP call (no event per launch);
//   * a device form starts with settle_unless(st): work pending on the same
//     stream is ordered before it by the stream itself, on another stream it
//     is waited for;
//   * everything else that rewrites or reuses that state -- a new grid, the
//     host forms, the timing calls on the handle's own stream -- starts with
//     settle().
// settle() waits for the device, not for the noted stream: the caller may have
// destroyed that stream since, and a handle value may have been given out
// again.  The handle's device must be current.
struct DevPending {
    bool pending = false;
    hipStream_t pending_on = nullptr;
    void launched_on(hipStream_t st) { pending = true, pending_on = st; }
    // the host has waited for st: nothing noted there is pending any more
    void waited_for(hipStream_t st)
    {
        if (pending && pending_on == st) pending = false;
    }
    int settle()
    {
        if (!pending) return MDP_OK;
        HIP_TRY(hipDeviceSynchronize());
        pending = false;
        return MDP_OK;
    }
    int settle_unless(hipStream_t st) { return pending && pending_on != st ? settle() : MDP_OK; }
};

// The one switch over a kernel template's width: fn(integral_constant<int, W>)
// for the W that equals w, or the refusal `what` (a format of w) for any other.
// (A left fold: the kernels fn names are then emitted in ascending W, the
// order of a switch; a right fold reverses them in the code object.)
template <int... W, typename F>
int dev_for_width(uint32_t w, const char *what, F &&fn)
{
    int rc = MDP_OK;
    if ((... || (w == (uint32_t)W && ((rc = fn(std::integral_constant<int, W>())), true)))) return rc;
    return mdp_set_error(MDP_EINVAL, what, w);
}
// the lane kernels' padded patch count, and the patch pairs per lane of the
// wave kernels
template <typename F>
int dev_for_padded(uint32_t nm, F &&fn)
{
    return dev_for_width<8, 16, 32, 64>(nm, "internal: padded patch count %u", fn);
}
template <typename F>
int dev_for_pairs(uint32_t np, F &&fn)
{
    return dev_for_width<1, 2, 4, 8>(np, "internal: %u patch pairs per lane", fn);
}

// The device, stream and timing events of a handle, as the BASE of the struct
// that holds its DevBufs.  The release order is by declaration: the handle's
// destructor body calls drain() (the device current, pending device forms and
// the stream waited for), then its members go (the buffers), then this base
// (the events, the stream).  A handle makes its first HIP call in open(); one
// that never got there has nothing on the device, and drain() makes no HIP
// call for it.
struct DevQueue : DevPending {
    int device = 0;
    bool opened = false;  // open() made the device current once: HIP calls were made for this handle
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevQueue() = default;
    DevQueue(const DevQueue &) = delete;
    DevQueue &operator=(const DevQueue &) = delete;
    // Makes `device` current and creates what is missing of the non-blocking
    // stream and (events) the two timing events.  The first call refuses a
    // device that is not there (MDP_ENODEV); a call after a failed one takes
    // up where that one stopped.
    int open(bool events = true)
    {
        if (!opened) {
            int ndev = 0;
            if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
                return mdp_set_error(MDP_ENODEV, "no HIP device available");
            if (device < 0 || device >= ndev) return mdp_set_error(MDP_ENODEV, "device %d not present", device);
        }
        HIP_TRY(hipSetDevice(device));
        opened = true;
        if (!stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (events && !ev0) HIP_TRY(hipEventCreate(&ev0));
        if (events && !ev1) HIP_TRY(hipEventCreate(&ev1));
        return MDP_OK;
    }
    // the mean time in ms of `reps` runs of launch() on st, between the two
    // events; the warm-up is the caller's
    template <typename F>
    int time(hipStream_t st, int reps, double *ms, F &&launch)
    {
        HIP_TRY(hipEventRecord(ev0, st));
        for (int i = 0; i < reps; ++i)
            if (int rc = launch()) return rc;
        HIP_TRY(hipEventRecord(ev1, st));
        HIP_TRY(hipEventSynchronize(ev1));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, ev0, ev1));
        *ms = (double)t / reps;
        return MDP_OK;
    }
    void drain()
    {
        if (!opened) return;
        (void)hipSetDevice(device);
        (void)settle();
        if (stream) (void)hipStreamSynchronize(stream);
    }
    ~DevQueue()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#endif
