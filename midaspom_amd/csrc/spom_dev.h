// midaspom_amd/csrc/spom_dev.h -- what the four HIP units share of their host
// side: the check of a HIP call and the device buffers.
#ifndef SPOM_DEV_H
#define SPOM_DEV_H
#include <hip/hip_runtime.h>

#include <vector>

#include "mdp_internal.h"

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return mdp_set_error(MDP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                 __FILE__, __LINE__);                                        \
    } while (0)

// grow-only device buffer of `need` elements of `elem` bytes (one element at
// the least): kept while it holds them, reallocated -- its contents dropped
// -- when it does not.  After a failed hipMalloc (MDP_ENOMEM) the pointer is
// null and the capacity 0.
template <typename T>
int dev_grow(T *&p, size_t &cap, size_t need, size_t elem = sizeof(T))
{
    if (p && need <= cap) return MDP_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (need == 0) need = 1;
    const hipError_t e = hipMalloc((void **)&p, need * elem);
    if (e != hipSuccess) {
        p = nullptr;
        return mdp_set_error(MDP_ENOMEM, "hipMalloc(%zu bytes) failed: %s", need * elem, hipGetErrorString(e));
    }
    cap = need;
    return MDP_OK;
}

// a fresh device buffer holding h (what p pointed to is not freed)
template <typename T>
int dev_upload(T *&p, const std::vector<T> &h)
{
    size_t cap = 0;
    p = nullptr;
    if (int rc = dev_grow(p, cap, h.size())) return rc;
    if (!h.empty()) HIP_TRY(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return MDP_OK;
}

#endif
