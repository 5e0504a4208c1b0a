// prim_stage_hip.hpp -- the device side of prim_stage.hpp, the one copy prim_api.hip and prim2_api.hip share: a call checks
// its arguments (PrimCall::arg / args_ok / pos_ok, no HIP call: a bad call is SPANGPU_ERR_BAD_ARG with or without a GPU), then
// the device (ready), then brings each array to the device or passes a device pointer through (stage), launches, and hands
// back what it wrote (finish).  Every count -- allocation, copy in, copy back -- is the extent prim_stage.hpp's rule gave.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#include "prim_stage.hpp"

namespace spg
{

struct PrimCall
{
    int mem;
    void *owned[8];
    int n_owned = 0;
    struct Back
    {
        void *host;
        const void *dev;
        size_t bytes;
    } back[3];
    int n_back = 0;

    explicit PrimCall(int mem_kind) : mem(mem_kind) {}
    PrimCall(const PrimCall &) = delete;
    PrimCall &operator=(const PrimCall &) = delete;
    ~PrimCall()
    {
        for (int i = 0;  i < n_owned;  i++)
            (void) hipFree(owned[i]);
    }

    // items, the row length, the pointers, where the arrays live
    int args_ok(int items, int n, std::initializer_list<const void *> arrays) const
    {
        if (items <= 0  ||  n <= 0)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
        for (const void *p : arrays)
        {
            if (p == nullptr)
                return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad arguments");
        }
        return mem_kind_ok(mem);
    }

    // an argument's stride against the rule, and its extent in elements
    static int arg(const PrimArg &a, long long stride, int items, int n, size_t *extent)
    {
        if (prim_arg_extent(a, stride, items, n, extent))
            return SPANGPU_OK;
        if (a.use != kIn)
            return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "the rows of a written array cannot overlap: its stride is at least a row long");
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a stride is 0 (one row for all items) or at least a row long");
    }

    // positions in host memory are looked at before anything is staged
    int pos_ok(const int32_t *pos, int items, int n) const
    {
        if (mem != SPANGPU_MEM_HOST)
            return SPANGPU_OK;
        for (int i = 0;  i < items;  i++)
        {
            if (pos[i] < 0  ||  pos[i] > n)
                return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "a position outside its row (0 <= pos <= n)");
        }
        return SPANGPU_OK;
    }

    // after every argument check: is there a device at all
    static int ready(int device)
    {
        if (spangpu_device_count() <= 0)
            return spangpu_set_error(SPANGPU_ERR_NO_DEVICE, "no HIP device: libspangpu has no CPU fallback");
        SPG_TRY(hipSetDevice(device));
        return SPANGPU_OK;
    }

    // `extent` elements of a host array on the device (copied in unless the call only writes them; noted for finish() where
    // it writes them), or the caller's device pointer as it is
    template <typename T>
    int stage(const PrimArg &a, const T *src, size_t extent, T **dev)
    {
        if (mem == SPANGPU_MEM_DEVICE)
        {
            *dev = (T *) src;
            return SPANGPU_OK;
        }
        const size_t bytes = extent*a.elem;
        SPG_TRY(hipMalloc((void **) dev, bytes + 16));
        owned[n_owned++] = *dev;
        if (a.use != kOut  &&  bytes != 0)
            SPG_TRY(hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice));
        if (a.use != kIn)
        {
            back[n_back].host = (void *) src;
            back[n_back].dev = *dev;
            back[n_back++].bytes = bytes;
        }
        return SPANGPU_OK;
    }

    // after the launch: host arrays get what the call wrote (the copies wait for the kernel); with device arrays the call waits
    int finish()
    {
        SPG_TRY(hipGetLastError());
        if (mem == SPANGPU_MEM_DEVICE)
        {
            SPG_TRY(hipDeviceSynchronize());
            return SPANGPU_OK;
        }
        for (int i = 0;  i < n_back;  i++)
        {
            if (back[i].bytes != 0)
                SPG_TRY(hipMemcpy(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost));
        }
        return SPANGPU_OK;
    }
};

}   // namespace spg
