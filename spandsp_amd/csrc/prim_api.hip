// prim_api.hip -- the inner primitives of the modem receivers as batched entry points of their own (include/spangpu.h:
// spangpu_vec_* / spangpu_cvec_* / spangpu_power_meter_*), SURVEY 8(a) rows a11, a12, a19.
//
// Inside the receiver kernels these run fused (quad_round_front.inc, v29_quad.hpp ...) and are proven through the receivers'
// bit-exact float state.  Here each is one launch over N independent items, one lane per item, with the reference's scalar
// order of operations (this file, like the rest of the library, is built -ffp-contract=off: every product and sum rounded by
// itself): the direct evidence that the arithmetic is the reference's, on inputs a receiver never produces -- denormals,
// cancellation, infinities.
//   vec_circular_dot_prodf   src/vector_float.c:890-900, 932-939      z = dot(x[pos:], y[:n-pos]) + dot(x[:pos], y[n-pos:])
//   vec_circular_lmsf        src/vector_float.c:982-1000 (leak 0.9999f, :942)
//   cvec_circular_dot_prodf  src/complex_vector_float.c:137-150, 187-196 (non-conjugating; the two parts added at the end)
//   cvec_circular_lmsf       src/complex_vector_float.c:201-219
//   power_meter_update       src/power_meter.c:65-70 (over a row of samples; the reading after the last one)
// Rows are item-major ([item][n]); x and y of an item may be the same for all items (stride 0).  Which strides a call takes and
// how many elements of an array it stages and copies back is prim_stage.hpp's rule, for this file and prim2_api.hip alike; the
// entry points hold no count of their own (prim_stage_hip.hpp: check, stage, finish).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#include "prim_stage_hip.hpp"

namespace {

__global__ void vec_circ_dot_kernel(const float *x, long long xs, const float *y, long long ys, const int32_t *pos, float *z, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float *xi = x + (size_t) i*xs;
    const float *yi = y + (size_t) i*ys;
    const int p = pos[i];
    if (p < 0  ||  p > n)
    {
        z[i] = __uint_as_float(0x7FC00000u);        // (a position outside the row: nothing is read; the result says so)
        return;
    }
    float a = 0.0f;
    for (int k = 0;  k < n - p;  k++)
        a += xi[p + k]*yi[k];
    float b = 0.0f;
    for (int k = 0;  k < p;  k++)
        b += xi[k]*yi[n - p + k];
    z[i] = a + b;
}

__global__ void vec_circ_lms_kernel(const float *x, long long xs, float *y, long long ys, const int32_t *pos, const float *err, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float *xi = x + (size_t) i*xs;
    float *yi = y + (size_t) i*ys;
    const int p = pos[i];
    if (p < 0  ||  p > n)
        return;                 // (a position outside the row: nothing is read or written for this item)
    const float e = err[i];
    for (int k = 0;  k < n - p;  k++)
        yi[k] = yi[k]*0.9999f + xi[p + k]*e;
    for (int k = 0;  k < p;  k++)
        yi[n - p + k] = yi[n - p + k]*0.9999f + xi[k]*e;
}

__global__ void cvec_circ_dot_kernel(const float2 *x, long long xs, const float2 *y, long long ys, const int32_t *pos, float2 *z, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float2 *xi = x + (size_t) i*xs;
    const float2 *yi = y + (size_t) i*ys;
    const int p = pos[i];
    if (p < 0  ||  p > n)
    {
        z[i] = make_float2(__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u));     // (nothing is read; the result says so)
        return;
    }
    float are = 0.0f;
    float aim = 0.0f;
    for (int k = 0;  k < n - p;  k++)
    {
        are += (xi[p + k].x*yi[k].x - xi[p + k].y*yi[k].y);
        aim += (xi[p + k].x*yi[k].y + xi[p + k].y*yi[k].x);
    }
    float bre = 0.0f;
    float bim = 0.0f;
    for (int k = 0;  k < p;  k++)
    {
        bre += (xi[k].x*yi[n - p + k].x - xi[k].y*yi[n - p + k].y);
        bim += (xi[k].x*yi[n - p + k].y + xi[k].y*yi[n - p + k].x);
    }
    z[i] = make_float2(are + bre, aim + bim);
}

__global__ void cvec_circ_lms_kernel(const float2 *x, long long xs, float2 *y, long long ys, const int32_t *pos, const float2 *err, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float2 *xi = x + (size_t) i*xs;
    float2 *yi = y + (size_t) i*ys;
    const int p = pos[i];
    if (p < 0  ||  p > n)
        return;                 // (a position outside the row: nothing is read or written for this item)
    const float2 e = err[i];
    for (int k = 0;  k < n;  k++)
    {
        const float2 xv = (k < n - p)  ?  xi[p + k]  :  xi[k - (n - p)];
        float2 yv = yi[k];
        yv.x = yv.x*0.9999f + (xv.y*e.y + xv.x*e.x);
        yv.y = yv.y*0.9999f + (xv.x*e.y - xv.y*e.x);
        yi[k] = yv;
    }
}

__global__ void power_meter_kernel(const int16_t *amp, long long stride, int32_t *reading, const int32_t *shift, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const int16_t *a = amp + (size_t) i*stride;
    int32_t r = reading[i];
    const int sh = shift[i] & 31;            // (what a 32-bit arithmetic shift does with its count on the reference's x86-64, too)
    for (int k = 0;  k < n;  k++)
        r += ((a[k]*a[k] - r) >> sh);
    reading[i] = r;
}

// godard_ted_rx(), godard.c:144-162: the two band edge filters over a row of samples (state and descriptor words: spangpu.h)
__global__ void godard_rx_kernel(uint32_t *state, const uint32_t *desc, long long ds, const float *samples, long long stride, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    uint32_t *st = state + (size_t) i*8;
    const uint32_t *d = desc + (size_t) i*ds;
    const float lc0 = __uint_as_float(d[0]), lc1 = __uint_as_float(d[1]);
    const float hc0 = __uint_as_float(d[3]), hc1 = __uint_as_float(d[4]);
    float l0 = __uint_as_float(st[0]), l1 = __uint_as_float(st[1]);
    float h0 = __uint_as_float(st[2]), h1 = __uint_as_float(st[3]);
    const float *x = samples + (size_t) i*stride;
    for (int k = 0;  k < n;  k++)
    {
        const float sample = x[k];
        float v = l0*lc0 + l1*lc1 + sample;
        l1 = l0;
        l0 = v;
        v = h0*hc0 + h1*hc1 + sample;
        h1 = h0;
        h0 = v;
    }
    st[0] = __float_as_uint(l0);
    st[1] = __float_as_uint(l1);
    st[2] = __float_as_uint(h0);
    st[3] = __float_as_uint(h1);
}

// godard_ted_per_baud(), godard.c:165-220
__global__ void godard_baud_kernel(uint32_t *state, const uint32_t *desc, long long ds, int32_t *correction, int items)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    uint32_t *st = state + (size_t) i*8;
    const uint32_t *d = desc + (size_t) i*ds;
    const float l0 = __uint_as_float(st[0]), l1 = __uint_as_float(st[1]);
    const float h0 = __uint_as_float(st[2]), h1 = __uint_as_float(st[3]);
    float v = l1*h0*__uint_as_float(d[2]) - l0*h1*__uint_as_float(d[5]) + l1*h1*__uint_as_float(d[6]);
    const float p = v - __uint_as_float(st[5]);
    st[5] = st[4];
    st[4] = __float_as_uint(v);
    const float phase = __uint_as_float(st[6]) - p;
    st[6] = __float_as_uint(phase);
    v = fabsf(phase);
    int corr = 0;
    if (v > __uint_as_float(d[8]))                          // fine_trigger
    {
        int step = (v > __uint_as_float(d[7]))  ?  (int32_t) d[9]  :  (int32_t) d[10];
        if (phase < 0.0f)
            step = -step;
        corr = step;
        st[7] = (uint32_t) ((int32_t) st[7] + step);
    }
    correction[i] = corr;
}

}   // namespace

using namespace spg;

extern "C" {

int spangpu_vec_circular_dot_prodf_batch(int device, const float *x, long long x_stride, const float *y, long long y_stride, const int32_t *pos,
                                         float *z, int items, int n, int mem)
{
    PrimCall call(mem);
    size_t ex, ey, ep, ez;
    int rc;
    if ((rc = call.args_ok(items, n, {x, y, pos, z})) < 0  ||  (rc = call.arg(kVecDotX, x_stride, items, n, &ex)) < 0
        ||  (rc = call.arg(kVecDotY, y_stride, items, n, &ey)) < 0  ||  (rc = call.arg(kVecDotPos, 0, items, n, &ep)) < 0
        ||  (rc = call.arg(kVecDotZ, 0, items, n, &ez)) < 0  ||  (rc = call.pos_ok(pos, items, n)) < 0  ||  (rc = call.ready(device)) < 0)
        return rc;
    float *dx, *dy, *dz;
    int32_t *dp;
    if ((rc = call.stage(kVecDotX, x, ex, &dx)) < 0  ||  (rc = call.stage(kVecDotY, y, ey, &dy)) < 0
        ||  (rc = call.stage(kVecDotPos, pos, ep, &dp)) < 0  ||  (rc = call.stage(kVecDotZ, (const float *) z, ez, &dz)) < 0)
        return rc;
    hipLaunchKernelGGL(vec_circ_dot_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dx, x_stride, dy, y_stride, dp, dz, items, n);
    return call.finish();
}

int spangpu_vec_circular_lmsf_batch(int device, const float *x, long long x_stride, float *y, long long y_stride, const int32_t *pos,
                                    const float *error, int items, int n, int mem)
{
    PrimCall call(mem);
    size_t ex, ey, ep, ee;
    int rc;
    if ((rc = call.args_ok(items, n, {x, y, pos, error})) < 0  ||  (rc = call.arg(kVecLmsX, x_stride, items, n, &ex)) < 0
        ||  (rc = call.arg(kVecLmsY, y_stride, items, n, &ey)) < 0  ||  (rc = call.arg(kVecLmsPos, 0, items, n, &ep)) < 0
        ||  (rc = call.arg(kVecLmsErr, 0, items, n, &ee)) < 0  ||  (rc = call.pos_ok(pos, items, n)) < 0  ||  (rc = call.ready(device)) < 0)
        return rc;
    float *dx, *dy, *de;
    int32_t *dp;
    if ((rc = call.stage(kVecLmsX, x, ex, &dx)) < 0  ||  (rc = call.stage(kVecLmsY, (const float *) y, ey, &dy)) < 0
        ||  (rc = call.stage(kVecLmsPos, pos, ep, &dp)) < 0  ||  (rc = call.stage(kVecLmsErr, error, ee, &de)) < 0)
        return rc;
    hipLaunchKernelGGL(vec_circ_lms_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dx, x_stride, dy, y_stride, dp, de, items, n);
    return call.finish();
}

// complex values as {re, im} float pairs (complexf_t); strides in complex elements
int spangpu_cvec_circular_dot_prodf_batch(int device, const float *x, long long x_stride, const float *y, long long y_stride, const int32_t *pos,
                                          float *z, int items, int n, int mem)
{
    PrimCall call(mem);
    size_t ex, ey, ep, ez;
    int rc;
    if ((rc = call.args_ok(items, n, {x, y, pos, z})) < 0  ||  (rc = call.arg(kCvecDotX, x_stride, items, n, &ex)) < 0
        ||  (rc = call.arg(kCvecDotY, y_stride, items, n, &ey)) < 0  ||  (rc = call.arg(kCvecDotPos, 0, items, n, &ep)) < 0
        ||  (rc = call.arg(kCvecDotZ, 0, items, n, &ez)) < 0  ||  (rc = call.pos_ok(pos, items, n)) < 0  ||  (rc = call.ready(device)) < 0)
        return rc;
    const float2 *cx = (const float2 *) x, *cy = (const float2 *) y;
    float2 *dx, *dy, *dz;
    int32_t *dp;
    if ((rc = call.stage(kCvecDotX, cx, ex, &dx)) < 0  ||  (rc = call.stage(kCvecDotY, cy, ey, &dy)) < 0
        ||  (rc = call.stage(kCvecDotPos, pos, ep, &dp)) < 0  ||  (rc = call.stage(kCvecDotZ, (const float2 *) z, ez, &dz)) < 0)
        return rc;
    hipLaunchKernelGGL(cvec_circ_dot_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dx, x_stride, dy, y_stride, dp, dz, items, n);
    return call.finish();
}

int spangpu_cvec_circular_lmsf_batch(int device, const float *x, long long x_stride, float *y, long long y_stride, const int32_t *pos,
                                     const float *error, int items, int n, int mem)
{
    PrimCall call(mem);
    size_t ex, ey, ep, ee;
    int rc;
    if ((rc = call.args_ok(items, n, {x, y, pos, error})) < 0  ||  (rc = call.arg(kCvecLmsX, x_stride, items, n, &ex)) < 0
        ||  (rc = call.arg(kCvecLmsY, y_stride, items, n, &ey)) < 0  ||  (rc = call.arg(kCvecLmsPos, 0, items, n, &ep)) < 0
        ||  (rc = call.arg(kCvecLmsErr, 0, items, n, &ee)) < 0  ||  (rc = call.pos_ok(pos, items, n)) < 0  ||  (rc = call.ready(device)) < 0)
        return rc;
    float2 *dx, *dy, *de;
    int32_t *dp;
    if ((rc = call.stage(kCvecLmsX, (const float2 *) x, ex, &dx)) < 0  ||  (rc = call.stage(kCvecLmsY, (const float2 *) y, ey, &dy)) < 0
        ||  (rc = call.stage(kCvecLmsPos, pos, ep, &dp)) < 0  ||  (rc = call.stage(kCvecLmsErr, (const float2 *) error, ee, &de)) < 0)
        return rc;
    hipLaunchKernelGGL(cvec_circ_lms_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dx, x_stride, dy, y_stride, dp, de, items, n);
    return call.finish();
}

// reading[i] after power_meter_update() over amp[i*stride .. + n) with shift[i], starting from reading[i]
int spangpu_power_meter_update_batch(int device, const int16_t *amp, long long stride, int32_t *reading, const int32_t *shift, int items, int n, int mem)
{
    PrimCall call(mem);
    size_t ea, er, es;
    int rc;
    if ((rc = call.args_ok(items, n, {amp, reading, shift})) < 0  ||  (rc = call.arg(kPowerAmp, stride, items, n, &ea)) < 0
        ||  (rc = call.arg(kPowerReading, 0, items, n, &er)) < 0  ||  (rc = call.arg(kPowerShift, 0, items, n, &es)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    int16_t *da;
    int32_t *dr, *ds;
    if ((rc = call.stage(kPowerAmp, amp, ea, &da)) < 0  ||  (rc = call.stage(kPowerReading, (const int32_t *) reading, er, &dr)) < 0
        ||  (rc = call.stage(kPowerShift, shift, es, &ds)) < 0)
        return rc;
    hipLaunchKernelGGL(power_meter_kernel, dim3((items + 63)/64), dim3(64), 0, 0, da, stride, dr, ds, items, n);
    return call.finish();
}

// items Godard timing error detectors, each over its row of n samples (godard_ted_rx() n times)
int spangpu_godard_ted_rx_batch(int device, uint32_t *state, const uint32_t *desc, long long desc_stride, const float *samples, long long stride,
                                int items, int n, int mem)
{
    PrimCall call(mem);
    size_t est, ed, ex;
    int rc;
    if ((rc = call.args_ok(items, n, {state, desc, samples})) < 0  ||  (rc = call.arg(kGodardRxState, 0, items, n, &est)) < 0
        ||  (rc = call.arg(kGodardRxDesc, desc_stride, items, n, &ed)) < 0  ||  (rc = call.arg(kGodardRxSamples, stride, items, n, &ex)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    uint32_t *dst, *dd;
    float *dx;
    if ((rc = call.stage(kGodardRxState, (const uint32_t *) state, est, &dst)) < 0  ||  (rc = call.stage(kGodardRxDesc, desc, ed, &dd)) < 0
        ||  (rc = call.stage(kGodardRxSamples, samples, ex, &dx)) < 0)
        return rc;
    hipLaunchKernelGGL(godard_rx_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dst, dd, desc_stride, dx, stride, items, n);
    return call.finish();
}

// godard_ted_per_baud() of every item: correction[i] = what the call returns (the step to add to eq_put_step)
int spangpu_godard_ted_per_baud_batch(int device, uint32_t *state, const uint32_t *desc, long long desc_stride, int32_t *correction, int items, int mem)
{
    PrimCall call(mem);
    size_t est, ed, ec;
    int rc;
    if ((rc = call.args_ok(items, 1, {state, desc, correction})) < 0  ||  (rc = call.arg(kGodardBaudState, 0, items, 1, &est)) < 0
        ||  (rc = call.arg(kGodardBaudDesc, desc_stride, items, 1, &ed)) < 0  ||  (rc = call.arg(kGodardBaudCorr, 0, items, 1, &ec)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    uint32_t *dst, *dd;
    int32_t *dc;
    if ((rc = call.stage(kGodardBaudState, (const uint32_t *) state, est, &dst)) < 0  ||  (rc = call.stage(kGodardBaudDesc, desc, ed, &dd)) < 0
        ||  (rc = call.stage(kGodardBaudCorr, (const int32_t *) correction, ec, &dc)) < 0)
        return rc;
    hipLaunchKernelGGL(godard_baud_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dst, dd, desc_stride, dc, items);
    return call.finish();
}

}   // extern "C"
