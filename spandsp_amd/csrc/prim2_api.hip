// prim2_api.hip -- the rest of SURVEY 8(a)'s primitives as batched entry points of their own (round 6):
//   periodogram(), periodogram_prepare(), periodogram_apply(), periodogram_freq_error()     src/tone_detect.c:208-250, :299-312
//   fixed_sqrt32()                                          src/math_fixed.c:158-169 (table: make_math_fixed_tables.c)
//   dds_lookup_complexf(), dds_complexf() (= lookup + dds_advancef())                       src/dds_float.c:2135-2187
//   arctan2()                                               src/spandsp/arctan2.h:47-80
// The last three run inside the receiver kernels (quad_round_front.inc, v29_dev.hpp ...: the AGC's root of the signal power,
// the carrier's phasor, the decision's angle) and are proven there through the receivers' state words; here each is one
// launch over N independent items, one lane per item, on the same tables (modem_tables.c) and, for arctan2, the same device
// function (v29_common.hpp) -- the direct evidence, over their whole domains (tests/test_prim2_gpu.py).  The periodograms
// are not used by any receiver of the path; SURVEY section 2 lists them with the Goertzel core (tone_detect.h:202-249).
// Built -ffp-contract=off like the rest: every product and sum rounded by itself, in the reference's order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "../../include/spangpu.h"
#include "bank_host.hpp"
#include "prim_stage_hip.hpp"
#include "modem_tables.h"
#include "v29_common.hpp"

namespace {

// periodogram(), tone_detect.c:208-225: x += coeffs[i] "times" the folded pair, real and imaginary sums each in index order
__global__ void periodogram_kernel(const float2 *coeffs, long long cs, const float2 *amp, long long as, float2 *out, int items, int len)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float2 *c = coeffs + (size_t) i*cs;
    const float2 *a = amp + (size_t) i*as;
    float xre = 0.0f;
    float xim = 0.0f;
    for (int k = 0;  k < len/2;  k++)
    {
        const float2 p = a[k];
        const float2 q = a[len - 1 - k];
        const float sre = p.x + q.x, sim = p.y + q.y;
        const float dre = p.x - q.x, dim = p.y - q.y;
        xre += (c[k].x*sre - c[k].y*dim);
        xim += (c[k].x*sim + c[k].y*dre);
    }
    out[i] = make_float2(xre, xim);
}

// periodogram_prepare(), tone_detect.c:228-239
__global__ void periodogram_prepare_kernel(const float2 *amp, long long as, float2 *sum, float2 *diff, int items, int len)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float2 *a = amp + (size_t) i*as;
    float2 *s = sum + (size_t) i*(len/2);
    float2 *d = diff + (size_t) i*(len/2);
    for (int k = 0;  k < len/2;  k++)
    {
        const float2 p = a[k];
        const float2 q = a[len - 1 - k];
        s[k] = make_float2(p.x + q.x, p.y + q.y);
        d[k] = make_float2(p.x - q.x, p.y - q.y);
    }
}

// periodogram_apply(), tone_detect.c:242-255
__global__ void periodogram_apply_kernel(const float2 *coeffs, long long cs, const float2 *sum, const float2 *diff, float2 *out, int items, int len)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float2 *c = coeffs + (size_t) i*cs;
    const float2 *s = sum + (size_t) i*(len/2);
    const float2 *d = diff + (size_t) i*(len/2);
    float xre = 0.0f;
    float xim = 0.0f;
    for (int k = 0;  k < len/2;  k++)
    {
        xre += (c[k].x*s[k].x - c[k].y*d[k].y);
        xim += (c[k].x*s[k].y + c[k].y*d[k].x);
    }
    out[i] = make_float2(xre, xim);
}

// periodogram_freq_error(), tone_detect.c:299-310 (complex_mulf: re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re)
__global__ void periodogram_freq_error_kernel(float2 offset, float scale, const float2 *last, const float2 *now, float *out, int items)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    const float2 l = last[i];
    const float2 r = now[i];
    const float pre = l.x*offset.x - l.y*offset.y;
    const float pim = l.x*offset.y + l.y*offset.x;
    out[i] = scale*(r.y*pre - r.x*pim)/(r.x*r.x + r.y*r.y);
}

// fixed_sqrt32(), math_fixed.c:158-169, on the receivers' table (V29Tables::sqrt_tab, from spg_make_sqrt_table())
__global__ void fixed_sqrt32_kernel(const uint16_t *tab, const uint32_t *x, uint16_t *out, int items)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    uint32_t xx = x[i];
    uint16_t r = 0;
    if (xx != 0)
    {
        const int top = 31 - __builtin_clz(xx);
        const int shift = 30 - (top & ~1);
        xx <<= shift;
        r = (uint16_t) (tab[((xx >> 24) & 0xFF) - 64] >> (shift >> 1));
    }
    out[i] = r;
}

// dds_complexf(), dds_float.c:2179-2187, n times: the phasor of every step and the accumulator after the last one
// (n = 1, rate 0 is dds_lookup_complexf(); the accumulator moves as dds_advancef() moves it)
__global__ void dds_complexf_kernel(const float *sine, uint32_t *acc, const int32_t *rate, float2 *out, int items, int n)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    uint32_t a = acc[i];
    const uint32_t r = (uint32_t) rate[i];
    float2 *o = out + (size_t) i*n;
    for (int k = 0;  k < n;  k++)
    {
        o[k] = make_float2(sine[(uint32_t) (a + (1u << 30)) >> 21], sine[a >> 21]);
        a += r;
    }
    acc[i] = a;
}

__global__ void arctan2_kernel(const float *y, const float *x, int32_t *out, int items)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i >= items)
        return;
    out[i] = spg::v29_arctan2(y[i], x[i]);
}

// the receivers' sine and square root tables on a device, made once per device (host code: modem_tables.c)
constexpr int kMaxDevices = 16;
float *g_sine[kMaxDevices];
uint16_t *g_sqrt[kMaxDevices];
std::mutex g_tables_lock;

int tables(int device, const float **sine, const uint16_t **sq)
{
    if (device < 0  ||  device >= kMaxDevices)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "device out of range");
    std::lock_guard<std::mutex> guard(g_tables_lock);
    if (g_sine[device] == nullptr)
    {
        float s[SPG_SINE_LEN];
        uint16_t q[194];
        spg_make_sine_table(s);
        spg_make_sqrt_table(q);
        q[193] = 0;
        float *ds = nullptr;
        uint16_t *dq = nullptr;
        SPG_TRY(hipMalloc((void **) &ds, sizeof(s)));
        SPG_TRY(hipMalloc((void **) &dq, sizeof(q)));
        SPG_TRY(hipMemcpy(ds, s, sizeof(s), hipMemcpyHostToDevice));
        SPG_TRY(hipMemcpy(dq, q, sizeof(q), hipMemcpyHostToDevice));
        g_sine[device] = ds;
        g_sqrt[device] = dq;
    }
    *sine = g_sine[device];
    *sq = g_sqrt[device];
    return SPANGPU_OK;
}

}   // namespace

using namespace spg;

extern "C" {

// complex values as {re, im} float pairs (complexf_t); strides in complex elements, 0 = the same row for every item
// (len 1: a coefficient row of none, nothing of coeffs is read and the result is (0, 0), the reference's loop of no iterations)
int spangpu_periodogram_batch(int device, const float *coeffs, long long c_stride, const float *amp, long long a_stride, float *out,
                              int items, int len, int mem)
{
    PrimCall call(mem);
    size_t ec, ea, eo;
    int rc;
    if ((rc = call.args_ok(items, len, {coeffs, amp, out})) < 0  ||  (rc = call.arg(kPgramCoeffs, c_stride, items, len, &ec)) < 0
        ||  (rc = call.arg(kPgramAmp, a_stride, items, len, &ea)) < 0  ||  (rc = call.arg(kPgramOut, 0, items, len, &eo)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    float2 *dc, *da, *dout;
    if ((rc = call.stage(kPgramCoeffs, (const float2 *) coeffs, ec, &dc)) < 0  ||  (rc = call.stage(kPgramAmp, (const float2 *) amp, ea, &da)) < 0
        ||  (rc = call.stage(kPgramOut, (const float2 *) out, eo, &dout)) < 0)
        return rc;
    hipLaunchKernelGGL(periodogram_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dc, c_stride, da, a_stride, dout, items, len);
    return call.finish();
}

// sum and diff: [items][len/2] complex each
int spangpu_periodogram_prepare_batch(int device, const float *amp, long long a_stride, float *sum, float *diff, int items, int len, int mem)
{
    PrimCall call(mem);
    size_t ea, es, ed;
    int rc;
    if ((rc = call.args_ok(items, len, {amp, sum, diff})) < 0)
        return rc;
    if (len < 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad length");
    if ((rc = call.arg(kPrepAmp, a_stride, items, len, &ea)) < 0  ||  (rc = call.arg(kPrepSum, 0, items, len, &es)) < 0
        ||  (rc = call.arg(kPrepDiff, 0, items, len, &ed)) < 0  ||  (rc = call.ready(device)) < 0)
        return rc;
    float2 *da, *ds, *dd;
    if ((rc = call.stage(kPrepAmp, (const float2 *) amp, ea, &da)) < 0  ||  (rc = call.stage(kPrepSum, (const float2 *) sum, es, &ds)) < 0
        ||  (rc = call.stage(kPrepDiff, (const float2 *) diff, ed, &dd)) < 0)
        return rc;
    hipLaunchKernelGGL(periodogram_prepare_kernel, dim3((items + 63)/64), dim3(64), 0, 0, da, a_stride, ds, dd, items, len);
    if ((rc = call.finish()) < 0)
        return rc;
    return len/2;
}

int spangpu_periodogram_apply_batch(int device, const float *coeffs, long long c_stride, const float *sum, const float *diff, float *out,
                                    int items, int len, int mem)
{
    PrimCall call(mem);
    size_t ec, es, ed, eo;
    int rc;
    if ((rc = call.args_ok(items, len, {coeffs, sum, diff, out})) < 0)
        return rc;
    if (len < 2)
        return spangpu_set_error(SPANGPU_ERR_BAD_ARG, "bad length");
    if ((rc = call.arg(kApplyCoeffs, c_stride, items, len, &ec)) < 0  ||  (rc = call.arg(kApplySum, 0, items, len, &es)) < 0
        ||  (rc = call.arg(kApplyDiff, 0, items, len, &ed)) < 0  ||  (rc = call.arg(kApplyOut, 0, items, len, &eo)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    float2 *dc, *ds, *dd, *dout;
    if ((rc = call.stage(kApplyCoeffs, (const float2 *) coeffs, ec, &dc)) < 0  ||  (rc = call.stage(kApplySum, (const float2 *) sum, es, &ds)) < 0
        ||  (rc = call.stage(kApplyDiff, (const float2 *) diff, ed, &dd)) < 0  ||  (rc = call.stage(kApplyOut, (const float2 *) out, eo, &dout)) < 0)
        return rc;
    hipLaunchKernelGGL(periodogram_apply_kernel, dim3((items + 63)/64), dim3(64), 0, 0, dc, c_stride, ds, dd, dout, items, len);
    return call.finish();
}

// phase_offset: the {re, im} periodogram_generate_phase_offset() made (host memory, whatever mem says); last / result: [items] complex
int spangpu_periodogram_freq_error_batch(int device, const float *phase_offset, float scale, const float *last_result, const float *result,
                                         float *out, int items, int mem)
{
    PrimCall call(mem);
    size_t el, er, eo;
    int rc;
    if ((rc = call.args_ok(items, 1, {phase_offset, last_result, result, out})) < 0  ||  (rc = call.arg(kFreqErrLast, 0, items, 1, &el)) < 0
        ||  (rc = call.arg(kFreqErrNow, 0, items, 1, &er)) < 0  ||  (rc = call.arg(kFreqErrOut, 0, items, 1, &eo)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    float2 *dl, *dr;
    float *dout;
    if ((rc = call.stage(kFreqErrLast, (const float2 *) last_result, el, &dl)) < 0  ||  (rc = call.stage(kFreqErrNow, (const float2 *) result, er, &dr)) < 0
        ||  (rc = call.stage(kFreqErrOut, (const float *) out, eo, &dout)) < 0)
        return rc;
    hipLaunchKernelGGL(periodogram_freq_error_kernel, dim3((items + 63)/64), dim3(64), 0, 0, make_float2(phase_offset[0], phase_offset[1]), scale,
                       dl, dr, dout, items);
    return call.finish();
}

int spangpu_fixed_sqrt32_batch(int device, const uint32_t *x, uint16_t *out, int items, int mem)
{
    PrimCall call(mem);
    size_t ex, eo;
    int rc;
    if ((rc = call.args_ok(items, 1, {x, out})) < 0  ||  (rc = call.arg(kSqrtX, 0, items, 1, &ex)) < 0
        ||  (rc = call.arg(kSqrtOut, 0, items, 1, &eo)) < 0  ||  (rc = call.ready(device)) < 0)
        return rc;
    const float *sine;
    const uint16_t *sq;
    if ((rc = tables(device, &sine, &sq)) < 0)
        return rc;
    uint32_t *dx;
    uint16_t *dout;
    if ((rc = call.stage(kSqrtX, x, ex, &dx)) < 0  ||  (rc = call.stage(kSqrtOut, (const uint16_t *) out, eo, &dout)) < 0)
        return rc;
    hipLaunchKernelGGL(fixed_sqrt32_kernel, dim3((items + 255)/256), dim3(256), 0, 0, sq, dx, dout, items);
    return call.finish();
}

// out: [items][n] complex; phase_acc[items] is advanced n times by phase_rate[items]
int spangpu_dds_complexf_batch(int device, uint32_t *phase_acc, const int32_t *phase_rate, float *out, int items, int n, int mem)
{
    PrimCall call(mem);
    size_t ea, er, eo;
    int rc;
    if ((rc = call.args_ok(items, n, {phase_acc, phase_rate, out})) < 0  ||  (rc = call.arg(kDdsAcc, 0, items, n, &ea)) < 0
        ||  (rc = call.arg(kDdsRate, 0, items, n, &er)) < 0  ||  (rc = call.arg(kDdsOut, 0, items, n, &eo)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    const float *sine;
    const uint16_t *sq;
    if ((rc = tables(device, &sine, &sq)) < 0)
        return rc;
    uint32_t *da;
    int32_t *dr;
    float2 *dout;
    if ((rc = call.stage(kDdsAcc, (const uint32_t *) phase_acc, ea, &da)) < 0  ||  (rc = call.stage(kDdsRate, phase_rate, er, &dr)) < 0
        ||  (rc = call.stage(kDdsOut, (const float2 *) out, eo, &dout)) < 0)
        return rc;
    hipLaunchKernelGGL(dds_complexf_kernel, dim3((items + 63)/64), dim3(64), 0, 0, sine, da, dr, dout, items, n);
    return call.finish();
}

int spangpu_arctan2_batch(int device, const float *y, const float *x, int32_t *out, int items, int mem)
{
    PrimCall call(mem);
    size_t ey, ex, eo;
    int rc;
    if ((rc = call.args_ok(items, 1, {y, x, out})) < 0  ||  (rc = call.arg(kAtanY, 0, items, 1, &ey)) < 0
        ||  (rc = call.arg(kAtanX, 0, items, 1, &ex)) < 0  ||  (rc = call.arg(kAtanOut, 0, items, 1, &eo)) < 0
        ||  (rc = call.ready(device)) < 0)
        return rc;
    float *dy, *dx;
    int32_t *dout;
    if ((rc = call.stage(kAtanY, y, ey, &dy)) < 0  ||  (rc = call.stage(kAtanX, x, ex, &dx)) < 0
        ||  (rc = call.stage(kAtanOut, (const int32_t *) out, eo, &dout)) < 0)
        return rc;
    hipLaunchKernelGGL(arctan2_kernel, dim3((items + 255)/256), dim3(256), 0, 0, dy, dx, dout, items);
    return call.finish();
}

}   // extern "C"
