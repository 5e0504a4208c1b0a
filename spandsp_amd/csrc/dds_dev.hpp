// dds_dev.hpp -- the integer DDS's table look-up (src/dds_int.c of the reference), for every device unit that makes or
// correlates against a sine: the FSK receivers and senders, the connect tones, the signalling tones.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spg
{

// dds_lookup(), dds_int.c:340-355: one quadrant of a sine (257 int16 entries), mirrored and negated; phase >> 22 is the step
__device__ __forceinline__ int32_t dds_int_lookup(const int16_t *quarter, uint32_t phase)
{
    const uint32_t p = phase >> 22;
    uint32_t step = p & 255u;
    step = (p & 256u)  ?  (256u - step)  :  step;
    const int32_t amp = quarter[step];
    return (p & 512u)  ?  -amp  :  amp;
}

}   // namespace spg
