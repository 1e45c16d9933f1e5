// iq_common.h -- what iq_disc.hip and afc.hip share: the lane vectors of the [row][channel] layout and the phase formula of the complex-baseband definition (include/gnuais_hip.h, above gnuais_batch_run_iq)
// from ax = |re| onward: the discriminator (iq_disc.hip) enters it with the fp32 products of two pairs, the
// carrier-error estimate (afc.hip) with its window sums converted to fp32.  One text, so the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnuais {

// the fp32 constants of the definition, as bit patterns
__device__ __forceinline__ float f32_bits(uint32_t u) { return __uint_as_float(u); }

__device__ __forceinline__ int16_t iq_phase(float re, float im)
{
    const float A1 = f32_bits(0x3f7ff738u), A3 = f32_bits(0xbea91d04u), A5 = f32_bits(0x3e3876e2u),
                A7 = f32_bits(0xbdae5a36u), A9 = f32_bits(0x3caaae5fu);
    const float PI = f32_bits(0x40490fdbu), HALF_PI = f32_bits(0x3fc90fdbu), G = f32_bits(0x4622f983u);
    const float ax = fabsf(re), ay = fabsf(im);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = (mx == 0.0f) ? 0.0f : mn / mx;
    const float s = t * t;
    float p = t * (A1 + s * (A3 + s * (A5 + s * (A7 + s * A9))));
    if (ay > ax) p = HALF_PI - p;
    if (re < 0.0f) p = PI - p;                   // ordered compares: -0.0 is not < 0
    if (im < 0.0f) p = -p;
    const float o = fminf(fmaxf(rintf(p * G), -32768.0f), 32767.0f);
    return (int16_t) (int) o;
}

// A lane owns CPL adjacent channels: its load of one I/Q row and its store of one audio row
template <int CPL> struct Vec;
template <> struct Vec<1> { using In = uint32_t; using Out = int16_t; };
template <> struct Vec<2> { using In = uint2; using Out = uint32_t; };
template <> struct Vec<4> { using In = uint4; using Out = uint2; };

__device__ __forceinline__ void words(uint32_t v, uint32_t *w) { w[0] = v; }
__device__ __forceinline__ void words(uint2 v, uint32_t *w) { w[0] = v.x; w[1] = v.y; }
__device__ __forceinline__ void words(uint4 v, uint32_t *w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }

__device__ __forceinline__ uint32_t pack2(int16_t a, int16_t b)
{
    return (uint32_t) (uint16_t) a | ((uint32_t) (uint16_t) b << 16);
}

} // namespace gnuais
