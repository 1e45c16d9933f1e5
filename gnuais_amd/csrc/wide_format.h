// wide_format.h -- the sample formats of wideband input (include/gnuais_hip.h, GNUAIS_FMT_*): how one wide (I, Q) pair
// lies in memory and how it becomes the int16 pair of the channeliser's definition.  The one statement of each
// conversion: the kernels (wide_kernels.h) and the host's gnuais_convert_samples (wide_format.cpp) both call these.
// Plain C++ for host and device; no HIP needed to include it.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define WIDE_FMT_HD __host__ __device__ inline
#else
#define WIDE_FMT_HD inline
#endif

namespace gnuais {

// the values of GNUAIS_FMT_* (include/gnuais_hip.h)
constexpr int FMT_CS16 = 0, FMT_CU8 = 1, FMT_CS8 = 2, FMT_CF32 = 3;

// bytes of one (I, Q) pair, 0 for an unknown format
WIDE_FMT_HD int wide_format_bytes(int fmt)
{
    return fmt == FMT_CS16 ? 4 : fmt == FMT_CU8 || fmt == FMT_CS8 ? 2 : fmt == FMT_CF32 ? 8 : 0;
}
// the input pointer's alignment: the width of the pair for the 8- and 16-bit formats, of one component for cf32
WIDE_FMT_HD int wide_format_align(int fmt) { return fmt == FMT_CU8 || fmt == FMT_CS8 ? 2 : 4; }
WIDE_FMT_HD const char *wide_format_name(int fmt)
{
    return fmt == FMT_CS16 ? "cs16" : fmt == FMT_CU8 ? "cu8" : fmt == FMT_CS8 ? "cs8" : fmt == FMT_CF32 ? "cf32" : "?";
}

// A pair of 8-bit components, p = I | Q << 8 (the 16-bit word as it lies in memory, little-endian), to the channeliser's
// word (I lo, Q hi).  cs8: v = 256 s, each byte placed in the high half of its component.
// On the device the placement is one v_perm_b32: selector bytes 0x0c = zero, 0x00 / 0x01 = the pair's I / Q byte.
WIDE_FMT_HD uint32_t wide_word_cs8(uint32_t p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, p, 0x010c000cu);
#else
    return (p & 0xffu) << 8 | (p & 0xff00u) << 16;
#endif
}
// cu8: v = 256 u - 32640 = (u << 8) ^ 0x8080 on the 16-bit word: the same placement, then both components at once
WIDE_FMT_HD uint32_t wide_word_cu8(uint32_t p) { return wide_word_cs8(p) ^ 0x80808080u; }

// cf32: y = x * 32768 (one fp32 product), r = rint(y) ties to even, NaN -> 0, v = clamp(r, -32768, 32767) (+-inf too)
WIDE_FMT_HD int wide_int_cf32(float x)
{
    const float y = x * 32768.0f;
    float r = __builtin_rintf(y);
    r = r != r ? 0.0f : r;
    return (int) __builtin_fminf(__builtin_fmaxf(r, -32768.0f), 32767.0f);      // on the device: one v_med3_f32
}
WIDE_FMT_HD uint32_t wide_word_cf32(float i, float q)
{
    return (uint32_t) (uint16_t) wide_int_cf32(i) | (uint32_t) (uint16_t) wide_int_cf32(q) << 16;
}

} // namespace gnuais
