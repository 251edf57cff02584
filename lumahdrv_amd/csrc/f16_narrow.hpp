// f16_narrow.hpp -- float -> binary16 narrowing of the f16 frame outputs (k_decode<..., OUT16>, lumahip_f16_narrow_probe_device).
//
// The bits equal ExrInterface::floatToHalf (facade/exr_interface.cpp), which reproduces what the reference's lumadec writes into
// its EXR (Imf::Rgba halves): round to nearest even, binary16 denormals, overflow to +-inf, the sign of zero kept, and a NaN stays a
// NaN with the payload sign | 0x7e00 | (mantissa >> 13).  The conversion itself is the compiler's float -> _Float16 (one
// v_cvt_f16_f32 on gfx950, the compiler runtime's conversion on the host); only NaN is fixed up, by a class test and a select,
// because what the conversion does with a NaN payload is not specified.  A host compiler without _Float16 (g++ before 12) gets
// the same rounding in integer arithmetic instead.  tests/cpp/f16_narrow_check.cpp compiles this header with the host compilers
// and compares it with floatToHalf over all 2^32 float bit patterns; tests/test_gpu_f16_frames.py does the same for the device
// through lumahip_f16_narrow_probe_device.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_F16_HD __host__ __device__ __forceinline__
#else
#define LH_F16_HD inline
#endif

namespace lh {

LH_F16_HD uint16_t f16_narrow(float x)
{
    uint32_t b;
    memcpy(&b, &x, 4);
#if defined(__FLT16_MANT_DIG__) || defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)x;
    uint16_t r;
    memcpy(&r, &h, 2);
#else
    const uint32_t a = b & 0x7fffffffu;
    uint32_t r;
    if (a >= 0x47800000u) {                 // >= 65536 (and inf / NaN: fixed up below)
        r = 0x7c00u;
    } else if (a < 0x38800000u) {           // below 2^-14: a binary16 denormal or zero
        const int shift = 126 - (int)(a >> 23);   // 14 - (e - 112)
        if (shift > 24) {
            r = 0;
        } else {
            const uint32_t m = (a & 0x7fffffu) | 0x800000u;
            const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1), hw = 1u << (shift - 1);
            r = q + (rem > hw || (rem == hw && (q & 1)));
        }
    } else {
        r = ((a >> 13) - (112u << 10));
        const uint32_t rem = a & 0x1fffu;
        r += (rem > 0x1000u || (rem == 0x1000u && (r & 1)));   // may carry up to infinity
    }
    r |= (b >> 16) & 0x8000u;
#endif
    const uint16_t nan = (uint16_t)(((b >> 16) & 0x8000u) | 0x7e00u | ((b >> 13) & 0x3ffu));
    return __builtin_isnan(x) ? nan : (uint16_t)r;
}

}  // namespace lh
