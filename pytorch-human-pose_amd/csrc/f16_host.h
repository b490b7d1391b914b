// Host-side fp16 (IEEE binary16) conversions of the engine: what hh_finalize packs the BN-folded weights of an HH_DTYPE_F16 handle with
// and what hh_tap_read widens its taps with.  Same semantics as the device's v_cvt_f16_f32 (mfma_dev.h, ElemF16): round to nearest
// even, subnormals kept (a value below 2^-14 loses bits, one below 2^-25 becomes zero), a value beyond +-65504 becomes +-inf.
// Plain C++ (no HIP): tools/f16_host_check.cpp builds it with the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

static inline uint16_t hh_f32_to_f16(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x3ffu));  // NaN stays NaN
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to inf (65504 + half an ulp), inf stays inf
    if (a < 0x33000000u) return sign;                         // < 2^-25: zero (2^-25 itself is a tie to even = zero, handled below)
    const int e = (int)(a >> 23) - 127;                       // unbiased exponent
    uint32_t m = (a & 0x7fffffu) | 0x800000u;                 // 24-bit significand
    int shift = 13;                                           // normal: keep 11 bits
    uint32_t base = (uint32_t)(e + 15) << 10;                 // exponent field, the significand's leading 1 is added on top of it
    if (e < -14) { shift = 13 + (-14 - e); base = 0; }        // subnormal: the leading 1 lands inside the mantissa field
    else base -= 0x400u;                                      // (the leading 1 of `m >> 13` carries into the exponent field)
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t h = base + q;
    if (rem > half || (rem == half && (q & 1u))) ++h;          // nearest even; a carry walks into the exponent, up to inf
    return (uint16_t)(sign | h);
}

static inline float hh_f16_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0x1fu) u = sign | 0x7f800000u | (m << 13);
    else if (e) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (!m) u = sign;
    else {  // subnormal: m * 2^-24
        int s = 0;
        uint32_t mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; ++s; }
        u = sign | ((uint32_t)(113 - s) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// an fp16 bit pattern that is +-inf: what a finite fp32 weight beyond the range rounds to
static inline bool hh_f16_is_inf(uint16_t h) { return (h & 0x7fffu) == 0x7c00u; }
