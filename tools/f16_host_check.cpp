// The host-side fp16 conversions of the engine (pytorch-human-pose_amd/csrc/f16_host.h: what hh_finalize packs the BN-folded weights of an
// HH_DTYPE_F16 handle with, its range check, and what hh_tap_read widens taps with) against the compiler's own _Float16 conversions,
// under the host sanitizers and without a GPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/f16_host_check.cpp -o /tmp/f16_host_check && /tmp/f16_host_check
//   (a compiler that has _Float16 on the host: clang, e.g. ROCm's; gcc from version 12)
//
// Checked: every one of the 65536 fp16 patterns widens to the float the compiler widens it to and narrows back to itself; 2^27 fp32
// patterns (every 32nd, plus all patterns around the rounding boundaries: the subnormal range, the ties at 2^-25 and 65520) narrow to
// the pattern the compiler narrows them to (round to nearest even, subnormals kept, +-inf beyond +-65504, NaN stays NaN); the range
// check flags exactly the infinities.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "f16_host.h"

static uint16_t ref_narrow(float f)
{
    const _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static float ref_widen(uint16_t u)
{
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}
static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static long long checked = 0;
static void narrow_one(uint32_t u)
{
    const float f = from_bits(u);
    const uint16_t got = hh_f32_to_f16(f), want = ref_narrow(f);
    ++checked;
    if (std::isnan(f) ? !((got & 0x7c00u) == 0x7c00u && (got & 0x3ffu) && (got & 0x8000u) == ((u >> 16) & 0x8000u)) : got != want) {
        printf("hh_f32_to_f16(%a = 0x%08x) = 0x%04x, the compiler gives 0x%04x\n", f, u, got, want);
        exit(1);
    }
}

int main()
{
    for (uint32_t h = 0; h < 65536; ++h) {
        const float got = hh_f16_to_f32((uint16_t)h), want = ref_widen((uint16_t)h);
        if (bits(got) != bits(want) && !(std::isnan(got) && std::isnan(want))) {
            printf("hh_f16_to_f32(0x%04x) = %a, the compiler gives %a\n", h, got, want);
            return 1;
        }
        if (!std::isnan(got) && hh_f32_to_f16(got) != (uint16_t)h) {
            printf("0x%04x does not survive the round trip: 0x%04x\n", h, hh_f32_to_f16(got));
            return 1;
        }
        const bool inf = (h & 0x7fffu) == 0x7c00u;
        if (hh_f16_is_inf((uint16_t)h) != inf) { printf("hh_f16_is_inf(0x%04x)\n", h); return 1; }
    }
    for (uint64_t u = 0; u < (1ull << 32); u += 32) narrow_one((uint32_t)u);
    // every pattern of both signs: below and around the smallest subnormal (2^-26 .. 2^-23), around 2^-14, and 65472 .. 65600
    const uint32_t ranges[][2] = {{0x32000000u, 0x34100000u}, {0x38700000u, 0x38900000u}, {0x477fc000u, 0x47802000u}, {0x7f7ffff0u, 0x7f800010u}};
    for (const auto &r : ranges)
        for (uint32_t u = r[0]; u < r[1]; ++u) { narrow_one(u); narrow_one(u | 0x80000000u); }
    // the statements of include/hhrnet.h
    if (hh_f32_to_f16(65504.f) != 0x7bffu || hh_f32_to_f16(65519.99f) != 0x7bffu || !hh_f16_is_inf(hh_f32_to_f16(65520.f)) ||
        !hh_f16_is_inf(hh_f32_to_f16(1e5f)) || hh_f32_to_f16(-1e5f) != 0xfc00u || hh_f32_to_f16(std::ldexp(1.f, -25)) != 0 ||
        hh_f32_to_f16(std::ldexp(1.0001f, -25)) != 1 || hh_f32_to_f16(std::ldexp(1.f, -24)) != 1 || hh_f32_to_f16(1.f) != 0x3c00u) {
        printf("a stated boundary value is wrong\n");
        return 1;
    }
    printf("f16_host_check ok: 65536 fp16 patterns, %lld fp32 patterns\n", checked);
    return 0;
}
