// Device-side idioms shared by the MFMA kernels (and, for the barrier and static_for, by the decode kernels): vector types, bf16 /
// fp8 packing, the compile-time loop, hand-pinned LDS reads, the LDS-only barrier.  One definition each; kernels.h stays the
// host <-> kernel launch interface.  Everything here is __forceinline__: a kernel's code is what it was with the helper written
// out in its own file (tools/isa_diff.py compares the assembly of two trees).  The host side of the two tile-form BasicBlock
// kernels (basicblock_fused.hip, basicblock_fused_c64.hip) is at the end.
#pragma once
#include "kernels.h"

#include <utility>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));  // fp16: the training path and HH_DTYPE_F16 inference handles
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // native vector: HIP's uint4 struct kept staging arrays in scratch
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef int i32x8 __attribute__((ext_vector_type(8)));  // the 32 k bytes of a lane's fp8 MFMA operand

namespace {

// Compile-time loop: indices are constant expressions in the front end, so per-thread staging arrays are
// promoted to registers (a "#pragma unroll" loop left them in scratch: guide rule 20).
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// ---- bf16 pairs in a dword
// Round a pair to bf16 and clamp it from below as signed 16-bit integers: floor = {0,0} is ReLU (every negative bf16,
// -0 included, is a negative int16; non-negative ones keep their bits), floor = {-32768,-32768} is the identity.
// One v_pk_max_i16 per pair instead of two canonicalise + two v_max_f32 on the fp32 values.
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b, i16x2 floor)
{
    f32x2 f = {a, b};
    const i16x2 v = __builtin_bit_cast(i16x2, __builtin_convertvector(f, bf16x2));
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(v, floor));
}
__device__ __forceinline__ unsigned pack_relu_bf16x2(float a, float b) { return pack_bf16x2(a, b, i16x2{0, 0}); }
// round and pack only (no v_pk_max_i16): upadd_kernel's pack
__device__ __forceinline__ unsigned round_bf16x2(float a, float b)
{
    f32x2 f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
__device__ __forceinline__ unsigned short f2bf_dev(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }

// ---- fp16 pairs in a dword (the second element type of the training path and of the inference engine)
// Semantics of every fp16 store of the training and inference kernels:
//   * round to nearest even (v_cvt_pk_f16_f32 / v_cvt_f16_f32);
//   * a value beyond +-65504 becomes +-inf, it is NOT saturated: the loss scaler detects an overflowing scale by it;
//   * NaN / inf pass through (an operand of an MFMA or of the fp32 arithmetic around it, they reach every sum they enter);
//   * subnormals are kept (the kernels are compiled in the default mode, which keeps fp16 subnormals).
// The int16 clamp works as for bf16: fp16 is sign-magnitude too, so every negative value (-0 included) is a negative int16.
__device__ __forceinline__ unsigned pack_f16x2(float a, float b, i16x2 floor)
{
    f32x2 f = {a, b};
    const i16x2 v = __builtin_bit_cast(i16x2, __builtin_convertvector(f, f16x2));
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(v, floor));
}
__device__ __forceinline__ unsigned round_f16x2(float a, float b)
{
    f32x2 f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, f16x2));
}
__device__ __forceinline__ float f16_lo(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu)); }
__device__ __forceinline__ float f16_hi(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }
__device__ __forceinline__ unsigned short f2h_dev(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }

// ---- fp8 (e4m3) path
// four fp32 -> four e4m3 bytes (round to nearest even), clamped to the finite range +-448 ...
__device__ __forceinline__ unsigned pack_fp8x4_sat(float a, float b, float c, float d)
{
    a = __builtin_amdgcn_fmed3f(a, -448.f, 448.f); b = __builtin_amdgcn_fmed3f(b, -448.f, 448.f);
    c = __builtin_amdgcn_fmed3f(c, -448.f, 448.f); d = __builtin_amdgcn_fmed3f(d, -448.f, 448.f);
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (unsigned)w;
}
// ... and clamped from above only.  Contract: inputs are ReLU outputs (>= 0); a value below -448 would not be clamped.
__device__ __forceinline__ unsigned pack_fp8x4_nonneg(float a, float b, float c, float d)
{
    a = fminf(a, 448.f); b = fminf(b, 448.f); c = fminf(c, 448.f); d = fminf(d, 448.f);
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (unsigned)w;
}
// the two 16-byte pieces of a lane's k-step as one MFMA operand
__device__ __forceinline__ i32x8 frag(const u32x4 &lo, const u32x4 &hi)
{
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// ---- LDS
// LDS fragment reads whose place in the instruction stream and whose wait are fixed by hand.  Left to the compiler, the
// reads of a software pipeline end up right in front of their MFMAs (it renames the rotating fragment registers and
// waits lgkmcnt(0)), which exposes a full LDS round trip per step.  The read is an asm statement (volatile: the statements keep
// their order); its result may only be used through lds_wait<N>(), which waits until at most N younger LDS operations are
// outstanding (LDS operations complete in order; compiler-issued ones in between only make the wait conservative).
template <int OFF>
__device__ __forceinline__ u32x4 lds_read_async(int addr)
{
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int N>
__device__ __forceinline__ void lds_wait(u32x4 &v)
{
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N));
}

// Workgroup barrier that waits for LDS traffic only.  __syncthreads() also drains vmcnt, i.e. it parks the wave until every
// global load it has in flight (the next tile's prefetch, issued to be consumed a phase later) has arrived and every global
// store it has issued is acknowledged by memory: a full round trip per barrier that no thread of the workgroup depends on.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace

// ---- the element type of a kernel as a compile-time parameter: the 16-bit storage format of the activations and of the
// packed weights, and the MFMA form that multiplies them.  Everything else of a kernel (tiling, staging, the fp32 accumulators,
// the int16 ReLU clamp, the transposing LDS reads) does not depend on it.  ElemBF16 is the code the kernels had written out.  (Outside the
// unnamed namespace: a kernel instantiated over these types keeps an ordinary external symbol.)
struct ElemBF16 {
    static constexpr unsigned ONE = 0x3f80u;  // 1.0
    static __device__ __forceinline__ unsigned pack(float a, float b, i16x2 floor) { return pack_bf16x2(a, b, floor); }
    static __device__ __forceinline__ unsigned round2(float a, float b) { return round_bf16x2(a, b); }
    static __device__ __forceinline__ float lo(unsigned u) { return bf16_lo(u); }
    static __device__ __forceinline__ float hi(unsigned u) { return bf16_hi(u); }
    static __device__ __forceinline__ unsigned short cvt(float f) { return f2bf_dev(f); }
    template <typename V>  // V: 16 bytes of eight elements (u32x4, or the i16x8 of the transposing reads)
    static __device__ __forceinline__ f32x16 mfma(const V &a, const V &b, const f32x16 &c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
struct ElemF16 {
    static constexpr unsigned ONE = 0x3c00u;  // 1.0
    static __device__ __forceinline__ unsigned pack(float a, float b, i16x2 floor) { return pack_f16x2(a, b, floor); }
    static __device__ __forceinline__ unsigned round2(float a, float b) { return round_f16x2(a, b); }
    static __device__ __forceinline__ float lo(unsigned u) { return f16_lo(u); }
    static __device__ __forceinline__ float hi(unsigned u) { return f16_hi(u); }
    static __device__ __forceinline__ unsigned short cvt(float f) { return f2h_dev(f); }
    template <typename V>
    static __device__ __forceinline__ f32x16 mfma(const V &a, const V &b, const f32x16 &c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

namespace {
// 32 couts of one pixel: lanes (r,0) hold couts 8g..8g+3, lanes (r,1) couts 8g+4..8g+7 in acc[4g..4g+3].
// Returns for m = 0,1 the 16 bytes (E elements, ReLU applied) of couts 16m+8h .. 16m+8h+7 of this lane's pixel.
template <typename E>
__device__ __forceinline__ void pack_rows16(const f32x16 &acc, u32x4 out[2])
{
    const i16x2 relu = {0, 0};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        unsigned x0 = E::pack(acc[8 * m + 0], acc[8 * m + 1], relu), x1 = E::pack(acc[8 * m + 2], acc[8 * m + 3], relu);
        unsigned y0 = E::pack(acc[8 * m + 4], acc[8 * m + 5], relu), y1 = E::pack(acc[8 * m + 6], acc[8 * m + 7], relu);
        // lanes 0-31: X = couts 16m..+3, Y = 16m+8..+11; lanes 32-63: X = 16m+4..+7, Y = 16m+12..+15.
        // swap X[32..63] <-> Y[0..31]: lanes 0-31 end with (X,Y) = couts 16m..16m+7, lanes 32-63 with 16m+8..16m+15
        auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
        auto s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
        out[m] = u32x4{s0[0], s1[0], s0[1], s1[1]};
    }
}

// Identity A fragments (rows = couts, k = cin) of lane (r, h): fragment kk has A[r][k] = 1 where 16*kk + k == r.  A residual added
// as two more MFMAs against them is exact (x * 1.0 in fp32).
template <typename E>
__device__ __forceinline__ void ident_frags(int r, int h, u32x4 ident[2])
{
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int j = r - 16 * kk - 8 * h;  // element index inside this lane's 8-wide k slice
        const unsigned one = (j & 1) ? E::ONE << 16 : E::ONE;  // E's 1.0 in the high / low half of a dword
        const bool on = j >= 0 && j < 8;
        ident[kk] = u32x4{on && (j >> 1) == 0 ? one : 0u, on && (j >> 1) == 1 ? one : 0u, on && (j >> 1) == 2 ? one : 0u,
                          on && (j >> 1) == 3 ? one : 0u};
    }
}
}  // namespace

// ---- host side of the tile-form BasicBlock kernels: one persistent workgroup per CU walks TH x TW output tiles
typedef void (*BBTileKernel)(const BBParams);
// per device: a 256-byte line every lane may scribble on (the stores of lanes outside the image; write-only garbage, so the
// kernels share it)
inline bf16_raw *g_bb_trash[64] = {};

inline hipError_t bb_tile_init(BBTileKernel kernel, size_t lds_bytes)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!g_bb_trash[dev & 63]) {
        e = hipMalloc((void **)&g_bb_trash[dev & 63], 256);
        if (e != hipSuccess) return e;
    }
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

inline hipError_t bb_tile_launch(BBTileKernel kernel, int th, int tw, int nthr, size_t lds_bytes, BBParams p, int num_cus, hipStream_t s)
{
    p.tiles_x = (p.W + tw - 1) / tw;
    p.tiles_y = (p.H + th - 1) / th;
    p.ntiles = p.B * p.tiles_x * p.tiles_y;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || !g_bb_trash[dev & 63]) return hipErrorNotInitialized;  // *_init() not called on this device
    p.trash = g_bb_trash[dev & 63];
    const int grid = p.ntiles < num_cus ? p.ntiles : num_cus;
    HH_LAUNCH(kernel, dim3(grid), dim3(nthr), lds_bytes, s, p);
    return hipGetLastError();
}
