// Output 0 of a FusionLayer (hrnet.py:166-229) in ONE launch, 32-channel branch 0 (bf16 and fp16 handles; written out for bf16 below):
//
//     out = relu(x0 + up(u1) + up(u2) [+ up(u3)]),   u_j = bf16(b_j + W_j x_j)   (1x1 conv + folded BN at the resolution of x_j)
//
// The plan used to run this as one conv_mfma launch per source (u_j to HBM) and upadd_kernel behind them.  Here a workgroup
// owns an 8 x 32 tile of the branch-0 map; the tile covers 4 x 16 pixels of x1, 2 x 8 of x2 and 1 x 4 of x3, so every u_j is
// computed ONCE per low-resolution pixel, kept in LDS as bf16, and broadcast by index shift in the sum -- nothing but x0, the
// sources and the output touch HBM.
//
// Bit-identical to the launches it replaces, by construction:
//   * the 1x1 terms run conv_mfma's arithmetic: accumulators start at bias + 0 (its no-residual prologue), the same
//     v_mfma_f32_32x32x16_bf16 with the same operand roles (A = 32 couts x 16 channels, B = 16 channels x 32 pixels; lane half h
//     holds channels 8h..8h+7 of a k-step), k-steps of 16 channels in ascending order, the same bf16 pack;
//   * the sum is upadd_kernel's: base first, then the sources in j order, in fp32, one rounding, ReLU.
#include "mfma_dev.h"

namespace {

constexpr int TH = 8, TW = 32, CO = 32;  // branch-0 tile, output channels

// One wave: u_J for 32 consecutive pixels (index 32 * COL ..) of the tile's J-shifted footprint, into LDS [pixel][32] bf16.
// x_J has 32 << J channels = (2 << J) k-steps.
template <typename E, int J, int COL>
__device__ __forceinline__ void source_tile(const FusionUpParams &p, int b, int oy0, int ox0, bf16_raw *lds_u, int lane)
{
    constexpr int FW = TW >> J, NPX = (TH >> J) * FW, NSTEP = 2 << J;
    const int r = lane & 31, h = lane >> 5;
    const int q = 32 * COL + r;  // pixel of the footprint
    const int Hj = p.H >> J, Wj = p.W >> J;
    const int gy = (oy0 >> J) + q / FW, gx = (ox0 >> J) + q % FW;
    const bool ok = q < NPX && gy < Hj && gx < Wj;
    // (a lane without a pixel reads its image's first one: valid memory, its result is never used)
    const bf16_raw *src = p.src[J - 1] + ((size_t)b * Hj * Wj + (ok ? (size_t)gy * Wj + gx : 0)) * p.src_cs[J - 1] + 8 * h;
    const u32x4 *w = reinterpret_cast<const u32x4 *>(p.w[J - 1]) + 32 * h + r;  // packed 1x1, KC = 32, COUT_T = 32: [cin/8][32][8]
    u32x4 fa[NSTEP], fb[NSTEP];
    static_for<NSTEP>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        fa[s] = w[64 * s];
        fb[s] = *reinterpret_cast<const u32x4 *>(src + 16 * s);
    });
    f32x16 acc;
    const float *bias = p.bias[J - 1];
    static_for<4>([&](auto gc) {  // acc[4g + k] <-> cout 8g + 4h + k (MFMA C layout)
        constexpr int g = decltype(gc)::value;
        const float4 bv = *reinterpret_cast<const float4 *>(bias + 8 * g + 4 * h);
        const float z = __builtin_bit_cast(float, 0u);  // conv_mfma: bias + (bf16 residual = +0)
        acc[4 * g + 0] = bv.x + z; acc[4 * g + 1] = bv.y + z; acc[4 * g + 2] = bv.z + z; acc[4 * g + 3] = bv.w + z;
    });
    static_for<NSTEP>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        acc = E::mfma(fa[s], fb[s], acc);
    });
    if (q < NPX) {
        unsigned *dst = reinterpret_cast<unsigned *>(lds_u + q * CO + 4 * h);
        const i16x2 nofloor = {(short)-32768, (short)-32768};  // conv_mfma's pack with the identity floor (the 1x1 terms have no ReLU)
        static_for<4>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            *reinterpret_cast<uint2 *>(dst + 4 * g) =
                make_uint2(E::pack(acc[4 * g + 0], acc[4 * g + 1], nofloor), E::pack(acc[4 * g + 2], acc[4 * g + 3], nofloor));
        });
    }
}

}  // namespace

// E: the element type (ElemBF16 / ElemF16 of mfma_dev.h)
template <typename E>
__global__ __launch_bounds__(256) void fusion_up_kernel(const FusionUpParams p)
{
    __shared__ __attribute__((aligned(16))) bf16_raw u1[(TH >> 1) * (TW >> 1) * CO];
    __shared__ __attribute__((aligned(16))) bf16_raw u2[(TH >> 2) * (TW >> 2) * CO];
    __shared__ __attribute__((aligned(16))) bf16_raw u3[(TH >> 3) * (TW >> 3) * CO];
    const int tid = threadIdx.x;
    if (p.clk && tid == 0 && blockIdx.x < 256) atomicMin(p.clk, wall_clock64());
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x; bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;

    // the base x0 of this thread's four 8-channel units, loaded ahead of the 1x1 work (unit = pixel * 4 + 8-channel group)
    u32x4 base[4];
    size_t opix[4];
    bool valid[4];
    static_for<4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int u = 256 * i + tid, px = u >> 2, c8 = u & 3;
        const int y = oy0 + px / TW, x = ox0 + px % TW;
        valid[i] = y < p.H && x < p.W;
        opix[i] = valid[i] ? ((size_t)b * p.H + y) * p.W + x : 0;
        base[i] = *reinterpret_cast<const u32x4 *>(p.x0 + opix[i] * p.x0_cs + c8 * 8);
    });

    // 1x1 terms: wave 0 / 1 = the two 32-pixel halves of x1's footprint, wave 2 = x2's, wave 3 = x3's (wave-uniform branches)
    const int wave = tid >> 6, lane = tid & 63;
    if (wave == 0) source_tile<E, 1, 0>(p, b, oy0, ox0, u1, lane);
    else if (wave == 1) source_tile<E, 1, 1>(p, b, oy0, ox0, u1, lane);
    else if (wave == 2) { if (p.nsrc >= 2) source_tile<E, 2, 0>(p, b, oy0, ox0, u2, lane); }
    else if (p.nsrc >= 3) source_tile<E, 3, 0>(p, b, oy0, ox0, u3, lane);
    __syncthreads();

    // upadd_kernel's sum: base, then the sources in j order, fp32, ReLU, one rounding
    static_for<4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int u = 256 * i + tid, px = u >> 2, c8 = u & 3;
        const int ly = px / TW, lx = px % TW;
        const u32x4 bv = base[i];
        float v[8] = {E::lo(bv[0]), E::hi(bv[0]), E::lo(bv[1]), E::hi(bv[1]),
                      E::lo(bv[2]), E::hi(bv[2]), E::lo(bv[3]), E::hi(bv[3])};
        auto add = [&](const bf16_raw *lds, int J) {
            const u32x4 uv = *reinterpret_cast<const u32x4 *>(lds + ((ly >> J) * (TW >> J) + (lx >> J)) * CO + c8 * 8);
            v[0] += E::lo(uv[0]); v[1] += E::hi(uv[0]); v[2] += E::lo(uv[1]); v[3] += E::hi(uv[1]);
            v[4] += E::lo(uv[2]); v[5] += E::hi(uv[2]); v[6] += E::lo(uv[3]); v[7] += E::hi(uv[3]);
        };
        add(u1, 1);
        if (p.nsrc >= 2) add(u2, 2);
        if (p.nsrc >= 3) add(u3, 3);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
        if (valid[i])
            *reinterpret_cast<u32x4 *>(p.out + opix[i] * p.out_cs + c8 * 8) =  // (upadd_kernel's pack)
                u32x4{E::round2(v[0], v[1]), E::round2(v[2], v[3]), E::round2(v[4], v[5]), E::round2(v[6], v[7])};
    });
    if (p.clk && tid == 0 && blockIdx.x + 256 >= gridDim.x) atomicMax(p.clk + 1, wall_clock64());
}

bool fusion_up_supported(int C, int nsrc) { return C == CO && nsrc >= 1 && nsrc <= 3; }

hipError_t fusion_up_launch(FusionUpParams p, hipStream_t s, int act_dtype)
{
    if (!fusion_up_supported(CO, p.nsrc) || (act_dtype != 0 && act_dtype != 1)) return hipErrorInvalidValue;
    p.tiles_x = (p.W + TW - 1) / TW;
    p.tiles_y = (p.H + TH - 1) / TH;
    const unsigned grid = (unsigned)p.B * p.tiles_y * p.tiles_x;
    if (act_dtype) HH_LAUNCH(fusion_up_kernel<ElemF16>, dim3(grid), dim3(256), 0, s, p);
    else HH_LAUNCH(fusion_up_kernel<ElemBF16>, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}
