// The whole stem in one kernel (/root/reference/src/keypoints/architectures/hrnet.py:354-358,378-384):
//   conv3x3 s2 (3 -> 64) + BN + ReLU  ->  conv3x3 s2 (64 -> 64) + BN + ReLU,   fp32 NCHW images in, bf16 NHWC at 1/4 resolution out.
// Why: run as two launches the 64-channel half-resolution intermediate (268 MB at B = 32, 512x512) is written by stem_conv.hip
// (105 us, HBM-bound) and read back by a stride-2 conv_mfma launch (119 us); fused it lives in LDS and the stem moves 100 MB in
// and 67 MB out.
//
// One workgroup (512 threads, persistent over tiles) = a 2 x 32 tile of the final map at a time, in two wave groups that work one
// tile apart, as in basicblock_fused_pc.hip: ONE workgroup barrier per tile, patch and intermediate tile double buffered (120 KB).
//   waves 0-3 (producers), iteration i:
//     patch   the (4*2+3) rows x 136 columns x 3 planes of tile i+1 as 34 aligned float4 per row (kernels.h: stem_unit; columns
//             4 ox0 - 4 .. 4 ox0 + 131, W % 4 == 0 so a vector is wholly inside or wholly outside the image, outside the buffer load
//             returns 0 = conv1's padding): loads issued first, converted and written (4 elements per ds_write_b64) last;
//     conv1   of tile i: the 5 x 65 intermediate pixels the tile needs, flattened into 11 column tiles of 32 lanes (3, 3, 3, 2 per
//             wave); each lane gathers its pixel's 27 taps (K padded to 32 = two k-steps; the padded taps read a zero region behind
//             the patch that every pixel's base offset stays inside) as in stem_conv.hip; BN shift + ReLU, 16-bit, into LDS in two
//             column-parity planes (even / odd intermediate columns) so that conv2's stride-2 reads (column 2r + kx for lane r) touch
//             consecutive pixels of one plane: conflict-free ds_read_b128.  Intermediate pixels outside the half-resolution image
//             are conv2's zero padding;
//   waves 4-7 (consumers), iteration i:
//     conv2   of tile i-1: wave 4 + w = (output row w >> 1, 32-cout tile w & 1): 36 k-steps into one accumulator, its 36 weight
//             fragments stay in 144 VGPRs for the life of the workgroup (no weight reads), pixel fragments by hand-pinned asm reads
//             three steps ahead; ReLU, 16-byte stores.
// No wave holds both the conv2 weights and the staging / gather registers, so the kernel fits two waves per SIMD; the producer's
// gathers, packs and LDS writes run beside the MFMAs of the consumer on its SIMD (waves w and w + 4).
// The arithmetic is that of the one-group form this replaces, operand for operand: the outputs are bit-identical
// (tests/test_gpu_stem_pc.py against tests/golden/stem_bits.npz, recorded from that form).
#include "mfma_dev.h"

namespace {
// (the LDS fragment reads are pinned by hand as in basicblock_fused_pc.hip: lds_read_async / lds_wait of mfma_dev.h)
constexpr int T2H = STEM_T2H, T2W = STEM_T2W;               // tile of the final (1/4 resolution) map
constexpr int MR = 2 * T2H + 1, MC = 2 * T2W + 1;           // 5 x 65 intermediate (1/2 resolution) pixels
constexpr int MPIX = MR * MC, NQ = (MPIX + 31) / 32;        // 325 -> 11 column tiles
constexpr int NQW = (NQ + 3) / 4;                           // 3 column tiles per producer wave (wave 3: 2)
constexpr int PRS = STEM_PRS, PLANE = STEM_PROWS * PRS, NVAL = 3 * PLANE;  // 136, 1496, 4488 patch elements
// a pixel's gather base is (2 my) * PRS + 2 mx + 1 <= GBASE_MAX: the padded taps read NVAL + base, zeros written once per workgroup
constexpr int GBASE_MAX = 2 * (MR - 1) * PRS + 2 * (MC - 1) + 1, NZPAD = (GBASE_MAX + 1 + 7) / 8 * 8;  // 1217, 1224
constexpr int NROUND = STEM_ROUNDS, ROUND_BYTES = STEM_ROUND_ROWS * PRS * 2;  // 5 staging rounds, 1904 bytes of patch apart
constexpr int PS2 = 144, HALF = (MC + 1) / 2;               // intermediate pixel stride (128 B + 16: odd number of 16-B slots), 33 pixels per parity plane row
constexpr int MID_BYTES = MR * 2 * HALF * PS2;              // 47,520
constexpr int PATCH_BYTES = (NVAL + NZPAD) * 2;             // 11,424
constexpr int OFF_PATCH = 2 * MID_BYTES, OFF_BIAS = OFF_PATCH + 2 * PATCH_BYTES, OFF_TRASH = OFF_BIAS + 2 * 64 * 4;
constexpr int LDS_BYTES = OFF_TRASH + 32 * PS2;  // 123,008; the trash rows: 32 pixels that conv1's lanes without a pixel store into
constexpr int NTHR = 512;
constexpr int RD = 3, NFB = RD + 1;
static_assert(MID_BYTES % 16 == 0 && PATCH_BYTES % 16 == 0 && (NVAL * 2) % 16 == 0 && NZPAD % 8 == 0, "16-byte LDS units");
static_assert(STEM_STAGE_THREADS == NTHR / 2 && NROUND * STEM_ROUND_ROWS >= 3 * STEM_PROWS, "the producers stage the whole patch");
static_assert(LDS_BYTES <= 160 * 1024, "LDS");
}  // namespace

#ifdef HH_STAMP  // diagnostic build (EXTRA=-DHH_STAMP): s_memtime stamps of workgroup 0 in its third iteration (steady state), 8 slots per wave:
// 0 top of the iteration, 1 producer: patch loads issued / consumer: accumulator ready, 2 MFMAs and intermediate stores / MFMAs done,
// 3 patch written / output stored, 4 behind the barrier; slots 64..67: s_memtime and s_memrealtime at the workgroup's start and end
__device__ unsigned long long g_stem_stamps[72];
#define PSTAMP(i) do { if (blockIdx.x == 0 && it == 2 && lane == 0) g_stem_stamps[wave * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
extern "C" int hh_debug_stem_stamps(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stem_stamps), sizeof(g_stem_stamps)); }
#else
#define PSTAMP(i)
#endif

// E: the element type (ElemBF16 / ElemF16 of mfma_dev.h)
template <typename E>
__global__ __launch_bounds__(NTHR, 1) void stem_fused_kernel(const StemFusedParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    if (p.clk && tid == 0) atomicMin(p.clk, wall_clock64());
#ifdef HH_STAMP
    if (blockIdx.x == 0 && tid == 0) { g_stem_stamps[64] = __builtin_amdgcn_s_memtime(); g_stem_stamps[65] = __builtin_amdgcn_s_memrealtime(); }
#endif
    const int lds0 = (int)(size_t)(__attribute__((address_space(3))) char *)smem;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 31, h = lane >> 5;
    const bool producer = wave < 4;
    const int wj = wave & 3;
    const int H1 = p.H >> 1, W1 = p.W >> 1, H2 = p.H >> 2, W2 = p.W >> 2;
    // one buffer descriptor per IMAGE (32-bit offsets inside it): no limit on the batch
    const size_t img_elems = (size_t)3 * p.H * p.W, out_elems = (size_t)H2 * W2 * p.out_cs;
    constexpr unsigned OOB = 0x80000000u;

    if (tid < 64) {
        reinterpret_cast<float *>(smem + OFF_BIAS)[tid] = p.b1[tid];
        reinterpret_cast<float *>(smem + OFF_BIAS)[64 + tid] = p.b2[tid];
    }
    // the zero regions of the padded taps 27..31, behind both patches
    if (tid >= 64 && tid < 64 + 2 * (NZPAD / 8)) {
        const int z = tid - 64, buf = z / (NZPAD / 8), k = z - buf * (NZPAD / 8);
        *reinterpret_cast<u32x4 *>(smem + OFF_PATCH + buf * PATCH_BYTES + NVAL * 2 + k * 16) = u32x4{0u, 0u, 0u, 0u};
    }
    auto bias_acc = [&](int off) {
        f32x16 b0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bv = *reinterpret_cast<const float4 *>(smem + OFF_BIAS + (off + 8 * q + 4 * h) * 4);
            b0[4 * q + 0] = bv.x; b0[4 * q + 1] = bv.y; b0[4 * q + 2] = bv.z; b0[4 * q + 3] = bv.w;
        }
        return b0;
    };

    // ---- tiles: this workgroup's k-th tile is tile blockIdx.x + k gridDim.x, walked by adding the grid's (image, row, column) step
    const int tiles_x = (W2 + T2W - 1) / T2W, tiles_y = (H2 + T2H - 1) / T2H, ntiles = p.B * tiles_x * tiles_y;
    const int nloc = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    struct Geom { int b, ty, tx; };
    auto split = [&](int t) { return Geom{t / (tiles_x * tiles_y), (t / tiles_x) % tiles_y, t % tiles_x}; };
    const Geom g_first = split((int)blockIdx.x), g_step = split((int)gridDim.x);
    auto advance = [&](Geom g) {
        g.tx += g_step.tx;
        if (g.tx >= tiles_x) { g.tx -= tiles_x; ++g.ty; }
        g.ty += g_step.ty;
        if (g.ty >= tiles_y) { g.ty -= tiles_y; ++g.b; }
        g.b += g_step.b;
        return g;
    };

    // The two roles run separate copies of the tile loop (a prologue barrier and nloc + 1 iterations of one barrier each, both), so
    // that neither carries the other's registers.
    if (producer) {
        // ---- conv1's four A fragments [cout tile][k-step] as stem_conv.hip
        u32x4 a1[2][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) a1[ct][kk] = reinterpret_cast<const u32x4 *>(p.w1)[((ct * 2 + kk) * 2 + h) * 32 + r];

        // ---- patch staging (kernels.h: stem_unit).  Per round one word: the unit's byte offset from the tile origin (a multiple of 16)
        // with its patch row in the low four bits, -1 for a round in which this thread has no unit.
        int gp[NROUND];
        const StemUnit u0 = stem_unit(tid, 0);
        const int st_v = u0.v, st_slot = stem_unit_slot(u0) * 2;  // round i: + i * ROUND_BYTES (seven patch rows)
#pragma unroll
        for (int i = 0; i < NROUND; ++i) {
            const StemUnit u = stem_unit(tid, i);
            gp[i] = u.act ? (stem_unit_goff(u, p.H, p.W) * 4) | u.py : -1;
        }
        u32x4 pv[NROUND];
        auto patch_load = [&](const Geom &g) {
            const int oy0 = g.ty * T2H, ox0 = g.tx * T2W;
            const auto rs_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.images + (size_t)g.b * img_elems), 0, (int)(img_elems * 4), 0x00020000);
            const int origin = stem_tile_origin(oy0, ox0, p.W) * 4;
            const bool xok = stem_unit_col_ok(st_v, ox0, p.W);
            static_for<NROUND>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const bool ok = (gp[i] >= 0) & xok & stem_unit_row_ok(gp[i] & 15, oy0, p.H);
                const unsigned voff = ok ? (unsigned)(origin + (gp[i] & ~15)) : OOB;  // outside: 0 = conv1's padding
                pv[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_img, (int)voff, 0, 0));
            });
        };
        auto patch_write = [&](int buf) {
            char *dst = smem + OFF_PATCH + buf * PATCH_BYTES + st_slot;
            static_for<NROUND>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if (gp[i] >= 0) {
                    // (each word by value through __uint_as_float: __builtin_bit_cast of a vector ELEMENT read element 0 four times)
                    const unsigned w0 = pv[i][0], w1 = pv[i][1], w2 = pv[i][2], w3 = pv[i][3];
                    const unsigned lo = E::round2(__uint_as_float(w0), __uint_as_float(w1)), hi = E::round2(__uint_as_float(w2), __uint_as_float(w3));
                    *reinterpret_cast<u32x2 *>(dst + i * ROUND_BYTES) = u32x2{lo, hi};
                }
            });
        };
        // ---- conv1 gather: tap t = kk*16 + 8h + j -> (c, ky, kx) = (t / 9, (t % 9) / 3, t % 3) at patch column 2 mx + kx + 1; taps >= 27
        // read the zero region
        int off[2][8];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = kk * 16 + 8 * h + j;
                off[kk][j] = (t < 27 ? (t / 9) * PLANE + ((t % 9) / 3) * PRS + (t % 3) : NVAL) * 2;
            }
        // this lane's pixels: column tile q = wj + 4 qi, pixel m = 32 q + r = (my, mx) of the 5 x 65 intermediate tile.  A pixel past the
        // tile (lanes 5.. of column tile 10, all of wave 3's third) gathers the last pixel's taps and stores into the trash rows: no
        // branch in conv1, so the six accumulator chains of a wave can be scheduled as one block.
        int gbase[NQW], mdst[NQW], myx[NQW];
#pragma unroll
        for (int qi = 0; qi < NQW; ++qi) {
            const int m = (wj + 4 * qi) * 32 + r, mc = m < MPIX ? m : MPIX - 1;
            const int my = mc / MC, mx = mc - my * MC;
            gbase[qi] = ((2 * my) * PRS + 2 * mx + 1) * 2;
            mdst[qi] = m < MPIX ? ((my * 2 + (mx & 1)) * HALF + (mx >> 1)) * PS2 + h * 16 : -1;
            myx[qi] = my | (mx << 8);
        }
        char *const trash = smem + OFF_TRASH + r * PS2 + h * 16;

        Geom g = g_first, gn = advance(g_first);
        patch_load(g);
        patch_write(0);
        lds_barrier();

        for (int it = 0; it <= nloc; ++it) {
            PSTAMP(0);
            if (it < nloc) {
                const bool more = it + 1 < nloc;
                if (more) patch_load(gn);  // the next tile's input: in flight during conv1, to LDS behind it
                PSTAMP(1);
                const int oy0 = g.ty * T2H, ox0 = g.tx * T2W;
                const unsigned short *patch = reinterpret_cast<const unsigned short *>(smem + OFF_PATCH + (it & 1) * PATCH_BYTES);
                char *mid = smem + (it & 1) * MID_BYTES;

                // ================= conv1 + bn1 + relu -> intermediate tile (LDS, 16-bit, column-parity planes) =================
                u32x4 bf[NQW][2];
#pragma unroll
                for (int qi = 0; qi < NQW; ++qi)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        unsigned short v[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const unsigned short *>(reinterpret_cast<const char *>(patch) + gbase[qi] + off[kk][j]);
                        bf[qi][kk] = u32x4{(unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16),
                                           (unsigned)v[4] | ((unsigned)v[5] << 16), (unsigned)v[6] | ((unsigned)v[7] << 16)};
                    }
                const f32x16 bias1[2] = {bias_acc(0), bias_acc(32)};
                f32x16 acc[NQW][2];  // six independent chains of two k-steps: all first steps, then all second steps
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int qi = 0; qi < NQW; ++qi)
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) acc[qi][ct] = E::mfma(a1[ct][kk], bf[qi][kk], kk == 0 ? bias1[ct] : acc[qi][ct]);
#pragma unroll
                for (int qi = 0; qi < NQW; ++qi) {
                    const int my = myx[qi] & 255, mx = myx[qi] >> 8;
                    const int gy = 2 * oy0 - 1 + my, gx = 2 * ox0 - 1 + mx;
                    const bool inside = ((unsigned)gy < (unsigned)H1) & ((unsigned)gx < (unsigned)W1);  // else conv2's zero padding
                    char *dst = mdst[qi] >= 0 ? mid + mdst[qi] : trash;
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        u32x4 o[2];
                        pack_rows16<E>(acc[qi][ct], o);
                        *reinterpret_cast<u32x4 *>(dst + ct * 64) = inside ? o[0] : u32x4{0u, 0u, 0u, 0u};
                        *reinterpret_cast<u32x4 *>(dst + ct * 64 + 32) = inside ? o[1] : u32x4{0u, 0u, 0u, 0u};
                    }
                }
                PSTAMP(2);
                if (more) patch_write((it + 1) & 1);
                g = gn;
                gn = advance(gn);
            }  // (last iteration: nothing to produce and nothing to stage)
            PSTAMP(3);
            lds_barrier();  // the intermediate tile and the next patch are complete; the other two buffers are free
            PSTAMP(4);
        }
    } else {
        // ---- conv2's 36 fragments of this wave's cout tile
        const int row2 = wj >> 1, ct2 = wj & 1;
        u32x4 w2r[36];
        {
            const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw *>(p.w2), 0, 9 * 8 * 64 * 16, 0x00020000);
            static_for<36>([&](auto fc) {  // packed [tap][cin / 8][64 couts][8]: fragment (tap, kk) = rows (kk*2 + h) of that tap
                constexpr int f = decltype(fc)::value, tap = f >> 2, kk = f & 3;
                w2r[f] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, (((tap * 8 + kk * 2 + h) * 64) + ct2 * 32 + r) * 16, 0, 0));
            });
        }
        const int ma0 = lds0 + (row2 * 4 * HALF + r) * PS2 + h * 16;  // intermediate row 2 row2 (+ ky), plane row pair, pixel r (+ kx >> 1)
        Geom g = g_first;  // the tile of iteration it - 1
        lds_barrier();

        for (int it = 0; it <= nloc; ++it) {
            PSTAMP(0);
            if (it >= 1) {
                // ================= conv2 + bn2 + relu: wave = (output row, cout tile) =================
                f32x16 acc = bias_acc(64 + ct2 * 32);
                PSTAMP(1);
                const int ma = ma0 + ((it - 1) & 1) * MID_BYTES;
                u32x4 fb[NFB];
                auto ldb = [&](auto sc, int buf) {  // step s = tap * 4 + kk: intermediate pixel (2 row2 + ky, 2 r + kx), channels 16 kk + 8 h ..
                    constexpr int s = decltype(sc)::value, tap = s >> 2, kk = s & 3, ky = tap / 3, kx = tap % 3;
                    fb[buf] = lds_read_async<((ky * 2 + (kx & 1)) * HALF + (kx >> 1)) * PS2 + kk * 32>(ma);
                };
                static_for<RD>([&](auto sc) { ldb(sc, decltype(sc)::value); });
                static_for<36>([&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    if constexpr (s + RD < 36) ldb(std::integral_constant<int, s + RD>{}, (s + RD) % NFB);
                    lds_wait<(35 - s < RD ? 35 - s : RD)>(fb[s % NFB]);
                    acc = E::mfma(w2r[s], fb[s % NFB], acc);
                });
                PSTAMP(2);
                u32x4 o[2];
                pack_rows16<E>(acc, o);
                const int oy = g.ty * T2H + row2, ox = g.tx * T2W + r;
                const bool ok = (oy < H2) & (ox < W2);
                const auto rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)g.b * out_elems, 0, (int)(out_elems * 2), 0x00020000);
                const unsigned voff = ok ? (unsigned)(((oy * W2 + ox) * p.out_cs + ct2 * 32 + 8 * h) * 2) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(o[0], rs_out, (int)voff, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(o[1], rs_out, (int)voff, 32, 0);
                g = advance(g);
            }
            PSTAMP(3);
            lds_barrier();  // the intermediate tile is free, the next one is complete
            PSTAMP(4);
        }
    }
    if (p.clk && tid == 0) atomicMax(p.clk + 1, wall_clock64());
#ifdef HH_STAMP
    if (blockIdx.x == 0 && tid == 0) { g_stem_stamps[66] = __builtin_amdgcn_s_memtime(); g_stem_stamps[67] = __builtin_amdgcn_s_memrealtime(); }
#endif
}

hipError_t stem_fused_init()
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(stem_fused_kernel<ElemBF16>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(stem_fused_kernel<ElemF16>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
}

bool stem_fused_supported(const StemFusedParams &p)
{
    return p.H % 4 == 0 && p.W % 4 == 0 && (size_t)3 * p.H * p.W * 4 < 0x7fffffffull && (size_t)(p.H / 4) * (p.W / 4) * p.out_cs * 2 < 0x7fffffffull;
}

hipError_t stem_fused_launch(const StemFusedParams &p, int num_cus, hipStream_t s, int act_dtype)
{
    if (act_dtype != 0 && act_dtype != 1) return hipErrorInvalidValue;
    const int H2 = p.H >> 2, W2 = p.W >> 2;
    const int ntiles = p.B * ((H2 + T2H - 1) / T2H) * ((W2 + T2W - 1) / T2W);
    const int grid = ntiles < num_cus ? ntiles : num_cus;
    if (act_dtype) HH_LAUNCH(stem_fused_kernel<ElemF16>, dim3(grid), dim3(NTHR), LDS_BYTES, s, p);
    else HH_LAUNCH(stem_fused_kernel<ElemBF16>, dim3(grid), dim3(NTHR), LDS_BYTES, s, p);
    return hipGetLastError();
}
