// Internal launch interface between the host engine and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hip/hip_ext.h>

// The descriptor tables that cross the C boundary are the structs of the public header, the only definition of their layout: kernels
// and launchers take the hh_* types themselves.  Each size is asserted once, beside the code that owns the struct (ABI version 3).
#include "../../include/hhrnet.h"

typedef uint16_t bf16_raw;  // storage type of a bf16 element in HBM (and of an fp16 one: the training path's fp16 form, HH_DTYPE_F16 handles)
// act_dtype of the training launchers: the element type of activations and packed weights, 0 = bf16, 1 = fp16 (HH_ACT_BF16 / HH_ACT_F16
// of hhrnet.h); anything else is hipErrorInvalidValue.  The fused inference kernels take the same parameter: an HH_DTYPE_F16 handle
// passes 1.

// Per-launch timing probe (bench.py's roofline line).  When the engine arms it, the NEXT forward-path kernel launch of this
// thread goes through hipExtLaunchKernelGGL with a start / stop event pair: the runtime fills those from the dispatch packet's
// own begin / end timestamps, i.e. hipEventElapsedTime(start, stop) is the kernel duration that rocprofv3's kernel trace
// reports (no marker packets, no dispatch gap inside the bracket).
struct LaunchProbe { hipEvent_t start = nullptr, stop = nullptr; };
LaunchProbe &hh_launch_probe();  // thread-local, consumed (reset) by the launch that uses it
#define HH_LAUNCH(kernel, grid, block, lds, stream, ...)                                                            \
    do {                                                                                                            \
        LaunchProbe &lp_ = hh_launch_probe();                                                                       \
        if (lp_.start) {                                                                                            \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, lp_.start, lp_.stop, 0, __VA_ARGS__);           \
            lp_ = LaunchProbe{};                                                                                    \
        } else {                                                                                                    \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                      \
        }                                                                                                           \
    } while (0)

// One convolution launch (3x3 / 1x1 / 2x2-phase-of-deconv; stride 1 or 2) on NHWC bf16.
struct ConvParams {
    const bf16_raw *in;   // [B, Hin, Win, in_cs]
    int in_cs, in_coff;   // pixel stride / first channel (elements, multiples of 8)
    int Hin, Win;
    const bf16_raw *w;    // packed [cout_group][cin_chunk][tap][KC/8][COUT_T][8]
    const float *bias;    // [ncg*COUT_T] folded BN shift (or conv bias), zero padded
    const bf16_raw *res;  // optional residual, same pixel grid as `out`
    int res_cs, res_coff;
    bf16_raw *out;        // optional bf16 NHWC output [B, Hob, Wob, out_cs]
    int out_cs, out_coff;
    float *out_f32;       // optional fp32 NCHW output [B, cout_real, Hob, Wob]
    int Hob, Wob;         // output buffer spatial dims
    int osy, ooy, osx, oox;  // output scatter: Y = oy*osy + ooy (deconv phases use 2, phase)
    int Ho, Wo;           // conv output grid (before scatter)
    int cin;              // padded input channels (multiple of KC)
    int cout_real, cout_store;
    int relu;
    int pad_y, pad_x;     // top/left zero padding
    int B, tiles_x, tiles_y, ncg;
    int nphase;           // 4: the four 2x2 phases of a 4x4 stride-2 transposed conv in ONE launch (pad / output offset follow the
    size_t phase_stride;  //    phase index, weights of phase f start at w + f * phase_stride elements); 0 or 1: plain conv
    unsigned long long *stamps;  // diagnostic build (-DHH_STAMP) only
    unsigned long long *clk;     // optional {min start, max end} of the launch in wall_clock64() ticks (profiling probe)
    // Several input tensors as ONE conv over their concatenated channels (the summed stride-2 convs of a fusion layer,
    // hrnet.py:166-229): same spatial dims and the same pixel stride as `in`; chunks [0, nch0) come from `in`, the next nch1 from
    // in + src_delta1 elements, the rest from in + src_delta2.  nch0 = 0: a single input.
    int nch0, nch1;
    ptrdiff_t src_delta1, src_delta2;
    // Dual launch (conv_dual_launch): a second, stride-2 3x3 conv (pad 1, 64 couts, ReLU as `relu`) over the SAME input, computed from
    // the patch the first one stages.  w2: its weights packed as for its own launch (KC = 16, COUT_T = 64), bias2: 64 floats,
    // out2: [B, Ho2, Wo2, out2_cs] with Ho2 = Hin / 2, Wo2 = Win / 2.
    const bf16_raw *w2;
    const float *bias2;
    bf16_raw *out2;
    int out2_cs, out2_coff;
    int Ho2, Wo2;
};

// Tile configuration of one kernel instantiation.
struct ConvConfig {
    int KS, S, KC, NT, WC, PT, TW;
    int DB;  // 1: the K loop runs on two LDS buffers (conv_mfma.hip), each followed by 16 bytes per thread for staging units without a destination
    int cout_t() const { return 32 * NT * WC; }
    int th() const { return (4 / WC) * PT * (32 / TW); }
    size_t lds_bytes() const {
        int PH = (th() - 1) * S + KS, PW = (TW - 1) * S + KS;
        size_t patch = ((size_t)PH * PW * (KC * 2 + 16) + 15) & ~(size_t)15;
        const size_t buf = patch + (size_t)KS * KS * KC * cout_t() * 2;
        return DB ? 2 * (buf + 256 * 16) : buf;
    }
};

// Returns the number of instantiated configs / the i-th one.
int conv_num_configs();
const ConvConfig &conv_config(int i);
// Launches config `cfg_index`; the grid is B*tiles_y*tiles_x*ncg blocks of 256 threads.
hipError_t conv_launch(int cfg_index, const ConvParams &p, hipStream_t stream, int act_dtype = 0);
hipError_t conv_init();  // raises the dynamic-LDS limit of every instantiation
// The stage-0 -> 1 transition pair as ONE launch: config 0 (3x3 stride 1, 32 couts, 8x32 tiles; `p` as for conv_launch) plus the
// stride-2 64-cout conv of p.w2 / p.bias2 / p.out2 over the same staged patch.  Needs ncg = 1, no residual, no fp32 output.
#define HH_CFG_TRANS_DUAL 108  // pseudo instantiation index used by the profiler
hipError_t conv_dual_launch(const ConvParams &p, hipStream_t stream, int act_dtype = 0);

// ---- fp8 path (conv_fp8.hip): e4m3 NHWC activations with one scale per tensor, e4m3 weights with one scale per cout
struct Fp8ConvParams {
    const unsigned char *in;  // [B, Hin, Win, in_cs] e4m3
    int in_cs, in_coff;       // pixel stride / first channel (bytes, multiples of 16)
    int Hin, Win;
    const unsigned char *w;   // packed [cout_group][cin_chunk][k-step][lane half][piece 0/1][COUT_T][16]
    const float *mult;        // [ncg*COUT_T] s_in * s_w[co] (0 for padding couts)
    const float *bias;        // [ncg*COUT_T] folded BN shift / conv bias
    const unsigned char *res; // optional residual (e4m3), same pixel grid as `out`
    int res_cs, res_coff;
    float res_scale;
    const bf16_raw *res16;    // optional residual in bf16 (real values, no scale): the residual TRUNK of an fp8 net stays bf16
    int res16_cs, res16_coff; //   (elements); takes precedence over `res`
    unsigned char *out;       // optional e4m3 NHWC output
    int out_cs, out_coff;
    float out_inv_scale;      // 1 / s_out
    bf16_raw *out16;          // optional bf16 NHWC output of the same values (the trunk's second representation: read back as a
    int out16_cs, out16_coff; //   residual / by the fusion sums; the e4m3 one feeds the next conv's MFMA); elements
    float *out_f32;           // optional fp32 NCHW output [B, cout_real, Hob, Wob]
    int Hob, Wob;
    int osy, ooy, osx, oox;
    int Ho, Wo;
    int cin;                  // padded input channels (multiple of KC)
    int cout_real, cout_store;
    int relu;
    int pad_y, pad_x;
    int B, tiles_x, tiles_y, ncg;
    int nphase;
    size_t phase_stride;      // bytes between the weight sets of two transposed-conv phases
    unsigned *absmax;         // calibration: atomicMax of the bits of max |y| over the launch (NULL = off)
};
struct Fp8ConvConfig {
    int KS, S, KC, NT, PT, TW;
    // bytes per staged pixel: KC + padding to an ODD number of 16-byte slots (bank-conflict-free ds_read_b128 across pixels)
    static constexpr int pixel_stride(int kc) { return ((kc / 16 + 1) | 1) * 16; }
    int cout_t() const { return 32 * NT; }
    int th() const { return 4 * PT * (32 / TW); }
    int nstep() const { return (KS * KS * (KC / 16) + 3) / 4; }
    size_t lds_bytes() const {
        const int PH = (th() - 1) * S + KS, PW = (TW - 1) * S + KS;
        const size_t patch = ((size_t)PH * PW * pixel_stride(KC) + 15) & ~(size_t)15;
        return patch + (size_t)nstep() * 4 * cout_t() * 16;
    }
};
int conv_fp8_num_configs();
const Fp8ConvConfig &conv_fp8_config(int i);
hipError_t conv_fp8_launch(int cfg_index, const Fp8ConvParams &p, hipStream_t stream);
hipError_t conv_fp8_init();

// fused BasicBlock on e4m3 tensors (basicblock_fused_fp8.hip): weights packed as conv_fp8 packs a 3x3 conv with KC = C, NT = 2
struct Fp8BBParams {
    const unsigned char *in; int in_cs;   // [B,H,W,in_cs bytes], channels 0..C-1
    unsigned char *out; int out_cs;       // must not alias `in`
    const unsigned char *w1, *w2;
    const float *mult1, *bias1, *mult2, *bias2;  // [64]: s_in * s_w1[co], shift1, s_mid * s_w2[co], shift2 (0 for padding couts)
    float mid_inv_scale, res_scale, out_inv_scale;
    const bf16_raw *res16; int res16_cs;  // optional: the block input in bf16 (same pixels as `in`): residual read from it instead of
                                          // from the e4m3 patch
    bf16_raw *out16; int out16_cs;        // optional: the block output in bf16 beside the e4m3 one
    int B, H, W;
    int tiles_x, tiles_y, ntiles;         // filled by the launcher
    unsigned *amax_mid, *amax_out;        // calibration (NULL = off): atomicMax of the bits of the tensors' maxima
};
bool bb_fp8_supported(int C);
hipError_t bb_fp8_launch(int C, const Fp8BBParams &p, int num_cus, hipStream_t s);
#define HH_CFG_BB_FP8 105

// Fused 32-channel BasicBlock (basicblock_fused.hip): out = relu(conv2(relu(conv1(in))) + in), BN folded.
struct BBParams {
    const bf16_raw *in; int in_cs;   // [B,H,W,in_cs], channels 0..31
    bf16_raw *out; int out_cs;       // must not alias `in` (tiles read a 2-pixel halo of their neighbours)
    const bf16_raw *w1, *w2;         // packed as conv_mfma family (KS=3,S=1,KC=32,NT=1): [tap][4][32][8]
    const float *b1, *b2;            // [32]
    int B, H, W;
    int tiles_x, tiles_y, ntiles;    // filled by bb_fused_launch
    int tall;                        // bbpc_launch: 1 = lay the batch out as one tall image when that needs fewer tiles (2: always), 0 = never
    int VH;                          // filled by bbpc_launch: rows per image in the tall layout (H + 2), or 2^30
    bf16_raw *trash;                 // filled by bb_fused_launch: dummy line for the stores of lanes outside the image
    // bbpc_launch only: the 1x1 head behind the block, run in its epilogue (fin_out != nullptr; `out` is then not written)
    const bf16_raw *fin_w;           // [k half 2][lane half 2][32 couts][8 cin] bf16, couts >= fin_K zero
    const float *fin_b;              // [32]
    float *fin_out;                  // [B, fin_K, H, W] fp32
    int fin_K;
    unsigned long long *stamps;      // diagnostic build (-DHH_STAMP) only
    unsigned long long *clk;         // optional {min start, max end} of the launch in wall_clock64() ticks
};
// Tile geometry of the producer / consumer form (basicblock_fused_pc.hip) for its kernel and for bbpc_cover, the host walk behind
// hh_debug_bb_cover.  bbpc_geom and bbpc_rowmap are the kernel's own code.  bbpc_band and bbpc_patch_wrap / bbpc_patch_row RESTATE
// two expressions the kernel keeps written out (its `band` lambda and the row test in pf_load: as calls they changed its register
// allocation): whoever edits one side edits the other.
constexpr int BBPC_TH = 14, BBPC_TW = 32;  // output tile
struct BBGeom { int b, oy0, ox0; };        // image of the tile's first output row, that row's index inside it, first column
// XCD-aware tile order: position i of the launch's tile sequence -> tile  (= `band` in bbpc_body)
__host__ __device__ inline int bbpc_band(int i, int ntiles, unsigned grid)
{
    return ((ntiles & 7) == 0 && (grid & 7) == 0) ? (i & 7) * (ntiles >> 3) + (i >> 3) : i;
}
__host__ __device__ __forceinline__ BBGeom bbpc_geom(int tb, int tiles_x, int tiles_per_img, int VH)
{
    const int u = tb / tiles_per_img, tt = tb % tiles_per_img;
    const int oy = (tt / tiles_x) * BBPC_TH, bq = oy / VH;
    return BBGeom{u + bq, oy - bq * VH, (tt % tiles_x) * BBPC_TW};
}
// row y = oy0 + d of the tile of image b -> flat row (image * H + row) of the tensor, or -1 outside every image
__host__ __device__ __forceinline__ int bbpc_rowmap(int b, int y, int B, int H, int VH)
{
    const bool wrap = y >= VH;
    const int ya = wrap ? y - VH : y, bb = wrap ? b + 1 : b;
    return (((unsigned)ya < (unsigned)H) & (bb < B)) ? bb * H + ya : -1;
}
// patch row yy (counted from the first row of image b): does it belong to image b + 1 (tall layout), and is it a row of an image at
// all (`next`: image b + 1 exists)?  Outside every image the patch holds zeros, conv1's padding.  (= `wrap`, `ok` in pf_load)
__host__ __device__ inline bool bbpc_patch_wrap(int yy, int VH) { return yy >= VH; }
__host__ __device__ inline bool bbpc_patch_row(int yy, bool wrap, bool next, int H, int VH)
{
    return ((unsigned)(wrap ? yy - VH : yy) < (unsigned)H) & (!wrap | next);
}
bool bbpc_cover(int B, int H, int W, int tall, int num_cus, long long counts[4]);

#define HH_PROF_SLOTS 1024   // launches per forward the device-clock probe can record
#define HH_CFG_BB_FUSED 100  // pseudo instantiation index used by the profiler
hipError_t bb_fused_init();
hipError_t bb_fused_launch(BBParams p, int num_cus, hipStream_t s);
// producer / consumer form of the same block (basicblock_fused_pc.hip): weights resident in registers, row-band fragment reuse
hipError_t bbpc_init();
bool bbpc_supported(const BBParams &p);
bool bbpc_final_supported(const BBParams &p);
hipError_t bbpc_launch(BBParams p, int num_cus, hipStream_t s, int act_dtype = 0);
// the same block for the 64-channel branch (basicblock_fused_c64.hip): weights packed KS=3,S=1,KC=32,NT=2 ([chunk][tap][4][64][8])
#define HH_CFG_BB64_FUSED 103
hipError_t bb64_fused_init();
hipError_t bb64_fused_launch(BBParams p, int num_cus, hipStream_t s, int act_dtype = 0);

// Junction of two stage-0 Bottlenecks (bottleneck_junction.hip): y = relu(W3 t2 + shift (+ Wd x | + res)), t1 = relu(W1 y + shift1)
struct JuncParams {
    const bf16_raw *t2; int t2_cs;     // [npix, 64]  conv2 output of this unit
    const bf16_raw *res; int res_cs;   // [npix, 256] previous y (units 1-3), or nullptr
    const bf16_raw *x; int x_cs;       // [npix, 64]  unit-0 input of the downsample conv, or nullptr
    const bf16_raw *t2a; int t2a_cs;   // pair mode: conv2 output of the PREVIOUS unit, whose y is made again here instead of read (else nullptr)
    const bf16_raw *w3a; const float *b3a;  // pair mode: the previous unit's conv3 (its downsample, if it is unit 0, is wd / bd with x)
    const bf16_raw *w3, *wd, *w1;      // packed as the conv_mfma family packs 1x1 KC=32 NT=2 layers; wd / w1 may be nullptr
    const float *b3, *bd, *b1;
    bf16_raw *y; int y_cs;             // [npix, 256]; nullptr: not stored (the next junction makes it again, pair mode)
    bf16_raw *t1; int t1_cs;           // [npix, 64] (only when w1)
    int npix;
    unsigned long long *clk;           // optional {min start, max end} device-clock probe
};
#define HH_CFG_JUNCTION 101  // pseudo instantiation index used by the profiler
hipError_t junction_init();
hipError_t junction_launch(const JuncParams &p, int num_cus, hipStream_t s, int act_dtype = 0);

// First stem conv (stem_conv.hip): fp32 NCHW images -> conv3x3 s2 p1 (3->64) + BN + ReLU -> bf16 NHWC [B,H/2,W/2,out_cs]
struct StemParams {
    const float *images;      // [B,3,H,W]
    const bf16_raw *w;        // [cout tile 2][k-step 2][half 2][32 couts][8 taps] bf16, tap = c*9 + ky*3 + kx, BN scale folded, taps 27..31 zero
    const float *bias;        // [64]
    bf16_raw *out; int out_cs;
    int B, H, W;              // H, W even
    unsigned long long *clk;  // optional device-clock probe
    unsigned char *out_fp8;   // fp8 path: e4m3 NHWC output [B,H/2,W/2,out_cs bytes] instead of `out`, q = e4m3(y * out_inv_scale)
    float out_inv_scale;
    unsigned *absmax;         // fp8 calibration: atomicMax of the bits of max |y|
};
#define HH_CFG_STEM 102  // pseudo instantiation index used by the profiler
hipError_t stem_conv_launch(const StemParams &p, hipStream_t s);
// Both stem convolutions in one kernel (stem_fused.hip): conv3x3 s2 3->64 + BN + ReLU -> conv3x3 s2 64->64 + BN + ReLU.
struct StemFusedParams {
    const float *images;      // [B,3,H,W], H and W multiples of 4
    const bf16_raw *w1;       // conv1 as StemParams::w
    const float *b1;          // [64]
    const bf16_raw *w2;       // conv2 packed [tap 9][cin/8 8][64 couts][8] (hh_pack_weights with KC = 64, COUT_T = 64), BN scale folded
    const float *b2;          // [64]
    bf16_raw *out; int out_cs;  // [B,H/4,W/4,out_cs], channels 0..63
    int B, H, W;
    unsigned long long *clk;  // optional device-clock probe
};
#define HH_CFG_STEM_FUSED 106
// Input staging of stem_fused.hip, shared with the host walk of tools/stem_stage_host_check.cpp.  A tile of 2 x 32 outputs needs input
// rows 4 oy0 - 3 .. 4 oy0 + 7 and columns 4 ox0 - 3 .. 4 ox0 + 127 of the three channel planes.  A patch row is staged as 34 aligned
// float4 (columns 4 ox0 - 4 .. 4 ox0 + 131) and kept in LDS as 136 16-bit values: 3 x 11 rows x 34 = 1122 units of 16 bytes.  The
// 256 staging threads move seven patch rows per round (thread = row tid / 34 of the round, vector tid % 34; threads 238..255 idle),
// five rounds per tile.  Everything about a unit but its two range tests is the same for every tile.
constexpr int STEM_T2H = 2, STEM_T2W = 32;              // tile of the final (1/4 resolution) map
constexpr int STEM_PROWS = 4 * STEM_T2H + 3;            // 11 patch rows per channel plane
constexpr int STEM_PVEC = (4 * STEM_T2W + 4 + 4) / 4;   // 34 float4 per patch row
constexpr int STEM_PRS = 4 * STEM_PVEC;                 // 136: patch row stride in elements
constexpr int STEM_STAGE_THREADS = 256, STEM_ROUND_ROWS = STEM_STAGE_THREADS / STEM_PVEC;                           // 7
constexpr int STEM_ROUNDS = (3 * STEM_PROWS + STEM_ROUND_ROWS - 1) / STEM_ROUND_ROWS;                               // 5
struct StemUnit { int c, py, v; bool act; };  // channel plane, patch row, float4 index inside the row; act: the thread has a unit this round
__host__ __device__ inline StemUnit stem_unit(int tid, int round)
{
    const int rr = tid / STEM_PVEC, row = STEM_ROUND_ROWS * round + rr, c = row / STEM_PROWS;
    return StemUnit{c, row - c * STEM_PROWS, tid - rr * STEM_PVEC, rr < STEM_ROUND_ROWS && row < 3 * STEM_PROWS};
}
// element offset of the unit's first value inside one image, relative to the tile's origin (row 4 oy0 - 3, column 4 ox0 - 4 of plane 0)
__host__ __device__ inline int stem_unit_goff(const StemUnit &u, int H, int W) { return (u.c * H + u.py) * W + 4 * u.v; }
__host__ __device__ inline int stem_tile_origin(int oy0, int ox0, int W) { return (4 * oy0 - 3) * W + 4 * ox0 - 4; }
// the patch element (of 3 * STEM_PROWS * STEM_PRS) that receives the unit's first value
__host__ __device__ inline int stem_unit_slot(const StemUnit &u) { return (u.c * STEM_PROWS + u.py) * STEM_PRS + 4 * u.v; }
// the two range tests: outside the image a unit is conv1's zero padding (W % 4 == 0: the four columns are inside or outside together)
__host__ __device__ inline bool stem_unit_row_ok(int py, int oy0, int H) { return (unsigned)(4 * oy0 - 3 + py) < (unsigned)H; }
__host__ __device__ inline bool stem_unit_col_ok(int v, int ox0, int W) { return (unsigned)(4 * ox0 - 4 + 4 * v) < (unsigned)W; }
hipError_t stem_fused_init();
bool stem_fused_supported(const StemFusedParams &p);
hipError_t stem_fused_launch(const StemFusedParams &p, int num_cus, hipStream_t s, int act_dtype = 0);


// out[b,y,x,c] = act(base[b,y,x,c] + sum_j up_j[b, y>>sh_j, x>>sh_j, c]),  c in [0,C)
struct UpAddParams {
    const bf16_raw *base; int base_cs, base_coff;
    const bf16_raw *up[3]; int up_cs[3]; int up_shift[3]; int nup;
    bf16_raw *out; int out_cs, out_coff;
    int B, H, W, C, relu;
};
hipError_t launch_upadd(const UpAddParams &p, hipStream_t s, int act_dtype = 0);
// Output 0 of a fusion layer in one launch (fusion_up.hip), 32 channels:
// out[b,y,x,c] = relu(x0[b,y,x,c] + sum_j u_j[b, y>>j, x>>j, c]),  u_j = bf16(bias_j + W_j x_j) for the sources j = 1..nsrc
struct FusionUpParams {
    const bf16_raw *x0; int x0_cs;      // [B, H, W, x0_cs], channels 0..31
    const bf16_raw *src[3];             // x_j: [B, H >> j, W >> j, src_cs], 32 << j channels
    int src_cs[3];
    const bf16_raw *w[3];               // 1x1 conv + BN of source j, packed as conv_mfma packs KC = 32, NT = 1 layers: [cin/8][32][8]
    const float *bias[3];               // [32]
    int nsrc;                           // 1..3
    bf16_raw *out; int out_cs;          // channels 0..31 written (out may be a wider buffer)
    int B, H, W;                        // branch-0 map
    int tiles_x, tiles_y;               // filled by fusion_up_launch
    unsigned long long *clk;            // optional {min start, max end} device-clock probe
};
#define HH_CFG_FUSION_UP 107  // pseudo instantiation index used by the profiler
bool fusion_up_supported(int C, int nsrc);
hipError_t fusion_up_launch(FusionUpParams p, hipStream_t s, int act_dtype = 0);
hipError_t launch_upadd_backward(const bf16_raw *dy, const bf16_raw *out, int relu, int B, int H, int W, int C, bf16_raw *g, bf16_raw *const *dup,
                                 const int *up_shift, int nup, hipStream_t s, int act_dtype = 0);
// the same on e4m3 tensors: out = e4m3(act(base * base_scale + sum_j up_j * up_scale[j]) * out_inv_scale); C multiple of 16
struct UpAddFp8Params {
    const unsigned char *base; int base_cs; float base_scale;
    const unsigned char *up[3]; int up_cs[3]; int up_shift[3]; float up_scale[3]; int nup;
    // an operand given in bf16 (real values) instead of e4m3 * scale: base16 / up16[j] non-NULL take precedence
    const bf16_raw *base16; int base16_cs;
    const bf16_raw *up16[3]; int up16_cs[3];
    unsigned char *out; int out_cs;       // optional e4m3 output
    float out_inv_scale;
    bf16_raw *out16; int out16_cs;        // optional bf16 output
    int B, H, W, C, relu;
    unsigned *absmax;
};
hipError_t launch_upadd_fp8(const UpAddFp8Params &p, hipStream_t s);
// bf16 tensor -> its e4m3 representation (q = e4m3(x * inv_scale)); n16 = groups of 16 channels per pixel; absmax: calibration
hipError_t launch_quant_fp8(const bf16_raw *in, int in_cs, unsigned char *out, int out_cs, size_t npix, int C, float inv_scale, unsigned *absmax,
                            hipStream_t s);

// ClassificationHead tail: global average pool (bf16 NHWC -> fp32 [B,C]) and Linear (fp32)
hipError_t launch_lds_poison(int num_cus, hipStream_t s);  // debug: NaN patterns into every CU's LDS (misc_kernels.hip)
hipError_t launch_avgpool(const bf16_raw *in, int in_cs, float *out, int B, int HW, int C, hipStream_t s, int act_dtype = 0);
hipError_t launch_linear(const float *x, const float *w, const float *bias, float *y, int B, int K, int N, hipStream_t s);
// The same tail in training form (cls_tail.hip): the pool's backward, the Linear's three gradients, softmax cross-entropy
hipError_t launch_avgpool_backward(const float *g, bf16_raw *dx, int B, int HW, int C, hipStream_t s, int act_dtype = 0);
hipError_t launch_linear_backward(const float *x, const float *w, const float *dy, int B, int K, int N, float *dx, float *dw, float *db,
                                  hipStream_t s);
static_assert(sizeof(hh_xent_result) == 16, "ABI 3");
hipError_t launch_softmax_xent(const float *logits, const long long *targets, int B, int N, float *dlogits, hh_xent_result *result, hipStream_t s);

static_assert(sizeof(hh_image_desc) == 64, "ABI 3");  // one raw image of a batch
hipError_t launch_preprocess_batch(const unsigned char *base, const hh_image_desc *descs, int n, float *out, int H, int W,
                                   const float mean[3], const float stdv[3], hipStream_t s);
hipError_t launch_warp_affine_u8(const unsigned char *img, int h, int w, const double inv[6], unsigned char *out, int H, int W, hipStream_t s);
hipError_t launch_preprocess(const unsigned char *img, int h, int w, const double inv[6], float *out, int H, int W,
                             const float mean[3], const float stdv[3], hipStream_t s);
// The training input (hh_train_desc of include/hhrnet.h): one sample's raw image and crowd mask in the batch buffer, its flip
// flag, and the destination -> source affines of the image and of every stage's mask.
static_assert(sizeof(hh_train_desc) == 272, "ABI 3");
struct TrainMaskStages { float *out[HH_TRAIN_MAX_STAGES]; int h[HH_TRAIN_MAX_STAGES], w[HH_TRAIN_MAX_STAGES], n; };
hipError_t launch_train_images(const unsigned char *base, const hh_train_desc *descs, int n, float *out, int H, int W, const float mean[3],
                               const float stdv[3], hipStream_t s);
hipError_t launch_train_masks(const unsigned char *base, const hh_train_desc *descs, int n, const TrainMaskStages &st, hipStream_t s);
// The classifier's input (hh_crop_desc of include/hhrnet.h, cls_input.hip): one sample's raw image, its source rectangle, the size of
// the virtual resized crop and the output window inside it.  56 bytes.
static_assert(sizeof(hh_crop_desc) == 56, "ABI 3");
hipError_t launch_resized_crop(const unsigned char *base, const hh_crop_desc *descs, int n, float *out, int H, int W, const float mean[3],
                               const float stdv[3], hipStream_t s);
// The mosaic of the training input (hh_mosaic_desc of include/hhrnet.h, train_mosaic.hip): four raw tiles (image + crowd mask) and the
// two canvases they are resized into, all as byte offsets from the batch's base pointer.  112 bytes.
static_assert(sizeof(hh_mosaic_tile) == 24 && sizeof(hh_mosaic_desc) == 112, "ABI 3");
hipError_t launch_mosaic(unsigned char *base, const hh_mosaic_desc *descs, int n, int S, hipStream_t s);
// Pose overlays (hh_render_desc / hh_render_prim of include/hhrnet.h; structs and arithmetic in render_math.h, kernels in render.hip):
// n frames in one launch, `max_tiles` = the largest frame's tile count; the same walk on the host for one frame; the general 8-bit resize.
hipError_t launch_render_poses(unsigned char *base, const hh_render_desc *descs, const hh_render_prim *prims, int n, int max_tiles, hipStream_t s);
void render_debug_host(const unsigned char *src, unsigned char *dst, const hh_render_desc &d, const hh_render_prim *prims);
hipError_t launch_resize_u8(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, hipStream_t s);
hipError_t launch_resize_u8_scaled(const unsigned char *src, int h, int w, int channels, unsigned char *dst, int H, int W, double fx, double fy, hipStream_t s);
// Text labels (hh_text_desc / hh_text_prim of include/hhrnet.h; arithmetic in text_math.h, kernel in text.hip): the listed tiles of a
// batch of frames in one launch, `tiles` = num_tiles (frame, tile) pairs; the same walk on the host for one frame.
hipError_t launch_text_labels(unsigned char *base, const hh_text_desc *descs, const hh_text_prim *prims, const uint8_t *atlas, const void *tiles,
                              long long num_tiles, hipStream_t s);
void text_debug_host(unsigned char *frame, const hh_text_desc &d, const hh_text_prim *prims, const uint8_t *atlas, const void *tiles, long long num_tiles);
// Segmentation overlays (hh_seg_desc and the shape rows of include/hhrnet.h; arithmetic, host walk and validation in seg_overlay_math.h,
// kernel in seg_overlay.hip): n frames in one launch, `max_tiles` = the largest frame's tile count.
hipError_t launch_seg_overlay(unsigned char *base, const hh_seg_desc *descs, const int32_t *shapes, const unsigned int *toggles, int n, int max_tiles, hipStream_t s);
// Baseline JPEG (hh_jpeg_desc of include/hhrnet.h; struct and arithmetic in jpeg_math.h, kernels in jpeg.hip): n frames in three
// launches, `max_mcus` / `max_rows` = the largest frame's MCU count / MCU rows.
hipError_t launch_jpeg_encode(unsigned char *base, const hh_jpeg_desc *descs, int n, int max_mcus, int max_rows, unsigned char *ws, int32_t *lengths,
                              hipStream_t s);
// Baseline JPEG decode (hh_jpeg_dec_desc of include/hhrnet.h; structs and arithmetic in jpeg_dec_math.h, kernels in jpeg_decode.hip): n
// streams in three launches behind the clearing of `status`.  Desc: JpegDecDesc (the whole image) or JpegWinDesc (hh_jpeg_win_desc: a
// window); the grids are sized by the largest count of (selected) segments, the largest MCU rectangle's blocks and the largest window.
template <class Desc>
hipError_t launch_jpeg_decode(unsigned char *base, const Desc *descs, int n, int max_seg, int max_blk, int max_h, int max_w, unsigned char *ws,
                              int32_t *status, hipStream_t s);
// The index of restart-less streams built on the device (jpeg_index.hip; the rule: hh_jpeg_index_device_batch in include/hhrnet.h): one
// launch, one workgroup per image, behind the clearing of `status`; it fills the entries of the table blocks that ask for it.
hipError_t launch_jpeg_index(unsigned char *base, const hh_jpeg_dec_desc *descs, int n, int mps, int subseq_bytes, int32_t *status, hipStream_t s);
// Heatmap panels (hh_panel_map of include/hhrnet.h; struct and arithmetic in panel_math.h, kernels in panels.hip): the min/max launch
// (only if any_minmax) and the paint launch of one figure; the same figure on the host; the un-normalise of the model input.
struct PanelRange;
hipError_t launch_panels(const hh_panel_map *maps, int n, bool any_minmax, const unsigned char *image, int H, int W, const unsigned char *lut,
                         unsigned char *canvas, int Hc, int Wc, long long pitch, float *parts, hipStream_t s);
void panels_debug_host(const hh_panel_map *maps, int n, const unsigned char *image, int H, int W, const unsigned char *lut, unsigned char *canvas, int Hc,
                       int Wc, long long pitch, PanelRange *ranges);
hipError_t launch_unnormalize_u8(const float *x, int H, int W, unsigned char *out, const double *mean, const double *stdv, hipStream_t s);
// COCO keypoint scoring (hh_coco_tables of include/hhrnet.h; struct, OKS and matching walk in coco_eval_math.h, kernel in coco_eval.hip):
// mode 0 = OKS + matching fused, 1 = OKS only into oks_out, 2 = matching only from oks_in; the same on the host.
hipError_t launch_coco_eval(int mode, const hh_coco_tables &dev, const double *oks_in, double *oks_out, int32_t *dt_match, uint8_t *dt_ignore, uint8_t *gt_ignore,
                            hipStream_t s);
void coco_eval_host(const hh_coco_tables &t, const double *oks_in, double *oks_out, bool match, int32_t *dt_match, uint8_t *dt_ignore, uint8_t *gt_ignore);
// Pose tracking across frames (hh_track_params of include/hhrnet.h; struct, state layout and per-slot / per-joint code in track_math.h, kernels in
// track.hip): S streams of F frames in one launch; the similarity matrices alone; the greedy assignment alone on n matrices; the step on the host.
hipError_t launch_track_step(const hh_track_params &p, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags, int S,
                             int F, int32_t *track_ids, float *smooth, int32_t *out_flags, hipStream_t s);
hipError_t launch_track_similarity(const hh_track_params &p, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags,
                                   int S, double *sim, hipStream_t s);
hipError_t launch_track_assign(const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, int32_t *match, hipStream_t s);
void track_step_host(const hh_track_params &p, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags, int S, int F,
                     int32_t *track_ids, float *smooth, int32_t *out_flags);
// Per-image OKS / PCKh against annotations behind the decode (hh_pose_score_batch of include/hhrnet.h; tables, arithmetic and validation in
// pose_score_math.h, kernel in pose_score.hip): B images in one launch, `max_P` = the largest prediction count an image can have (sizes
// the LDS); the same on the host.
struct PoseTables;
hipError_t launch_pose_score(const PoseTables &t, int max_P, double *value, double *obj, double *kpt, int32_t *match, int32_t *status, hipStream_t s);
void pose_score_host(const PoseTables &t, double *value, double *obj, double *kpt, int32_t *match, int32_t *status);
// Evaluation of the classifier (hh_cls_score_batch of include/hhrnet.h; layout, order and the host's row in cls_score_math.h, kernels in
// cls_score.hip): B <= HH_CLS_MAX_B rows in one launch, plus the one-wave fold when targets and an accumulator are given.
hipError_t launch_cls_eval_reset(void *acc, int N, int with_confusion, hipStream_t s);
hipError_t launch_cls_score(const float *logits, const long long *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob,
                            int32_t *rank, float *row_loss, hipStream_t s);
void cls_score_host(const float *logits, const long long *targets, int B, int N, int k, void *acc, int32_t *topk_idx, float *topk_prob, int32_t *rank,
                    float *row_loss);
// Crowd masks from toggle lists (hh_crowd_mask_desc / hh_crowd_seg_desc of include/hhrnet.h; structs, predicate, tile walk and the host's
// polygon walk in crowd_mask_math.h, kernel in crowd_mask.hip): n masks in one launch, `max_tiles` = the largest mask's tile count.
hipError_t launch_crowd_masks(unsigned char *base, const hh_crowd_mask_desc *descs, const hh_crowd_seg_desc *segs, int n, int max_tiles, hipStream_t s);
// target heatmaps from the packed joints (train_input.hip); n = table side = 2 * reach + 1 <= HH_RENDER_MAX_N, w <= HH_RENDER_MAX_W
#define HH_RENDER_MAX_N 63
#define HH_RENDER_MAX_W 4096
hipError_t launch_render_heatmaps(const int32_t *joints, const int32_t *num_people, int B, int P, int K, const float *table, int n, int reach,
                                  float *out, int h, int w, hipStream_t s);
hipError_t launch_flip_images(const float *in, float *out, int B, int C, int H, int W, hipStream_t s);
struct FlipPerm { unsigned char v[64]; };
hipError_t launch_flip_merge(float *hm, int64_t hm_bs, const float *hmf, int64_t hmf_bs, const float *tf, int64_t tf_bs,
                             float *to, int64_t to_bs, const int32_t *perm_host, int B, int K, int h, int w, hipStream_t s);

// Training loss (loss_kernels.hip).  scratch: >= max(HH_LOSS_SCRATCH, 2*B) doubles of device memory.
#define HH_LOSS_SCRATCH 1024
hipError_t launch_masked_mse(const float *pred, int64_t pred_bs, const float *target, const float *mask, int B, int K, int h, int w,
                             float *loss, float *grad, int64_t grad_bs, double *scratch, hipStream_t s);
hipError_t launch_ae_grouping(const float *tags, int64_t tags_bs, const int32_t *joints, const int32_t *num_people, int B, int P, int K,
                              int h, int w, float *push_pull, float *grad, int64_t grad_bs, float push_scale, float pull_scale,
                              double *scratch, hipStream_t s);

// Training building blocks (train_ops.hip)
#define HH_BN_BLOCKS 256  // partial-sum blocks of the BatchNorm reductions; scratch = HH_BN_BLOCKS * C * 2 doubles
// one weight set of a batched packing launch (launch_pack_weights_batch)
struct PackDesc {
    const float *W;
    bf16_raw *packed;
    long long total;
    int cout, cin, ks, mode, KC, COUT_T, py, px;
};
hipError_t launch_pack_weights_batch(const PackDesc *descs_dev, int n, hipStream_t s, int act_dtype = 0);
hipError_t launch_pack_weights(const float *W, int cout, int cin, int ks, int mode, int KC, int COUT_T, bf16_raw *packed, size_t total,
                               hipStream_t s, int py = 0, int px = 0, int act_dtype = 0);
hipError_t launch_bn_train_forward(const bf16_raw *x, int cs, size_t P, int C, const float *gamma, const float *beta, float eps,
                                   const bf16_raw *res, int relu, bf16_raw *y, float *mean, float *invstd, double *scratch, hipStream_t s, int act_dtype = 0);
hipError_t launch_bn_train_backward(const bf16_raw *x, const bf16_raw *y, const bf16_raw *dy, int cs, size_t P, int C, const float *mean,
                                    const float *invstd, const float *gamma, const float *beta, int relu, bf16_raw *dx, bf16_raw *dres,
                                    float *dgamma, float *dbeta, double *scratch, hipStream_t s, int act_dtype = 0);  // y == nullptr: no residual, mask from x
hipError_t launch_bn_train_stats(const bf16_raw *x, int cs, size_t P, int C, double *sums, double *scratch, hipStream_t s, int act_dtype = 0);
hipError_t launch_bn_train_normalize(const bf16_raw *x, int cs, size_t P, int C, const double *sums, double count, const float *gamma,
                                     const float *beta, float eps, const bf16_raw *res, int relu, bf16_raw *y, float *mean, float *invstd,
                                     hipStream_t s, int act_dtype = 0);
hipError_t launch_bn_train_backward_stats(const bf16_raw *x, const bf16_raw *y, const bf16_raw *dy, int cs, size_t P, int C, const float *mean,
                                          const float *invstd, int relu, double *sums, float *dgamma, float *dbeta, double *scratch,
                                          hipStream_t s, int act_dtype = 0);
hipError_t launch_bn_train_backward_apply(const bf16_raw *x, const bf16_raw *y, const bf16_raw *dy, int cs, size_t P, int C, const float *mean,
                                          const float *invstd, const float *gamma, int relu, const double *sums, double count, bf16_raw *dx,
                                          bf16_raw *dres, double *scratch, hipStream_t s, int act_dtype = 0);

// Convolution weight gradient (conv_wgrad.hip): ks in {1,3} x stride 1, and 3x3 stride 2; channels multiples of 8
struct WgradParams {
    const bf16_raw *x;   // [B,H,W,cin]
    const bf16_raw *dy;  // [B,Ho,Wo,cout]
    float *partial;      // workspace: workers * ks*ks * roundup(cout,64) * roundup(cin,64) floats
    int B, H, W, Ho, Wo, cin, cout;
    int pad_y, pad_x;    // top / left zero padding of x
};
#define HH_WGRAD_WORKERS 128  // base count of persistent pixel-tile workers per channel block (64 .. 512, see conv_wgrad_num_workers)
int conv_wgrad_num_workers(int B, int Ho, int Wo, int ks, int stride, int cin, int cout);
int conv_wgrad_num_tiles(int B, int Ho, int Wo, int variant);  // with the tile width of that variant's kernel
int conv_wgrad_variant(int ks, int stride, int Wo, int cin, int cout);  // 0..5 (conv_wgrad.hip), -1: no kernel
hipError_t conv_wgrad_launch(const WgradParams &p, int ks, int stride, float *dw, hipStream_t s, int act_dtype = 0);

// Device optimizer step (optim.hip): one launch over a device-resident table.  The table's structs and the arithmetic are in
// optim_math.h (shared with a host build).
struct OptimChunk;
hipError_t launch_optim_step(int algo, const hh_optim_tensor *tensors, int ntensors, const hh_optim_group *groups, const OptimChunk *chunks, int nchunks,
                             const float *grad_scale, const float *found_inf, int advance_steps, hipStream_t s);
hipError_t launch_grads_nonfinite(const hh_optim_tensor *tensors, const OptimChunk *chunks, int nchunks, const float *inv_scale, float *found_inf,
                                  hipStream_t s);
// Gradient statistics and clipping by global norm over the same table (grad_stats.hip; arithmetic and the workspace's layout in
// grad_stats_math.h).  `work` is the device workspace of grad_work_bytes(ntensors, nchunks).
hipError_t launch_grad_stats(const hh_optim_tensor *tensors, int ntensors, const OptimChunk *chunks, int nchunks, const float *inv_scale,
                             float *found_inf, void *work, hipStream_t s);
hipError_t launch_grad_clip(const hh_optim_tensor *tensors, int ntensors, const OptimChunk *chunks, int nchunks, float max_norm, int norm_type,
                            const float *found_inf, void *work, hipStream_t s);
// Weight EMA (ema.hip; arithmetic in ema_math.h): the optimizer step with the average as a fifth stream plus `nonly` chunks of rows the
// optimizer does not step, the stand-alone update, and the swap.  The update launches are followed by the one-workgroup tail that
// advances the counters.
hipError_t launch_optim_step_ema(int algo, const hh_optim_tensor *tensors, int ntensors, const hh_optim_group *groups, const OptimChunk *chunks, int nchunks,
                                 const float *grad_scale, const float *found_inf, int advance_steps, const hh_ema_row *rows, const int *row_of,
                                 const OptimChunk *only_chunks, int nonly, double decay, int warmup, long long *n_averaged, hipStream_t s);
hipError_t launch_ema_update(const hh_ema_row *rows, const OptimChunk *chunks, int nchunks, double decay, int warmup, long long *n_averaged,
                             const float *found_inf, hipStream_t s);
hipError_t launch_ema_swap(const hh_ema_row *rows, const OptimChunk *chunks, int nchunks, hipStream_t s);
