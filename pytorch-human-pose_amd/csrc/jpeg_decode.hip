// Baseline JPEG decoded on the GPU for a batch of streams of mixed sizes, samplings and tables: three launches per call, whatever the
// batch.  The rule is stated at hh_jpeg_decode_u8_batch in include/hhrnet.h; its arithmetic is jpeg_dec_math.h, shared with the host.
//
// jpeg_dec_entropy_kernel: one lane per segment, a workgroup's 64 lanes from one image (blockIdx.z), neighbouring lanes on neighbouring
// segments.  The image's eight Huffman tables are copied to LDS once per workgroup; a lane walks its MCUs with a 64-bit bit buffer
// (jpeg_dec_segment) and writes int16 coefficients in natural order.  Bounds are structural: the reader never passes the segment's
// end, itself cut to the scan's end and the stream's length; a segment's MCU range is cut to the image's grid.  A violation raises
// status[image] and ends the lane.
//
// jpeg_dec_idct_kernel: 8 lanes per block, 32 blocks per workgroup.  Lane t of a block dequantises and transforms column t into LDS
// (block stride 72 words: the column writes of a 32-lane group fall on 32 banks), then transforms row t and stores its 8 samples as
// one 8-byte vector into the component's plane.
//
// jpeg_dec_colour_kernel: one lane per output pixel: fancy upsampling of the two chroma planes at the components' true edges, the
// colour step, three bytes into the destination.
#include "kernels.h"
#include "jpeg_dec_math.h"

__device__ __forceinline__ const unsigned char *jpeg_dec_tables(const unsigned char *base, const JpegDecDesc &d) { return base + d.tables_offset; }

__global__ __launch_bounds__(64) void jpeg_dec_entropy_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                              const JpegDecDesc *__restrict__ descs, int32_t *__restrict__ status)
{
    __shared__ JpegHuff huff[8];
    const JpegDecDesc d = descs[blockIdx.z];
    if ((int)blockIdx.x * 64 >= d.nseg) return;  // (the whole workgroup: the grid is sized for the image with most segments)
    const unsigned char *tab = jpeg_dec_tables(base, d);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + JPEG_DEC_TABLES_AT + offsetof(JpegDecTables, huff));
    for (int i = threadIdx.x; i < (int)(sizeof(huff) / 4); i += 64) reinterpret_cast<uint32_t *>(huff)[i] = src[i];
    __syncthreads();
    const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (s >= d.nseg) return;
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    const JpegSegment sg = reinterpret_cast<const JpegSegment *>(tab + JPEG_DEC_SEGS_AT)[s];
    const int st = jpeg_dec_segment<true>(base + d.stream_offset, d.stream_length, I, huff, sg, reinterpret_cast<int16_t *>(ws + d.ws_offset), nullptr, nullptr);
    if (st) atomicMax(status + blockIdx.z, st);
}

__global__ __launch_bounds__(8 * JPEG_DEC_IDCT_BLOCKS) void jpeg_dec_idct_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                                                 const JpegDecDesc *__restrict__ descs)
{
    __shared__ int32_t tmp[JPEG_DEC_IDCT_BLOCKS * JPEG_DEC_LDS_STRIDE];
    const JpegDecDesc d = descs[blockIdx.z];
    const unsigned char *tab = jpeg_dec_tables(base, d);
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    const JpegDecGeom g = jpeg_dec_geom(I);
    if ((int)blockIdx.x * JPEG_DEC_IDCT_BLOCKS >= g.nblk) return;  // (the whole workgroup)
    const int t = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int blk = (int)blockIdx.x * JPEG_DEC_IDCT_BLOCKS + lb;
    const bool have = blk < g.nblk;
    unsigned char *iws = ws + d.ws_offset;
    int c = 0;
    long long at = 0;
    if (have) {
        jpeg_dec_block_place(I, g, blk, c, at);
        const uint16_t *q = reinterpret_cast<const uint16_t *>(tab + JPEG_DEC_TABLES_AT) + (I.qt[c] & 3) * 64;
        jpeg_idct_col(reinterpret_cast<const int16_t *>(iws) + (size_t)blk * 64, q, t, tmp + lb * JPEG_DEC_LDS_STRIDE);
    }
    __syncthreads();
    if (have) {
        // row t of the block: 8 bytes at a multiple of 8 inside the plane (plane_at and pw are multiples of 8)
        *reinterpret_cast<JpegRow8 *>(iws + at + (size_t)t * g.pw[c]) = jpeg_idct_row(tmp + lb * JPEG_DEC_LDS_STRIDE + t * 8);
    }
}

__global__ __launch_bounds__(256) void jpeg_dec_colour_kernel(unsigned char *__restrict__ base, const unsigned char *__restrict__ ws,
                                                              const JpegDecDesc *__restrict__ descs)
{
    const JpegDecDesc d = descs[blockIdx.z];
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(jpeg_dec_tables(base, d));
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (x >= I.w || y >= I.h) return;
    const JpegDecGeom g = jpeg_dec_geom(I);
    jpeg_dec_pixel(ws + d.ws_offset, I, g, y, x, d.flags & 1, base + d.dst_offset + (size_t)y * (size_t)d.pitch + (size_t)x * 3);
}

hipError_t launch_jpeg_decode(unsigned char *base, const JpegDecDesc *descs, int n, int max_seg, int max_blk, int max_h, int max_w, unsigned char *ws,
                              int32_t *status, hipStream_t s)
{
    hipLaunchKernelGGL(jpeg_dec_entropy_kernel, dim3((max_seg + 63) / 64, 1, n), dim3(64), 0, s, base, ws, descs, status);
    hipLaunchKernelGGL(jpeg_dec_idct_kernel, dim3((max_blk + JPEG_DEC_IDCT_BLOCKS - 1) / JPEG_DEC_IDCT_BLOCKS, 1, n), dim3(8 * JPEG_DEC_IDCT_BLOCKS), 0, s,
                       base, ws, descs);
    hipLaunchKernelGGL(jpeg_dec_colour_kernel, dim3((max_w + 63) / 64, (max_h + 3) / 4, n), dim3(64, 4), 0, s, base, ws, descs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- window decode
// hh_jpeg_decode_window_u8_batch: the same three launches over a window's MCU rectangle (jpeg_win_rect).  The table block holds only
// the segments with an MCU in the rectangle, and the stream is the slice they need, offsets rebased to it (jpeg_win_tables): a lane
// walks its segment from its first MCU to its last MCU inside the rectangle and stores only the MCUs inside; the IDCT covers the
// rectangle's blocks, the colour launch the window's pixels.  Coefficients and planes are laid out for the rectangle (jpeg_win_geom).
__global__ __launch_bounds__(64) void jpeg_win_entropy_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                              const JpegWinDesc *__restrict__ descs, int32_t *__restrict__ status)
{
    __shared__ JpegHuff huff[8];
    const JpegWinDesc wd = descs[blockIdx.z];
    const JpegDecDesc &d = wd.d;
    if ((int)blockIdx.x * 64 >= d.nseg) return;  // (the whole workgroup: the grid is sized for the image with most selected segments)
    const unsigned char *tab = jpeg_dec_tables(base, d);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + JPEG_DEC_TABLES_AT + offsetof(JpegDecTables, huff));
    for (int i = threadIdx.x; i < (int)(sizeof(huff) / 4); i += 64) reinterpret_cast<uint32_t *>(huff)[i] = src[i];
    __syncthreads();
    const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (s >= d.nseg) return;
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    const JpegSegment sg = reinterpret_cast<const JpegSegment *>(tab + JPEG_DEC_SEGS_AT)[s];
    const int st = jpeg_dec_window_segment(base + d.stream_offset, d.stream_length, I, huff, sg, jpeg_win_rect(I, wd.win),
                                           reinterpret_cast<int16_t *>(ws + d.ws_offset), nullptr, nullptr);
    if (st) atomicMax(status + blockIdx.z, st);
}

__global__ __launch_bounds__(8 * JPEG_DEC_IDCT_BLOCKS) void jpeg_win_idct_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                                                 const JpegWinDesc *__restrict__ descs)
{
    __shared__ int32_t tmp[JPEG_DEC_IDCT_BLOCKS * JPEG_DEC_LDS_STRIDE];
    const JpegWinDesc wd = descs[blockIdx.z];
    const unsigned char *tab = jpeg_dec_tables(base, wd.d);
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    const JpegWinRect R = jpeg_win_rect(I, wd.win);
    const JpegDecGeom g = jpeg_win_geom(I, R);
    if ((int)blockIdx.x * JPEG_DEC_IDCT_BLOCKS >= g.nblk) return;  // (the whole workgroup)
    const int t = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int blk = (int)blockIdx.x * JPEG_DEC_IDCT_BLOCKS + lb;
    const bool have = blk < g.nblk;
    unsigned char *iws = ws + wd.d.ws_offset;
    int c = 0;
    long long at = 0;
    if (have) {
        jpeg_win_block_place(I, R, g, blk, c, at);
        const uint16_t *q = reinterpret_cast<const uint16_t *>(tab + JPEG_DEC_TABLES_AT) + (I.qt[c] & 3) * 64;
        jpeg_idct_col(reinterpret_cast<const int16_t *>(iws) + (size_t)blk * 64, q, t, tmp + lb * JPEG_DEC_LDS_STRIDE);
    }
    __syncthreads();
    if (have) *reinterpret_cast<JpegRow8 *>(iws + at + (size_t)t * g.pw[c]) = jpeg_idct_row(tmp + lb * JPEG_DEC_LDS_STRIDE + t * 8);
}

__global__ __launch_bounds__(256) void jpeg_win_colour_kernel(unsigned char *__restrict__ base, const unsigned char *__restrict__ ws,
                                                              const JpegWinDesc *__restrict__ descs)
{
    const JpegWinDesc wd = descs[blockIdx.z];
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (x >= wd.win.width || y >= wd.win.height) return;
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(jpeg_dec_tables(base, wd.d));
    const JpegWinRect R = jpeg_win_rect(I, wd.win);
    jpeg_win_pixel(ws + wd.d.ws_offset, I, R, jpeg_win_geom(I, R), wd.win.top + y, wd.win.left + x, wd.d.flags & 1,
                   base + wd.d.dst_offset + (size_t)y * (size_t)wd.d.pitch + (size_t)x * 3);
}

hipError_t launch_jpeg_decode_window(unsigned char *base, const JpegWinDesc *descs, int n, int max_seg, int max_blk, int max_h, int max_w,
                                     unsigned char *ws, int32_t *status, hipStream_t s)
{
    hipLaunchKernelGGL(jpeg_win_entropy_kernel, dim3((max_seg + 63) / 64, 1, n), dim3(64), 0, s, base, ws, descs, status);
    hipLaunchKernelGGL(jpeg_win_idct_kernel, dim3((max_blk + JPEG_DEC_IDCT_BLOCKS - 1) / JPEG_DEC_IDCT_BLOCKS, 1, n), dim3(8 * JPEG_DEC_IDCT_BLOCKS), 0, s,
                       base, ws, descs);
    hipLaunchKernelGGL(jpeg_win_colour_kernel, dim3((max_w + 63) / 64, (max_h + 3) / 4, n), dim3(64, 4), 0, s, base, ws, descs);
    return hipGetLastError();
}
