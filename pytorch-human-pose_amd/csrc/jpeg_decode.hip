// Baseline JPEG decoded on the GPU for a batch of streams of mixed sizes, samplings and tables: three launches per call, whatever the
// batch.  The rule is stated at hh_jpeg_decode_u8_batch and hh_jpeg_decode_window_u8_batch in include/hhrnet.h; its arithmetic is
// jpeg_dec_math.h, shared with the host.
//
// A decode is the decode of a window's MCU rectangle (jpeg_win_rect): coefficients and planes are laid out for the rectangle
// (jpeg_dec_geom).  Each kernel is written once over the descriptor type: a JpegWinDesc carries its window, its table block holds only
// the segments with an MCU in the rectangle, and its stream is the slice they need, offsets rebased to it (jpeg_win_tables); a
// JpegDecDesc stands for the window that is the whole image, whose rectangle is the MCU grid.
//
// jpeg_dec_entropy_kernel: one lane per segment, a workgroup's 64 lanes from one image (blockIdx.z), neighbouring lanes on neighbouring
// segments.  The image's eight Huffman tables are copied to LDS once per workgroup; a lane walks its segment with a 64-bit bit buffer
// from its first MCU to its last MCU inside the rectangle (jpeg_dec_segment) and writes int16 coefficients in natural order for the
// MCUs inside.  Bounds are structural: the reader never passes the segment's end, itself cut to the scan's end and the stream's
// length; a segment's MCU range is cut to the image's grid.  A violation raises status[image] and ends the lane.
//
// jpeg_dec_idct_kernel: 8 lanes per block of the rectangle, 32 blocks per workgroup.  Lane t of a block dequantises and transforms
// column t into LDS (block stride 72 words: the column writes of a 32-lane group fall on 32 banks), then transforms row t and stores
// its 8 samples as one 8-byte vector into the component's plane.
//
// jpeg_dec_colour_kernel: one lane per pixel of the window: fancy upsampling of the two chroma planes at the components' true edges,
// the colour step, three bytes into the destination.
#include "kernels.h"
#include "jpeg_dec_math.h"

// What the two descriptor types say: the JpegDecDesc part, and the window.
__device__ __forceinline__ const JpegDecDesc &jpeg_desc(const JpegDecDesc &d) { return d; }
__device__ __forceinline__ const JpegDecDesc &jpeg_desc(const JpegWinDesc &wd) { return wd.d; }
__device__ __forceinline__ JpegWindow jpeg_desc_window(const JpegDecDesc &, const JpegStreamInfo &I) { return jpeg_full_window(I); }
__device__ __forceinline__ JpegWindow jpeg_desc_window(const JpegWinDesc &wd, const JpegStreamInfo &) { return wd.window; }

template <class Desc>
__global__ __launch_bounds__(64) void jpeg_dec_entropy_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                              const Desc *__restrict__ descs, int32_t *__restrict__ status)
{
    __shared__ JpegHuff huff[8];
    const Desc desc = descs[blockIdx.z];
    const JpegDecDesc &d = jpeg_desc(desc);
    if ((int)blockIdx.x * 64 >= d.nseg) return;  // (the whole workgroup: the grid is sized for the image with most segments)
    const unsigned char *tab = base + d.tables_offset;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + JPEG_DEC_TABLES_AT + offsetof(JpegDecTables, huff));
    for (int i = threadIdx.x; i < (int)(sizeof(huff) / 4); i += 64) reinterpret_cast<uint32_t *>(huff)[i] = src[i];
    __syncthreads();
    const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (s >= d.nseg) return;
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    if (I.reserved[0]) return;  // (the device index met an error in this stream and left its entries unfinished: jpeg_index.hip)
    const JpegSegment sg = reinterpret_cast<const JpegSegment *>(tab + JPEG_DEC_SEGS_AT)[s];
    const int st = jpeg_dec_segment(base + d.stream_offset, d.stream_length, I, huff, sg, jpeg_win_rect(I, jpeg_desc_window(desc, I)),
                                    reinterpret_cast<int16_t *>(ws + d.ws_offset), nullptr, nullptr);
    if (st) atomicMax(status + blockIdx.z, st);
}

template <class Desc>
__global__ __launch_bounds__(8 * JPEG_DEC_IDCT_BLOCKS) void jpeg_dec_idct_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                                                 const Desc *__restrict__ descs)
{
    __shared__ int32_t tmp[JPEG_DEC_IDCT_BLOCKS * JPEG_DEC_LDS_STRIDE];
    const Desc desc = descs[blockIdx.z];
    const JpegDecDesc &d = jpeg_desc(desc);
    const unsigned char *tab = base + d.tables_offset;
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    const JpegWinRect R = jpeg_win_rect(I, jpeg_desc_window(desc, I));
    const JpegDecGeom g = jpeg_dec_geom(I, R);
    if ((int)blockIdx.x * JPEG_DEC_IDCT_BLOCKS >= g.nblk) return;  // (the whole workgroup)
    const int t = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int blk = (int)blockIdx.x * JPEG_DEC_IDCT_BLOCKS + lb;
    const bool have = blk < g.nblk;
    unsigned char *iws = ws + d.ws_offset;
    int c = 0;
    long long at = 0;
    if (have) {
        jpeg_dec_block_place(I, R, g, blk, c, at);
        const uint16_t *q = reinterpret_cast<const uint16_t *>(tab + JPEG_DEC_TABLES_AT) + (I.qt[c] & 3) * 64;
        jpeg_idct_col(reinterpret_cast<const int16_t *>(iws) + (size_t)blk * 64, q, t, tmp + lb * JPEG_DEC_LDS_STRIDE);
    }
    __syncthreads();
    if (have) {
        // row t of the block: 8 bytes at a multiple of 8 inside the plane (plane_at and pw are multiples of 8)
        *reinterpret_cast<JpegRow8 *>(iws + at + (size_t)t * g.pw[c]) = jpeg_idct_row(tmp + lb * JPEG_DEC_LDS_STRIDE + t * 8);
    }
}

template <class Desc>
__global__ __launch_bounds__(256) void jpeg_dec_colour_kernel(unsigned char *__restrict__ base, const unsigned char *__restrict__ ws,
                                                              const Desc *__restrict__ descs)
{
    const Desc desc = descs[blockIdx.z];
    const JpegDecDesc &d = jpeg_desc(desc);
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(base + d.tables_offset);
    const JpegWindow W = jpeg_desc_window(desc, I);
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * 4 + (int)threadIdx.y;
    if (x >= W.width || y >= W.height) return;
    const JpegWinRect R = jpeg_win_rect(I, W);
    jpeg_dec_pixel(ws + d.ws_offset, I, R, jpeg_dec_geom(I, R), W.top + y, W.left + x, d.flags & 1,
                   base + d.dst_offset + (size_t)y * (size_t)d.pitch + (size_t)x * 3);
}

template <class Desc>
hipError_t launch_jpeg_decode(unsigned char *base, const Desc *descs, int n, int max_seg, int max_blk, int max_h, int max_w, unsigned char *ws,
                              int32_t *status, hipStream_t s)
{
    hipLaunchKernelGGL(jpeg_dec_entropy_kernel<Desc>, dim3((max_seg + 63) / 64, 1, n), dim3(64), 0, s, base, ws, descs, status);
    hipLaunchKernelGGL(jpeg_dec_idct_kernel<Desc>, dim3((max_blk + JPEG_DEC_IDCT_BLOCKS - 1) / JPEG_DEC_IDCT_BLOCKS, 1, n), dim3(8 * JPEG_DEC_IDCT_BLOCKS), 0,
                       s, base, ws, descs);
    hipLaunchKernelGGL(jpeg_dec_colour_kernel<Desc>, dim3((max_w + 63) / 64, (max_h + 3) / 4, n), dim3(64, 4), 0, s, base, ws, descs);
    return hipGetLastError();
}
template hipError_t launch_jpeg_decode<JpegDecDesc>(unsigned char *, const JpegDecDesc *, int, int, int, int, int, unsigned char *, int32_t *, hipStream_t);
template hipError_t launch_jpeg_decode<JpegWinDesc>(unsigned char *, const JpegWinDesc *, int, int, int, int, int, unsigned char *, int32_t *, hipStream_t);
