// Text labels on the GPU: put_txt of the reference (utils/image.py:64-119) for a batch of uint8 [h,w,3] frames of mixed sizes in ONE
// launch, in place, on the frames where the render and resize launches left them.  The rule (the two primitive kinds, their pixel
// arithmetic, the order) is stated at hh_text_labels_u8_batch in include/hhrnet.h; its arithmetic is text_math.h, shared with the
// host.  The host forms the primitive table (keypoints/text.py layout_put_txt), one descriptor per frame and the list of the tiles
// that some primitive touches (text_list_tiles): work scales with the labelled area, not with the frame.
//
// text_labels_kernel: a workgroup of 256 threads owns one listed TEXT_TH x TEXT_TW = 16 x 64 tile of one frame, a thread TEXT_PX = 4
// horizontally adjacent pixels of it.  The frame's primitives are walked TEXT_CHUNK = 256 at a time exactly as render_poses_kernel
// walks its own: each lane tests one primitive's box against the tile, the survivors are compacted into LDS in draw order (ballot
// within a wave, the four waves' counts prefixed through LDS), and every thread walks that list, all lanes reading the same entry at
// the same time (an LDS broadcast).  A thread keeps its pixels in registers across the list and across chunks, so the draw order holds
// within and across chunks and the list never needs more than one chunk of room (8 KB).  A pixel is loaded when the first primitive
// that covers it is applied and stored at the end only if it was loaded: a pixel that no primitive covers is neither read nor
// written, and every covered byte is written exactly once by exactly one thread (the tile list names no tile twice).  Frames are
// tightly packed, any alignment: dword loads and stores where a primitive covers all four pixels of a thread and their 12 bytes are
// 4-byte aligned, bytes otherwise.  The coverage bytes are read from global memory: 30 KB for the whole atlas, a glyph's rows are
// adjacent bytes read by adjacent lanes.
#include "kernels.h"
#include "text_math.h"

#define TEXT_WAVES (TEXT_THREADS / 64)

__global__ __launch_bounds__(TEXT_THREADS) void text_labels_kernel(unsigned char *base, const TextDesc *__restrict__ descs, const TextPrim *__restrict__ prims,
                                                                   const uint8_t *__restrict__ atlas, const TextTile *__restrict__ tiles)
{
    __shared__ TextPrim list[TEXT_CHUNK];
    __shared__ int wave_count[TEXT_WAVES];
    const TextTile t = tiles[blockIdx.x];
    const TextDesc d = descs[t.frame];
    const int xtiles = text_xtiles(d.w);
    const int ty0 = t.tile / xtiles * TEXT_TH, tx0 = t.tile % xtiles * TEXT_TW;  // inside the frame: checked on the host
    const int ty1 = min(ty0 + TEXT_TH, d.h) - 1, tx1 = min(tx0 + TEXT_TW, d.w) - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y = ty0 + tid / (TEXT_TW / TEXT_PX), x = tx0 + (tid % (TEXT_TW / TEXT_PX)) * TEXT_PX;
    const int npx = (y <= ty1) ? min(TEXT_PX, tx1 - x + 1) : 0;  // pixels of this thread inside the frame (<= 0: none)
    // y < h and x + e < w for e < npx, so every byte touched below is inside the frame's h * w * 3
    unsigned char *ptr = base + d.src_offset + ((size_t)(npx > 0 ? y : 0) * d.w + (npx > 0 ? x : 0)) * 3;
    const bool wide = npx == TEXT_PX && ((uintptr_t)ptr & 3) == 0;
    uint32_t px[TEXT_PX];  // r | g << 8 | b << 16 of the pixels loaded so far
#pragma unroll
    for (int e = 0; e < TEXT_PX; ++e) px[e] = 0;
    unsigned loaded = 0;

    for (int chunk = 0; chunk < d.prim_count; chunk += TEXT_CHUNK) {  // (uniform over the workgroup)
        const int i = chunk + tid;
        TextPrim mine;
        bool keep = false;
        if (i < d.prim_count) {  // prim_offset + i < the table's length: checked on the host
            mine = prims[d.prim_offset + i];
            keep = render_box_meets(mine, tx0, ty0, tx1, ty1);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_count[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < TEXT_WAVES; ++v) {
            const int c = wave_count[v];
            before += v < wave ? c : 0;
            total += c;
        }
        if (keep) list[before + __popcll(m & ((1ull << lane) - 1ull))] = mine;  // < total <= TEXT_CHUNK
        __syncthreads();
        if (npx > 0)
            for (int k = 0; k < total; ++k) {
                const TextPrim p = list[k];
                if (y < p.y0 || y > p.y1 || x + npx - 1 < p.x0 || x > p.x1) continue;
                unsigned hit = 0;
#pragma unroll
                for (int e = 0; e < TEXT_PX; ++e) hit |= (e < npx && x + e >= p.x0 && x + e <= p.x1) ? 1u << e : 0u;
                const unsigned need = hit & ~loaded;
                if (need == (1u << TEXT_PX) - 1u && wide) {
                    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(ptr);
                    const uint32_t a = s4[0], b = s4[1], c = s4[2];
                    px[0] = a & 0xffffffu, px[1] = (a >> 24) | (b & 0xffffu) << 8, px[2] = (b >> 16) | (c & 0xffu) << 16, px[3] = c >> 8;
                } else if (need) {
#pragma unroll
                    for (int e = 0; e < TEXT_PX; ++e)
                        if (need >> e & 1) px[e] = ptr[e * 3] | ptr[e * 3 + 1] << 8 | ptr[e * 3 + 2] << 16;
                }
                loaded |= need;
#pragma unroll
                for (int e = 0; e < TEXT_PX; ++e)
                    if (hit >> e & 1) px[e] = text_apply(p, atlas, x + e, y, px[e]);
            }
        __syncthreads();  // the next chunk overwrites the list and the counts
    }
    if (!loaded) return;
    if (loaded == (1u << TEXT_PX) - 1u && wide) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(ptr);
        o4[0] = px[0] | px[1] << 24, o4[1] = px[1] >> 8 | px[2] << 16, o4[2] = px[2] >> 16 | px[3] << 8;
    } else {
#pragma unroll
        for (int e = 0; e < TEXT_PX; ++e)
            if (loaded >> e & 1) ptr[e * 3] = px[e] & 255, ptr[e * 3 + 1] = (px[e] >> 8) & 255, ptr[e * 3 + 2] = (px[e] >> 16) & 255;
    }
}

hipError_t launch_text_labels(unsigned char *base, const TextDesc *descs, const TextPrim *prims, const uint8_t *atlas, const void *tiles, long long num_tiles,
                              hipStream_t s)
{
    hipLaunchKernelGGL(text_labels_kernel, dim3((unsigned)num_tiles), dim3(TEXT_THREADS), 0, s, base, descs, prims, atlas, static_cast<const TextTile *>(tiles));
    return hipGetLastError();
}

void text_debug_host(unsigned char *frame, const TextDesc &d, const TextPrim *prims, const uint8_t *atlas, const void *tiles, long long num_tiles)
{
    TextPrim list[TEXT_CHUNK];
    for (long long i = 0; i < num_tiles; ++i) text_tile_host(frame, d, prims, atlas, static_cast<const TextTile *>(tiles)[i].tile, list);
}
