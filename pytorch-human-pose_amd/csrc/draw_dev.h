// Device-side pieces shared by the uint8 drawing kernels (render, text, seg_overlay, panels, train_mosaic): the tile of host_dev.h
// seen from one thread, the cull of a chunk of items against a tile, and the two forms a thread keeps its four RGB pixels in.  One
// definition each, all __forceinline__; tools/isa_diff.py compares a kernel's code with what it was with the piece written out.
#ifndef HH_DRAW_DEV_H
#define HH_DRAW_DEV_H
#include <stdint.h>
#include "host_dev.h"

// ---- the tile: tile `tile` of the xtiles tiles across an h x w frame, and thread tid's DRAW_PX pixels of it
// -> the tile's bounds (inclusive, clipped to the frame), the thread's row and first column, its pixels inside the frame (<= 0: none)
struct DrawTile { int ty0, tx0, ty1, tx1, y, x, npx; };
template <class Index>  // blockIdx.x (unsigned) or an entry of a tile list (int): the division stays in the index's own type
__device__ __forceinline__ DrawTile draw_tile(Index tile, int xtiles, int h, int w, int tid)
{
    DrawTile t;
    t.ty0 = (int)(tile / xtiles) * DRAW_TH, t.tx0 = (int)(tile % xtiles) * DRAW_TW;
    t.ty1 = min(t.ty0 + DRAW_TH, h) - 1, t.tx1 = min(t.tx0 + DRAW_TW, w) - 1;
    t.y = t.ty0 + tid / (DRAW_TW / DRAW_PX), t.x = t.tx0 + (tid % (DRAW_TW / DRAW_PX)) * DRAW_PX;
    t.npx = (t.y <= t.ty1) ? min(DRAW_PX, t.tx1 - t.x + 1) : 0;
    return t;
}

// ---- the cull: each lane of a workgroup of WAVES waves has tested one item (`keep`); the kept ones get consecutive slots of a list
// in LDS.  Slots ascend with the thread index = the item's index in its table, so the list is in draw order: every thread walks it
// front to back, a later hit overwriting an earlier one (the byte-exact tests hinge on it).  A ballot orders the lanes of a wave,
// the waves' counts are prefixed through wave_count[WAVES] in LDS.  -> this lane's slot (< total; -1: it keeps nothing) and the
// workgroup's total.  The barrier between the counts and their sums is in here; the caller stores what it keeps per slot and
// closes with its own barrier before the list is read, and with another before the next cull overwrites list and counts.
struct DrawSlot { int slot, total; };
template <int WAVES>
__device__ __forceinline__ DrawSlot draw_cull_slot(bool keep, int lane, int wave, int *wave_count)
{
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) {
        const int c = wave_count[v];
        before += v < wave ? c : 0;
        total += c;
    }
    return DrawSlot{keep ? before + (int)__popcll(m & ((1ull << lane) - 1ull)) : -1, total};
}

// ---- pixel groups as bytes (render's blend, panels, the resizes): N dwords <-> 4 N bytes of a thread's byte array, little-endian, at
// a 4-byte aligned address.  The array is reached through an accessor, [&](int i) { return px[i]; }: handed over as a pointer it
// is promoted to registers along another path and the kernel's code changes.  For the same reason the callers keep their own "whole
// group and aligned, else byte by byte" (with the byte loop in here resize_u8_kernel<3> goes from 70 to 61 VGPRs, paint from 54 to 53).
__device__ __forceinline__ uint32_t draw_pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) { return b0 | b1 << 8 | b2 << 16 | b3 << 24; }
template <int N, class Get>
__device__ __forceinline__ void draw_store_dwords(unsigned char *o, Get get)
{
    uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
#pragma unroll
    for (int q = 0; q < N; ++q) o4[q] = draw_pack4(get(q * 4), get(q * 4 + 1), get(q * 4 + 2), get(q * 4 + 3));
}
template <int N, class Put>
__device__ __forceinline__ void draw_load_dwords(const unsigned char *p, Put put)
{
    const uint32_t *p4 = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const uint32_t v = p4[q];
        put(q * 4, v & 255), put(q * 4 + 1, (v >> 8) & 255), put(q * 4 + 2, (v >> 16) & 255), put(q * 4 + 3, v >> 24);
    }
}

// ---- pixel groups as words: a pixel is r | g << 8 | b << 16, as text and seg keep theirs
__device__ __forceinline__ uint32_t draw_load_px(const unsigned char *p) { return p[0] | p[1] << 8 | p[2] << 16; }
__device__ __forceinline__ void draw_store_px(unsigned char *p, uint32_t v) { p[0] = v & 255, p[1] = v >> 8 & 255, p[2] = v >> 16 & 255; }

// Four pixels from and to their 12 bytes at a 4-byte aligned `p`: one dwordx3 access.  The store takes an accessor as above.
struct DrawWide { uint32_t a, b, c; };
struct DrawPx4 { uint32_t v[4]; };
__device__ __forceinline__ DrawPx4 draw_load_px4(const unsigned char *p)
{
    const DrawWide q = *reinterpret_cast<const DrawWide *>(p);
    return DrawPx4{{q.a & 0xffffffu, (q.a >> 24) | (q.b & 0xffffu) << 8, (q.b >> 16) | (q.c & 0xffu) << 16, q.c >> 8}};
}
template <class Get>
__device__ __forceinline__ void draw_store_px4(unsigned char *p, Get get)
{
    *reinterpret_cast<DrawWide *>(p) = DrawWide{get(0) | get(1) << 24, get(1) >> 8 | get(2) << 16, get(2) >> 16 | get(3) << 8};
}
#endif
