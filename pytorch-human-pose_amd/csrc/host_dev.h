// In front of every *_math.h, whose text compiles for the kernels and for the host (capi.cpp's hh_debug_* twins, the
// tools/*_host_check.cpp programs): the function qualifier and the rounding rule.  One definition each.
#ifndef HH_HOST_DEV_H
#define HH_HOST_DEV_H

#if defined(__HIPCC__)
#define HH_HD __host__ __device__ __forceinline__
#else
#define HH_HD inline
#endif
#if defined(__clang__)  // every floating-point operation rounds on its own, whatever the including file's flags
#pragma clang fp contract(off)
#endif

// The tile of render_poses, text_labels and panels_paint (draw_dev.h: draw_tile): a workgroup of DRAW_THREADS owns DRAW_TH x DRAW_TW
// pixels, a thread DRAW_PX adjacent ones of a row; the items to draw are culled against the tile one per lane.
enum { DRAW_TH = 16, DRAW_TW = 64, DRAW_PX = 4, DRAW_THREADS = DRAW_TH * DRAW_TW / DRAW_PX };
static_assert(DRAW_THREADS == 256 && DRAW_TW % DRAW_PX == 0, "one lane per item of a chunk, whole pixel groups per tile row");
#endif
