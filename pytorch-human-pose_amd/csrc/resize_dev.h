// The tap arithmetic of the 8-bit cv2.resize(src, (W, H)) stated at hh_mosaic_u8_batch in include/hhrnet.h (INTER_LINEAR with 11-bit
// weights), shared by the mosaic kernel (train_mosaic.hip) and the general resize (render.hip).  Both files are compiled with
// -ffp-contract=off: the product and the difference of the coordinate round separately.
#ifndef HH_RESIZE_DEV_H
#define HH_RESIZE_DEV_H

struct AxisTap {
    int i0, i1;  // the two source indices
    int w0, w1;  // their weights, sum 2048 (shorts in OpenCV)
};

// cv2.resize's INTER_LINEAR tap of destination index d on an axis of `src` source samples.  Columns zero the fraction at the
// borders; rows keep it and clamp the two indices instead (resize.cpp: the x loop of resize() and resizeGeneric_Invoker).
__device__ __forceinline__ AxisTap axis_tap(int d, int src, double scale, bool column)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    AxisTap t;
    if (column) {
        if (s < 0) s = 0, f = 0.f;
        if (s >= src - 1) s = src - 1, f = 0.f;
        t.i0 = s;
        t.i1 = min(s + 1, src - 1);
    } else {
        t.i0 = min(max(s, 0), src - 1);
        t.i1 = min(max(s + 1, 0), src - 1);
    }
    t.w0 = (int)(short)__float2int_rn((1.f - f) * 2048.f);  // cvRound: half to even
    t.w1 = (int)(short)__float2int_rn(f * 2048.f);
    return t;
}

__device__ __forceinline__ int vertical_pass(int h0, int h1, int b0, int b1) { return (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2; }

#endif
