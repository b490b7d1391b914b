"""The reference of the device-composed mosaic (hh_mosaic_u8_batch, keypoints/train_input.py): a numpy restatement of
cv2.resize(src, (S, S)) for 8-bit sources as include/hhrnet.h states it at hh_mosaic_u8_batch (OpenCV 4.x resize.cpp, INTER_LINEAR with
11-bit weights and the INTER_AREA shortcut at an exact factor of 2 on both axes), and `mosaic_reference`, the mosaic of
keypoints/datasets/coco.py:300-370 written straight from the reference with that resize.

cv2 is not installed where the fixtures are made: parity of the resized pixels with cv2 itself is UNPINNED, as for
oracle.transforms.warp_affine.  Shared by tests/test_train_mosaic_cpu.py, tests/test_gpu_train_mosaic.py,
tools/make_train_mosaic_golden.py (which binds cv2.resize to `resize`) and tools/train_input_time.py."""
import numpy as np

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS  # INTER_RESIZE_COEF_SCALE = 2048


def axis_taps(dst: int, src: int, column: bool):
    """-> (i0, i1, w0, w1) int32 [dst]: the two source indices and their weights of every destination index on one axis.  Columns
    zero the fraction at the borders; rows keep it and clamp the indices instead."""
    scale = 1.0 / (float(dst) / src)                                   # double
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)                    # (float)((dx + 0.5) * scale - 0.5): product and difference in double
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)                                        # fp32
    if column:
        low, high = s < 0, s >= src - 1
        s = np.where(low, 0, np.where(high, src - 1, s)).astype(np.int32)
        f = np.where(low | high, np.float32(0), f).astype(np.float32)
        i0, i1 = s, np.minimum(s + 1, src - 1)
    else:
        i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    w0 = np.rint((np.float32(1) - f) * np.float32(COEF_ONE)).astype(np.int16).astype(np.int32)  # cvRound: half to even; stored as shorts
    w1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int16).astype(np.int32)
    return i0.astype(np.int32), i1.astype(np.int32), w0, w1


def bilinear(s: np.ndarray, W: int, H: int) -> np.ndarray:
    """The two fixed-point passes on an int32 [h,w,c] array -> int32 [H,W,c]."""
    h, w = s.shape[:2]
    x0, x1, a0, a1 = axis_taps(W, w, True)
    y0, y1, b0, b1 = axis_taps(H, h, False)
    hor = s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]           # [h,W,c] int
    h0, h1 = hor[y0], hor[y1]
    return (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2


def area_2x2(s: np.ndarray) -> np.ndarray:
    """INTER_AREA at a factor of exactly 2 on both axes: the rounded mean of every 2 x 2 block."""
    return (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2


def resize(src, dsize, *args, **kwargs) -> np.ndarray:
    """cv2.resize(src, (width, height)) for a uint8 [h,w] or [h,w,c] array, INTER_LINEAR (the default: the reference passes nothing
    else, coco.py:327-328)."""
    assert not args and not kwargs, "only cv2.resize(src, dsize) is restated"
    src = np.ascontiguousarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    W, H = int(dsize[0]), int(dsize[1])
    h, w = src.shape[:2]
    s = src.reshape(h, w, -1).astype(np.int32)
    out = area_2x2(s) if h == 2 * H and w == 2 * W else bilinear(s, W, H)  # both scales exactly 2: OpenCV switches to INTER_AREA
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape((H, W) + src.shape[2:])


def mosaic_reference(tiles, S: int):
    """get_raw_mosaiced_data (coco.py:300-370) on four raw samples (uint8 [h,w,3] image, bool [h,w] crowd mask, [P,K,3] joints, integer
    or float) -> (canvas uint8 [2S,2S,3], canvas mask bool [2S,2S], joints float64 [P_total,K,3]) with get_coco_joints' float64
    (coco.py:68-74) applied to the four tiles' people in tile order.  The inputs are not modified."""
    assert len(tiles) == 4
    canvas = np.zeros([2 * S, 2 * S, 3], dtype=np.uint8)
    canvas_mask = np.empty([2 * S, 2 * S], dtype=np.bool_)
    people = []
    for i, (img, mask, joints) in enumerate(tiles):
        img_h, img_w = img.shape[:2]
        s_y, s_x = (i // 2) * S, (i % 2) * S
        new_img = resize(img, (S, S))
        new_mask = resize((mask * 255).astype(np.uint8), (S, S)) > 0.5
        scale_y, scale_x = S / img_h, S / img_w
        for person in joints:
            kpts = np.array(person).reshape([-1, 3])  # keeps the dtype: an integer array truncates on assignment, as in the reference
            vis_mask = kpts[:, 2] <= 0
            kpts[:, 0] = kpts[:, 0] * scale_x + s_x
            kpts[:, 1] = kpts[:, 1] * scale_y + s_y
            kpts[vis_mask] = kpts[vis_mask] * 0
            people.append(kpts)
        canvas[s_y:s_y + S, s_x:s_x + S] = new_img
        canvas_mask[s_y:s_y + S, s_x:s_x + S] = new_mask
    K = next((np.asarray(t[2]).shape[1] for t in tiles if np.asarray(t[2]).ndim == 3), 17)
    joints = np.zeros((len(people), K, 3))
    for i, kpts in enumerate(people):
        joints[i] = kpts
    return canvas, canvas_mask, joints
