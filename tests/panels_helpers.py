"""Shared by tests/test_panels_cpu.py and tests/test_gpu_panels.py: the lattice of heatmap-panel figures.

A figure of the lattice has one grid per source kind (DIRECT, SINGLE, NESTED, AVERAGE), K maps each, so that every figure mixes all four
value paths; the flags of map k of kind j in case c are (k + j + c) % 4, which walks neither / clip / min-max / both through every
kind.  Sizes (hq, wq) in {(8, 12), (16, 16), (5, 7)} with H = 4 hq, W = 4 wq: cells narrower than a paint tile, exactly one tile wide,
and several tiles with origins that are odd in bytes (pad = 5).  K in {1, 3, 17}, nrows in {1, 2}: K = 3 with two rows leaves a cell
unused.  Maps come from a seeded generator around 0.3 with sigma 0.8: values below 0 and above 1.  In the K = 17 figures the first
three maps of every kind are a constant map (min-max gives 0 / 0), a map with one NaN and a map with +inf and -inf, as DIRECT maps and
as sources of every resample.  The `kind*_flags*` cases are one kind with one flag setting and just those three special maps."""
import numpy as np

import panels_ref as pr

SIZES = [(8, 12), (16, 16), (5, 7)]
KS = [1, 3, 17]
NROWS = [1, 2]
PAD = 5


def image_of(H, W, seed):
    return np.random.default_rng(7000 + 131 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def special(a, which):
    """which 0: constant, 1: one NaN, 2: +inf and -inf; otherwise unchanged."""
    a = a.copy()
    h, w = a.shape
    if which == 0:
        a[:] = np.float32(0.37)
    elif which == 1:
        a[h // 2, w // 3] = np.nan
    elif which == 2:
        a[h // 3, w // 2] = np.inf
        a[h - 1, 0] = -np.inf
    return a


def maps_of(kind, K, hq, wq, rng, flags_of, specials):
    """K maps of one kind as (kind, src, src2, flags)."""
    out = []
    for k in range(K):
        shape = (4 * hq, 4 * wq) if kind == pr.DIRECT else (hq, wq)
        src = rng.normal(0.3, 0.8, shape).astype(np.float32)
        if specials:
            src = special(src, k)
        src2 = rng.normal(0.3, 0.8, (2 * hq, 2 * wq)).astype(np.float32) if kind == pr.AVERAGE else None
        out.append((kind, src, src2, flags_of(k)))
    return out


def lattice():
    """-> list of (name, image [H,W,3], grids) with grids = [(maps, nrows, pad)]."""
    out = []
    c = 0
    for hq, wq in SIZES:
        for K in KS:
            for nrows in NROWS:
                rng = np.random.default_rng(100 * c + 17)
                grids = [(maps_of(kind, K, hq, wq, rng, lambda k, j=kind, c=c: (k + j + c) % 4, K >= 17), nrows, PAD) for kind in range(4)]
                out.append((f"mixed_{hq}x{wq}_K{K}_r{nrows}", image_of(4 * hq, 4 * wq, c), grids))
                c += 1
    hq, wq = SIZES[2]
    for kind in range(4):
        for flags in range(4):
            rng = np.random.default_rng(5000 + 10 * kind + flags)
            grids = [(maps_of(kind, 3, hq, wq, rng, lambda k, f=flags: f, True), 2, PAD)]
            out.append((f"kind{kind}_flags{flags}", image_of(4 * hq, 4 * wq, 50 + c), grids))
            c += 1
    return out


def nibble_lut():
    """A colour table that the blend keeps injective: entry c = (16 (c & 15), 16 (c >> 4), 0); over a black image the output is
    (12 (c & 15), 12 (c >> 4), 0)."""
    c = np.arange(256)
    return np.stack([16 * (c & 15), 16 * (c >> 4), 0 * c], 1).astype(np.uint8)


def levels_from(cells):
    """The colour index of every pixel of figures painted with nibble_lut over a black image."""
    return cells[..., 0].astype(np.int32) // 12 + 16 * (cells[..., 1].astype(np.int32) // 12)


def quantiser_sweep():
    """Values v whose q = v * 255 covers [-255, 255] densely, every integer q with its fp32 neighbours, and the special values."""
    ints = (np.arange(-256, 257, dtype=np.float32) / np.float32(255))
    near = np.concatenate([np.nextafter(ints, np.float32(-9)), ints, np.nextafter(ints, np.float32(9))])
    dense = np.linspace(-1.01, 1.01, 6001, dtype=np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-30, -1e-30, 3.7 / 255, -3.7 / 255, 2.0, -2.0, 1000.0, -1000.0, 8.4e6, -8.4e6, 8.5e6, -8.5e6, 1e12,
                    -1e12, 3e38, -3e38], np.float32)
    return np.concatenate([near, dense, odd]).astype(np.float32)
