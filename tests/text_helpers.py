"""Shared by tests/test_text_cpu.py and tests/test_gpu_text.py: the golden, hand-built primitive rows (from the atlas as text_ref reads
it, not from keypoints/text.py) and the tables aimed at the text kernel's tile, chunk and pixel-group edges (hh_text_config)."""
import importlib
import json
import os

import numpy as np
import pytest

import text_ref as tr
from conftest import GOLDEN, PKG


@pytest.fixture(scope="session")
def tx():
    return importlib.import_module(PKG + ".keypoints.text")


@pytest.fixture(scope="session")
def text_golden():
    return json.load(open(os.path.join(GOLDEN, "text_meta.json"))), np.load(os.path.join(GOLDEN, "text.npz"))


def _clip(x0, y0, x1, y1, h, w):
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else (0, 0, -1, -1)


def box_row(tx, h, w, x0, y0, x1, y1, colour, alpha):
    """A BOX over the inclusive rectangle, clipped to the h x w frame; alpha None = opaque."""
    row = np.zeros(1, tx.PRIM)
    opaque = alpha is None
    row[0] = (0, 0, 1 if opaque else 0, 0, 0.0 if opaque else np.float32(1.0 - alpha), 1.0 if opaque else np.float32(alpha), colour, tr.BOX,
              *_clip(x0, y0, x1, y1, h, w))
    return row


def glyph_row(tx, h, w, k, ch, cx, cy, colour):
    """Character `ch` of size class k with its bitmap's top-left at (cx, cy), clipped to the h x w frame."""
    _, bw, bh, _, _, off = (int(v) for v in tr.GLYPHS[k, ord(ch) - 0x20])
    assert bw and bh
    row = np.zeros(1, tx.PRIM)
    row[0] = (cx, cy, bw, bh, float(off), 0.0, colour, tr.GLYPH, *_clip(cx, cy, cx + bw - 1, cy + bh - 1, h, w))
    return row


def edge_cases(tx, cfg):
    """[(name, image, table)]: what the kernel's address arithmetic can get wrong, on frames of a few tiles."""
    TH, TW, CHUNK, PX = cfg
    cat = np.concatenate
    out = []
    # the sizes around one tile, and tiny frames; widths 1, 30, TW + 1, TW - 1 give rows of 3, 90, 195, 189 bytes: none a multiple of 4
    for n, (h, w) in enumerate([(1, 1), (20, 30), (TH - 1, TW + 1), (TH + 1, TW - 1)]):
        img = tr.image(100 + n, h, w)
        out.append((f"put_txt_{h}x{w}", img, tx.layout_put_txt(h, w, ["Hg", "jq|"], vspace=3, alpha=0.8, font_scale=0.3)))
    h, w = TH + 5, TW + 7
    img = tr.image(110, h, w)
    out.append(("empty_table", img, np.zeros(0, tx.PRIM)))
    out.append(("box_clipped_on_four_sides", img, box_row(tx, h, w, -9, -4, w + 30, h + 2, (10, 200, 90), 0.6)))
    out.append(("opaque_box_clipped_on_four_sides", img, box_row(tx, h, w, -1, -1, w, h, (10, 200, 90), None)))
    out.append(("box_wholly_outside", img, cat([box_row(tx, h, w, w, 0, w + 5, 3, (1, 2, 3), None), box_row(tx, h, w, 2, -9, 8, -1, (1, 2, 3), 0.5)])))
    for a in (1.0, 0.8, 0.6, 0.0):
        out.append((f"alpha_{a}", img, tx.layout_put_txt(h, w, ["alpha", str(a)], vspace=4, alpha=a, loc="bc", bg_color=(200, 30, 90), txt_color=(3, 250, 7))))
    # glyphs hanging off every edge, negative origins, at every pixel-group phase
    rows = []
    for i, (cx, cy) in enumerate([(-3, -4), (w - 5, 3), (w - 1, h - 1), (5, h - 6), (-7, h - 3), (w - 9, -9), (TW - 2, TH - 3), (TW - 6, 2), (-40, 5), (7, h + 3)]):
        rows.append(glyph_row(tx, h, w, 2, "W@#Mg"[i % 5], cx, cy, (255 - 20 * i, 10 * i, 128)))
    rows += [glyph_row(tx, h, w, 1, "Q", 9 + e, 2 + 2 * e, (250, 250, 0)) for e in range(4)]
    out.append(("glyphs_off_every_edge", img, cat(rows)))
    # order: two overlapping put_txt tables, tl then br, and the reverse
    h, w = 40, 70
    img = tr.image(111, h, w)
    a = tx.layout_put_txt(h, w, ["first", "box"], vspace=5, alpha=0.8, font_scale=0.3)
    b = tx.layout_put_txt(h, w, ["second"], vspace=5, alpha=1.0, loc="br", font_scale=0.5, bg_color=(0, 90, 0), txt_color=(80, 255, 80))
    out += [("order_tl_br", img, cat([a, b])), ("order_br_tl", img, cat([b, a]))]
    # more glyphs over one tile than a chunk holds: the chunk boundary falls inside the second tile of the first tile row
    h, w = TH + 3, 2 * TW + 5
    img = tr.image(112, h, w)
    rs = np.random.RandomState(5)
    rows = [box_row(tx, h, w, 0, 0, w - 1, h - 1, (40, 40, 40), 0.3)]
    for i in range(CHUNK + 44):
        rows.append(glyph_row(tx, h, w, i % 3, chr(0x21 + i % 94), TW + int(rs.randint(-6, TW - 4)), int(rs.randint(-5, TH)), tuple(int(v) for v in rs.randint(0, 256, 3))))
    rows.append(box_row(tx, h, w, TW + 3, 2, TW + 20, 9, (255, 0, 0), 0.5))  # (behind the boundary: must land on top)
    out.append((f"stack_{CHUNK + 45}", img, cat(rows)))
    # every glyph of every size class once
    h, w = 9 * 28, 32 * 24 + 3  # three lines of 32 cells per class
    img = tr.image(113, h, w)
    rows = []
    for k in range(3):
        for i in range(1, 95):
            rows.append(glyph_row(tx, h, w, k, chr(0x20 + i), 2 + (i % 32) * 24, (3 * k + i // 32) * 28 + 3, (255, 255 - 2 * i, 40 * k)))
    out.append(("every_glyph", img, cat(rows)))
    return out
