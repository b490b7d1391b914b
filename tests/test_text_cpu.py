"""The text labels without a GPU: keypoints/text.py's layout, classification's plot_top_preds tables and video_labels against every
case of tests/golden/text.npz (recorded from the reference's own put_txt, plot_top_preds and draw_labels: box rectangle, the
alpha == 1 inclusive one included, blend weights, colours, each label's origin and string); the kernel's tile walk compiled for the
host (hh_debug_text_host) against the numpy restatement tests/text_ref.py on the golden cases and on tables aimed at the tile, chunk
and pixel-group edges; every refusal of the validation by name, before any launch; the atlas file.  Byte for byte, no tolerance."""
import ctypes as C
import importlib
import sys

import numpy as np
import pytest

import text_ref as tr
from conftest import PKG
from text_helpers import box_row, edge_cases, glyph_row, text_golden, tx  # noqa: F401


def _check_call(lay, table_row, box, h, w):
    """One put_txt call's layout and BOX row against the recorded rectangle / addWeighted row."""
    x0, y0, x1, y1, opaque, w0, w1, r, g, b, _ = box
    assert lay["box"] == (x0, y0, x1, y1) and lay["opaque"] == bool(opaque) and lay["bg_color"] == (r, g, b)
    assert table_row["kind"] == tr.BOX and tuple(table_row["rgb"]) == (r, g, b) and table_row["A"] == int(opaque)
    if not opaque:  # the doubles the reference passed, and their one rounding to fp32
        assert lay["weights"] == (w0, w1) and table_row["c"] == np.float32(w0) and table_row["s"] == np.float32(w1)
    assert (table_row["x0"], table_row["y0"], table_row["x1"], table_row["y1"]) == (max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1))


def _check_texts(lay, labels, texts, strings, font_scale):
    assert labels == strings and lay["origins"] == [(t[0], t[1]) for t in texts]
    for t in texts:
        assert t[2] == font_scale and lay["txt_color"] == tuple(t[3:6]) and t[6] == 1


def test_layout_reproduces_the_golden_put_txt_cases(tx, text_golden):
    meta, data = text_golden
    cases = [c for c in meta["cases"] if c["kind"] == "put_txt"]
    assert len(cases) == 36 and {c["loc"] for c in cases} == set(tx.LOCS) and {c["alpha"] for c in cases} == {1.0, 0.8}
    for c in cases:
        boxes, texts = data[c["tag"] + ".boxes"], data[c["tag"] + ".texts"]
        table, lay = tx.layout_put_txt(c["h"], c["w"], c["labels"], loc=c["loc"], alpha=c["alpha"], return_layout=True)
        assert len(boxes) == 1 and boxes[0, 10] == 0, c["tag"]
        _check_call(lay, table[0], boxes[0], c["h"], c["w"])
        _check_texts(lay, c["labels"], texts, c["strings"], 0.5)
        assert (table["kind"][1:] == tr.GLYPH).all() and len(table) == 1 + sum(ch != " " for s in c["labels"] for ch in s), c["tag"]


def test_plot_top_preds_reproduces_the_golden(pkg, tx, text_golden):
    meta, data = text_golden
    vis = importlib.import_module(PKG + ".classification.visualization")
    idx2label = dict(enumerate(meta["idx2label"]))
    cases = [c for c in meta["cases"] if c["kind"] == "plot_top_preds"]
    assert len(cases) == 6
    for c, scale in zip(cases, (0.3, 0.3, 0.5, 0.5, 0.7, 0.7)):
        boxes, texts = data[c["tag"] + ".boxes"], data[c["tag"] + ".texts"]
        table, calls = vis.top_preds_table(c["h"], c["w"], data["probs"], idx2label, 5, c["target_label"], return_layout=True)
        assert len(calls) == len(boxes) == (2 if c["target_label"] else 1), c["tag"]
        first_text, row = 0, 0
        for (labels, lay), box in zip(calls, boxes):
            _check_call(lay, table[row], box, c["h"], c["w"])
            n = len(labels)
            # the call order: a box, then its labels
            assert list(texts[first_text:first_text + n, 7]) == list(range(int(box[10]) + 1, int(box[10]) + 1 + n))
            _check_texts(lay, labels, texts[first_text:first_text + n], c["strings"][first_text:first_text + n], scale)
            first_text += n
            row += 1 + sum(ch != " " for s in labels for ch in s)
        assert first_text == len(texts) and row == len(table)


def test_video_labels_reproduce_the_golden(tx, text_golden):
    meta, data = text_golden
    c = next(c for c in meta["cases"] if c["kind"] == "draw_labels")
    labels = tx.video_labels(c["idx"], c["num_frames"], c["model_input_shape"], c["speed_ms"])
    assert labels == c["strings"] and len(labels) == 6
    table, lay = tx.layout_put_txt(c["h"], c["w"], labels, loc="tl", alpha=0.6, font_scale=0.5, return_layout=True)
    _check_call(lay, table[0], data["draw_labels.boxes"][0], c["h"], c["w"])
    _check_texts(lay, labels, data["draw_labels.texts"], c["strings"], 0.5)
    assert np.array_equal(tx.video_table(c["h"], c["w"], labels), table)


def test_host_twin_equals_the_restatement_on_every_golden_case(pkg, tx, text_golden):
    meta, data = text_golden
    vis = importlib.import_module(PKG + ".classification.visualization")
    idx2label = dict(enumerate(meta["idx2label"]))
    for c in meta["cases"]:
        img = tr.image(c["seed"], c["h"], c["w"])
        if c["kind"] == "put_txt":
            table, want = tx.layout_put_txt(c["h"], c["w"], c["labels"], loc=c["loc"], alpha=c["alpha"]), tr.put_txt(img, c["labels"], loc=c["loc"], alpha=c["alpha"])
        elif c["kind"] == "plot_top_preds":
            table = vis.top_preds_table(c["h"], c["w"], data["probs"], idx2label, 5, c["target_label"])
            want = tr.plot_top_preds(img, data["probs"], idx2label, 5, c["target_label"])
        else:
            table, want = tx.video_table(c["h"], c["w"], c["strings"]), tr.put_txt(img, c["strings"], loc="tl", alpha=0.6, font_scale=0.5)
        before = img.copy()
        got = tx.put_txt_host(img, table)
        assert np.array_equal(got, want) and (got != img).any() and np.array_equal(img, before), c["tag"]


def test_host_twin_equals_the_restatement_on_the_edge_tables(tx):
    cases = edge_cases(tx, tx.text_config())
    assert len(cases) > 15
    for name, img, table in cases:
        want = tr.apply_table(img, table)
        assert np.array_equal(tx.put_txt_host(img, table), want), name
        if name in ("empty_table", "box_wholly_outside", "alpha_0.0"):
            pass
        else:
            assert (want != img).any(), name
    by_name = {name: (img, table) for name, img, table in cases}
    for name in ("empty_table", "box_wholly_outside"):
        assert np.array_equal(tx.put_txt_host(*by_name[name]), by_name[name][0]), name
    # at alpha 0 the box leaves every byte as it was: only the glyphs change the frame
    img, table = by_name["alpha_0.0"]
    assert np.array_equal(tx.put_txt_host(img, table[:1]), img) and table["kind"][0] == tr.BOX
    # the order matters where the two boxes overlap
    assert not np.array_equal(tx.put_txt_host(*by_name["order_tl_br"]), tx.put_txt_host(*by_name["order_br_tl"]))
    # a maximal table on a 1 x 1 frame and on a two-tile frame
    TH, TW, CHUNK, PX = tx.text_config()
    for h, w in ((1, 1), (TH, TW + PX + 1)):
        img = tr.image(7, h, w)
        rs = np.random.RandomState(h)
        rows = [glyph_row(tx, h, w, i % 3, chr(0x21 + i % 94), int(rs.randint(-20, w + 2)), int(rs.randint(-20, h + 2)), (i % 256, 255 - i % 256, 7))
                if i % 5 else box_row(tx, h, w, int(rs.randint(-5, w)), int(rs.randint(-5, h)), int(rs.randint(0, w + 5)), int(rs.randint(0, h + 5)), (9, i % 256, 200), 0.4)
                for i in range(tx.MAX_PRIMS)]
        table = np.concatenate(rows)
        assert np.array_equal(tx.put_txt_host(img, table), tr.apply_table(img, table)), (h, w)


def _refused(pkg, match, call):
    with pytest.raises(pkg._lib.HHError, match=match):
        pkg._lib.check(call())


def test_every_refusal_by_name_before_a_launch(pkg, tx):
    """hh_text_check is the validation of hh_text_labels_u8_batch alone (it launches nothing); what only the launching entry point
    checks (device pointers, their alignment) is asked of it with an empty tile list, with which it launches nothing either."""
    lib = pkg._lib.load()
    h, w = 20, 30
    atlas_len = len(tx.font().coverage)
    good = np.concatenate([box_row(tx, h, w, 2, 2, 9, 9, (1, 2, 3), 0.5), glyph_row(tx, h, w, 1, "A", 3, 3, (4, 5, 6))])
    tiles = np.array([[0, 0]], np.int32)
    DEVP = 0x10000  # stands for device memory: never dereferenced

    def call(desc=None, prims=good, n=1, tiles=tiles, num_tiles=None, alen=atlas_len):
        d = np.zeros(max(n, 1), tx.DESC)
        d[:] = (0, 0, h, w, 0, len(prims), 0.0, 0.0, 0, 0) if desc is None else desc
        num_tiles = len(tiles) if num_tiles is None else num_tiles
        return lambda: lib.hh_text_check(d.ctypes.data, prims.ctypes.data if len(prims) else None, len(prims), n, alen, tiles.ctypes.data, num_tiles)

    def launch(base=DEVP, descs_dev=DEVP, atlas=DEVP, prims_dev=DEVP, descs_host=True):
        d = np.zeros(1, tx.DESC)
        d[0] = (0, 0, h, w, 0, len(good), 0.0, 0.0, 0, 0)
        return lambda: lib.hh_text_labels_u8_batch(base, descs_dev, d.ctypes.data if descs_host else None, prims_dev, good.ctypes.data, len(good), 1, atlas,
                                                   atlas_len, None, None, 0, None)

    assert call()() == 0 and launch()() == 0  # (accepted; the latter has no tile to draw)
    def edited(row, **fields):
        t = good.copy()
        for k, v in fields.items():
            t[k][row] = v
        return t

    _refused(pkg, "null pointer", launch(base=None))
    _refused(pkg, "null pointer", launch(descs_dev=None))
    _refused(pkg, "null pointer", launch(atlas=None))
    _refused(pkg, "null pointer", launch(prims_dev=None))
    _refused(pkg, "null pointer", launch(descs_host=False))
    _refused(pkg, "aligned", launch(descs_dev=DEVP + 4))
    _refused(pkg, "aligned", launch(prims_dev=DEVP + 2))
    _refused(pkg, "null pointer", lambda: lib.hh_text_check(None, None, 0, 1, atlas_len, None, 0))
    _refused(pkg, "n <= 65535", call(n=0))
    _refused(pkg, "n <= 65535", call(n=65536))
    for size in ((0, w), (h, 0), (16385, w), (h, 16385)):
        _refused(pkg, "frame size outside 1..16384", call(desc=(0, 0, *size, 0, 0, 0.0, 0.0, 0, 0), prims=good[:0]))
    _refused(pkg, "negative offset", call(desc=(-1, -1, h, w, 0, 2, 0.0, 0.0, 0, 0)))
    _refused(pkg, "dst_offset must equal src_offset", call(desc=(0, 64, h, w, 0, 2, 0.0, 0.0, 0, 0)))
    _refused(pkg, "primitive range outside the table", call(desc=(0, 0, h, w, 1, 2, 0.0, 0.0, 0, 0)))
    _refused(pkg, "primitive range outside the table", call(desc=(0, 0, h, w, -1, 2, 0.0, 0.0, 0, 0)))
    many = np.concatenate([good[:1]] * (tx.MAX_PRIMS + 1))
    _refused(pkg, "more than HH_TEXT_MAX_PRIMS", call(prims=many))
    _refused(pkg, "unknown flag", call(desc=(0, 0, h, w, 0, 2, 0.0, 0.0, 1, 0)))
    for bad in (np.nan, np.inf, -np.inf):
        _refused(pkg, "blend weight not finite", call(prims=edited(0, c=bad)))
        _refused(pkg, "blend weight not finite", call(prims=edited(0, s=bad)))
    _refused(pkg, "unknown primitive kind", call(prims=edited(0, kind=2)))
    _refused(pkg, "unknown flag", call(prims=edited(0, A=2)))
    _refused(pkg, "empty or inverted glyph bitmap", call(prims=edited(1, A=0)))
    _refused(pkg, "empty or inverted glyph bitmap", call(prims=edited(1, B=0)))
    _refused(pkg, "coverage range leaves the atlas", call(prims=edited(1, c=float(atlas_len - 3))))
    _refused(pkg, "coverage range leaves the atlas", call(alen=10))
    _refused(pkg, "coverage offset is not an integer", call(prims=edited(1, c=2.5)))
    _refused(pkg, "coverage offset is not an integer", call(prims=edited(1, c=-1.0)))
    _refused(pkg, "coordinate beyond 2\\^23", call(prims=edited(1, cx=(1 << 23) + 1, x1=-1)))
    _refused(pkg, "coordinate beyond 2\\^23", call(prims=edited(1, cy=-(1 << 23) - 1, x1=-1)))
    _refused(pkg, "box outside the frame", call(prims=edited(0, x1=w)))
    _refused(pkg, "box outside the frame", call(prims=edited(0, y0=-1)))
    _refused(pkg, "glyph box outside its bitmap", call(prims=edited(1, x0=2)))
    _refused(pkg, "glyph box outside its bitmap", call(prims=edited(1, y1=19)))
    _refused(pkg, "names no tile of its frame", call(tiles=np.array([[1, 0]], np.int32)))
    _refused(pkg, "names no tile of its frame", call(tiles=np.array([[0, 2]], np.int32)))  # (20 x 30: two tiles)
    _refused(pkg, "names no tile of its frame", call(tiles=np.array([[0, -1]], np.int32)))
    _refused(pkg, "ascend strictly", call(tiles=np.array([[0, 0], [0, 0]], np.int32)))
    _refused(pkg, "num_tiles", call(num_tiles=-1))
    # the Python layer refuses by name as well, and the host twin runs the same checks
    with pytest.raises(pkg._lib.HHError, match="more than HH_TEXT_MAX_PRIMS"):
        tx.put_txt_host(tr.image(1, h, w), many)
    with pytest.raises(pkg._lib.HHError, match="unknown primitive kind"):
        tx.put_txt_host(tr.image(1, h, w), edited(0, kind=7))
    with pytest.raises(ValueError, match="loc"):
        tx.layout_put_txt(h, w, ["a"], loc="mid")
    with pytest.raises(ValueError, match="alpha"):
        tx.layout_put_txt(h, w, ["a"], alpha=float("nan"))
    # hh_text_tiles lists what the boxes touch, in order, and sizes the list when there is no room
    TH, TW, _, _ = tx.text_config()
    hh, ww = 3 * TH, 3 * TW
    table = np.concatenate([box_row(tx, hh, ww, TW - 1, TH, TW, TH, (1, 1, 1), None), glyph_row(tx, hh, ww, 2, "W", 2 * TW + 1, 2 * TH + 3, (2, 2, 2))])
    d = np.zeros(1, tx.DESC)
    d[0] = (0, 0, hh, ww, 0, 2, 0.0, 0.0, 0, 0)
    count = C.c_longlong(-1)
    pkg._lib.check(lib.hh_text_tiles(d.ctypes.data, table.ctypes.data, 2, 1, atlas_len, None, 0, C.byref(count)))
    assert count.value == 3
    listed = np.full((3, 2), -1, np.int32)
    pkg._lib.check(lib.hh_text_tiles(d.ctypes.data, table.ctypes.data, 2, 1, atlas_len, listed.ctypes.data, 3, C.byref(count)))
    assert count.value == 3 and listed.tolist() == [[0, 3], [0, 4], [0, 8]]


def test_atlas_file(tx, monkeypatch):
    for name in ("PIL", "PIL.ImageFont", "PIL.Image", "matplotlib", "matplotlib.font_manager"):  # neither FreeType nor the font file is needed
        monkeypatch.setitem(sys.modules, name, None)
    font = tx.Font(tx.DEFAULT_FONT)
    assert font.cap_height.tolist() == [7, 11, 15] and [float(s) for s in font.font_scale] == [0.3, 0.5, 0.7]
    g = font.glyphs
    assert g.shape == (3, 95, 6) and g[..., 0].sum(axis=1).tolist() == [560, 863, 1187]
    assert g[:, [0, ord("H") - 32, ord("i") - 32, ord("W") - 32], 0].tolist() == [[3, 8, 3, 10], [5, 11, 4, 15], [7, 16, 6, 21]]
    assert (g[:, ord("H") - 32, 2] == font.cap_height).all() and (g[:, ord("H") - 32, 4] == -font.cap_height).all()
    # every glyph's coverage range lies inside the file, the ranges follow each other without a gap, only the space has no ink
    area = g[..., 1] * g[..., 2]
    assert len(font.coverage) == 30076 and (g[..., 5] >= 0).all() and (g[..., 5] + area <= len(font.coverage)).all()
    assert np.array_equal(g[..., 5].reshape(-1), np.concatenate([[0], np.cumsum(area.reshape(-1))[:-1]]))
    assert (area[:, 0] == 0).all() and (area[:, 1:] > 0).all() and (g[..., 0] > 0).all()
    assert font.coverage.max() == 255 and np.array_equal(font.coverage, tr.COVERAGE) and np.array_equal(g, tr.GLYPHS)
    import os
    assert os.path.exists(os.path.join(os.path.dirname(tx.DEFAULT_FONT), "LICENSE_DEJAVU"))
    # load_font replaces the atlas, as jet_lut's table can be replaced
    try:
        assert tx.load_font(tx.DEFAULT_FONT) is tx.font() and tx.font() is not font
        with pytest.raises(Exception):
            tx.load_font(os.path.join(os.path.dirname(tx.DEFAULT_FONT), "LICENSE_DEJAVU"))
    finally:
        tx.load_font()


def test_font_scale_thickness_and_characters(tx):
    f = tx.font()
    assert [f.size_class(s) for s in (0.3, 0.5, 0.7)] == [0, 1, 2]
    assert [f.size_class(s) for s in (0.1, 0.39, 0.4, 0.41, 0.59, 0.6, 0.61, 1.0, 2.5)] == [0, 0, 0, 1, 1, 1, 2, 2, 2]  # the smaller on a tie
    assert [tx.text_size("0.912:  goldfish", s) for s in (0.3, 0.5, 0.7)] == [(75, 7), (120, 11), (162, 15)]
    assert tx.text_size("", 0.5) == (0, 11) and tx.text_size("Hello", 0.5) == tr.text_size("Hello", 0.5) == (37, 11)
    for call in (lambda: tx.text_size("a", 0.5, thickness=2), lambda: tx.layout_put_txt(50, 50, ["a"], thickness=2),
                 lambda: tx.put_txt(np.zeros((50, 50, 3), np.uint8), ["a"], thickness=2)):
        with pytest.raises(ValueError, match="thickness"):
            call()
    # a character outside 0x20..0x7E draws as '?'
    assert tx.text_size("café 中\t", 0.5) == tx.text_size("caf? ??", 0.5)
    assert np.array_equal(tx.layout_put_txt(60, 90, ["café 中\x7f"]), tx.layout_put_txt(60, 90, ["caf? ??"]))
    img = tr.image(3, 60, 90)
    assert np.array_equal(tx.put_txt_host(img, tx.layout_put_txt(60, 90, ["é"], alpha=0.5)), tr.put_txt(img, ["?"], alpha=0.5))
    # bgr: colours given as R,G,B for a frame stored B,G,R
    a, b = tx.layout_put_txt(60, 90, ["x"], bg_color=(1, 2, 3), txt_color=(4, 5, 6)), tx.layout_put_txt(60, 90, ["x"], bg_color=(3, 2, 1), txt_color=(6, 5, 4), bgr=True)
    assert np.array_equal(a, b)
