#!/usr/bin/env python3
"""Generate tests/golden/sample_plot.npz + sample_plot_meta.json by RUNNING the reference's CocoKeypointsDataset.plot_raw and .plot
(src/keypoints/datasets/coco.py:377-449) and ExplorerDataset.plot_examples (src/base/datasets/base.py:55-58), as unbound functions over
a stub dataset whose samples are tests/sample_plot_helpers.golden_items().

  PYTHONDONTWRITEBYTECODE=1 python3 tools/make_sample_plot_golden.py [path to a checkout of the reference, default /root/reference] [output directory]

Needs a checkout of the reference (thawro/pytorch-human-pose); nothing of it is copied: the fixture holds numbers and strings only.

What runs is the reference's own code and is therefore pinned by the fixture: the polygons as cv2.fillPoly / drawContours receive them
(truncation, order, colours), the overlay's blend weights, every plot_connections call (ellipses, circles, blend), the letterbox
PARAMETERS, every put_txt call (which cell, box, weights, strings, origins, font scale), what plot_heatmaps is given, every cv2.resize
call, the placements of make_grid and stack_horizontally, the final sizes.
What is NOT the reference's: cv2 and albumentations are not installed where the fixtures are made.  cv2 is a recording stand-in (the
recorders of tests/render_ref.py and tests/text_ref.py; getTextSize answers from this project's font atlas); albumentations is a
stand-in whose LongestMaxSize / PadIfNeeded record their arguments and apply this project's restatement of the letterbox.  Parity of
the rasterised pixels with cv2 and of the letterbox arithmetic with albumentations therefore stays UNPINNED.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
if not os.path.isdir(os.path.join(REF, "src", "keypoints")):
    raise SystemExit(f"{REF} is no checkout of the reference\n" + __doc__)
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import render_ref  # noqa: E402
import text_ref  # noqa: E402
from sample_plot_helpers import golden_items  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute is a do-nothing callable."""
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


class Log:
    """Everything one `plot` call does through cv2, albumentations, make_grid and stack_horizontally."""

    def __init__(self):
        self.render, self.text = render_ref.Recorder(), text_ref.Recorder()
        self.keep = []        # arrays whose identity names a cell (kept alive so that no id is reused)
        self.cell = {}        # id(array) -> cell: 0 image, 1 crowd mask, 2 + k heatmap k, -1 the raw pane
        self.resizes, self.heatmaps, self.skeletons, self.polygons, self.grids = [], [], [], [], []
        self.overlay_weights = self.letterbox = self.last_resized = None
        self.hm_count = 0

    def name(self, arr, cell):
        self.keep.append(arr)
        self.cell[id(arr)] = cell
        return arr


LOG = Log()

try:
    importlib.import_module("cv2")
    raise SystemExit("a real cv2 is importable: bind nothing and record that the rasteriser is cv2's")
except ImportError:
    cv2 = sys.modules["cv2"] = _Anything("cv2")
cv2.FONT_HERSHEY_SIMPLEX = text_ref.Recorder.FONT
cv2.BORDER_CONSTANT, cv2.COLORMAP_JET, cv2.COLOR_GRAY2RGB = 0, 2, 8


def _resize(img, dsize, *a, **k):
    assert not a and not k, "a resize with more than (src, dsize)"
    LOG.resizes.append([int(img.shape[0]), int(img.shape[1]), int(dsize[0]), int(dsize[1])])
    # (a one-colour image stays that colour: the marker images of `_placing` survive make_grid's match_size)
    LOG.last_resized = np.full((int(dsize[1]), int(dsize[0])) + img.shape[2:], img.flat[0] if (img == img.flat[0]).all() else 0, img.dtype)
    return LOG.last_resized


def _cvt(img, code):
    assert code == cv2.COLOR_GRAY2RGB and img.ndim == 2
    return LOG.name(np.stack([img] * 3, -1), 1)


def _colormap(hm, code):
    assert code == cv2.COLORMAP_JET and hm.dtype == np.uint8 and hm.ndim == 2
    out = np.zeros(hm.shape + (3,), np.uint8)
    LOG.keep.append(out)
    LOG.cell[id(out)] = "colormap"
    return out


def _poly(call):
    def record(img, pts, *a, color, thickness=None):
        assert len(pts) == 1 and pts[0].dtype == np.int32 and (call == "fillPoly" and not a or call == "drawContours" and a == (-1,))
        LOG.polygons.append(dict(call=call, colour=[int(c) for c in color], vertices=pts[0].tolist(), thickness=thickness))
        return img
    return record


def _add_weighted(a, wa, b, wb, gamma):
    if LOG.text.calls and LOG.text.calls[-1][0] == "box" and LOG.text.calls[-1][-1] is b:      # put_txt's alpha < 1 box
        return LOG.text.addWeighted(a, wa, b, wb, gamma)
    if LOG.cell.get(id(b)) == "colormap":                                                       # plot_heatmaps
        assert (wa, wb, gamma) == (0.25, 0.75, 0) and a is LOG.last_resized
        LOG.hm_count += 1
        return LOG.name(np.zeros_like(a), 2 + LOG.hm_count - 1)
    if wa == 0.4:                                                                               # plot_raw's overlay
        assert gamma == 0
        LOG.overlay_weights = [float(wa), float(wb)]
        return np.zeros_like(a)
    out = LOG.render.addWeighted(a, wa, b, wb, gamma)                                           # plot_connections
    LOG.skeletons.append(LOG.render.rows())
    LOG.render.calls = []
    return LOG.name(out, 0)


cv2.resize, cv2.cvtColor, cv2.applyColorMap, cv2.addWeighted = _resize, _cvt, _colormap, _add_weighted
cv2.fillPoly, cv2.drawContours = _poly("fillPoly"), _poly("drawContours")
cv2.ellipse, cv2.circle = (lambda *a: LOG.render.ellipse(*a)), (lambda *a: LOG.render.circle(*a))
cv2.getTextSize, cv2.rectangle, cv2.putText = (lambda *a: LOG.text.getTextSize(*a)), (lambda *a: LOG.text.rectangle(*a)), (lambda *a: LOG.text.putText(*a))

# albumentations: the two transforms record their arguments; Compose applies this project's restatement of the letterbox (UNPINNED)
A = sys.modules["albumentations"] = types.ModuleType("albumentations")
A.LongestMaxSize = lambda max_size: ("LongestMaxSize", int(max_size))
A.PadIfNeeded = lambda min_height, min_width, border_mode: ("PadIfNeeded", int(min_height), int(min_width), int(border_mode))


def _compose(transforms):
    (n0, max_size), (n1, min_h, min_w, border) = transforms
    assert (n0, n1) == ("LongestMaxSize", "PadIfNeeded")

    def apply(image):
        h, w = image.shape[:2]
        scale = max_size / max(h, w)
        new_h, new_w = int(round(h * scale)), int(round(w * scale))
        top, left = (min_h - new_h) // 2, (min_w - new_w) // 2
        LOG.letterbox = dict(max_size=max_size, min_height=min_h, min_width=min_w, border_mode=border, image=[int(h), int(w)], restated=[new_h, new_w, top, left])
        return {"image": LOG.name(np.zeros((min_h, min_w, 3), np.uint8), -1)}
    return apply


A.Compose = _compose

# the packages' __init__ files pull in configuration code that is not needed here; neither are the logger, the model base and the loaders
for _pkg in ("src", "src.utils", "src.base", "src.base.datasets", "src.base.transforms", "src.keypoints", "src.keypoints.datasets"):
    m = types.ModuleType(_pkg)
    m.__path__ = [os.path.join(REF, *_pkg.split("."))]
    sys.modules[_pkg] = m
for _name, _attrs in (("src.logger", {}), ("src.logger.pylogger", {"log": None}), ("src.base.model", {"BaseInferenceModel": object}),
                      ("src.utils.files", {"load_yaml": None, "save_yaml": None}), ("src.utils.utils", {"get_rank": None}),
                      ("pycocotools", {}), ("pycocotools.coco", {"COCO": object}), ("natsort", {})):
    m = types.ModuleType(_name)
    m.__dict__.update(_attrs)
    sys.modules[_name] = m
for _name in ("seaborn", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
    sys.modules.setdefault(_name, _Anything(_name))

base = importlib.import_module("src.base.datasets.base")
sys.modules["src.base.datasets"].BaseImageDataset = base.BaseImageDataset
coco = importlib.import_module("src.keypoints.datasets.coco")


def _placing(fn, name):
    """make_grid / stack_horizontally are numpy only: run them as they are, and once more on marker images to read every input's place."""
    def wrapped(images, *a, **k):
        out = fn(images, *a, **k)
        before = len(LOG.resizes)
        marked = fn([np.full(im.shape[:2] + (3,), 1 + i, np.uint8) for i, im in enumerate(images)], *a, **k)
        resized = LOG.resizes[before:]
        del LOG.resizes[before:]   # (the marker run's resizes repeat the real run's)
        places = []
        for i in range(len(images)):
            ys, xs = np.nonzero((marked == 1 + i).all(-1))
            places.append([int(ys.min()), int(xs.min()), int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)])
        LOG.grids.append(dict(fn=name, args=[int(v) for v in a], kwargs={kk: int(v) for kk, v in k.items()}, inputs=[list(im.shape[:2]) for im in images],
                              places=places, resized=resized, out=list(out.shape[:2])))
        return out
    return wrapped


def _plot_heatmaps(image, heatmaps, **kwargs):
    LOG.heatmaps.append(dict(image_is_the_resized_input=bool(image is LOG.last_resized), shape=list(heatmaps.shape), sum=float(np.float64(heatmaps).sum()),
                             kwargs={k: bool(v) for k, v in kwargs.items()}))
    LOG.hm_count = 0
    return _real_plot_heatmaps(image, heatmaps, **kwargs)


_real_plot_heatmaps = coco.plot_heatmaps
coco.plot_heatmaps = _plot_heatmaps
coco.make_grid, coco.stack_horizontally = _placing(coco.make_grid, "make_grid"), _placing(coco.stack_horizontally, "stack_horizontally")
base.make_grid = _placing(base.make_grid, "make_grid")

ITEMS = golden_items()


class Stub:
    """What plot_raw / plot read of a CocoKeypointsDataset."""
    limbs, labels = coco.COCO_LIMBS, coco.COCO_LABELS
    images_filepaths = [f"images/{stem}.jpg" for *_, stem in ITEMS]
    plot_raw, plot, plot_examples_of_base = coco.CocoKeypointsDataset.plot_raw, coco.CocoKeypointsDataset.plot, base.ExplorerDataset.plot_examples

    def get_raw_data(self, idx):
        raw, annot, _, _ = ITEMS[idx]
        return raw.copy(), annot, np.ones(raw.shape[:2], bool)

    def __getitem__(self, idx):
        img, heatmaps, masks, joints = ITEMS[idx][2]
        return torch.from_numpy(img), heatmaps, masks, joints


def puts(calls):
    """text_ref.Recorder's calls grouped into put_txt calls: one box, then its labels."""
    out = []
    for c in calls:
        if c[0] == "box":
            frame = c[-1]
            out.append(dict(cell=LOG.cell[id(frame)], frame=list(frame.shape[:2]), box=c[1:5], opaque=c[5], weights=[c[6], c[7]], bg_color=list(c[8]),
                            strings=[], origins=[], font_scale=None, txt_color=None, thickness=None))
        else:
            p = out[-1]
            p["strings"].append(c[1]), p["origins"].append([c[2], c[3]])
            assert p["font_scale"] in (None, c[4])
            p["font_scale"], p["txt_color"], p["thickness"] = c[4], list(c[5]), c[6]
    return out


def main():
    global LOG
    arrays, samples = {}, []
    ds = Stub()
    cases = [dict(tag="plot_default", idx=0, kwargs={}), dict(tag="examples_0", idx=0, kwargs=dict(nrows=1, stage_idxs=[1, 0])),
             dict(tag="examples_1", idx=1, kwargs=dict(nrows=1, stage_idxs=[1, 0]))]
    for case in cases:
        LOG = Log()
        out = ds.plot(case["idx"], **case["kwargs"])
        for n, rows in enumerate(LOG.skeletons):
            arrays[f"{case['tag']}.skeleton{n}"] = rows
        samples.append(dict(case, resizes=LOG.resizes, heatmaps=LOG.heatmaps, skeletons=len(LOG.skeletons), puts=puts(LOG.text.calls), polygons=LOG.polygons,
                            overlay_weights=LOG.overlay_weights, letterbox=LOG.letterbox, grids=LOG.grids, size=list(out.shape[:2])))
        print(case["tag"], "size", out.shape, "puts", len(samples[-1]["puts"]), "polygons", len(LOG.polygons), "resizes", len(LOG.resizes))
    LOG = Log()
    grid = ds.plot_examples_of_base([0, 1], nrows=1, stage_idxs=[1, 0])   # CocoKeypointsDataset.plot_examples' own call (coco.py:375)
    examples = dict(grid=LOG.grids[-1], size=list(grid.shape[:2]))
    print("plot_examples", grid.shape)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "sample_plot.npz"), **arrays)
    meta = dict(samples=samples, examples=examples, labels=list(coco.COCO_LABELS), limbs=[list(l) for l in coco.COCO_LIMBS],
                inputs="tests/sample_plot_helpers.golden_items(): out_size 128, stages 32 and 64, raw images 90 x 140 and 120 x 80",
                skeleton_rows="float64 [N,10] per plot_connections call, in call order (the stages as plotted, then the raw pane): the rows of "
                              "tests/render_ref.py's Recorder, the blend last",
                puts="per put_txt call: cell (0 image, 1 crowd mask, 2 + k heatmap k, -1 raw pane), the frame's size, the box as the reference passed "
                     "it (inclusive, not clipped), opaque, the two weights, colours, strings, origins, font scale",
                places="y, x, height, width of every input in the grid (after make_grid's match_size resize, listed in `resized`)",
                unpinned="cv2 and albumentations are stand-ins: the rasterised pixels, the text metrics (this project's atlas) and the letterbox "
                         "arithmetic ('restated') are this project's; calls, arguments, order and placements are the reference's own code")
    with open(os.path.join(OUT, "sample_plot_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", os.path.getsize(os.path.join(OUT, "sample_plot.npz")), "+", os.path.getsize(os.path.join(OUT, "sample_plot_meta.json")), "bytes")


if __name__ == "__main__":
    main()
