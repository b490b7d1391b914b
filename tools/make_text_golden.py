#!/usr/bin/env python3
"""Generate tests/golden/text.npz + text_meta.json by RUNNING the reference's put_txt (src/utils/image.py), plot_top_preds
(src/classification/visualization.py) and InferenceVideoDataset.draw_labels (src/base/datasets/video.py).

  PYTHONDONTWRITEBYTECODE=1 python3 tools/make_text_golden.py <path to a checkout of the reference>

Needs a checkout of the reference (thawro/pytorch-human-pose); nothing of it is copied: the fixture holds numbers and strings only.

What is imported from the reference and therefore pinned by the fixture: the box size from the text sizes, the six locs, _x / _y, the
alpha < 1 slice against the inclusive cv2.rectangle of alpha == 1, the blend weights, the colours, every label's origin and string,
plot_top_preds' font scale, top-k order, label format and its two put_txt calls, draw_labels' strings and arguments.
What is NOT the reference's: cv2 is not installed where the fixtures are made.  It is replaced by a stand-in module whose getTextSize
answers from this project's font atlas (tests/text_ref.py) and whose rectangle / addWeighted / putText are the recorders of
tests/text_ref.py.  Parity of text metrics and glyph shapes with cv2's Hershey font therefore stays UNPINNED.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden")

import text_ref  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute is a do-nothing callable (cv2.VideoCapture in an annotation, ...)."""
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


try:
    importlib.import_module("cv2")
    raise SystemExit("a real cv2 is importable: bind nothing and record that the metrics and the rasteriser are cv2's")
except ImportError:
    cv2 = sys.modules["cv2"] = _Anything("cv2")
cv2.FONT_HERSHEY_SIMPLEX = text_ref.Recorder.FONT
# the packages' __init__ files pull in configuration code that is not needed here; neither are the logger and the key bindings
for _pkg in ("src", "src.utils", "src.classification", "src.base", "src.base.datasets"):
    m = types.ModuleType(_pkg)
    m.__path__ = [os.path.join(REF, *_pkg.split("."))]
    sys.modules[_pkg] = m
for _name, _attrs in (("src.logger", {}), ("src.logger.pylogger", {"log": None}), ("src.base.datasets.base", {"KeyBinds": object})):
    m = types.ModuleType(_name)
    m.__dict__.update(_attrs)
    sys.modules[_name] = m

put_txt = importlib.import_module("src.utils.image").put_txt
plot_top_preds = importlib.import_module("src.classification.visualization").plot_top_preds
draw_labels = importlib.import_module("src.base.datasets.video").InferenceVideoDataset.draw_labels

LABELS = {"one": ["A single label"], "five": ["a", "Label 2", "third label", "x: 0.5", "The widest of these"], "empty": ["above", "", "below the empty one"]}
SIZES = [(120, 220), (121, 223), (133, 207)]
LOCS = ("tl", "tc", "tr", "bl", "bc", "br")
IDX2LABEL = {i: name for i, name in enumerate(["tench", "goldfish", "great white shark", "tiger shark", "hammerhead", "electric ray", "stingray", "cock",
                                                "hen", "ostrich"])}
PROBS = np.array([0.011, 0.302, 0.021, 0.153, 0.005, 0.251, 0.101, 0.043, 0.081, 0.032])


def record(fn):
    rec = text_ref.Recorder()
    cv2.getTextSize, cv2.rectangle, cv2.addWeighted, cv2.putText = rec.getTextSize, rec.rectangle, rec.addWeighted, rec.putText
    out = fn()
    return rec.rows(), out


def main():
    out, cases = {}, []

    def keep(tag, kind, rows, **info):
        boxes, texts, strings = rows
        out[f"{tag}.boxes"], out[f"{tag}.texts"] = boxes, texts
        cases.append(dict(tag=tag, kind=kind, strings=strings, **info))
        print(tag, "boxes", len(boxes), "texts", len(texts))

    n = 0
    for loc in LOCS:
        for alpha in (1.0, 0.8):
            for name, labels in LABELS.items():
                h, w = SIZES[n % len(SIZES)]
                n += 1
                img = text_ref.image(n, h, w)
                rows, got = record(lambda: put_txt(img.copy(), list(labels), loc=loc, alpha=alpha))
                assert np.array_equal(got, text_ref.put_txt(img, labels, loc=loc, alpha=alpha)), "the restated layout differs from the reference's"
                b = rows[0][0]
                assert b[0] >= 0 and b[1] >= 0 and b[2] <= (w - 1 if alpha < 1 else w) and b[3] <= (h - 1 if alpha < 1 else h), "box outside the image"
                keep(f"put_{loc}_{'a1' if alpha == 1.0 else 'a08'}_{name}", "put_txt", rows, h=h, w=w, seed=n, labels=labels, loc=loc, alpha=alpha)
    for h, w in ((224, 300), (400, 300), (512, 640)):
        for target in (None, "stingray"):
            img = text_ref.image(h, h, w)
            rows, got = record(lambda: plot_top_preds(img, PROBS, IDX2LABEL, k=5, target_label=target))
            assert np.array_equal(got, text_ref.plot_top_preds(img, PROBS, IDX2LABEL, 5, target))
            keep(f"top_{min(h, w)}_{'target' if target else 'plain'}", "plot_top_preds", rows, h=h, w=w, seed=h, target_label=target)
    h, w = 640, 853
    stand_in = types.SimpleNamespace(idx=7, num_frames=120)
    result = types.SimpleNamespace(model_input_shape=(512, 704), speed_ms={"preprocess": 3, "model": 21, "postprocess": 5})
    img = text_ref.image(5, h, w)
    rows, _ = record(lambda: draw_labels(stand_in, img, result))
    keep("draw_labels", "draw_labels", rows, h=h, w=w, seed=5, idx=7, num_frames=120, model_input_shape=[512, 704], speed_ms=result.speed_ms)

    out["probs"] = PROBS
    np.savez_compressed(os.path.join(OUT, "text.npz"), **out)
    meta = dict(cases=cases, idx2label=[IDX2LABEL[i] for i in range(len(IDX2LABEL))],
                boxes_row="float64 [Nb,11]: x0, y0, x1, y1 (inclusive, frame coordinates, as the reference passed them: not clipped), opaque (1: "
                          "cv2.rectangle on the frame; 0: addWeighted on the slice), the two weights as the doubles the reference passed, r, g, b, "
                          "position in the call order",
                texts_row="float64 [Nt,8]: x, y of the origin the reference passed to putText, font_scale, r, g, b, thickness, position in the "
                          "call order; the strings are in `strings`",
                metrics="cv2.getTextSize answered from pytorch-human-pose_amd/keypoints/data/dejavu_sans_atlas.json (sum of advances, cap height): "
                        "parity of text metrics and glyph shapes with cv2's Hershey font is UNPINNED; box arithmetic, locs, weights, colours, "
                        "origins and strings are the reference's own code")
    with open(os.path.join(OUT, "text_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", os.path.getsize(os.path.join(OUT, "text.npz")), "bytes")


if __name__ == "__main__":
    main()
