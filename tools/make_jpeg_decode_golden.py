"""Writes tests/golden/jpeg_decode.npz (+ jpeg_decode_meta.json): JPEG streams made by Pillow (libjpeg-turbo) and by this project's own
host encoder, each with Pillow's decoded RGB, `np.array(Image.open(...).convert("RGB"))`: the bytes the decoder must reproduce.  Needs
Pillow; the tests that read the file do not.  Run from the repository root after build():

    python tools/make_jpeg_decode_golden.py

Content comes from tests/test_jpeg_cpu.picture (scene, noise, flat).  Keys: s_<name> the stream, p_<name> the pixels.
This Pillow writes custom quantiser tables with entries above 255 as SOF1 (extended sequential), which the decoder refuses by name; the
16-bit-table case is therefore a Pillow SOF0 stream whose DQT segments are rewritten here at 16-bit precision, decoded by Pillow."""
import importlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PIL_SUB = {420: 2, 422: 1, 444: 0}

# (sampling, h, w, content, quality, variant); sampling 400: grayscale
CASES = [(420, h, w, "scene", 90, "plain") for h, w in [(1, 1), (8, 8), (16, 4), (16, 5), (17, 23), (33, 50), (130, 24)]]
CASES += [(420, 36, 44, "noise", q, "plain") for q in (1, 90)]
CASES += [(420, h, w, "noise", 75, "plain") for h, w in [(1, 1), (16, 4), (16, 5)]]
CASES += [(420, h, w, c, q, "plain") for h, w in [(17, 23), (33, 50)] for c in ("scene", "noise") for q in (1, 30, 75, 100)]
CASES += [(420, 8, 8, "flat", 90, "plain"), (420, 16, 5, "flat", 75, "plain")]
CASES += [(422, h, w, c, 90, "plain") for h, w in [(9, 37), (21, 43), (8, 4)] for c in ("scene", "noise")]
CASES += [(422, 21, 43, "noise", 1, "plain"), (444, 17, 23, "scene", 90, "plain"), (444, 17, 23, "noise", 30, "plain"),
          (400, 17, 23, "scene", 90, "plain"), (400, 17, 23, "noise", 75, "plain")]
CASES += [(420, 33, 50, "noise", 75, "optimize"), (420, 17, 23, "scene", 75, "q16")]
CASES += [(420, 33, 50, "scene", 90, "rows1"), (420, 130, 24, "noise", 90, "rows1"), (422, 21, 43, "noise", 90, "rows1"),
          (444, 17, 23, "noise", 75, "rows1"), (400, 17, 23, "noise", 75, "rows1")]
CASES += [(420, 33, 50, "noise", 90, "blocks3"), (422, 9, 37, "scene", 75, "blocks3")]
CASES += [(420, 120, 200, "scene", 90, "plain"), (420, 120, 200, "scene", 90, "rows1")]  # (large enough for the bytes-saved comparison)
CASES += [(420, 33, 50, "scene", 90, "own"), (444, 17, 23, "noise", 75, "own"), (420, 130, 24, "scene", 90, "own")]


def name_of(case) -> str:
    sub, h, w, content, q, variant = case
    return f"{sub}_{h}x{w}_{content}_q{q}_{variant}"


def widen_dqt(data: bytes) -> bytes:
    """The same stream with every DQT table at 16-bit precision."""
    out, i = bytearray(data[:2]), 2
    while True:
        m, L = data[i + 1], data[i + 2] << 8 | data[i + 3]
        if m == 0xdb:
            s, k, body = data[i + 4:i + 2 + L], 0, bytearray()
            while k < L - 2:
                assert s[k] >> 4 == 0
                body.append(0x10 | s[k])
                for v in s[k + 1:k + 65]:
                    body += bytes([0, v])
                k += 65
            out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
        else:
            out += data[i:i + 2 + L]
        i += 2 + L
        if m == 0xda:
            return bytes(out) + data[i:]


def make(J=None) -> tuple[dict, list]:
    from PIL import Image
    from test_jpeg_cpu import picture
    if J is None:
        J = importlib.import_module("pytorch-human-pose_amd.keypoints.jpeg")
    arrays, meta = {}, []
    for case in CASES:
        sub, h, w, content, q, variant = case
        img = picture(content, h, w)
        if variant == "own":
            data = J.encode_jpeg_host(img, q, sub)
        else:
            kw = {"optimize": dict(optimize=True), "rows1": dict(restart_marker_rows=1), "blocks3": dict(restart_marker_blocks=3)}.get(variant, {})
            buf = io.BytesIO()
            if sub == 400:
                Image.fromarray(img[:, :, 1]).save(buf, "JPEG", quality=q, **kw)
            else:
                Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=PIL_SUB[sub], **kw)
            data = buf.getvalue()
            if variant == "q16":
                data = widen_dqt(data)
        pixels = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
        assert pixels.shape == (h, w, 3)
        name = name_of(case)
        arrays["s_" + name] = np.frombuffer(data, np.uint8)
        arrays["p_" + name] = pixels
        meta.append(dict(name=name, sampling=sub, h=h, w=w, content=content, quality=q, variant=variant, bytes=len(data)))
    return arrays, meta


if __name__ == "__main__":
    import PIL
    from PIL import features
    arrays, meta = make()
    out = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out, "jpeg_decode.npz"), **arrays)
    with open(os.path.join(out, "jpeg_decode_meta.json"), "w") as f:
        json.dump(dict(pillow=PIL.__version__, libjpeg=features.version("jpg"), libjpeg_turbo=bool(features.check_feature("libjpeg_turbo")), entries=meta), f,
                  indent=1)
    print(len(meta), "entries,", os.path.getsize(os.path.join(out, "jpeg_decode.npz")), "bytes")
