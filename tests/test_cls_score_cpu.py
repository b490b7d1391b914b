"""The classifier's scoring tail without a GPU: the host twin hh_cls_score_host against the restatement of the rule
(tests/cls_score_ref.py) -- integers exactly, floating outputs inside the derived budgets --, top-1 / top-k against the reference's
get_metrics on tie-free rows, the fp32 model inside every budget and every planted defect outside one, the batching invariance of the
twin's accumulator bytes, the Python around the kernel, and the public names."""
import importlib
import os

import numpy as np
import pytest
import torch

import cls_score_ref as cr
from conftest import PKG

CASES = {cr.shape_id(s): (*cr.random_case(s[0], s[1]), s[2]) for s in cr.SHAPES}
CASES.update({name: (z, t, 5) for name, (z, t) in cr.content_cases().items()})


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module")
def refs():
    return {name: cr.restate(z, t, k) for name, (z, t, k) in CASES.items()}


# ------------------------------------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("name", CASES)
def test_host_twin_matches_the_restatement(lib, refs, name):
    z, t, k = CASES[name]
    got = cr.host_twin(lib, z, t, k)
    assert cr.mismatches(got, refs[name], name) == []
    assert not got["scratch"].any(), "the call scratch is zero between calls"


@pytest.mark.parametrize("name", ["33x1000x5", "minus-inf", "ties"])
def test_host_twin_double_loss_within_the_row_budget(lib, refs, name):
    """The accumulator keeps the double loss: after a one-row call loss_sum IS that double.  It is held to xent_refs' per-row term as it
    stands (no fp32 rounding in it)."""
    z, t, k = CASES[name]
    ref, allowed = refs[name]["loss64"]
    for b in torch.nonzero(refs[name]["scored"]).view(-1).tolist():
        got = cr.host_twin(lib, z[b:b + 1], t[b:b + 1], k, confusion=False)["loss_sum"]
        if torch.isinf(ref[b]):
            assert float(got) == float("inf")
        else:
            cr.check(got, ref[b:b + 1], allowed[b:b + 1], f"{name} row {b} double loss", spatial=False)


def test_host_twin_without_targets_or_accumulator(lib):
    z, t, k = CASES["5x65x5"]
    full = cr.host_twin(lib, z, t, k)
    no_t = cr.host_twin(lib, z, None, k)  # an accumulator is passed and must stay as reset
    assert torch.equal(no_t["topk_idx"], full["topk_idx"]) and torch.equal(no_t["topk_prob"], full["topk_prob"])
    assert no_t["rank"].tolist() == [-1] * 5 and no_t["row_loss"].tolist() == [0.0] * 5
    assert (no_t["rows"], no_t["nonfinite"], no_t["flags"], float(no_t["loss_sum"])) == (0, 0, 0, 0.0) and not no_t["per_class"].any()
    no_acc = cr.host_twin(lib, z, t, k, with_acc=False)
    for key in ("topk_idx", "topk_prob", "rank", "row_loss"):
        assert torch.equal(no_acc[key], full[key]), key
    # every output pointer may be NULL
    zn, tn = z.numpy(), t.numpy()
    assert lib.hh_cls_score_host(zn.ctypes.data, tn.ctypes.data, 5, 65, 5, None, None, None, None, None) == 0


def test_host_twin_refuses_bad_arguments(lib):
    z = np.zeros((2, 4), np.float32)
    for B, N, k in ((1025, 4, 1), (-1, 4, 1), (2, 0, 1), (2, 65537, 1), (2, 4, 0), (2, 4, 9)):
        assert lib.hh_cls_score_host(z.ctypes.data, None, B, N, k, None, None, None, None, None) == 1, (B, N, k)
    assert lib.hh_cls_score_host(None, None, 2, 4, 1, None, None, None, None, None) == 1
    assert lib.hh_cls_score_host(z.ctypes.data, None, 2, 4, 1, None, z.ctypes.data + 2, None, None, None) == 1  # misaligned output
    assert lib.hh_cls_eval_bytes(0, 0) == -1 and lib.hh_cls_eval_bytes(10, 2) == -1
    assert lib.hh_cls_eval_bytes(1000, 0) == 64 + 12 * 1000 + 12 * 1024
    assert lib.hh_cls_eval_bytes(5, 1) == 64 + 60 + 100 + 12 * 1024
    # an accumulator reset for another N: the call raises the layout flag and touches nothing else
    acc = np.zeros(lib.hh_cls_eval_bytes(4, 1) // 8, np.int64)
    assert lib.hh_cls_eval_reset_host(acc.ctypes.data, 3, 0) == 0
    before = acc.copy()
    t = np.array([1, 2], np.int64)
    assert lib.hh_cls_score_host(z.ctypes.data, t.ctypes.data, 2, 4, 1, acc.ctypes.data, None, None, None, None) == 0
    flags = acc.view(np.uint32)[12]
    assert flags == 4
    acc.view(np.uint32)[12] = 0
    assert np.array_equal(acc, before)


@pytest.mark.parametrize("confusion", [False, True])
@pytest.mark.parametrize("name", ["33x1000x5", "nan-and-inf-rows", "out-of-range", "3x1025x5"])
def test_host_twin_batching_invariance(lib, name, confusion):
    z, t, k = CASES[name]
    B = z.shape[0]
    one = cr.host_twin(lib, z, t, k, confusion)["raw"]
    split = cr.host_twin(lib, z, t, k, confusion, calls=[1, 2, B - 3])["raw"]
    assert one.tobytes() == split.tobytes()


# ------------------------------------------------------------------------------------------------ against the reference's metrics
def test_top1_topk_equal_the_references_get_metrics_on_tie_free_rows(lib):
    """src/classification/module.py get_metrics: torch.topk(logits, 5) on the CPU, hits where the target is among them."""
    for name in ("33x1000x5", "4x1001x8", "7x64x5"):
        z, t, k = CASES[name]
        assert all(len(set(row.tolist())) == z.shape[1] for row in z), "tie-free"
        top = torch.topk(z, k, dim=1).indices
        top1, topk = int((top[:, 0] == t).sum()), int((top == t.view(-1, 1)).any(1).sum())
        got = cr.host_twin(lib, z, t, k)
        assert (got["top1"], got["topk"]) == (top1, topk)
        assert torch.equal(got["topk_idx"].long(), top)


# ------------------------------------------------------------------------------------------------ the model and its defects
@pytest.mark.parametrize("name", CASES)
def test_model_within_every_budget(refs, name):
    z, t, k = CASES[name]
    assert cr.mismatches(cr.model(z, t, k), refs[name], name) == []


def _found(defect, names, calls=None):
    return {n: cr.mismatches(cr.model(*CASES[n][:2], CASES[n][2], calls=calls, defect=defect), cr.restate(*CASES[n]), n) for n in names}


def test_every_planted_defect_leaves_a_named_case():
    assert _found("tie_high", ["ties", "all-equal"]) == {"ties": ["topk_idx", "rank", "topk", "per_class", "conf"],
                                                          "all-equal": ["topk_idx", "rank", "per_class", "conf"]}
    assert _found("le_hit", ["ties"]) == {"ties": ["topk", "per_class"]}                      # rows 2 and 3 have rank exactly 5
    assert _found("conf_T", ["33x1000x5"]) == {"33x1000x5": ["conf"]}
    assert {"rank", "rows", "per_class", "row_loss", "loss_sum"} <= set(_found("bad_counted", ["out-of-range"])["out-of-range"])
    assert {"rows", "nonfinite", "flags"} <= set(_found("nan_scored", ["nan-and-inf-rows"])["nan-and-inf-rows"])
    assert _found("k_unclamped", ["3x3x5"]) == {"3x3x5": ["topk_idx", "topk_prob"]}
    # loss_sum folded per call in fp32: the rows' own budgets (33 x 6 U32 and more) hide an fp32 rounding of the sum, so the named case is
    # the batching invariance: the result depends on the split
    z, t, k = CASES["33x1000x5"]
    a, b = cr.model(z, t, k, defect="fp32_fold")["loss_sum"], cr.model(z, t, k, calls=[1, 2, 30], defect="fp32_fold")["loss_sum"]
    assert float(a) != float(b)
    assert float(cr.model(z, t, k)["loss_sum"]) == float(cr.model(z, t, k, calls=[1, 2, 30])["loss_sum"])


# ------------------------------------------------------------------------------------------------ the Python around the kernel
@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".classification.evaluation")


def test_image_folder_items(ev, tmp_path):
    for d, files in (("n02", ["b.JPEG", "a.jpg", "notes.txt"]), ("n01", ["x.png"]), ("n10", [])):
        os.makedirs(tmp_path / d)
        for f in files:
            (tmp_path / d / f).write_bytes(b"")
    os.makedirs(tmp_path / "n02" / "sub")
    (tmp_path / "n02" / "sub" / "c.jpg").write_bytes(b"")
    (tmp_path / "stray.jpg").write_bytes(b"")
    paths, targets, idx2label = ev.image_folder_items(str(tmp_path))
    rel = [os.path.relpath(p, tmp_path) for p in paths]
    assert rel == ["n01/x.png", "n02/a.jpg", "n02/b.JPEG", "n02/sub/c.jpg"] and targets == [0, 1, 1, 1]
    assert idx2label == {0: "n01", 1: "n02", 2: "n10"}
    _, _, named = ev.image_folder_items(str(tmp_path), {"0": ["n01", "tench"], "1": ["n02", "goldfish"], 2: ["n10", "shark"]})
    assert named == {0: "tench", 1: "goldfish", 2: "shark"}
    with pytest.raises(FileNotFoundError):
        ev.image_folder_items(str(tmp_path / "n10"))


def test_most_confused_ordering(ev):
    conf = np.zeros((4, 4), np.int32)
    conf[2, 2] = 50                       # the diagonal never counts
    conf[3, 0], conf[1, 2], conf[0, 1], conf[2, 3] = 4, 4, 7, 1
    assert ev.most_confused(conf, 10) == [(0, 1, 7), (1, 2, 4), (3, 0, 4), (2, 3, 1)]
    assert ev.most_confused(conf, 2) == [(0, 1, 7), (1, 2, 4)]


def test_state_roundtrip_merge_and_summary(ev, lib):
    z, t, k = CASES["ties"]
    N = z.shape[1]
    a = cr.host_twin(lib, z[:2], t[:2], k)["raw"]
    b = cr.host_twin(lib, z[2:], t[2:], k)["raw"]
    whole = cr.host_twin(lib, z, t, k)["raw"]
    n = ev.state_bytes(N, True)
    sa, sb = ev.parse_state(a[:n], N, True), ev.parse_state(b[:n], N, True)
    assert ev.pack_state(sa).tobytes() == a[:n].tobytes()
    merged = ev.merge_states(sa, sb)
    sw = ev.parse_state(whole[:n], N, True)
    assert float(merged["header"]["loss_sum"]) == float(sa["header"]["loss_sum"]) + float(sb["header"]["loss_sum"])
    assert float(merged["header"]["loss_sum"]) == pytest.approx(float(sw["header"]["loss_sum"]), rel=1e-14)
    merged["header"]["loss_sum"] = sw["header"]["loss_sum"]      # (the sum of two shard sums is another order of additions)
    assert ev.pack_state(merged).tobytes() == whole[:n].tobytes()
    r = ev.summarize(merged, k)
    assert (r["n"], r["top-1_error"], r["top-5_error"]) == (6, 1 - 1 / 6, 1 - 4 / 6)
    assert r["loss"] == float(merged["header"]["loss_sum"]) / 6 and r["per_class_count"].tolist() == [0, 0, 1, 0, 2, 3, 0, 0, 0, 0]
    assert np.isnan(r["per_class_accuracy"][0]) and r["per_class_accuracy"][2] == 1.0 and r["confusion"].sum() == 6
    z, t = cr.content_cases()["out-of-range"]
    s = ev.parse_state(cr.host_twin(lib, z, t, 5)["raw"][:ev.state_bytes(10, True)], 10, True)
    with pytest.raises(IndexError, match="bad_target"):
        ev.summarize(s, 5)
    assert ev.summarize(s, 5, allow_bad_targets=True)["bad_target"] == 2


def test_public_names(pkg, lib):
    for name in ("hh_cls_eval_bytes", "hh_cls_eval_reset", "hh_cls_eval_reset_host", "hh_cls_score_batch", "hh_cls_score_host"):
        assert name in pkg._lib.exported_symbols() and hasattr(lib, name), name
    assert lib.hh_abi_version() == 3
    assert (pkg._lib.const("CLS_TOPK_MAX"), pkg._lib.const("CLS_ROW_REGS")) == (cr.K_MAX, cr.ROW_REGS)
    ev = importlib.import_module(PKG + ".classification.evaluation")
    assert ev.ACC_HEADER.itemsize == 64 and "hh_cls_eval_acc" not in pkg._lib.parse_structs(open(pkg._lib.HEADER).read())  # (the ABI's set of structs is closed)
    cls = importlib.import_module(PKG + ".classification")
    for name in ("ClsEvaluator", "evaluate_images", "image_folder_items", "ClsTopK", "score_logits"):
        assert hasattr(cls, name) and name in cls.__all__, name
    assert hasattr(cls.InferenceClassificationModel, "infer_topk")
    import inspect
    assert inspect.signature(cls.ClassificationModule.__init__).parameters["evaluator"].default is None
