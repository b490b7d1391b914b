"""hh_cls_score_batch on the GPU, through the C-ABI and through ClsEvaluator, against the host twin and the restatement of the rule
(tests/cls_score_ref.py): integer outputs exactly, floating outputs inside the derived budgets, loss_sum / B against hh_softmax_xent,
the accumulator's bytes under every split, evaluate_images against infer_images' logits, validation_step with an evaluator.
The shapes are the smallest at which the kernel can go wrong (cls_score_ref.SHAPES: both sides of HH_CLS_ROW_REGS included)."""
import importlib

import numpy as np
import pytest
import torch

import cls_score_ref as cr
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = {cr.shape_id(s): (*cr.random_case(s[0], s[1]), s[2]) for s in cr.SHAPES}
CASES.update({name: (z, t, 5) for name, (z, t) in cr.content_cases().items()})


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module")
def cls():
    return importlib.import_module(PKG + ".classification")


@pytest.fixture(scope="module")
def refs():
    return {name: cr.restate(z, t, k) for name, (z, t, k) in CASES.items()}


def gpu_score(pkg, lib, z, t, k, confusion=True, calls=None, with_acc=True) -> dict:
    """hh_cls_score_batch over `calls` on one accumulator -> cls_score_ref.host_twin's dict, from device memory"""
    B, N = z.shape
    zd, td = z.to(DEV), None if t is None else t.to(DEV)
    out = {"topk_idx": torch.full((B, k), -7, dtype=torch.int32, device=DEV), "topk_prob": torch.full((B, k), -7.0, device=DEV),
           "rank": torch.full((B,), -7, dtype=torch.int32, device=DEV), "row_loss": torch.full((B,), -7.0, device=DEV)}
    acc = None
    if with_acc:
        acc = torch.full((lib.hh_cls_eval_bytes(N, int(confusion)) // 8,), -1, dtype=torch.int64, device=DEV)
        pkg._lib.launch(DEV, lib.hh_cls_eval_reset, acc.data_ptr(), N, int(confusion))
    b = 0
    for n in calls or [B]:
        pkg._lib.launch(DEV, lib.hh_cls_score_batch, zd[b:].data_ptr(), None if td is None else td[b:].data_ptr(), n, N, k, pkg._lib.ptr(acc),
                        out["topk_idx"][b:].data_ptr(), out["topk_prob"][b:].data_ptr(), out["rank"][b:].data_ptr(), out["row_loss"][b:].data_ptr())
        b += n
    out = {key: v.cpu() for key, v in out.items()}
    if with_acc:
        out.update(cr.parse_acc(acc.cpu().numpy().view(np.uint8), N, confusion))
    return out


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_twin_and_the_restatement(pkg, lib, refs, name):
    z, t, k = CASES[name]
    got, twin = gpu_score(pkg, lib, z, t, k), cr.host_twin(lib, z, t, k)
    for key in cr.INT_KEYS:
        same = torch.equal(got[key], twin[key]) if isinstance(got[key], torch.Tensor) else got[key] == twin[key]
        assert same, f"{name}: {key} differs from the host twin's"
    assert cr.mismatches(got, refs[name], name) == []
    assert not got["scratch"].any(), "the call scratch is zero between calls"


def test_all_equal_row_and_equal_maxima(pkg, lib):
    z, t, k = CASES["all-equal"]
    got = gpu_score(pkg, lib, z, t, k)
    assert got["topk_idx"].tolist() == [[0, 1, 2, 3, 4]] * 2 and got["rank"].tolist() == [0, 69]
    z, t, k = CASES["equal-maxima"]
    got = gpu_score(pkg, lib, z, t, k)
    assert got["topk_idx"][:, :2].tolist() == [[0, 64], [63, 64]] and got["rank"].tolist() == [1, 1]
    z, t, k = CASES["signed-zeros"]
    assert gpu_score(pkg, lib, z, t, k)["topk_idx"][:, :2].tolist() == [[2, 5], [2, 5]]


def test_without_targets_or_accumulator(pkg, lib):
    z, t, k = CASES["5x65x5"]
    full = gpu_score(pkg, lib, z, t, k)
    no_t = gpu_score(pkg, lib, z, None, k)
    assert torch.equal(no_t["topk_idx"], full["topk_idx"]) and torch.equal(no_t["topk_prob"], full["topk_prob"])
    assert no_t["rank"].tolist() == [-1] * 5 and no_t["row_loss"].tolist() == [0.0] * 5
    assert (no_t["rows"], no_t["flags"], float(no_t["loss_sum"])) == (0, 0, 0.0) and not no_t["per_class"].any()
    no_acc = gpu_score(pkg, lib, z, t, k, with_acc=False)
    for key in ("topk_idx", "topk_prob", "rank", "row_loss"):
        assert torch.equal(no_acc[key], full[key]), key
    zd, td = z.to(DEV), t.to(DEV)
    pkg._lib.launch(DEV, lib.hh_cls_score_batch, zd.data_ptr(), td.data_ptr(), 5, 65, 5, None, None, None, None, None)  # every output may be NULL
    torch.cuda.synchronize()
    with pytest.raises(pkg._lib.HHError, match="k must"):
        pkg._lib.launch(DEV, lib.hh_cls_score_batch, zd.data_ptr(), td.data_ptr(), 5, 65, 9, None, None, None, None, None)


@pytest.mark.parametrize("name", ["33x1000x5", "7x64x5", "5x65x5", "ties"])
def test_loss_and_hits_against_softmax_xent(pkg, lib, name):
    """Both are double sums of the same B row terms in different orders, rounded once: float(loss_sum / B) is within one fp32 ulp of
    hh_softmax_xent's loss; top1 / top5 are equal."""
    from importlib import import_module
    ops = import_module(PKG + ".keypoints.train_ops")
    z, t, k = CASES[name]
    B = z.shape[0]
    got = gpu_score(pkg, lib, z, t, k, confusion=False)
    result, _ = ops.softmax_xent(z.to(DEV), t.to(DEV), want_grad=False)
    r = result.cpu()
    xent = np.float32(r[:1].view(torch.float32).item())
    mine = np.float32(float(got["loss_sum"]) / B)
    print(name, "loss_sum / B", mine, "hh_softmax_xent", xent)
    assert got["rows"] == B and abs(float(mine) - float(xent)) <= float(np.spacing(xent))
    assert (got["top1"], got["topk"]) == (int(r[1]), int(r[2]))


@pytest.mark.parametrize("confusion", [False, True], ids=["plain", "confusion"])
def test_accumulator_bytes_do_not_depend_on_the_split(pkg, lib, cls, confusion):
    z, t, k = CASES["33x1000x5"]
    one = gpu_score(pkg, lib, z, t, k, confusion)["raw"]
    split = gpu_score(pkg, lib, z, t, k, confusion, calls=[1, 2, 30])["raw"]
    assert one.tobytes() == split.tobytes()
    # the same through ClsEvaluator
    ev = cls.ClsEvaluator(1000, 5, confusion, DEV)
    zd, td = z.to(DEV), t.to(DEV)
    outs = [ev.update(zd[a:b], td[a:b]) for a, b in ((0, 1), (1, 3), (3, 33))]
    assert ev.raw_state().tobytes() == one[:len(ev.raw_state())].tobytes()
    ref = cr.restate(z, t, 5, confusion)
    assert torch.equal(torch.cat([o["rank"] for o in outs]).cpu(), ref["rank"])
    res = ev.result()
    assert (res["n"], res["top-1_error"], res["top-5_error"]) == (33, 1 - ref["top1"] / 33, 1 - ref["topk"] / 33)
    assert res["loss"] == float(np.frombuffer(one[40:48].tobytes(), np.float64)[0]) / 33 and res["flags"] == 0
    assert np.array_equal(res["per_class_count"], ref["per_class"][0].numpy())
    if confusion:
        assert np.array_equal(res["confusion"], ref["conf"].numpy())
        conf = ref["conf"].numpy()
        want = sorted(((int(a), int(b), int(conf[a, b])) for a, b in zip(*np.nonzero(conf)) if a != b), key=lambda v: (-v[2], v[0], v[1]))[:5]
        assert ev.most_confused(5) == want
    else:
        assert res["confusion"] is None
    ev.reset()
    assert ev.result()["n"] == 0
    other = cls.ClsEvaluator(1000, 5, confusion, DEV)
    ev.update(zd[:10], td[:10]), other.update(zd[10:], td[10:])
    merged = ev.merge_(other.state()).result()
    assert (merged["n"], merged["top-1_error"], merged["top-5_error"]) == (33, res["top-1_error"], res["top-5_error"])
    assert merged["loss"] == pytest.approx(res["loss"], rel=1e-14) and np.array_equal(merged["per_class_count"], res["per_class_count"])
    assert ev.all_reduce() is ev  # no process group: a no-op


def test_evaluator_bad_targets_and_nonfinite_rows(pkg, cls):
    z, t = cr.content_cases()["out-of-range"]
    ev = cls.ClsEvaluator(10, 5, False, DEV)
    ev.update(z.to(DEV), t.to(DEV))
    with pytest.raises(IndexError, match="bad_target"):
        ev.result()
    r = ev.result(allow_bad_targets=True)
    assert (r["n"], r["bad_target"], r["flags"]) == (2, 2, 1)
    z, t = cr.content_cases()["nan-and-inf-rows"]
    ev = cls.ClsEvaluator(66, 5, False, DEV)
    ev.update(z.to(DEV), t.to(DEV))
    r = ev.result()
    assert (r["n"], r["nonfinite"], r["flags"]) == (3, 2, 2) and np.isfinite(r["loss"])
    with pytest.raises(ValueError):
        ev.update(z[:, :10].to(DEV), t.to(DEV))


@pytest.fixture(scope="module")
def tiny_model(pkg, cls):
    """a W32 net with seeded weights at 32 x 32, the smallest input the engine takes"""
    net = pkg.ClassificationHRNet(32, 1000)
    net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 3)) for k, v in net.state_dict().items()})
    return cls.InferenceClassificationModel(net, {i: f"class-{i}" for i in range(1000)}, input_size=32, device=DEV)


def test_evaluate_images_equals_scoring_infer_images_logits(pkg, cls, tiny_model):
    jp = importlib.import_module(PKG + ".keypoints.jpeg")
    rs = np.random.RandomState(5)
    arrays = [rs.randint(0, 256, (40 + 3 * i, 56 - 2 * i, 3)).astype(np.uint8) for i in range(12)]
    images = [jp.encode_jpeg_host(a, 90, "420") if i % 3 == 1 else a for i, a in enumerate(arrays)]  # arrays and JPEG bytes, mixed
    records = tiny_model.infer_images(images, max_batch=5)
    logits = torch.from_numpy(np.stack([r.logits for r in records]))
    targets = [int(torch.topk(logits[i], 8).indices[i % 8]) for i in range(12)]  # ranks 0..7: hits and misses of both kinds
    ref = cr.restate(logits, torch.tensor(targets), 5)
    result, light = cls.evaluate_images(tiny_model, images, targets, max_batch=5, k=5, confusion=True, records=True)
    assert (result["n"], result["top-1_error"], result["top-5_error"]) == (12, 1 - ref["top1"] / 12, 1 - ref["topk"] / 12)
    assert ref["top1"] == 2 and ref["topk"] == 9
    assert np.array_equal(result["confusion"], ref["conf"].numpy()) and np.array_equal(result["per_class_count"], ref["per_class"][0].numpy())
    cr.check(torch.tensor([result["loss"] * 12]), *ref["loss_sum"], "evaluate_images loss_sum", spatial=False)
    assert len(light) == 12
    for i, rec in enumerate(light):
        assert rec.topk_idx.tolist() == ref["topk_idx"][i].tolist() and rec.rank == int(ref["rank"][i]) == i % 8
        assert rec.labels == [f"class-{j}" for j in rec.topk_idx] and rec.target_label == f"class-{targets[i]}"
        assert rec.topk_idx[0] == records[i].prediction
    cr.check(torch.from_numpy(np.stack([r.topk_prob for r in light])), *ref["topk_prob"], "records' topk_prob", spatial=False)
    plain = cls.evaluate_images(tiny_model, images, targets, max_batch=5)
    assert plain["confusion"] is None and (plain["n"], plain["top-1_error"], plain["loss"]) == (12, result["top-1_error"], result["loss"])
    # infer_topk: the same records without an evaluator; labels or indices as targets
    top = tiny_model.infer_topk(images, target_labels=[f"class-{t}" for t in targets[:6]] + targets[6:11] + ["no such label"], k=5, max_batch=5)
    assert [r.rank for r in top] == [i % 8 for i in range(11)] + [-1]
    assert all(a.topk_idx.tolist() == b.topk_idx.tolist() and np.array_equal(a.topk_prob, b.topk_prob) for a, b in zip(top, light))
    assert [r.rank for r in tiny_model.infer_topk(images[:2], k=3)] == [-1, -1]


def test_validation_step_with_an_evaluator(pkg, cls, tiny_model):
    model = cls.ClassificationModel(tiny_model.net)
    opt = torch.optim.SGD(model.net.parameters(), lr=0.01)
    batch = (torch.from_numpy(pkg.synth.synth_images(4, 32, 32, seed=2)).to(DEV), torch.tensor([3, 141, 592, 653], device=DEV))
    metrics0, results0 = cls.ClassificationModule(model, cls.ClassificationLoss(), opt).validation_step(batch, 0)
    ev = cls.ClsEvaluator(1000, 5, True, DEV)
    module = cls.ClassificationModule(model, cls.ClassificationLoss(), opt, evaluator=ev)
    metrics1, results1 = module.validation_step(batch, 0)
    assert metrics1 == metrics0 and all(np.array_equal(a.logits, b.logits) and a.prediction == b.prediction for a, b in zip(results0, results1))
    r = ev.result()
    assert (r["n"], r["top-1_error"], r["top-5_error"]) == (4, metrics0["top-1_error"], metrics0["top-5_error"])
    assert abs(np.float32(r["loss"]) - np.float32(metrics0["loss"])) <= np.spacing(np.float32(metrics0["loss"]))
    module.validation_step(batch, 1)
    assert ev.result()["n"] == 8
