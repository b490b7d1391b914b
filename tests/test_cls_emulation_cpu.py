"""The figures that widen two bounds of tests/test_gpu_cls_train.py are what tests/cls_emulation.py gives: its bf16-storage emulation of
the classifier's training step, run here on the CPU against the golden and the fp32 oracle, reproduces the recorded EMULATION_DEVIATION
(to the third decimal: thread counts reorder fp32 sums), and is itself inside the bounds the GPU test derives from it."""
import cls_emulation as ce


def test_recorded_emulation_deviation_is_what_the_emulation_gives():
    got = ce.measure()
    print({k: (round(v, 5) if isinstance(v, float) else v) for k, v in got.items() if not hasattr(v, "shape")})
    for k, want in ce.EMULATION_DEVIATION.items():
        tol = 2e-5 if k == "loss_rel" else 5e-3
        assert abs(got[k] - want) < tol, (k, got[k], want)
    for k, want in ce.EMULATION_STAT_DISTANCE.items():
        assert abs(got["stat_distance"][k] - want) < 0.05 * want, (k, got["stat_distance"][k], want)
    # the unwidened bounds that the emulation itself keeps: loss within 0.3 %, logits within 4 % of max, median norm ratio within 2 %
    assert got["loss_rel"] < 3e-3 and got["logits"] < 4e-2 and abs(got["ratio_median"] - 1) < 0.02
    # ... and the two it does not, which is why the GPU test takes 1.5 x its deviation instead: norms within 10 %, cosine > 0.92 / median > 0.98
    assert got["ratio_min"] < 0.90 and got["ratio_max"] > 1.10 and got["cos_min"] < 0.92 and got["cos_median"] < 0.98
