"""The fused stem's input staging geometry (csrc/kernels.h: stem_unit and its helpers, shared by stem_fused.hip and the host) walked on
the host over every tile of H, W in {4 .. 140 step 4}: tools/stem_stage_host_check.cpp, built as a stand-alone program with
AddressSanitizer and UndefinedBehaviorSanitizer, checks that each patch element is covered exactly once and that every 16-byte
vector lies wholly inside or wholly outside the image."""
import os
import subprocess

from conftest import PKG, REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_stem_staging_covers_every_patch_element_once(tmp_path):
    exe = str(tmp_path / "stem_stage_host_check")
    build = subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=all", "-I", os.path.join(REPO, PKG, "csrc"), os.path.join(REPO, "tools", "stem_stage_host_check.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stem_stage_host_check: clean" in run.stdout and "12312 tiles" in run.stdout, run.stdout
