"""CPU: what hipcc makes of the k-NN kernel of csrc/skinning.hip.  Its per-lane K-entry list must live in LDS (a dynamically indexed
register array would go to scratch: private segment), and its LDS use is what DESIGN.md "Deformer construction" states: the list
32 x 256 x (4 + 4) B = 65,536 B plus the 512-vertex float4 tile 8,192 B = 73,728 B, two workgroups per CU."""
import os
import subprocess

import pytest

from tests.test_codegen_cpu import _body, _meta

KNN = "knn_kernel"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from intrinsicavatar_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path_factory.mktemp("codegen") / "skinning.s")
    cmd = [hipcc] + build.COMMON + build.SOURCES["skinning.hip"] + ["--offload-device-only", "-S",
                                                                    os.path.join(build.CSRC, "skinning.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return open(out).read()


def test_knn_kernel_has_no_private_segment_and_the_stated_lds(asm):
    m = _meta(asm, KNN)
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 32 * 256 * 8 + 512 * 16 == 73728, m
    assert m["vgpr_count"] <= 128, m                       # LDS allows 2 workgroups = 2 waves per SIMD; registers must not cut that


def test_knn_kernel_list_is_addressed_as_lds_without_atomics(asm):
    body = _body(asm, KNN)
    assert "ds_read" in body or "ds_load" in body
    assert "flat_load" not in body and "flat_store" not in body and "scratch_" not in body
    assert "atomic" not in body


@pytest.mark.parametrize("tag", ["skin_blend_kernel", "skin_smooth_kernel", "skin_grid_points_kernel"])
def test_other_kernels_have_no_scratch(asm, tag):
    m = _meta(asm, tag)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
