"""CPU: what hipcc makes of the early-filter search kernel (broyden_spec_kernel<false, true, 256, 1>, the product instantiation of
csrc/snarf.hip).  The kernel runs 5 waves per SIMD only inside 96 VGPRs and 31,540 B of LDS, with no scratch; its fetch serves the
leader cell of the wave through scalar loads (s_load_dwordx8 / s_load_dwordx4 at an SGPR offset off the grid base).  A change that
loses any of that compiles cleanly and runs slower, so it is checked here, without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "broyden_spec_kernelILb0ELb1ELi256ELi1E"      # <COUNT = false, PACK = true, WG = 256, SCELLS = 1>
PLAIN = "broyden_spec_kernelILb0ELb1ELi256ELi0E"       # IA_BR_SPEC_SCALAR=0


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from intrinsicavatar_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path_factory.mktemp("codegen") / "snarf.s")
    cmd = [hipcc] + build.COMMON + build.SOURCES["snarf.hip"] + ["--offload-device-only", "-S",
                                                                 os.path.join(build.CSRC, "snarf.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return open(out).read()


def _meta(asm, tag):
    """the amdhsa.kernels metadata entry of the one kernel whose symbol contains tag."""
    entries = [e for e in asm[asm.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name:\s+\S*" + tag, e)]
    assert len(entries) == 1, tag
    return {k: int(re.search(r"\." + k + r":\s+(\d+)", entries[0]).group(1))
            for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                      "group_segment_fixed_size")}


def _body(asm, tag):
    m = re.search(r"^(\S*" + tag + r"\S*):", asm, re.M)
    assert m, tag
    return asm[m.end():asm.index(".Lfunc_end", m.end())]


@pytest.mark.parametrize("tag", [KERNEL, PLAIN])
def test_search_kernel_keeps_five_waves_without_scratch(asm, tag):
    m = _meta(asm, tag)
    assert m["vgpr_count"] <= 96, m                    # 512 / 5 rounded down to the allocation granule: 5 waves per SIMD
    assert m["vgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m     # no scratch at all
    assert m["group_segment_fixed_size"] <= 31540, m   # five workgroups in the CU's 160 KB
    # SGPRs that do not fit are kept in lanes of a VGPR (v_writelane / v_readlane, counted in vgpr_count above), not in scratch.  The
    # plain kernel needs none; the scalar fetch's 24 SGPRs per phase push out the kernel-argument pointers of the refill and record
    # blocks (19 dwords), which measured faster than the variants that keep fewer of them there
    assert m["sgpr_spill_count"] <= (24 if tag == KERNEL else 0), m


def test_search_kernel_fetch_uses_scalar_loads(asm):
    body = _body(asm, KERNEL)
    # four (y, z) phases x two corners: 12 dwords each at a readfirstlane offset (SGPR soffset), 8 + 4
    x8 = re.findall(r"s_load_dwordx8 s\[\d+:\d+\], s\[\d+:\d+\], s\d+", body)
    x4 = re.findall(r"s_load_dwordx4 s\[\d+:\d+\], s\[\d+:\d+\], s\d+", body)
    assert len(x8) >= 8 and len(x4) >= 8, (len(x8), len(x4))
    assert len(re.findall(r"global_load_dwordx4", body)) == 24     # the other lanes: six 16-byte loads per phase, as before
    plain = _body(asm, PLAIN)
    assert not re.findall(r"s_load_dwordx\d+ s\[\d+:\d+\], s\[\d+:\d+\], s\d+", plain)
