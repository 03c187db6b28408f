"""Work areas without a GPU: the carver of intrinsicavatar_amd/csrc/ia_scratch.h under the address / undefined-behaviour sanitizers
(tests/scratch_harness.cpp, a stand-alone host program), the size queries of the built library against the table recorded from the
commit before the layout functions (tests/golden/scratch_sizes.json), the untimed entry points against the header, and the
spellings the layout functions replaced."""
import importlib.util
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "intrinsicavatar_amd")


def test_carver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scratch_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "scratch_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "scratch_harness OK" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]


def _make_sizes():
    spec = importlib.util.spec_from_file_location("make_scratch_sizes", os.path.join(HERE, "golden", "make_scratch_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def size_rows():
    """[(fn, args, bytes before the layout functions, bytes of this tree)]"""
    from intrinsicavatar_amd import build
    assert "IA_ENV_ACC_MIN_F" not in os.environ, "the recorded table holds the default threshold of ia_pbr_shade_bwd_scratch_bytes"
    new = _make_sizes().table(build.build())
    old = json.load(open(os.path.join(HERE, "golden", "scratch_sizes.json")))
    assert [(r["fn"], r["args"]) for r in new] == [(r["fn"], r["args"]) for r in old], "the recorded table has other rows than make_scratch_sizes.py"
    return [(o["fn"], o["args"], o["bytes"], n["bytes"]) for o, n in zip(old, new)]


def test_size_table_covers_every_query(size_rows):
    from intrinsicavatar_amd import _lib
    queries = {n for n in _lib.header_prototypes() if n.endswith("_bytes") or n == "ia_hashgrid_fwd_levels_jac_offset"}
    assert queries == {fn for fn, _, _, _ in size_rows}
    assert {"ia_pack_info_tmp_bytes", "ia_deform_rows_pack_split_tmp_bytes"} <= queries


def test_sizes_stay_within_the_footprint_bound(size_rows):
    """no layout has more than 8 pieces of at most 256 bytes of alignment each + 256 of base slack: a work area may grow by at most
    4096 bytes, and only excess slack may go (at most 4096 too); 0 / -1 (`no work area` / `bad arguments`) stay; the Jacobian
    offset, which Python reads through, is unchanged exactly."""
    bad = []
    for fn, args, old, new in size_rows:
        if fn == "ia_hashgrid_fwd_levels_jac_offset" or old in (0, -1):
            ok = new == old
        else:
            ok = old - 4096 <= new <= old + 4096
        if not ok:
            bad.append((fn, args, old, new))
    assert not bad, "\n".join(map(str, bad))


def test_untimed_entry_points_are_the_stream_less_prototypes():
    """the binding wraps an entry point (stream, status, events) iff it can launch work, i.e. iff its prototype takes an ia_stream_t"""
    from intrinsicavatar_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "ia_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    stream_less = {name for name, args in re.findall(r"\b(ia_\w+)\s*\(([^()]*)\)\s*;", hdr) if "ia_stream_t" not in args}
    assert _lib.header_host_only() == stream_less
    assert {"ia_scan_tmp_bytes", "ia_pbr_shade_bwd_scratch_bytes", "ia_sort_rank_mode", "ia_pack_info_tmp_bytes", "ia_version"} <= stream_less
    assert "ia_exclusive_scan_i32" not in stream_less and "ia_pack_info" not in stream_less
    build.build()
    l = _lib.lib()
    assert l._untimed == stream_less
    for name in _lib.header_prototypes():
        wrapped = getattr(l, name) is not getattr(l._cdll, name)
        assert wrapped == (name not in stream_less), name


def test_no_hand_written_alignment_or_size_arithmetic_left():
    """the spellings the layout functions replaced: rounding up to 256 by hand in the kernels' host code, and byte counts added by
    hand in the Python wrappers"""
    hits = []
    for d, ext, pats in ((os.path.join(PKG, "csrc"), (".hip",), ("+ 255) &", "+ 255) / 256")),
                         (PKG, (".py",), ("+ 255) &", "+ 255) / 256", "extra_bytes="))):
        for f in sorted(os.listdir(d)):
            if f.endswith(ext):
                for i, line in enumerate(open(os.path.join(d, f)), 1):
                    hits += [(f, i, p) for p in pats if p in line]
    assert not hits, hits
