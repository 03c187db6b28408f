"""Size table of every work-area query of the C ABI (`ia_*_bytes`, ia_hashgrid_fwd_levels_jac_offset).

    IA_AMD_LIB=<libia_amd.so of the commit to record> python tests/golden/make_scratch_sizes.py > tests/golden/scratch_sizes.json

No GPU: the queries are host arithmetic.  tests/test_scratch_cpu.py imports table() and compares the library of the tree with
the recorded file, which holds the figures of the commit BEFORE the layout functions (sizes summed by hand next to each carve).
Queries that commit did not have are recorded as what its Python callers allocated (PARENT_PYTHON below)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

COMMON = [0, 1, 4096, 540 * 540, (1 << 21) + 3]
HASH = dict(n_levels=16, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.447269237440378)       # fields.HASH


def around(*tiles):
    return sorted(set(COMMON + [t + d for t in tiles for d in (-1, 0, 1)]))


def _hash_bwd(n, n_levels):
    return (n, n_levels, HASH["log2_hashmap_size"], HASH["base_resolution"], HASH["per_level_scale"])


# query -> argument tuples: 0, 1, one below / at / one above the entry's own tile size (the constant named in the comment), 4096,
# 540 x 540, 2^21 + 3
CASES = {
    "ia_scan_tmp_bytes": [(n,) for n in around(1024, 1 << 15, 1 << 20)],                  # SCAN_TILE, SCAN_SMALL_MAX, SCAN_TILE^2
    "ia_traverse_scratch_bytes": [(n,) for n in COMMON],
    "ia_traverse_fused_scratch_bytes": [(n,) for n in around(256)],                       # TR_THREADS
    "ia_pack_info_tmp_bytes": [(n,) for n in around(1024, 1 << 15)],                      # the scan's
    "ia_resample_tmp_bytes": [(n, 4 * n, k) for n in around(64) for k in (2, 16)],        # 256-byte pieces of 4-byte elements
    "ia_spec_rows_overflow_bytes": [(n,) for n in around(1 << 24)],                       # N / 64 above the minimum capacity 2^18
    "ia_deform_rows_pack_split_tmp_bytes": [(n,) for n in around(1024)],                  # FIRST_TILE
    "ia_hashgrid_fwd_scratch_bytes": [(n, L, j) for n in around(32) for L in (HASH["n_levels"], 1) for j in (0, 1)],
    "ia_hashgrid_fwd_levels_jac_offset": [(n, L) for n in around(32) for L in (HASH["n_levels"], 1)],
    "ia_hashgrid_bwd_scratch_bytes": [_hash_bwd(n, L) for n in around(128, 1024) for L in (HASH["n_levels"], 1)],   # U_PTS, BIN_TILE
    "ia_deform_filter_compact_tmp_bytes": [(n,) for n in around(256)],                    # FCC_ROWS
    "ia_deform_filter_tiles_tmp_bytes": [(n,) for n in around(256)],
    "ia_pbr_shade_bwd_scratch_bytes": [(n,) for n in around(8192, 1 << 18)],              # ENV_TILE, ENV_ACC_MIN_F
    "ia_occgrid_tmp_bytes": [(n, 1, 1) for n in around(256)] + [(16, 16, 16), (64, 64, 64)],          # THREADS
    "ia_morton_order_tmp_bytes": [(n,) for n in around(16384, 1 << 20)],                  # TILE, SCAN_CHUNK tiles
    "ia_sg_image_bwd_tmp_bytes": [(k,) for k in (0, 1, 255, 256, 257, 4096)],
    "ia_envlight_pdf_tables_tmp_bytes": [(1, n) for n in around(1024)] + [(540, 540), (256, 512)],    # PDF_TILE
    "ia_phys_loss_tmp_bytes": [(n,) for n in around(1024, 16384)],
    "ia_mc_scratch_bytes": [(n, 1, 1) for n in around(256)] + [(3, 3, 3), (128, 128, 128)],           # MC_THREADS
    "ia_metric_tmp_bytes": [()],
    "ia_metric_ssim_tmp_bytes": [(h, w, 3) for h, w in ((0, 0), (1, 1), (24, 24), (37, 38), (38, 38), (39, 38), (540, 540), (4096, 4096))],   # TS + 2 SSIM_PAD
    "ia_flag_lists_scratch_bytes": [(2, n) for n in around(256)] + [(0, 0), (7, 540 * 540)],          # DT
}


def _scan(lib, n):
    return int(lib.ia_scan_tmp_bytes(C.c_int64(max(int(n), 1)))) + 64            # _lib.scan_tmp of that commit


# what the Python callers of the commit before the queries existed passed to the entry point
PARENT_PYTHON = {
    "ia_pack_info_tmp_bytes": lambda lib, n: _scan(lib, n) + 8 * n + 64,
    "ia_deform_rows_pack_split_tmp_bytes": lambda lib, n: _scan(lib, (n + 1023) // 1024 + 1) + 4 * ((n + 1023) // 1024) + 1024,
}


def table(so_path):
    """[{"fn", "args", "bytes"}] of the library at so_path, in the order of CASES"""
    from intrinsicavatar_amd import _lib
    lib = C.CDLL(so_path)
    protos = _lib.header_prototypes()
    every = {n for n in protos if n.endswith("_bytes") or n == "ia_hashgrid_fwd_levels_jac_offset"}
    assert every == set(CASES), sorted(every ^ set(CASES))
    lib.ia_scan_tmp_bytes.restype, lib.ia_scan_tmp_bytes.argtypes = protos["ia_scan_tmp_bytes"]
    rows = []
    for fn, cases in CASES.items():
        restype, argtypes = protos[fn]
        f = getattr(lib, fn, None)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
        for args in cases:
            if f is not None:
                v = f(*[t(a) for t, a in zip(argtypes, args)])
                v = int(v) if v < (1 << 63) else int(v) - (1 << 64)          # size_t: -1 stays -1
            else:
                v = PARENT_PYTHON[fn](lib, *args)
            rows.append({"fn": fn, "args": list(args), "bytes": v})
    return rows


if __name__ == "__main__":
    rows = table(os.environ["IA_AMD_LIB"])
    print("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]")
