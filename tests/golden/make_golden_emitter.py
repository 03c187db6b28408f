#!/usr/bin/env python3
"""Golden vectors of model.add_emitter: the reference's own IntrinsicAvatarModel.forward_ (models/intrinsic_avatar.py:950-1651) run again
on the scene of golden_forward.npz with `add_emitter=True` (configs/config.yaml:58, :1319-1333, :1455-1490).

  python tests/golden/make_golden_emitter.py          (needs /root/reference; CPU only; a few minutes)

The machinery is make_golden_forward.py, imported as a module and not edited: its shims, rig, parameters, config and HDRI.  Every random
tensor is REPLAYED from the draws golden_forward.npz recorded for the same run, in call order, so the two fixtures differ by the switch
alone.  Runs: light_16_nogi, uniform_light_512_gi, mis_16_gi, and light_16_nogi once more with model.albedo_only (:222, :1290).

Only DATA is written (tests/golden/golden_emitter.npz): comp_rgb_phys, comp_demod_phys and their `_full` forms per run.  Every other
key of the output dict is asserted here to EQUAL golden_forward.npz (the albedo-only run: against light_16_nogi), so the emitter
background touches nothing else."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden_forward as M      # noqa: E402

N = M.N
KEYS = ("comp_rgb_phys", "comp_demod_phys", "comp_rgb_phys_full", "comp_demod_phys_full")
RUNS = [("light_16_nogi", "light", 16, False, False), ("uniform_light_512_gi", "uniform_light", 512, True, False),
        ("mis_16_gi", "mis", 16, True, False), ("light_16_nogi_albedo_only", "light", 16, False, True)]


def recorded_draws(G, tag):
    kinds = [str(k) for k in G[tag + "_rng_kinds"]]
    out = []
    for i, k in enumerate(kinds):
        a = G[f"{tag}_rng_{i}"]
        if k in ("rand_formula", "rand_like_formula"):
            a = ((M.S.hash_table_values(int(a[1]), int(a[0]), 1.0).astype(np.float64) + 1.0) / 2.0).astype(np.float32)
        out.append((k, a))
    return out


class Replay(M.RngLog):
    """hands the recorded draws back in call order; the kinds and sizes must be the ones the run asks for"""

    def __init__(self, draws):
        super().__init__(0)
        self.draws, self.i = list(draws), 0

    def _next(self, kinds, shape, dtype=torch.float32):
        k, a = self.draws[self.i]
        self.i += 1
        assert k in kinds, (k, kinds, self.i)
        assert a.size == int(np.prod(shape)), (k, a.shape, tuple(shape))
        t = torch.from_numpy(np.ascontiguousarray(a)).reshape(tuple(shape)).to(dtype)
        self.log.append((k, t))
        return t

    def rand(self, *size, **kw):
        size = tuple(size[0] if (len(size) == 1 and not isinstance(size[0], int)) else size)
        return self._next(("rand", "rand_formula"), size)

    def rand_like(self, x, **kw):
        dt = kw.get("dtype", x.dtype if x.dtype.is_floating_point else torch.float32)
        return self._next(("rand_like", "rand_like_formula"), x.shape, dt)

    def randn_like(self, x, **kw):
        return self._next(("randn_like",), x.shape)

    def uniforms(self, tag, shape):
        return self._next((tag,), shape)


def main():
    assert os.path.isdir(M.REF), "needs /root/reference (build container only)"
    G = np.load(f"{HERE}/golden_forward.npz")
    torch.manual_seed(0)
    mods = M.import_reference_model()
    IA = mods["ia"]
    registry = mods["registry"]
    dummy = type("Dummy", (nn.Module,), {"__init__": lambda self, c=None: nn.Module.__init__(self), "forward": lambda self, *a, **k: None})
    registry["none"] = dummy
    wrap, rd, _ = M.build_rig(mods)
    registry["prebuilt"] = lambda cfg: wrap
    rays = torch.from_numpy(G["rays"])
    bg = torch.from_numpy(G["background_color"])
    out = {}
    for tag, mode, spp, gi, albedo_only in RUNS:
        src = tag.replace("_albedo_only", "")
        torch.manual_seed(0)
        cfg = M.model_config(mode, spp, gi)
        cfg["add_emitter"] = True
        with Replay(recorded_draws(G, src)) as rng:
            M.RNG = rng
            model = IA.IntrinsicAvatarModel(cfg)
            M.init_params(model)
            model.eval()
            model.update_step(250, 25000)
            assert model.enable_phys and model.importance_sample and model.add_emitter
            model.background_color = bg
            model.geometry.prepare_bbox(rd.bbox)
            model.radiance.prepare_bbox(rd.bbox)
            model.jitter_materials = False
            model.with_curvature_loss = False
            model.cond = None
            model.albedo_only = albedo_only
            model.prepare_test_occupancy_grid()
            assert np.array_equal(N(model.occupancy_grid_test.binaries), G[src + "_occ_binaries"])
            model.emitter.base = nn.Parameter(torch.from_numpy(G["hdri"]))
            model.emitter.pdf_scale = (model.emitter.base.shape[0] * model.emitter.base.shape[1]) / (2 * np.pi * np.pi)
            model.emitter.update_pdf()
            model.secondary_rays_d = model.emitter.sample(model.samples_per_pixel)
            with torch.no_grad():
                res = model.forward_(rays.clone())
            if not albedo_only:
                assert rng.i == len(rng.draws), (tag, rng.i, len(rng.draws))
        ref_keys = [str(k) for k in G[src + "_out_keys"]]
        assert sorted(res.keys()) == sorted(ref_keys), sorted(set(res.keys()) ^ set(ref_keys))
        for k in ref_keys:
            if k in KEYS:
                out[f"{tag}_{k}"] = N(res[k])
            else:
                assert np.array_equal(N(res[k]), G[f"{src}_out_{k}"]), (tag, k)
        d = N(res["comp_rgb_phys"]) - G[f"{src}_out_comp_rgb_phys"]
        print(tag, "rays moved by the emitter:", int((np.abs(d).max(-1) > 0).sum()), "of", d.shape[0], " max |difference|", float(np.abs(d).max()))
    torch.Tensor.cuda, torch.cuda.device = mods["restore"]
    np.savez_compressed(f"{HERE}/golden_emitter.npz", **out)
    print("golden_emitter.npz", os.path.getsize(f"{HERE}/golden_emitter.npz") // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
