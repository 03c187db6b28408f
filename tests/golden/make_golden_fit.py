#!/usr/bin/env python3
"""Golden data for intrinsicavatar_amd/fit.py, made from the REFERENCE at run time:

    BaseSystem.C    /root/reference/systems/base.py:33-88: the function definition is cut out of the parsed file and called with a
                    stand-in `self` (global_step, current_epoch) and config_to_primitive = identity, over every schedule value of
                    configs/config.yaml plus 3- and 4-lists with integer and float end_step, at the steps
                    {0, 1, start-1, start, mid, end-1, end, end+1} -- once as the global step (epoch 7), once as the epoch (step 7)
    FitConfig       configs/config.yaml through yaml.safe_load: the scalar entries of `model` (the `${...}` references to other
                    config groups are left out), `system.loss`, `trainer`, the scalar entries of `system`, the optimiser numbers

  python tests/golden/make_golden_fit.py          (build container only: needs /root/reference; CPU, a second)

Only DATA is written: tests/golden/golden_schedule.json."""
import ast
import json
import os
import types

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

EXTRA = [[1.5, 0.0, 5], [2.0, 0.5, 3.0], [5, 1.0e-5, 1.0e-5, 6], [10, 0.0, 1.0, 20], [2, 0.25, 0.75, 6.0], [0, 1.0, 0.0, 100],
         [100, 0.5, 2.5, 101]]


def reference_C():
    src = open(os.path.join(REF, "systems", "base.py")).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "C")
    ns = {"config_to_primitive": lambda v: v}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "systems/base.py", "exec"), ns)
    return ns["C"]


def steps_of(value):
    if not isinstance(value, list):
        return [0, 1]
    end = int(value[-1])
    start = int(value[0]) if len(value) == 4 else end
    return sorted({0, 1, max(start - 1, 0), start, (start + end) // 2, max(end - 1, 0), end, end + 1})


def main():
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "config.yaml")))
    C = reference_C()
    loss = cfg["system"]["loss"]
    values = [v for k, v in loss.items() if k.startswith("lambda_")] + EXTRA
    rows = []
    for v in values:
        for s in steps_of(v):
            for gs, ep in ((s, 7), (7, s)):
                rows.append(dict(value=v, global_step=gs, epoch=ep, result=C(types.SimpleNamespace(global_step=gs, current_epoch=ep), v)))
    scalar = lambda d: {k: v for k, v in d.items() if not isinstance(v, dict) and not (isinstance(v, str) and v.startswith("${"))}      # noqa: E731
    opt, sched = cfg["system"]["optimizer"], cfg["system"]["scheduler"]
    fit_config = dict(model=scalar(cfg["model"]), loss=loss, trainer=cfg["trainer"], system=scalar(cfg["system"]),
                      optimizer=dict(lr=opt["args"]["lr"], betas=opt["args"]["betas"], eps=opt["args"]["eps"], color_grid_wd=cfg["color_grid_wd"],
                                     milestones=sched["schedulers"][1]["args"]["milestones"], gamma=sched["schedulers"][1]["args"]["gamma"]))
    out = os.path.join(HERE, "golden_schedule.json")
    with open(out, "w") as fh:
        json.dump(dict(schedule=rows, fit_config=fit_config), fh, indent=1)
    print(out, len(rows), "schedule rows")


if __name__ == "__main__":
    main()
