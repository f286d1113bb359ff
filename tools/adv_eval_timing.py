#!/usr/bin/env python3
"""Wall time of the scenario-evaluation kernel (strive_scenario_eval_metrics) on 256 copies of the g18 fixture scenes with 12 future
steps: ONE batched call against B calls with one scene each (the same kernel, B = 1), map and latents included, collision features
asked for; events around the calls, inputs already on the device.  Information only, no gate.

Usage:  python tools/adv_eval_timing.py [--copies 256] [--iters 10] [--out profiles/r17_adv_eval_timing.md]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from strive_amd import eval_adv_gen as EA                                # noqa: E402

DEV = 'cuda:0'
SCEN_DIR = os.path.join(REPO, 'tests', 'golden', 'g18_scenarios')


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--copies', type=int, default=256)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    base = [s for c in EA.RES_NAMES for s in EA.read_adv_scenes(os.path.join(SCEN_DIR, c)) if s['fut_adv'].shape[1] == 12]
    scenes = [base[i % len(base)] for i in range(a.copies)]
    env = EA.SyntheticMapWorld()
    env.nusc_raster, env.nusc_dx = env.nusc_raster.to(DEV), env.nusc_dx.to(DEV)
    batched = EA._stack(scenes, DEV)
    single = [EA._stack([s], DEV) for s in scenes]
    one = lambda args, B: EA.scenario_eval_metrics(map_env=env, mapix=[0] * B, want_feat=[1] * B, **args)
    ms_batched = timed(lambda: one(batched, len(scenes)), a.iters)
    ms_single = timed(lambda: [one(args, 1) for args in single], max(1, a.iters // 5))
    res = dict(scenes=len(scenes), agents=int(batched['fut'].shape[0]), ms_one_batched_call=round(ms_batched, 3),
               ms_one_call_per_scene=round(ms_single, 3), device=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
