#!/usr/bin/env python3
"""Wall time of scenario rendering (strive_amd/render.py), information only, no gate: there is no earlier renderer to compare with.

  one scene    the overview of a 15-agent scene and its 16 video frames (17 pictures of 720 x 720) in one launch
  36 scenes    bench.py's adversarial batch (512 agents): 36 x 17 = 612 pictures in one launch
each split into  host     building the draw lists and packing the tables
                 kernel   the strive_render_pictures launch (the upload of the tables included), device synchronised
                 readback the pinned copy of the pictures to the host
                 png      write_png of every picture (zlib level 3) into a scratch directory
The two workloads ALTERNATE inside one process; medians of ``--reps`` repeats with minimum and maximum.

Usage:  python tools/render_bench.py [--reps 7] [--L 720] [--out profiles/r26_render_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_verdict_bench import ADV_SIZES, DEV, summary        # noqa: E402
from strive_amd import render, synth                            # noqa: E402
from strive_amd.constants import state_norm_tensors             # noqa: E402


def scene_tracks(sizes, key):
    """Per scene: (NA, 16, 4) unnormalised x, y, hx, hy (4 past + 12 future steps of the synthetic scenes) and (NA, 2) sizes."""
    batch, map_idx = synth.make_batch(sizes, key=key)
    mean, std = state_norm_tensors()
    traj = torch.cat([batch.past_gt[:, :, :4], batch.future_gt[:, :12, :4]], dim=1) * std[:4] + mean[:4]
    lw = batch.lw * torch.tensor([2.0, 1.0]) + torch.tensor([4.5, 2.0])
    ptr = batch.ptr.tolist()
    return [(traj[ptr[b]:ptr[b + 1]], lw[ptr[b]:ptr[b + 1]].abs() + 1.0) for b in range(len(sizes))]


def plans_of(scenes, L):
    plans = []
    for traj, lw in scenes:
        NA, NT, _ = traj.shape
        centre = torch.cat([traj[0, NT // 2, :2], torch.tensor([1.0, 0.0])])
        bound = max(30.0, float((traj[:, NT // 2, :2] - centre[:2]).abs().max()))
        bounds = [-bound, -bound, bound, bound]
        crop_traj, crop_lw = render.objs2crop(centre, traj.reshape(NA * NT, 4), lw, bounds, L, L)
        crop_traj = crop_traj.reshape(NA, NT, 4)
        dls = [render.build_draw_list(crop_traj, crop_lw, viz_traj=True, traj_markers=[False] * NA)] + render.frame_draw_lists(crop_traj, crop_lw)
        plans.append((centre, bounds, dls))
    return plans


def one_round(scenes, env, L, outdir):
    t = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plans = plans_of(scenes, L)
    kin = torch.stack([p[0] for p in plans for _ in p[2]])
    bounds = [p[1] for p in plans for _ in p[2]]
    dls = [dl for p in plans for dl in p[2]]
    prims, verts, ranges = render.pack_draw_lists(dls, render.px_per_pt(L))
    t['host'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    pics = render.render_tables(env, kin, [0] * len(dls), bounds, L, prims, verts, ranges)
    torch.cuda.synchronize()
    t['kernel'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = render.read_back(pics)
    t['readback'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i, pic in enumerate(host):
        render.write_png(os.path.join(outdir, '%04d.png' % i), pic)
    t['png'] = time.perf_counter() - t0
    return {k: v * 1e3 for k, v in t.items()}, len(dls), int(prims.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--L', type=int, default=720)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench measures on the GPU; there is none here')
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    work = {'1 scene / 15 agents': scene_tracks([15], 'render_bench/1'), '36 scenes / 512 agents': scene_tracks(ADV_SIZES, 'render_bench/36')}
    times = {k: {} for k in work}
    info = {}
    outdir = tempfile.mkdtemp()
    try:
        for r in range(a.reps + 1):                       # one warm-up round; the workloads take turns
            for name, scenes in work.items():
                t, npic, nprim = one_round(scenes, env, a.L, outdir)
                info[name] = {'pictures': npic, 'primitives': nprim}
                if r >= 1:
                    for k, v in t.items():
                        times[name].setdefault(k, []).append(v)
    finally:
        shutil.rmtree(outdir)
    result = {'device': torch.cuda.get_device_name(0), 'L': a.L, 'what': 'wall ms per phase, the two workloads alternating'}
    for name in work:
        result[name] = dict(info[name], **{k: summary(v) for k, v in times[name].items()})
        result[name]['kernel_ms_per_picture'] = result[name]['kernel']['median_ms'] / info[name]['pictures']
        print(name, json.dumps(result[name]))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
