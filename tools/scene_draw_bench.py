#!/usr/bin/env python3
"""Wall time of drawing a live batch (strive_amd/scene_draw.py), information only, no gate.  Two paths take turns in one process:

  device   strive_scene_draw_tables + strive_render_pictures + the one read-back (scene_draw.draw_calls)
  host     read the trajectories back, the restated viz_scene_graph (tests/scene_draw_restated.py: Python loops over agents, samples
           and steps, ending in render.build_draw_list), render.pack_draw_lists, render.render_tables, the read-back
on three workloads at L = 256:
  1 scene / 10 agents          the overview with trajectories over the ground truth, NS = 3
  36 scenes / 512 agents       per scene the overview with trajectories and the 16 frames of a one-sample video (with its own overview): 648 pictures
  roll-out, NS = 3             per scene test_traffic's roll-out call: the overview and 3 x 16 frames, 1764 pictures
and ``render.write_pngs`` of the roll-out's pictures at 1, 4, 8 and 16 workers.  Medians of ``--reps`` repeats with minimum and maximum.

Usage:  python tools/scene_draw_bench.py [--reps 7] [--out profiles/r29_scene_draw_bench.json]
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
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_verdict_bench import ADV_SIZES, DEV, summary        # noqa: E402
import scene_draw_restated as sr                                # noqa: E402
from strive_amd import render, scene_draw, synth                # noqa: E402

L_PIX = 256


class Env(object):
    def __init__(self, dev):
        r, dx = synth.make_raster(M=2)
        self.nusc_raster, self.nusc_dx, self.L, self.W = r.to(dev), dx.to(dev), L_PIX, L_PIX


def workload(sizes, kind, seed):
    batch, map_idx, ptr = sr.make_batch(sizes, seed=seed)
    B = len(sizes)
    if kind == 'overview':
        pred = sr.make_pred(batch, 3, 12, seed)
        calls = [dict(bidx=b, out_path='o%d' % b, future_pred=pred, viz_traj=True, make_video=False, show_gt=True) for b in range(B)]
    elif kind == 'video':
        pred = sr.make_pred(batch, 1, 12, seed)
        calls = [dict(bidx=b, out_path='v%d' % b, future_pred=pred, viz_traj=True, make_video=False, show_gt=True) for b in range(B)] + \
                [dict(bidx=b, out_path='w%d' % b, future_pred=pred, viz_traj=False, make_video=True) for b in range(B)]
    else:
        pred = sr.make_pred(batch, 3, 12, seed)
        calls = [dict(bidx=b, out_path='r%d' % b, future_pred=pred, viz_traj=False, make_video=True, viz_bounds=[-45.0, -45.0, 45.0, 45.0],
                      center_viz=True) for b in range(B)]
    return batch, map_idx, ptr, calls


def to_device(batch, map_idx, calls):
    moved = {}
    out = []
    for c in calls:
        c = dict(c)
        p = c['future_pred']
        if id(p) not in moved:
            moved[id(p)] = (p, p.to(DEV))
        c['future_pred'] = moved[id(p)][1]
        out.append(c)
    return batch.clone().to(DEV), map_idx.to(DEV), out


def device_path(env, dbatch, dmap, dcalls, ptr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    paths, pics, _ = scene_draw.draw_calls(dbatch, dmap, env, dcalls, *sr.normalizers(), ptr=ptr)
    return (time.perf_counter() - t0) * 1e3, pics


def host_path(env, dbatch, dmap, dcalls, ptr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batch = dbatch.clone().to('cpu')                                  # the trajectories come back first
    map_idx = dmap.cpu()
    back = {}
    dls, pose, mapix, bounds = [], [], [], []
    for c in dcalls:
        p = c['future_pred']
        if id(p) not in back:
            back[id(p)] = p.cpu()
        for pic in sr.restate(batch, ptr, map_idx, dict(c, future_pred=back[id(p)]), L_PIX):
            dls.append(pic['draw_list'])
            pose.append(torch.from_numpy(pic['pose']).to(torch.float32))
            mapix.append(pic['mapix'])
            bounds.append(pic['bounds'])
    prims, verts, ranges = render.pack_draw_lists(dls, render.px_per_pt(L_PIX))
    pics = render.read_back(render.render_tables(env, torch.stack(pose), mapix, bounds, L_PIX, prims, verts, ranges))
    return (time.perf_counter() - t0) * 1e3, pics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('scene_draw_bench measures on the GPU; there is none here')
    env = Env(DEV)
    work = {'1 scene / 10 agents': workload([10], 'overview', 1), '36 scenes / 512 agents': workload(ADV_SIZES, 'video', 2),
            'roll-out NS=3, 36 scenes': workload(ADV_SIZES, 'rollout', 3)}
    dev = {k: to_device(w[0], w[1], w[3]) for k, w in work.items()}
    times = {k: {'device': [], 'host': []} for k in work}
    info, last = {}, None
    for r in range(a.reps + 1):                           # one warm-up round; paths and workloads take turns
        for name, w in work.items():
            for path, fn in (('device', device_path), ('host', host_path)):
                ms, pics = fn(env, *dev[name], w[2])
                info[name] = {'pictures': int(pics.shape[0])}
                if r >= 1:
                    times[name][path].append(ms)
                if path == 'device':
                    last = pics
    result = {'device': torch.cuda.get_device_name(0), 'L': L_PIX, 'what': 'wall ms per path, paths and workloads alternating'}
    for name in work:
        result[name] = dict(info[name], **{k: summary(v) for k, v in times[name].items()})
        result[name]['host_over_device'] = result[name]['host']['median_ms'] / result[name]['device']['median_ms']
        print(name, json.dumps(result[name]))
    # write_pngs on the roll-out's pictures (the last device result), worker counts taking turns
    outdir = tempfile.mkdtemp()
    try:
        paths = [os.path.join(outdir, '%05d.png' % i) for i in range(last.shape[0])]
        png = {w: [] for w in (1, 4, 8, 16)}
        for r in range(a.reps):
            for w in png:
                t0 = time.perf_counter()
                render.write_pngs(paths, last, w)
                png[w].append((time.perf_counter() - t0) * 1e3)
    finally:
        shutil.rmtree(outdir)
    result['write_pngs'] = {'pictures': int(last.shape[0]), 'workers': {str(w): summary(v) for w, v in png.items()}}
    print('write_pngs', json.dumps(result['write_pngs']))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
