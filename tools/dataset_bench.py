#!/usr/bin/env python3
"""Batch assembly and post-processing of the scene dataset on the MI355X (information only, no gate; bench.py is the flagship
measurement and is untouched):
  (a) one batch of 32 windows of about 16 agents each through ``NuScenesDataset.get_batch`` (one strive_dataset_gather_batch launch)
  (b) the same batch on the host path a caller had before the dataset existed: per window a ``Data`` on the CPU the way the
      reference's ``__getitem__`` builds it (numpy selection over the scene's agents, ``torch.Tensor(np.stack(...))``, normalisation,
      the clique), then ``Batch.from_data_list``, then ``.to(device)``
  (c) construction of the dataset from a synthetic tracks file of nuScenes-mini size (10 scenes x 40 frames x 80 agents): the whole
      constructor (uploads, strive_dataset_post_process, strive_dataset_window_counts and the one read-back of the counts) on the
      host clock and between two events; the launch alone is not timed
Inputs are resident, two warm-up calls, the device synchronised before and after every timed call.

Usage:  python tools/dataset_bench.py [--reps 9] [--out profiles/r19_dataset_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from strive_amd import synth                                              # noqa: E402
from strive_amd.datasets.nuscenes_dataset import NuScenesDataset         # noqa: E402
from strive_amd.graph import Data, Batch, clique_edge_index              # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps):
    fn()
    fn()
    wall, ev = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {'wall_ms_median': statistics.median(wall), 'wall_ms_min': min(wall), 'wall_ms_max': max(wall),
            'events_ms_median': statistics.median(ev), 'reps': reps}


class HostPath(object):
    """The per-window host work of the reference's ``__getitem__`` (src/datasets/nuscenes_dataset.py:594-704) on host copies of the
    dataset's tables."""

    def __init__(self, ds):
        self.ds = ds
        self.traj, self.vis, self.kept = ds.traj.cpu().numpy(), ds.is_vis.cpu().numpy(), ds.kept.cpu().numpy()
        self.scenes = {}
        for name, s in ds._scene_index.items():
            a0, a1 = int(ds._agent_ptr[s]), int(ds._agent_ptr[s + 1])
            self.scenes[name] = [(a, int(ds._row_ptr[a]), int(ds._row_ptr[a + 1])) for a in range(a0, a1) if a == a0 or self.kept[a]]
        self.cat, self.lw_all = ds._cat_host, ds._lw_host

    def item(self, idx):
        ds = self.ds
        name, sidx = ds.seq_map[idx]
        midx, eidx = sidx + ds.npast, sidx + ds.seq_len
        past, future, sem, lw, pv, fv = [], [], [], [], [], []
        for j, (a, r0, r1) in enumerate(self.scenes[name]):
            tj = self.traj[r0:r1]
            if j > 0:
                if np.isnan(tj[midx - 1]).astype(int).sum() > 0:
                    continue
                if ds.require_full_past and np.isnan(tj[:midx]).sum() > 0:
                    continue
            past.append(tj[sidx:midx])
            future.append(tj[midx:eidx])
            sem.append(ds.cat2vec[ds.categories[self.cat[a]]])
            lw.append(self.lw_all[a])
            pv.append(self.vis[r0:r1][sidx:midx])
            fv.append(self.vis[r0:r1][midx:eidx])
        past, future = torch.Tensor(np.stack(past, axis=0)), torch.Tensor(np.stack(future, axis=0))
        sem, lw = torch.Tensor(np.stack(sem, axis=0)), torch.Tensor(np.stack(lw, axis=0))
        pv, fv = torch.Tensor(np.stack(pv, axis=0)), torch.Tensor(np.stack(fv, axis=0))
        n = past.size(0)
        return Data(x=torch.empty((n,)), pos=torch.empty((n,)), edge_index=clique_edge_index(n), past=ds.normalizer.normalize(past),
                    past_gt=ds.normalizer.normalize(past), future=ds.normalizer.normalize(future), future_gt=ds.normalizer.normalize(future),
                    sem=sem, lw=ds.veh_att_normalizer.normalize(lw), past_vis=pv, future_vis=fv), ds.scene2map[name][1]

    def batch(self, idx):
        items = [self.item(i) for i in idx]
        g = Batch.from_data_list([d for d, _ in items]).to(DEV)
        return g, torch.tensor([m for _, m in items], dtype=torch.long).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    res = {'device': torch.cuda.get_device_name(0)}

    ds = NuScenesDataset(synth.make_tracks(n_scenes=8, n_agents=22, T=40), env, device=DEV)
    order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0)).tolist()[:32]
    host = HostPath(ds)
    g, _ = ds.get_batch(order)
    h, _ = host.batch(order)
    assert torch.equal(g.ptr.cpu(), h.ptr.cpu()) and torch.equal(g.edge_index.cpu(), h.edge_index.cpu())
    for k in ('past', 'future', 'lw', 'sem', 'past_vis', 'future_vis'):
        assert torch.equal(torch.nan_to_num(g[k]).cpu(), torch.nan_to_num(h[k]).cpu()), k
    res['batch'] = {'windows': 32, 'agents_per_window': float(g.ptr[-1]) / 32.0, 'edges': int(g.edge_index.shape[1]),
                    'device_gather': timed(lambda: ds.get_batch(order), a.reps),
                    'host_getitem_collate_to_device': timed(lambda: host.batch(order), a.reps)}
    res['batch']['host_over_device_wall'] = res['batch']['host_getitem_collate_to_device']['wall_ms_median'] / \
        res['batch']['device_gather']['wall_ms_median']

    tr = synth.make_tracks(n_scenes=10, n_agents=80, T=40, key='tracks/mini')
    res['post_process'] = {'scenes': 10, 'agents': int(tr['lw'].shape[0]), 'observations': int(tr['obs'].shape[0]),
                           'constructor': timed(lambda: NuScenesDataset(tr, env, device=DEV), max(3, a.reps // 3))}
    big = NuScenesDataset(tr, env, device=DEV)
    res['post_process']['windows'] = len(big)
    res['post_process']['kept_agents'] = int(big.kept.sum())
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
