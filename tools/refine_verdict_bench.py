#!/usr/bin/env python3
"""Wall time of the refine driver's collision verdicts (strive_amd/refine_traffic_tracks.py), information only, no gate:

  (a) the loop the driver would run without strive_refine_verdicts: per scene of ``to_data_list()``, ``check_pairwise_veh_coll`` and
      ``compute_coll_rate_env`` on a single-scene graph (the reference's ``compute_metrics``, src/refine_traffic_optim.py:84-121, on
      the product's existing functions), results read back per scene as those functions do
  (b) ONE ``batch_verdicts`` call and the one read-back of its integers

at 36 scenes / 512 agents (bench.py's adversarial batch) and at one 10-agent scene (the shipped config's batch_size), 12 steps,
trajectories around the scenes' own futures, inputs on the device.  (a) and (b) ALTERNATE inside one process; every timed call is
bracketed by device synchronisations; medians of ``--reps`` repeats with minimum and maximum.  Both give the same verdicts: checked
before anything is timed.

``--epoch`` adds the driver's wall time per batch, split into optimise / verdicts / write, over one epoch of a ``synth.make_tracks``
file at ``--num_iters`` Adam iterations (the shipped config: 200).

Usage:  python tools/refine_verdict_bench.py [--reps 9] [--epoch] [--num_iters 200] [--out profiles/r24_refine_verdict_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from strive_amd import synth                                              # noqa: E402
from strive_amd import refine_traffic_tracks as RT                       # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors   # noqa: E402
from strive_amd.datasets.utils import MeanStdNormalizer                  # noqa: E402
from strive_amd.graph import Batch                                        # noqa: E402
from strive_amd.losses.adv_gen_nusc import check_pairwise_veh_coll       # noqa: E402
from strive_amd.losses.traffic_model import compute_coll_rate_env        # noqa: E402
from strive_amd.models.traffic_model import TrafficModel                 # noqa: E402

DEV = 'cuda:0'
ADV_SIZES = [15] * 8 + [14] * 28                 # 36 scenes, 512 agents


def make_model():
    m = TrafficModel(4, 12, 256, 2)
    m.load_state_dict(synth.fill_state_dict(m.state_dict()))
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    return m.eval().to(DEV)


def injected(batch, key, T=12):
    """(NA,1,T,4) NORMALISED: the scenes' own futures, moved a little per agent."""
    NA = batch.past.shape[0]
    traj = batch.future_gt[:, :T, :4].clone()
    traj[..., :2] += synth.f32(synth.counter_uniform((NA, 1, 2), key + '/off', -0.06, 0.06))
    return traj.unsqueeze(1).contiguous()


def per_scene_loop(traj, model, batch, env, map_idx):
    """(a): what compute_metrics does, scene by scene."""
    sn, an = model.get_normalizer(), model.get_att_normalizer()
    ptr = batch.ptr.tolist()
    out = []
    for b, scene in enumerate(batch.to_data_list()):
        g = Batch.from_data_list([scene])
        g.ptr, g.batch = g.ptr.to(traj.device), g.batch.to(traj.device)
        tr = traj[ptr[b]:ptr[b + 1]]
        veh = check_pairwise_veh_coll(sn.unnormalize(tr[:, 0]), an.unnormalize(g.lw))
        envd = compute_coll_rate_env(g, map_idx[b:b + 1], tr.contiguous(), env, sn, an, ego_only=False)
        fin = envd['did_collide'].cpu().numpy()[:, 0]
        out.append((int(veh['num_coll_veh']), int(fin.sum())))
    return out


def one_call(traj, model, batch, env, map_idx):
    """(b): the driver's verdicts and its read-back of them."""
    v = RT.batch_verdicts(traj, model, batch, env, map_idx)
    oi = torch.cat([v['out_i'].reshape(-1), v['status']]).cpu().numpy()
    B = int(map_idx.numel())
    return [(int(r[0]), int(r[2])) for r in oi[:B * 8].reshape(B, 8)]


def alternate(fns, reps):
    """{name: [ms]}: the functions take turns, ``reps`` rounds after two warm-up rounds."""
    times = {k: [] for k in fns}
    for r in range(reps + 2):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def summary(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'repeats': len(ms)}


def epoch_split(model, num_iters):
    """One epoch of the driver over a synthetic tracks file, the clock read (device synchronised) around its three parts."""
    from strive_amd.datasets.nuscenes_dataset import NuScenesDataset
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    ds = NuScenesDataset(synth.make_tracks(n_scenes=4, n_agents=12, T=36), env, seq_interval=10, device=DEV)
    src = RT.scene_source(ds)
    marks = []

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    def close_write():
        if marks and 'write_t0' in marks[-1]:
            marks[-1]['write_ms'] = (clock() - marks[-1].pop('write_t0')) * 1e3
    orig_verdicts, orig_dicts = RT.batch_verdicts, RT.batched_output_dicts

    def refine(*a, **k):
        close_write()                            # (the previous batch's files are written when the driver asks for the next batch)
        t0 = clock()
        res = RT.refine_traffic_optim(*a, **k)
        marks.append({'optimise_ms': (clock() - t0) * 1e3, 'agents': int(res[2].shape[0])})
        return res

    def verdicts(*a, **k):
        t0 = clock()
        res = orig_verdicts(*a, **k)
        marks[-1]['verdicts_ms'] = (clock() - t0) * 1e3
        return res

    def dicts(*a, **k):
        marks[-1]['write_t0'] = clock()
        return orig_dicts(*a, **k)
    RT.batch_verdicts, RT.batched_output_dicts = verdicts, dicts
    weights = {'coll_veh': 100.0, 'coll_env': 100.0, 'motion_prior': 1.0, 'init_z': 0.01}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            RT.run_one_epoch(src, 10, model, env, DEV, tmp, weights, feasibility_NA=2, samp_future_len=16, save_future_len=12,
                             optim_use_adam=True, num_iters=num_iters, lr=0.05, save=True, refine_fn=refine)
            close_write()
    finally:
        RT.batch_verdicts, RT.batched_output_dicts = orig_verdicts, orig_dicts
    return {'scenes': len(src), 'num_iters': num_iters, 'batches': marks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--epoch', action='store_true')
    ap.add_argument('--num_iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit('at least 7 repeats')
    if not torch.cuda.is_available():
        raise SystemExit('refine_verdict_bench measures on the GPU; there is none here')
    model = make_model()
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    result = {'device': torch.cuda.get_device_name(0), 'what': 'wall ms, device synchronised around every call, (a) and (b) alternating',
              'points': {}}
    for name, sizes in (('36 scenes / 512 agents', ADV_SIZES), ('1 scene / 10 agents', [10])):
        batch, mi = synth.make_batch(sizes, key='refine_bench/%d' % len(sizes))
        traj = injected(batch, 'refine_bench/%d' % len(sizes)).to(DEV)
        batch, mi = batch.to(DEV), mi.to(DEV)
        args = (traj, model, batch, env, mi)
        same = per_scene_loop(*args) == one_call(*args)
        t = alternate({'per_scene_loop': lambda: per_scene_loop(*args), 'one_call': lambda: one_call(*args)}, a.reps)
        result['points'][name] = {'same_verdicts': same, 'per_scene_loop': summary(t['per_scene_loop']), 'one_call': summary(t['one_call'])}
        print(name, json.dumps(result['points'][name]))
    if a.epoch:
        result['epoch'] = epoch_split(model, a.num_iters)
        print('epoch', json.dumps(result['epoch']))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
