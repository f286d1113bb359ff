#!/usr/bin/env python3
"""Wall time of the adv_scenario_gen driver's two batched calls (strive_amd/adv_scenario_gen_tracks.py), information only, no gate:

  verdicts   (a) the loop the driver would run without strive_ego_verdicts: per scene of ``to_data_list()``,
                 ``compute_adv_gen_success`` and ``compute_sol_success`` on a single-scene graph (reference
                 src/adv_scenario_gen.py:391-398, 445-451, on the product's existing functions), read back per scene as they do
             (b) TWO ``ego_verdicts`` calls (the attacker's flag; any hit and the ego's drivable test) and one read-back each
             at 36 scenes / 512 agents (bench.py's adversarial batch) and at one 10-agent scene, 12 steps
  screening  (a) scene by scene: ``sample_batched(NS = 20)`` + ``determine_feasibility_nusc`` + the reads of reference :166-207
             (b) chunks of ``--screen_agents`` agents: one ``sample_batched`` + one ``screen_batch`` + one read-back per chunk
             on the same 36 scenes

(a) and (b) ALTERNATE inside one process; every timed call is bracketed by device synchronisations; medians of ``--reps`` repeats
with minimum and maximum.  The verdicts of (a) and (b) are compared before anything is timed.  ``--also_screen_agents N ...`` repeats the
screening measurement at other chunk sizes (key ``screening_at_other_chunk_sizes``).

Usage:  python tools/adv_verdict_bench.py [--reps 9] [--screen_agents 256] [--also_screen_agents 64 1024]
            [--out profiles/r25_adv_verdict_bench.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_verdict_bench import ADV_SIZES, DEV, alternate, injected, make_model, summary   # noqa: E402
from strive_amd import synth                                                                # noqa: E402
from strive_amd import adv_scenario_gen_tracks as AG                                        # noqa: E402
from strive_amd.graph import Batch                                                          # noqa: E402
from strive_amd.utils.adv_gen_optim import compute_adv_gen_success                          # noqa: E402
from strive_amd.utils.scenario_gen import determine_feasibility_nusc                        # noqa: E402
from strive_amd.utils.sol_optim import compute_sol_success                                  # noqa: E402


def single_scenes(batch, map_idx):
    out = []
    for b, scene in enumerate(batch.to_data_list()):
        g = Batch.from_data_list([scene])
        g.ptr, g.batch = g.ptr.to(map_idx.device), g.batch.to(map_idx.device)
        out.append((g, map_idx[b:b + 1]))
    return out


def verdict_loop(traj, model, batch, env, map_idx, atk):
    """(a): the two success functions, scene by scene (the single-scene graphs are rebuilt every time, as the reference does)."""
    ptr = batch.ptr.tolist()
    out = []
    for b, (g, mi) in enumerate(single_scenes(batch, map_idx)):
        tr = traj[ptr[b]:ptr[b + 1]]
        out.append((bool(compute_adv_gen_success(tr, model, g, atk[b])), bool(compute_sol_success(tr[:, 0:1], model, g, env, mi))))
    return out


def verdict_calls(traj, model, batch, env, map_idx, atk_dev):
    """(b): the driver's two calls and their read-backs."""
    adv = AG.ego_verdicts(traj, model, batch, atk_dev)
    adv_i = torch.cat([adv['out_i'].reshape(-1), adv['status']]).cpu().numpy()
    sol = AG.ego_verdicts(traj, model, batch, None, env, map_idx)
    sol_i = torch.cat([sol['out_i'].reshape(-1), sol['status']]).cpu().numpy()
    B = int(map_idx.numel())
    adv_i, sol_i = adv_i[:B * 8].reshape(B, 8), sol_i[:B * 8].reshape(B, 8)
    return [(bool(adv_i[b, 2] == 1), bool(sol_i[b, 1] == 0 and sol_i[b, 4] == 0)) for b in range(B)]


def screen_loop(model, scenes, env, thresh, t0):
    """(a): reference :160-207 per scene, with the reads it makes."""
    nrm = model.get_normalizer()
    out = []
    for g, mi in scenes:
        with torch.no_grad():
            pred = model.sample_batched(g, mi, env, 20, include_mean=True)
        feas, step, dist = determine_feasibility_nusc(pred['future_pred'], nrm, thresh, t0, 0.0, 0.0, True, env, mi)
        ego_gt = nrm.unnormalize(g.future_gt[0])
        max_vel = torch.max(torch.norm(ego_gt[1:, :2] - ego_gt[:-1, :2], dim=-1)).cpu().item()
        out.append((max_vel, 0 if feas is None else int(torch.sum(feas).item())))
    return out


def screen_chunks(model, chunks, env, thresh, t0):
    """(b): one sample_batched, one screen_batch and one read-back per chunk."""
    out = []
    for g, mi in chunks:
        with torch.no_grad():
            pred = model.sample_batched(g, mi, env, 20, include_mean=True)
        scr = AG.screen_batch(pred['future_pred'], model, g, env, mi, thresh, t0, 0.0, 0.0, True, 'ego', 0.5)
        out.append(torch.cat([scr['out_i'].reshape(-1), scr['status']]).cpu().numpy())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--screen_agents', type=int, default=AG.DEFAULT_SCREEN_AGENTS)
    ap.add_argument('--also_screen_agents', type=int, nargs='*', default=[])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit('at least 7 repeats')
    if not torch.cuda.is_available():
        raise SystemExit('adv_verdict_bench measures on the GPU; there is none here')
    model = make_model()
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    result = {'device': torch.cuda.get_device_name(0), 'what': 'wall ms, device synchronised around every call, (a) and (b) alternating',
              'verdicts': {}, 'screening': {}}
    for name, sizes in (('36 scenes / 512 agents', ADV_SIZES), ('1 scene / 10 agents', [10])):
        batch, mi = synth.make_batch(sizes, key='adv_bench/%d' % len(sizes))
        traj = injected(batch, 'adv_bench/%d' % len(sizes)).to(DEV)
        batch, mi = batch.to(DEV), mi.to(DEV)
        atk = [1] * len(sizes)
        atk_dev = torch.tensor(atk, dtype=torch.int32, device=DEV)
        same = verdict_loop(traj, model, batch, env, mi, atk) == verdict_calls(traj, model, batch, env, mi, atk_dev)
        t = alternate({'per_scene_loop': lambda: verdict_loop(traj, model, batch, env, mi, atk),
                       'two_calls': lambda: verdict_calls(traj, model, batch, env, mi, atk_dev)}, a.reps)
        result['verdicts'][name] = {'same_verdicts': same, 'per_scene_loop': summary(t['per_scene_loop']), 'two_calls': summary(t['two_calls'])}
        print('verdicts', name, json.dumps(result['verdicts'][name]))
    batch, mi = synth.make_batch(ADV_SIZES, key='adv_bench/screen')
    batch, mi = batch.to(DEV), mi.to(DEV)
    scenes = single_scenes(batch, mi)
    graphs = batch.to_data_list()

    def screening(screen_agents):
        chunks, cur, tot = [], [], 0
        for b, n in enumerate(ADV_SIZES):
            cur.append(b)
            tot += n
            if tot >= screen_agents or b == len(ADV_SIZES) - 1:
                g = Batch.from_data_list([graphs[i] for i in cur]).to(DEV)
                chunks.append((g, mi[cur[0]:cur[-1] + 1]))
                cur, tot = [], 0
        t = alternate({'scene_by_scene': lambda: screen_loop(model, scenes, env, 10.0, 4),
                       'chunked': lambda: screen_chunks(model, chunks, env, 10.0, 4)}, a.reps)
        return {'scenes': len(ADV_SIZES), 'agents': sum(ADV_SIZES), 'screen_agents': screen_agents, 'chunks': len(chunks),
                'scene_by_scene': summary(t['scene_by_scene']), 'chunked': summary(t['chunked'])}
    result['screening'] = screening(a.screen_agents)
    print('screening', json.dumps(result['screening']))
    if a.also_screen_agents:
        result['screening_at_other_chunk_sizes'] = {str(n): screening(n) for n in a.also_screen_agents}
        print('screening at other chunk sizes', json.dumps(result['screening_at_other_chunk_sizes']))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
