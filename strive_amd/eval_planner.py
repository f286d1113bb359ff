"""Planner evaluation on scenario sets (reference src/eval_planner.py): collision rate of the rule-based planner, relative
speed at impact and forward / lateral / total acceleration before the crash, for a directory of generated (adversarial)
scenarios and, as the control, for regular scenes -- same function names, signatures, dictionary keys and output files.

The reference evaluates one scene at a time: ``planner.reset(..., 1, ...)``, a numpy planner rollout, then one shapely polygon
per agent and up-sampled step.  Here ``run_planner_eval`` collects up to ``batch_scenes`` scenes into ONE ``planner.reset`` /
``planner.rollout`` (``strive_planner_rollout``) and ONE metrics launch (``strive_planner_eval_metrics``,
strive_amd/csrc/eval_metrics.hip: up-sampling, box IoU of the ego against every agent and fine step, first hit, collision index,
impact speed and the acceleration series, float64).  The kernel returns per-scene sums and frame counts; the pooled means the
reference prints (``np.mean`` over the frames of all scenes) are total / count (utils/scenario_gen.py, ``PooledMetric``).

Command line (the nuScenes devkit and data are not needed for scenario directories written on the synthetic lane world):

    python -m strive_amd.eval_planner --scenario_dir DIR --skip_regular --lane_world synthetic --out OUT
"""
import csv
import json
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .eval_common import scene_jsons
from .utils.scenario_gen import log_metric_sum, log_freq_stat, print_metrics

INTERP_SCALE = 3                 # the reference up-samples x3 before checking collisions (src/eval_planner.py:129)
MAX_MAPS_PER_CALL = 4            # HardcodeNuscPlanner.reset packs at most 4 lane graphs
MISSING_METRICS = ['mean_accel', 'mean_accel_fwd', 'mean_accel_lat', 'coll_vel']
OUT_I = ('did_collide', 'coll_time', 'coll_agt', 'coll_idx', 'accel_count')
OUT_D = ('coll_vel', 'accel_sum', 'accel_max', 'accel_fwd_sum', 'accel_fwd_max', 'accel_lat_sum', 'accel_lat_max')


def read_adv_scenes(scene_path):
    """Every ``*.json`` scenario of a directory, sorted by name, as the dicts of the reference's evaluation (src/eval_planner.py
    :90-112): ``name, map, attack_t, past, init_state`` (last past step), ``veh_att``, ``adv_fut`` (agents 1..) and ``plan_fut``
    (agent 0 of ``fut_adv``)."""
    scenes = []
    for name, jd in scene_jsons(scene_path):
        if jd is None:
            continue
        fut = torch.tensor(jd['fut_adv'])
        past = torch.tensor(jd['past'])
        scenes.append({'name': name, 'map': jd['map'], 'attack_t': jd.get('attack_t'), 'past': past,
                       'init_state': past[:, -1, :], 'veh_att': torch.tensor(jd['lw']), 'adv_fut': fut[1:], 'plan_fut': fut[0]})
    return scenes


def planner_eval_metrics(plan, others, ptr, lw_ego, lw_others, dt, scale=INTERP_SCALE, lib=None):
    """The raw kernel: plan (B,T,4), others (NR,T,4) (NaN = unobserved), ptr (B+1) offsets of every scene's agents in
    ``others``, lw_ego (B,2), lw_others (NR,2) -> (out_i (B,5) int32 [OUT_I], out_d (B,7) float64 [OUT_D], status (B) int32) on the
    inputs' device.  Rows of scenes with a non-zero status (1: no other agent) are not written and come back as -1 / NaN."""
    lib = ops._lib_for(plan, others) if lib is None else lib
    dev = plan.device
    plan = plan.detach().to(torch.float64).contiguous()
    B, T = int(plan.shape[0]), int(plan.shape[1])
    others = others.detach().to(device=dev, dtype=torch.float32).reshape(-1, T, 4).contiguous()
    NR = int(others.shape[0])
    ptr = torch.as_tensor(ptr).to(device=dev, dtype=torch.int32).contiguous()
    lw_ego = lw_ego.detach().to(device=dev, dtype=torch.float32).reshape(B, 2).contiguous()
    lw_others = lw_others.detach().to(device=dev, dtype=torch.float32).reshape(NR, 2).contiguous()
    if tuple(plan.shape) != (B, T, 4) or ptr.numel() != B + 1:
        raise ValueError('planner_eval_metrics expects plan (B,T,4) and ptr (B+1)')
    out_i = torch.full((B, len(OUT_I)), -1, dtype=torch.int32, device=dev)
    out_d = torch.full((B, len(OUT_D)), float('nan'), dtype=torch.float64, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    if NR == 0:                                        # never hand a NULL pointer to the library
        others = torch.zeros((1, T, 4), dtype=torch.float32, device=dev)
        lw_others = torch.ones((1, 2), dtype=torch.float32, device=dev)
    lib.call('strive_planner_eval_metrics', L.ptr(plan), L.ptr(others), L.ptr(ptr), L.ptr(lw_ego), L.ptr(lw_others), B, NR, T,
             int(scale), float(dt), L.ptr(out_i), L.ptr(out_d), L.ptr(status), L.stream_ptr(plan))
    return out_i, out_d, status


def _log_scene(oi, od, metrics, freq_metrics_cnt, freq_metrics_total, prefix, log_no_prefix_copy):
    """One scene's kernel outputs (host rows) into the running dictionaries, in the reference's key order (:142-216)."""
    did, count = int(oi[0]), int(oi[4])
    names = [prefix] + (['total'] if log_no_prefix_copy else [])
    for p in names:
        freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, p + '_coll', did, 1)
    cur = {'did_collide': did}
    if did:
        for p in names:
            metrics = log_metric_sum(metrics, p + '_coll_vel', od[0], 1)
        cur['coll_vel'] = float(od[0])
    if count > 0:
        for key, col, seq in (('_accel', 1, 'mean_accel'), ('_accel_fwd', 3, 'mean_accel_fwd'), ('_accel_lat', 5, 'mean_accel_lat')):
            for p in names:
                metrics = log_metric_sum(metrics, p + key, od[col], count)
            cur[seq] = float(od[col]) / count
    return metrics, freq_metrics_cnt, freq_metrics_total, cur


def compute_metrics(planner_traj, non_ego_traj, veh_att, dt, metrics, freq_metrics_cnt, freq_metrics_total, prefix,
                    log_no_prefix_copy=True, ego_idx=0):
    """Metrics of ONE scene (reference src/eval_planner.py:114-218; the kernel with B = 1): planner_traj (T,4), non_ego_traj
    (NA-1,T,4) with NaN for unobserved frames, veh_att (NA,2) INCLUDING the ego at row ``ego_idx``; all unnormalised, on the
    device the kernel runs on.  Adds to ``metrics`` (``<prefix>_coll_vel, _accel, _accel_fwd, _accel_lat``) and to the
    frequency pair (``<prefix>_coll``), with ``total_`` copies unless ``log_no_prefix_copy`` is False, and returns
    ``(metrics, freq_metrics_cnt, freq_metrics_total, cur_seq_metrics)``; ``cur_seq_metrics`` has ``did_collide`` and, when they
    exist, ``coll_vel, mean_accel, mean_accel_fwd, mean_accel_lat``."""
    NA = int(veh_att.shape[0])
    if NA < 2 or int(non_ego_traj.shape[0]) != NA - 1:
        raise ValueError('compute_metrics needs at least one non-ego agent and veh_att (NA,2) for non_ego_traj (NA-1,T,4)')
    keep = [i for i in range(NA) if i != int(ego_idx)]
    out_i, out_d, status = planner_eval_metrics(planner_traj.unsqueeze(0), non_ego_traj, [0, NA - 1], veh_att[int(ego_idx)].view(1, 2),
                                                veh_att[keep], dt)
    assert int(status[0]) == 0
    return _log_scene(out_i[0].cpu().numpy(), out_d[0].cpu().numpy(), metrics, freq_metrics_cnt, freq_metrics_total, prefix,
                      log_no_prefix_copy)


def group_scenes(num_steps, map_names, batch_scenes, max_maps=MAX_MAPS_PER_CALL):
    """Consecutive groups of scene indices for one planner / metrics call each: at most ``batch_scenes`` scenes, one number of
    future steps per group, at most ``max_maps`` distinct maps per group.  A new group starts where either condition would
    break, so the concatenated groups are the input order."""
    if batch_scenes < 1:
        raise ValueError('batch_scenes must be at least 1')
    groups, cur, maps = [], [], []
    for i, (ft, name) in enumerate(zip(num_steps, map_names)):
        new_map = name not in maps
        if cur and (len(cur) >= batch_scenes or ft != num_steps[cur[0]] or (new_map and len(maps) >= max_maps)):
            groups.append(cur)
            cur, maps, new_map = [], [], True
        cur.append(i)
        if new_map:
            maps.append(name)
    if cur:
        groups.append(cur)
    return groups


def _gather_scenes(eval_loader, map_env, state_norm, att_norm, scenario_dir, skip_regular, filter_regular):
    """The work list in the reference's order: adversarial scenes as ``adv_<name>``, then regular ones as ``regular_seq_%05d``."""
    items = []
    adv_scene_list = None
    if scenario_dir is not None:
        print('Reading in adversarial scenarios...')
        adv_scene_list = read_adv_scenes(scenario_dir)
        for sc in adv_scene_list:
            if sc['init_state'].size(0) == 1:
                print('Only ego in scene, skipping...')
                continue
            items.append(dict(name='adv_' + sc['name'], prefix='adv', map=sc['map'], init_state=sc['init_state'], veh_att=sc['veh_att'],
                              others=sc['adv_fut'], replay=sc['plan_fut']))
    if not skip_regular:
        wanted = None
        if filter_regular:
            assert adv_scene_list is not None, 'filter_regular needs a scenario directory'
            wanted = set(int(sc['name'].split('_')[1]) for sc in adv_scene_list)
        for i, data in enumerate(eval_loader):
            if wanted is not None and i not in wanted:
                continue
            scene_graph, map_idx = data
            if scene_graph.past_gt.size(0) == 1:
                print('Only ego in scene, skipping...')
                continue
            fut = state_norm.unnormalize(scene_graph.future_gt[:, :, :4])
            items.append(dict(name='regular_seq_%05d' % i, prefix='regular', map=map_env.map_list[int(torch.as_tensor(map_idx).reshape(-1)[0])],
                              init_state=state_norm.unnormalize(scene_graph.past_gt[:, -1, :]), veh_att=att_norm.unnormalize(scene_graph.lw),
                              others=fut[1:], replay=fut[0]))
    return items


def run_planner_eval(plan_cfg, eval_loader, map_env, dt, device, out_path, state_norm, att_norm, scenario_dir=None,
                     skip_regular=False, eval_replay_planner=False, filter_regular=False, batch_scenes=64, details_out=None):
    """The reference's evaluation (src/eval_planner.py:221-380), batched: the scenarios of ``scenario_dir`` first (``adv_<name>``,
    sorted by file name), then -- unless ``skip_regular`` -- the scenes of ``eval_loader`` (any iterable of ``(scene_graph,
    map_idx)`` with one scene each; ``regular_seq_%05d``; with ``filter_regular`` only those whose index names a scenario).  The
    ego is agent 0; ego-only scenes are skipped.  Up to ``batch_scenes`` consecutive scenes with the same number of future steps
    and at most 4 distinct maps (``group_scenes``) go through ONE ``planner.reset`` / ``planner.rollout`` and ONE metrics launch
    on ``device``.  With ``eval_replay_planner`` no planner runs: the ego follows ``plan_fut`` of the JSON / its ground-truth
    future.  A planner failure raises, as in the reference.

    Returns ``(metrics, freq_metrics_cnt, freq_metrics_total, names, seq_metrics_list)`` (the reference returns nothing) and
    writes ``all_eval_results.csv`` (scene name + the per-scene metrics in sorted key order, NaN where a scene has none).
    Deviation: the reference writes that file only inside its ``if not skip_regular`` branch; here it is written whenever at
    least one scene was evaluated.  ``details_out`` is not part of the reference's signature: a list
    given here receives, per evaluated scene and in ``names`` order, a dict with the ego trajectory ``plan`` (FT,4) float64 and the
    kernel's discrete outputs ``coll_time, coll_agt, coll_idx, accel_count`` (diagnostics; the tests read them)."""
    from .planners.hardcode_goalcond_nusc import HardcodeNuscPlanner
    os.makedirs(out_path, exist_ok=True)
    device = torch.device(device)
    items = _gather_scenes(eval_loader, map_env, state_norm, att_norm, scenario_dir, skip_regular, filter_regular)
    planner = None if eval_replay_planner else HardcodeNuscPlanner(map_env, plan_cfg)
    metrics, freq_metrics_cnt, freq_metrics_total = {}, {}, {}
    names, seq_metrics_list = [], []
    groups = group_scenes([int(it['others'].shape[1]) for it in items], [it['map'] for it in items], int(batch_scenes))
    for group in groups:
        scenes = [items[i] for i in group]
        B, FT = len(scenes), int(scenes[0]['others'].shape[1])
        counts = [int(s['veh_att'].shape[0]) for s in scenes]
        others = torch.cat([s['others'][:, :, :4] for s in scenes], dim=0).to(device=device, dtype=torch.float32)
        veh_att = torch.cat([s['veh_att'] for s in scenes], dim=0).to(device=device, dtype=torch.float32)
        ptr = np.concatenate([[0], np.cumsum(counts)])
        non_ego_ptr = ptr - np.arange(B + 1)
        ego_rows = torch.as_tensor(ptr[:-1], dtype=torch.long, device=device)
        ego_mask = torch.zeros((int(ptr[-1]),), dtype=torch.bool, device=device)
        ego_mask[ego_rows] = True
        if eval_replay_planner:
            plan = torch.stack([s['replay'][:, :4] for s in scenes], dim=0).to(device=device, dtype=torch.float64)
        else:
            init_state = torch.cat([s['init_state'] for s in scenes], dim=0).to(device)
            batch_mask = torch.cat([torch.full((n,), b, dtype=torch.long) for b, n in enumerate(counts)]).to(device)
            map_idx = torch.tensor([map_env.map_list.index(s['map']) for s in scenes], dtype=torch.long)
            planner.reset(init_state, veh_att, batch_mask, B, map_idx, ego_idx=0)
            plan_t = np.linspace(dt, dt * FT, FT)
            plan = planner.rollout(others, plan_t, non_ego_ptr, plan_t, control_all=False)       # (B, FT, 4) float64
            planner.check(wait=True, on_error='raise')
        out_i, out_d, status = planner_eval_metrics(plan, others, non_ego_ptr, veh_att[ego_mask], veh_att[~ego_mask], dt)
        out_i, out_d, status = out_i.cpu().numpy(), out_d.cpu().numpy(), status.cpu().numpy()
        assert not status.any(), 'ego-only scenes are skipped before the kernel'
        plan_host = plan.cpu()
        for b, s in enumerate(scenes):
            metrics, freq_metrics_cnt, freq_metrics_total, cur = _log_scene(out_i[b], out_d[b], metrics, freq_metrics_cnt,
                                                                            freq_metrics_total, s['prefix'], True)
            for mm in MISSING_METRICS:
                if mm not in cur:
                    cur[mm] = np.nan
            names.append(s['name'])
            seq_metrics_list.append(cur)
            if details_out is not None:
                details_out.append(dict(plan=plan_host[b].clone(), coll_time=int(out_i[b][1]), coll_agt=int(out_i[b][2]),
                                        coll_idx=int(out_i[b][3]), accel_count=int(out_i[b][4])))
    if seq_metrics_list:
        with open(os.path.join(out_path, 'all_eval_results.csv'), 'w') as f:
            csvwrite = csv.writer(f)
            met_names = sorted(seq_metrics_list[0].keys())
            csvwrite.writerow(['scene'] + met_names)
            for name, cur in zip(names, seq_metrics_list):
                csvwrite.writerow([name] + [cur[k] for k in met_names])
    print('Final ================')
    print_metrics(metrics, freq_metrics_cnt, freq_metrics_total)
    return metrics, freq_metrics_cnt, freq_metrics_total, names, seq_metrics_list


class SyntheticLaneWorld(object):
    """Map environment of ``--lane_world synthetic``: the lane graph of strive_amd.synth.make_lane_graph under the map names
    the synthetic scenes carry (``synthetic-0`` ...).  The planner needs ``map_list`` and ``lane_graphs`` only."""

    def __init__(self, nmaps=MAX_MAPS_PER_CALL):
        from . import synth
        lg = synth.make_lane_graph()
        self.map_list = ['synthetic-%d' % i for i in range(nmaps)]
        self.lane_graphs = {m: lg for m in self.map_list}


def get_parser():
    import argparse
    from .planners.hardcode_goalcond_nusc import DEF_CONFIG
    p = argparse.ArgumentParser(description='Planner evaluation')
    p.add_argument('--out', type=str, default='./out/eval_planner_out', help='output directory')
    p.add_argument('--scenario_dir', type=str, default=None, help='directory of scenario JSON files to evaluate on')
    p.add_argument('--skip_regular', action='store_true', help='only evaluate the scenarios of --scenario_dir')
    p.add_argument('--tracks', type=str, default=None, help='tracks file (datasets/tracks.py) whose windows are the regular scenes')
    p.add_argument('--eval_replay_planner', action='store_true', help='evaluate the recorded ego trajectory instead of the planner')
    p.add_argument('--batch_scenes', type=int, default=64, help='scenes per planner / metrics call')
    p.add_argument('--lane_world', type=str, default=None, choices=['synthetic'], help='map environment with lane graphs')
    p.add_argument('--maps', type=str, default=None, help='a maps file (datasets/maps.py) with the maps the scenes name, instead of --lane_world')
    p.add_argument('--dt', type=float, default=0.5, help='time step of the scenarios')
    p.add_argument('--device', type=str, default='cuda:0')
    for k, v in DEF_CONFIG.items():
        if isinstance(v, list):
            p.add_argument('--planner_' + k, type=float, nargs='+', default=v)
        else:
            p.add_argument('--planner_' + k, type=type(v), default=v)
    return p


def main(argv=None):
    from .planners.planner import PlannerConfig
    from .planners.hardcode_goalcond_nusc import DEF_CONFIG
    cfg = vars(get_parser().parse_args(argv))
    from .eval_traffic_tracks import maps_file_env, one_map_source, scenario_map_names
    one_map_source(cfg, 'lane_world')
    if cfg['lane_world'] is None and cfg['maps'] is None:
        raise SystemExit('eval_planner: the nuScenes devkit and data are not available here; a map environment with lane graphs must '
                         'be supplied from Python (run_planner_eval(plan_cfg, loader, map_env, ...)), or use --lane_world synthetic')
    if not cfg['skip_regular'] and cfg['tracks'] is None:
        raise SystemExit('eval_planner: regular scenes need a dataset, which must be supplied from Python (run_planner_eval); '
                         'pass --tracks FILE, or --skip_regular to evaluate --scenario_dir alone')
    plan_cfg_dict = {k: cfg['planner_' + k] for k in DEF_CONFIG}
    os.makedirs(cfg['out'], exist_ok=True)
    with open(os.path.join(cfg['out'], 'plan_cfg.json'), 'w') as f:
        json.dump(plan_cfg_dict, f)
    regular = not (cfg['skip_regular'] or cfg['tracks'] is None)
    file_world = None
    if cfg['maps'] is not None:                  # the maps the scenes were driven on, lane graphs built on the device
        from .datasets.tracks import load_tracks
        needed = scenario_map_names(cfg['scenario_dir']) if cfg['scenario_dir'] is not None else []
        needed += [m for m in (load_tracks(cfg['tracks'])['scene_map'] if regular else []) if m not in needed]
        file_world = maps_file_env(cfg['maps'], needed, cfg['device'], load_lanegraph=True)
    if not regular:
        run_planner_eval(PlannerConfig(**plan_cfg_dict), None, file_world or SyntheticLaneWorld(), cfg['dt'], cfg['device'], cfg['out'], None, None,
                         scenario_dir=cfg['scenario_dir'], skip_regular=True, eval_replay_planner=cfg['eval_replay_planner'],
                         batch_scenes=cfg['batch_scenes'])
        return
    # regular scenes: every window of the tracks file, one scene per item as the reference's loader of batch size 1 yields them
    from . import synth
    from .datasets.nuscenes_dataset import NuScenesDataset
    if file_world is not None:
        world = file_world
    else:
        raster, dx = synth.make_raster(M=MAX_MAPS_PER_CALL)
        world = synth.SyntheticMapEnv(raster, dx, lane_graph=synth.make_lane_graph()).to(cfg['device'])
    ds = NuScenesDataset(cfg['tracks'], world, device=cfg['device'])
    run_planner_eval(PlannerConfig(**plan_cfg_dict), ds.loader(1), world, cfg['dt'], cfg['device'], cfg['out'], ds.get_state_normalizer(),
                     ds.get_att_normalizer(), scenario_dir=cfg['scenario_dir'], skip_regular=False,
                     eval_replay_planner=cfg['eval_replay_planner'], batch_scenes=cfg['batch_scenes'])


if __name__ == '__main__':
    main()
