#!/usr/bin/env python3
"""Generate tests/golden/g17_planner_eval.npz and tests/golden/g17_scenarios/*.json: the reference's planner evaluation
(src/eval_planner.py, ``run_planner_eval`` / ``compute_metrics``) run by the reference on scenario files of the synthetic lane world.

Like make_golden_gru.py this runs the reference itself in the build container and stores only its inputs and outputs.  It uses
make_golden's import stand-ins (PyG stubs, the EXACT shapely stand-in, ``_LaneEnv``) and stubs what eval_planner.py imports on top:
the nuScenes dataset module and configargparse (absent); matplotlib's Agg backend and tqdm are present.  One numeric stand-in for the
numpy the reference was written for: ``_widen_initial_world``.  The files are described in tests/golden/README_g17.md.

Scenes (dt 0.5 s; every agent drives straight at constant speed from a lane node, the ego is agent 0; designated agents instead
ride ``far`` metres beside the ego's recorded trajectory and jump to ``near`` metres at one coarse step):

  sc_0000_mid      T 12, 18 others; agent 5 cuts into the ego's lane at coarse step 5
  sc_0001_step0    T 12,  1 other ; overlaps the ego from the first fine step (coll_idx 0)
  sc_0002_cidx1    T  8,  3 others; hit at coarse step 1 (coll_idx 1: no acceleration block)
  sc_0003_last     T 12,  3 others; hit at the last coarse step
  sc_0004_none     T 12,  3 others; no collision
  sc_0005_pair     T 12,  4 others; agents 2 and 3 (others' rows 1, 2) first overlap the ego at the same fine step
  sc_0006_nantail  T  8,  3 others; the colliding agent is unobserved (NaN) from two steps after the hit

These properties hold for the RECORDED ego trajectory (``eval_replay_planner=True``) and are asserted below from the reference's
own outputs; with the reference's planner driving the ego the outcomes are whatever the planner makes of them (recorded too).
Regular scenes: four one-scene graphs (index 1 is ego-only and skipped, as the reference does), ``regular_inputs()``.

g17_planner_eval.npz, for mode in ('plan', 'replay'):
  <mode>/metric_keys, metric_mean, metric_count     run_planner_eval's ``metrics`` (captured at print_metrics): keys in insertion
                                                    order, np.mean and len of every list
  <mode>/freq_keys, freq_cnt, freq_total            the two frequency dictionaries
  <mode>/names                                      adv_<name> ... regular_seq_%05d ..., evaluation order
  <mode>/<name>/plan                                the ego trajectory handed to compute_metrics (float64 planner / fp32 replay)
  <mode>/<name>/did_collide, coll_time, coll_agt, coll_idx, coll_vel, mean_accel, mean_accel_fwd, mean_accel_lat, accel_count
                                                    cur_seq_metrics (NaN where absent), np.amin / np.argmin of
                                                    check_single_veh_coll's times, the collision index, frames in the accel block
  <mode>/<name>/iou                                 (others, T*3) the reference's IoU at EVERY pair (NaN = skipped frame)
Tie condition (asserted here and in tests/test_planner_eval.py): every IoU differs from the 0.02 threshold by more than 1e-3.

Usage:  python tests/golden/make_golden_planner_eval.py
"""
import contextlib
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                         # noqa: E402
from strive_amd import synth                                     # noqa: E402
from strive_amd.graph import Batch                               # noqa: E402
from strive_amd.constants import state_norm_tensors, att_norm_tensors    # noqa: E402

DT = 0.5
PT = 4
SCALE = 3
IOU_THRESH = 0.02
TIE_MARGIN = 1e-3
SCEN_DIR = os.path.join(HERE, 'g17_scenarios')
MAP_NAME = 'synthetic-0'

# name -> (T, agents, centre, [(agent, side, far, near, switch step, NaN from step or None)])
ADV_SCENES = [
    ('sc_0000_mid', 12, 19, (128.0, 128.0), [(5, +1, 8.0, 0.9, 5, None)]),
    ('sc_0001_step0', 12, 2, (168.0, 128.0), [(1, -1, 0.8, 0.8, 0, None)]),
    ('sc_0002_cidx1', 8, 4, (128.0, 168.0), [(2, +1, 8.0, 0.9, 1, None)]),
    ('sc_0003_last', 12, 4, (88.0, 128.0), [(1, -1, 8.0, 0.5, 11, None)]),
    ('sc_0004_none', 12, 4, (128.0, 88.0), []),
    ('sc_0005_pair', 12, 5, (88.0, 168.0), [(2, +1, 7.0, 0.9, 6, None), (3, -1, 7.0, 0.9, 6, None)]),
    ('sc_0006_nantail', 8, 4, (88.0, 88.0), [(3, +1, 8.0, 0.7, 3, 5)]),
]
REGULAR_SIZES = [4, 1, 3, 6]


def adv_scene_dict(name, T, n, centre, riders):
    """One scenario in the wire format of prepare_output_dict (keys as tests/golden/g9_scenario_full.json), fp32 values."""
    lg = synth.make_lane_graph()
    px, py, h, s = synth.lane_scene_poses(lg, n, 'g17/' + name, radius=38.0 if n <= 8 else 75.0, centre=centre, min_gap=9.0)
    t = (np.arange(PT + T) - (PT - 1)) * DT                               # 0 at the last past step
    c, sn = np.cos(h), np.sin(h)
    x = px[:, None] + (s * c)[:, None] * t[None]
    y = py[:, None] + (s * sn)[:, None] * t[None]
    state = np.stack([x, y, np.broadcast_to(c[:, None], x.shape), np.broadcast_to(sn[:, None], x.shape),
                      np.broadcast_to(s[:, None], x.shape), np.zeros_like(x)], -1)              # (n, PT+T, 6)
    for agent, side, far, near, switch, _ in riders:
        off = np.where(np.arange(PT + T) - PT < switch, far, near) * side
        state[agent, :, 0] = x[0] - sn[0] * off
        state[agent, :, 1] = y[0] + c[0] * off
        state[agent, :, 2:4] = state[0, :, 2:4]
        state[agent, :, 4] = s[0]
    lw = np.stack([4.2 + 0.4 * synth.counter_uniform((n,), 'g17/l/' + name), 1.9 + 0.2 * synth.counter_uniform((n,), 'g17/w/' + name)], -1)
    state = state.astype(np.float32)
    fut = state[:, PT:, :4].copy()
    for agent, _, _, _, _, nan_from in riders:
        if nan_from is not None:
            fut[agent, nan_from:] = np.nan
    sem = np.zeros((n, 2), dtype=np.float32)
    sem[:, 0] = 1.0
    out = {'N': n, 'dt': DT, 'map': MAP_NAME, 'lw': lw.astype(np.float32).tolist(), 'sem': sem.tolist(), 'past': state[:, :PT].tolist(),
           'fut_init': fut.tolist(), 'fut_adv': fut.tolist()}
    out['attack_agt'] = int(riders[0][0]) if riders else 1        # (the reference's reader requires attack_t)
    out['attack_t'] = int(riders[0][4]) if riders else 0
    return out


def regular_inputs():
    """[(scene_graph, map_idx)] with one NORMALISED scene each (what a batch-size-1 loader yields), agents on the lane graph."""
    lg = synth.make_lane_graph()
    out = []
    for b, n in enumerate(REGULAR_SIZES):
        poses = synth.lane_scene_poses(lg, n, 'g17/reg/%d' % b, radius=30.0, centre=(128.0 + 40.0 * (b % 2), 128.0 - 40.0 * (b // 2)),
                                       min_gap=9.0)
        out.append((Batch.from_data_list([synth.make_scene(n, 'g17/reg/%d' % b, poses=poses)]), torch.zeros((1,), dtype=torch.long)))
    return lg, out


def write_scenarios():
    os.makedirs(SCEN_DIR, exist_ok=True)
    for name, T, n, centre, riders in ADV_SCENES:
        with open(os.path.join(SCEN_DIR, name + '.json'), 'w') as f:
            json.dump(adv_scene_dict(name, T, n, centre, riders), f)
    print('wrote g17_scenarios/*.json (%d files)' % len(ADV_SCENES))


def save_deterministic(name, arrs):
    """np.savez_compressed with fixed member timestamps, so that a second run writes the same bytes."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())
    print('wrote %s (%.1f KB)' % (name, os.path.getsize(path) / 1024.0))


def import_eval_planner():
    R = mg.import_reference()
    mg._install_exact_shapely()
    stub = types.ModuleType('datasets.nuscenes_dataset')
    stub.NuScenesDataset = type('NuScenesDataset', (object,), {})
    sys.modules['datasets.nuscenes_dataset'] = stub
    if 'configargparse' not in sys.modules:
        sys.modules['configargparse'] = types.ModuleType('configargparse')
    import importlib
    R.eval_planner = importlib.import_module('eval_planner')
    _widen_initial_world(R)
    return R


def _widen_initial_world(R):
    """The reference is written for numpy 1.19 (its requirements.txt), where an fp32 scalar combined with a Python float gives
    float64.  Its planner keeps every object's initial x, y, h, s, l, w as the fp32 scalars of the state tensor (state_conv,
    src/planners/hardcode_goalcond_nusc.py:80-98); under numpy >= 2 (NEP 50) expressions such as ``1 + s * tmax`` then stay in
    fp32 and move a plan that reacts to another agent by ~3e-7 m (sc_0000_mid).  Like the ``np.int`` / ``np.product`` aliases of
    make_golden this restores the arithmetic the reference was written for: the initial world's scalars are widened (exactly) to
    Python floats."""
    P = R.planner.HardcodeNuscPlanner
    if getattr(P.state_conv, '_widened', False):
        return
    orig = P.state_conv

    def state_conv(self, graph_state, veh_att):
        wstate = orig(self, graph_state, veh_att)
        for obj in wstate['objs'].values():
            for k in obj:
                obj[k] = float(obj[k])
        return wstate
    state_conv._widened = True
    P.state_conv = state_conv


def all_pair_ious(R, traj_tgt, lw_tgt, traj_others, lw_others):
    """The IoU expression of check_single_veh_coll (reference src/losses/adv_gen_nusc.py:543-559) at EVERY (agent, step)."""
    from shapely.geometry import Polygon
    tgt, ltgt = traj_tgt.cpu().numpy(), lw_tgt.cpu().numpy()
    oth, loth = traj_others.cpu().numpy(), lw_others.cpu().numpy()
    NA, FT = oth.shape[0], oth.shape[1]
    iou = np.full((NA, FT), np.nan)
    polys = [Polygon(R.nutils.get_corners(tgt[t, :], ltgt)) for t in range(FT)]
    for aj in range(NA):
        for t in range(FT):
            if np.sum(np.isnan(oth[aj, t, :])) > 0:
                continue
            pj = Polygon(R.nutils.get_corners(oth[aj, t, :], loth[aj]))
            iou[aj, t] = polys[t].intersection(pj).area / polys[t].union(pj).area
    return iou


def run_mode(R, replay, tmp_out):
    E = R.eval_planner
    lg, regular = regular_inputs()
    env = mg._LaneEnv(lg)
    snorm = R.dutils.MeanStdNormalizer(*state_norm_tensors())
    anorm = R.dutils.MeanStdNormalizer(*att_norm_tensors())
    rec = {'scenes': [], 'final': None}
    orig_cm, orig_chk, orig_pm = E.compute_metrics, R.adv_losses.check_single_veh_coll, E.print_metrics

    def chk(traj_tgt, lw_tgt, traj_others, lw_others):
        coll, times = orig_chk(traj_tgt, lw_tgt, traj_others, lw_others)
        rec['cur'] = dict(times=np.asarray(times).copy(), iou=all_pair_ious(R, traj_tgt, lw_tgt, traj_others, lw_others))
        return coll, times

    def cm(planner_traj, non_ego_traj, veh_att, dt, metrics, cnt, tot, prefix, **kw):
        before = {k: len(v) for k, v in metrics.items()}
        res = orig_cm(planner_traj, non_ego_traj, veh_att, dt, metrics, cnt, tot, prefix, **kw)
        cur = rec.pop('cur')
        seq = dict(res[3])
        T = planner_traj.size(0)
        ct, ca = int(np.amin(cur['times'])), int(np.argmin(cur['times']))
        interp_dt = dt / float(SCALE)
        cidx = int((ct * interp_dt) / dt) if seq['did_collide'] else T - 1
        nacc = len(res[0].get(prefix + '_accel', [])) - before.get(prefix + '_accel', 0)
        rec['scenes'].append(dict(plan=planner_traj.numpy().copy(), seq=seq, coll_time=ct, coll_agt=ca, coll_idx=cidx, accel_count=nacc,
                                  iou=cur['iou']))
        return res

    def pm(metrics, cnt, tot):
        rec['final'] = ({k: list(v) for k, v in metrics.items()}, dict(cnt), dict(tot))

    E.compute_metrics, R.adv_losses.check_single_veh_coll, E.print_metrics = cm, chk, pm
    E.tqdm = types.SimpleNamespace(tqdm=lambda it: it)
    plan_cfg = R.planner_base.PlannerConfig(**R.planner.CONFIG_DICT['default'])
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            E.run_planner_eval(plan_cfg, regular, env, DT, torch.device('cpu'), tmp_out, snorm, anorm, scenario_dir=SCEN_DIR,
                               skip_regular=False, eval_replay_planner=replay, filter_regular=False)
    finally:
        E.compute_metrics, R.adv_losses.check_single_veh_coll, E.print_metrics = orig_cm, orig_chk, orig_pm
    names = ['adv_' + s[0] for s in ADV_SCENES] + ['regular_seq_%05d' % i for i, n in enumerate(REGULAR_SIZES) if n > 1]
    assert len(names) == len(rec['scenes'])
    return names, rec


def g17_planner_eval(R):
    import tempfile
    out = {}
    for mode, replay in (('plan', False), ('replay', True)):
        with tempfile.TemporaryDirectory() as tmp:
            names, rec = run_mode(R, replay, tmp)
        metrics, cnt, tot = rec['final']
        out[mode + '/metric_keys'] = np.asarray(list(metrics.keys()))
        out[mode + '/metric_mean'] = np.asarray([np.mean(v) for v in metrics.values()], dtype=np.float64)
        out[mode + '/metric_count'] = np.asarray([len(v) for v in metrics.values()], dtype=np.int64)
        out[mode + '/freq_keys'] = np.asarray(list(cnt.keys()))
        out[mode + '/freq_cnt'] = np.asarray([cnt[k] for k in cnt], dtype=np.int64)
        out[mode + '/freq_total'] = np.asarray([tot[k] for k in cnt], dtype=np.int64)
        out[mode + '/names'] = np.asarray(names)
        by_name = {}
        for name, sc in zip(names, rec['scenes']):
            p = '%s/%s/' % (mode, name)
            out[p + 'plan'] = sc['plan']
            out[p + 'iou'] = sc['iou']
            for k in ('coll_time', 'coll_agt', 'coll_idx', 'accel_count'):
                out[p + k] = np.asarray(sc[k], dtype=np.int64)
            out[p + 'did_collide'] = np.asarray(sc['seq']['did_collide'], dtype=np.int64)
            for k in ('coll_vel', 'mean_accel', 'mean_accel_fwd', 'mean_accel_lat'):
                out[p + k] = np.asarray(sc['seq'].get(k, np.nan), dtype=np.float64)
            margin = np.nanmin(np.abs(sc['iou'] - IOU_THRESH))
            assert margin > TIE_MARGIN, 'tie condition: %s %s has an IoU within %g of the threshold' % (mode, name, margin)
            by_name[name] = sc
            print('%-7s %-22s did %d time %2d agt %2d idx %2d nacc %2d vel %s margin %.4f' % (
                mode, name, sc['seq']['did_collide'], sc['coll_time'], sc['coll_agt'], sc['coll_idx'], sc['accel_count'],
                sc['seq'].get('coll_vel'), margin))
        if replay:
            check_cases(by_name)
    save_deterministic('g17_planner_eval.npz', out)


def check_cases(sc):
    """The properties the scene set exists for, from the reference's outputs in replay mode."""
    g = lambda n: sc['adv_' + n]
    assert g('sc_0000_mid')['seq']['did_collide'] and 3 <= g('sc_0000_mid')['coll_idx'] <= 8 and g('sc_0000_mid')['iou'].shape[0] >= 17
    assert g('sc_0001_step0')['coll_time'] == 0 and g('sc_0001_step0')['coll_idx'] == 0 and g('sc_0001_step0')['iou'].shape[0] == 1
    assert g('sc_0002_cidx1')['coll_idx'] == 1 and g('sc_0002_cidx1')['accel_count'] == 0 and g('sc_0002_cidx1')['plan'].shape[0] == 8
    assert g('sc_0003_last')['seq']['did_collide'] and g('sc_0003_last')['coll_idx'] == 11
    assert not g('sc_0004_none')['seq']['did_collide'] and g('sc_0004_none')['coll_time'] == 36 and g('sc_0004_none')['accel_count'] == 10
    tie = g('sc_0005_pair')
    first = [int(np.argmax(row > IOU_THRESH)) if (row > IOU_THRESH).any() else -1 for row in np.nan_to_num(tie['iou'], nan=0.0)]
    assert first[1] == first[2] == tie['coll_time'] and tie['coll_agt'] == 1 and first[0] != tie['coll_time']
    nt = g('sc_0006_nantail')
    assert nt['seq']['did_collide'] and nt['coll_agt'] == 2 and np.isnan(nt['iou'][2, -1]) and np.isfinite(nt['seq']['coll_vel'])


if __name__ == '__main__':
    torch.set_num_threads(8)
    write_scenarios()
    g17_planner_eval(import_eval_planner())
