#!/usr/bin/env python3
"""Generate tests/golden/g18_adv_eval.npz and tests/golden/g18_scenarios/{adv_sol_success,sol_failed,adv_failed}/*.json: the
reference's quantitative scenario evaluation (src/eval_adv_gen.py: ``quant_eval`` / ``compute_metrics`` / ``compute_coll_feat``) and
the features of src/cluster_scenarios.py (``compute_coll_feat``), run by the reference on scenario files over ``synth.make_raster``.

Like make_golden_planner_eval.py this runs the reference itself in the build container and stores only its inputs and outputs.  It
uses make_golden's import stand-ins and the EXACT shapely stand-in and stubs configargparse (absent); matplotlib (Agg) and
scikit-learn are present.  The raster is regenerated, not stored.  The files are described in tests/golden/README_g18.md.  The wall time of the
reference's compute_metrics per scene is printed (profiles/r17_adv_eval_timing.md quotes it), not stored: it varies from run to run.

Scenes (dt 0.5 s, 256 m world, 0.25 m pixels; roads are the 18 m bands y or x in [40 k, 40 k + 18)).  The ego (agent 0) drives
along +x; "riders" keep the ego's x and heading at a lateral offset that changes per step; "free" agents drive straight along their
own lane.  All coordinates, speeds and sizes are dyadic, so the fp32 chain of the reference is exact or nearly so.

  adv_sol_success/sc_0000_mid    T 12, 18 others; agent 5 closes in and hits at step 6 (attack_agt 5); agents 7, 8 overlap from
                                 step 4 (< CT); agents 9, 10 overlap only from step 7 (>= CT); agent 12 stands off the road; agent
                                 14 is NaN from step 8; fut_internal_ego present; two diagonal headings
  adv_sol_success/sc_0001_step0  T 12,  1 other ; overlap from step 0 (CT 0: rate block NaN, lr_coll_t 0), no "others"
  adv_sol_success/sc_0002_early  T  8,  3 others; agent 3 hits at step 2 (no attacker acceleration block) while half off the road;
                                 attack_agt 1 is not the colliding agent
  adv_sol_success/sc_0003_tie    T 12,  4 others; agents 2 and 3 first hit at the same step (attack_agt 3, coll_agt 2); nobody off
                                 the road; no fut_internal_ego
  sol_failed/sc_0004_offroad     T  8,  3 others; agent 1 (heading (0.96, 0.28)) hits at step 4, agent 2 stands off the road;
                                 fut_internal_ego present
  adv_failed/sc_0005_none        T 12,  3 others; no collision
  adv_failed/sc_0006_alone       T  8,  1 other ; no collision, no "others"

g18_adv_eval.npz:
  names, categories                         scenes in evaluation order and their directory
  <name>/seq_keys, seq_vals                 compute_metrics' seq_metrics (+ sol_success), insertion order
  <name>/coll_t, coll_agt, atk_agt, did_collide, n_others
  <name>/num_coll_veh, num_traj_veh, pair_marks   check_pairwise_veh_coll's outputs (-1 / empty with CT 0)
  <name>/env_coll (NA), env_L, env_W, env_ratio (2) = mean_lw / mean(dx), env_frac (NA, CT) drivable fraction (NaN = skipped frame)
  <name>/counts/<metric>                    number of values compute_metrics added to metrics[<metric>]
  <name>/iou_coarse (NA-1, T), iou_pairs (P, CT) [pairs in (i, j > i) order], iou_fine (NA-1, 5 T): the reference's IoU expression
                                            at EVERY pair (NaN = skipped frame)
  <name>/feat_hvec, feat_angvec, feat_rel_s, feat_h, feat_ang, fine_t, fine_agt, lr_coll_t    (crash scenes)
  metric_keys, metric_mean, metric_count, freq_keys, freq_cnt, freq_total     the three dictionaries after quant_eval
  success_rates (3), csv_names, csv/<file>  every CSV file quant_eval wrote (text)
  labels/<category>                         label_idx per scene; cluster_label_names
  km/feats (N,4), km/init (k,4), km/centers, km/labels, km/inertia, km/n_iter   scikit-learn KMeans(init=km/init, n_init=1,
                                            algorithm='lloyd') on synthetic unit-vector features; km/margin = the smallest gap between
                                            a point's nearest and second-nearest squared distance over all iterations
Tie conditions (asserted here and in tests/test_adv_eval.py): every IoU more than 1e-3 from 0.02; every drivable fraction more than
2 / (L W) from 0.95; both grid ratios more than 1e-3 from a half-integer; k-means distance gaps above 1e-9.

Usage:  python tests/golden/make_golden_adv_eval.py
"""
import contextlib
import io
import json
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                         # noqa: E402
from make_golden_planner_eval import save_deterministic         # noqa: E402
from strive_amd import synth                                     # noqa: E402

DT = 0.5
PT = 4
D_LATENT = 32
IOU_THRESH = 0.02
TIE_MARGIN = 1e-3
FEAT_SCALE = 5
SCEN_DIR = os.path.join(HERE, 'g18_scenarios')
MAP_NAME = 'synthetic-0'
CATEGORIES = ['adv_sol_success', 'sol_failed', 'adv_failed']
CLUSTER_NAMES = ['behind', 'front', 'left', 'right']
KM_N, KM_K = 40, 4

# 12 lanes that never meet: (y, direction)
LANES = [(124.0, 1), (128.0, -1), (132.0, 1), (164.0, -1), (168.0, 1), (172.0, -1), (44.0, 1), (48.0, -1), (52.0, 1), (8.0, 1)]
SIZES = [(4.5, 2.0), (4.125, 1.75), (5.0, 2.25), (4.625, 1.875), (4.0, 2.0)]


def filler(i):
    """Free agent number i of a scene: its own lane, dyadic start, speed and acceleration."""
    y, d = LANES[i % len(LANES)]
    x0 = 128.0 - d * 40.0 + 6.0 * (i % 3)
    return ('free', x0, y, (float(d), 0.0), 2.0 + 0.5 * (i % 7), (0.0, 0.25, -0.125)[i % 3])


def diag(x0, y0):
    return ('free', x0, y0, (0.6, 0.8), 0.5, 0.0)


# name -> dict(cat, T, ego_y, agents {index: spec}, attack_agt, fit, nan {agent: first NaN step}); unspecified agents are fillers
SCENES = [
    dict(name='sc_0000_mid', cat='adv_sol_success', T=12, n=19, ego_y=88.0, attack_agt=5, fit=True, nan={14: 8}, agents={
        5: ('ride', [8, 8, 8, 8, 6, 4, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5]),
        7: ('free', 200.0, 84.0, (1.0, 0.0), 0.0, 0.0), 8: ('free', 215.0, 84.0, (-1.0, 0.0), 5.0, 0.0),
        9: ('free', 30.0, 92.0, (1.0, 0.0), 0.0, 0.0), 10: ('free', 46.0, 92.0, (-1.0, 0.0), 3.0, 0.0),
        12: ('free', 145.0, 110.0, (1.0, 0.0), 0.0, 0.0), 16: diag(206.0, 204.0), 17: diag(166.0, 204.0)}),
    dict(name='sc_0001_step0', cat='adv_sol_success', T=12, n=2, ego_y=88.0, attack_agt=1, fit=True, nan={}, agents={
        1: ('ride', [-1.5] * 12)}),
    dict(name='sc_0002_early', cat='adv_sol_success', T=8, n=4, ego_y=96.5, attack_agt=1, fit=True, nan={}, agents={
        3: ('ride', [6, 3.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5])}),
    dict(name='sc_0003_tie', cat='adv_sol_success', T=12, n=5, ego_y=88.0, attack_agt=3, fit=False, nan={}, agents={
        2: ('ride', [5, 5, 5, 5, 4, 3, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5]), 3: ('ride', [-5, -5, -5, -5, -4, -3, -1.5, -1.5, -1.5, -1.5, -1.5, -1.5])}),
    dict(name='sc_0004_offroad', cat='sol_failed', T=8, n=4, ego_y=88.0, attack_agt=1, fit=True, nan={}, agents={
        1: ('ride', [-5, -5, -4, -3, -1.25, -1.25, -1.25, -1.25], (0.96, 0.28)), 2: ('free', 150.0, 108.0, (0.0, 1.0), 0.0, 0.0)}),
    dict(name='sc_0005_none', cat='adv_failed', T=12, n=4, ego_y=88.0, attack_agt=2, fit=False, nan={}, agents={}),
    dict(name='sc_0006_alone', cat='adv_failed', T=8, n=2, ego_y=88.0, attack_agt=1, fit=True, nan={}, agents={}, lw={1: (4.625, 1.875)}),
]


def scene_dict(sc):
    """One scenario in the wire format of prepare_output_dict (keys as tests/golden/g9_scenario_full.json), fp32 values."""
    T, n, name = sc['T'], sc['n'], sc['name']
    steps = np.arange(PT + T) - (PT - 1)                      # 0 at the last past step
    state = np.zeros((n, PT + T, 6))
    ego_v = 8.0 + 0.5 * (np.arange(PT + T) % 3)              # m/s over the step that ENDS at the frame
    state[0, :, 0] = 100.0 + np.cumsum(ego_v * DT) - np.sum(ego_v[:PT] * DT)
    state[0, :, 1] = sc['ego_y']
    state[0, :, 2] = 1.0
    state[0, :, 4] = ego_v
    nf = 0
    for a in range(1, n):
        spec = sc['agents'].get(a)
        if spec is None:
            spec = filler(nf + 3 * int(name[3:7]))
            nf += 1
        if spec[0] == 'ride':
            off = np.asarray([spec[1][0]] * PT + list(spec[1]), dtype=np.float64)
            state[a, :, 0] = state[0, :, 0]
            state[a, :, 1] = sc['ego_y'] + off
            state[a, :, 2], state[a, :, 3] = spec[2] if len(spec) > 2 else (1.0, 0.0)
            state[a, :, 4] = ego_v
        else:
            _, x0, y0, (hx, hy), v0, acc = spec
            v = np.maximum(v0 + acc * np.maximum(steps, 0), 0.0)
            dist = np.cumsum(v * DT) - np.sum(v[:PT] * DT)
            state[a, :, 0] = x0 + hx * dist
            state[a, :, 1] = y0 + hy * dist
            state[a, :, 2], state[a, :, 3], state[a, :, 4] = hx, hy, v
    lw = np.asarray([SIZES[(a + int(name[3:7])) % len(SIZES)] if a else SIZES[0] for a in range(n)])
    for a, spec in sc['agents'].items():
        if spec[0] == 'ride':
            lw[a] = (4.5, 2.0)
    for a, size in sc.get('lw', {}).items():
        lw[a] = size
    state = state.astype(np.float32)
    fut = state[:, PT:, :4].copy()
    for a, first in sc['nan'].items():
        fut[a, first:] = np.nan
    sem = np.zeros((n, 2), dtype=np.float32)
    sem[:, 0] = 1.0
    key = 'g18/' + name
    z = np.round(synth.counter_normal((n, D_LATENT), key + '/z') * 64.0) / 64.0
    mean = np.round(synth.counter_normal((n, D_LATENT), key + '/m') * 64.0) / 256.0
    var = 2.0 ** np.round(synth.counter_uniform((n, D_LATENT), key + '/v', -3.0, 1.0))
    out = {'N': n, 'dt': DT, 'map': MAP_NAME, 'lw': lw.astype(np.float32).tolist(), 'sem': sem.tolist(), 'past': state[:, :PT].tolist(),
           'fut_init': fut.tolist(), 'fut_adv': fut.tolist(), 'attack_agt': int(sc['attack_agt']), 'attack_t': T // 2,
           'z_adv': z.astype(np.float32).tolist(), 'z_prior': {'mean': mean.astype(np.float32).tolist(), 'var': var.astype(np.float32).tolist()}}
    if sc['fit']:
        fit = fut[0].copy()
        fit[:, 1] += 0.125 * (np.arange(T) % 3)
        fit[:, 0] -= 0.25 * (np.arange(T) % 2)
        fit[1::2, 2], fit[1::2, 3] = 0.8, 0.6
        out['fut_internal_ego'] = fit.astype(np.float32).tolist()
    return out


def write_scenarios():
    for cat in CATEGORIES:
        os.makedirs(os.path.join(SCEN_DIR, cat), exist_ok=True)
    for sc in SCENES:
        with open(os.path.join(SCEN_DIR, sc['cat'], sc['name'] + '.json'), 'w') as f:
            json.dump(scene_dict(sc), f)
    print('wrote g18_scenarios/*/*.json (%d files)' % len(SCENES))


def km_inputs():
    """Synthetic clustering features: (angvec, hvec) unit vectors around four collision types, and the starting centres."""
    base = np.asarray([[np.pi, 0.0], [0.0, np.pi], [0.5 * np.pi, 0.3], [-0.5 * np.pi, -0.3]])
    ang = base[np.arange(KM_N) % KM_K] + synth.counter_uniform((KM_N, 2), 'g18/km', -0.5, 0.5)
    feats = np.stack([np.cos(ang[:, 0]), np.sin(ang[:, 0]), np.cos(ang[:, 1]), np.sin(ang[:, 1])], 1)
    init = feats[[1, 4, 2, 7]] * 0.5 + feats[[3, 6, 0, 5]] * 0.5
    return feats, init


def lloyd_margins(feats, init, n_iter):
    """Replay of the Lloyd iterations in float64: the smallest nearest / second-nearest gap over the assignments made."""
    c, margin = init.copy(), np.inf
    for _ in range(n_iter + 1):
        d = ((feats[:, None, :] - c[None]) ** 2).sum(-1)
        srt = np.sort(d, axis=1)
        margin = min(margin, float((srt[:, 1] - srt[:, 0]).min()))
        lab = d.argmin(1)
        c = np.stack([feats[lab == j].mean(0) for j in range(c.shape[0])])
    return margin


def import_eval_adv_gen():
    R = mg.import_reference()
    mg._install_exact_shapely()
    if 'configargparse' not in sys.modules:
        sys.modules['configargparse'] = types.ModuleType('configargparse')
    import importlib
    R.eval_adv_gen = importlib.import_module('eval_adv_gen')
    R.cluster_scenarios = importlib.import_module('cluster_scenarios')
    return R


def all_ious(R, traj_a, lw_a, traj_b, lw_b):
    """The reference's IoU expression (src/losses/adv_gen_nusc.py:543-559) of box a against box b at every step; a (T,4), b (T,4)."""
    from shapely.geometry import Polygon
    out = np.full((traj_a.shape[0],), np.nan)
    for t in range(traj_a.shape[0]):
        if np.isnan(traj_a[t]).any() or np.isnan(traj_b[t]).any():
            continue
        pa, pb = Polygon(R.nutils.get_corners(traj_a[t], lw_a)), Polygon(R.nutils.get_corners(traj_b[t], lw_b))
        out[t] = pa.intersection(pb).area / pa.union(pb).area
    return out


def run_reference(R):
    E, C = R.eval_adv_gen, R.cluster_scenarios
    raster, dx = synth.make_raster(mg.RASTER_HW, mg.RASTER_HW, M=1)
    env = mg.ref_map_env(R, raster, dx)
    scenarios = {cat: E.read_adv_scenes(os.path.join(SCEN_DIR, cat)) for cat in CATEGORIES}
    feats, init = km_inputs()
    from sklearn.cluster import KMeans
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1):                      # (its threaded inertia sum differs in the last bit from run to run)
        km = KMeans(n_clusters=KM_K, init=init, n_init=1, algorithm='lloyd').fit(feats)
    rec = {'scenes': {}, 'feats': {}}
    orig = dict(cm=E.compute_metrics, single=R.adv_losses.check_single_veh_coll, pair=R.adv_losses.check_pairwise_veh_coll,
                layer=R.nutils.check_on_layer, feat=E.compute_coll_feat, esingle=E.check_single_veh_coll, csingle=C.check_single_veh_coll,
                plot=E.plot_scenario_distrib)

    def single(traj_tgt, lw_tgt, traj_others, lw_others):
        coll, times = orig['single'](traj_tgt, lw_tgt, traj_others, lw_others)
        tg, lt, ot, lo = traj_tgt.numpy(), lw_tgt.numpy(), traj_others.numpy(), lw_others.numpy()
        rec['single'] = dict(coll=np.asarray(coll).copy(), times=np.asarray(times).copy(),
                             iou=np.stack([all_ious(R, tg, lt, ot[a], lo[a]) for a in range(ot.shape[0])]))
        return coll, times

    def pair(traj, lw):
        res = orig['pair'](traj, lw)
        tr, l = traj.numpy(), lw.numpy()
        ious = [all_ious(R, tr[i], l[i], tr[j], l[j]) for i in range(tr.shape[0]) for j in range(i + 1, tr.shape[0])]
        rec['pair'] = dict(num_coll=int(res['num_coll_veh']), num_traj=int(res['num_traj_veh']), marks=np.asarray(res['did_collide']).copy(),
                           iou=np.stack(ious) if ious else np.zeros((0, tr.shape[1])))
        return res

    def layer(drivables, dxs, cars, lw, mapixes):
        frac = orig['layer'](drivables, dxs, cars, lw, mapixes)
        mdx, mlw = torch.mean(dxs), torch.mean(lw, dim=0)
        rec['layer'] = dict(frac=frac.numpy().copy(), ratio=np.asarray([float(mlw[0] / mdx), float(mlw[1] / mdx)]),
                            L=torch.round(mlw[0] / mdx).int().item(), W=torch.round(mlw[1] / mdx).int().item())
        return frac

    def cm(scene, map_env, map_idx, metrics, cnt, tot):
        before = {k: len(v) for k, v in metrics.items()}
        t0 = time.perf_counter()
        res = orig['cm'](scene, map_env, map_idx, metrics, cnt, tot)
        seconds = time.perf_counter() - t0
        cur = dict(seq=dict(res[3]), seconds=seconds, single=rec.pop('single'), pair=rec.pop('pair', None), layer=rec.pop('layer', None),
                   counts={k: len(v) - before.get(k, 0) for k, v in res[0].items() if len(v) - before.get(k, 0) > 0})
        rec['scenes'][scene['name']] = cur
        return res

    def feat(lw, scene_traj, dt):
        f = orig['feat'](lw, scene_traj, dt)
        s = rec.pop('single')
        f2 = C.compute_coll_feat(lw, scene_traj, dt)
        rec.pop('single')
        assert f2['hvec'] == f['hvec'] and f2['angvec'] == f['angvec']
        hit = s['times'][s['coll']]
        fine_t = int(np.amin(hit))
        fine_agt = int(np.nonzero(s['coll'])[0][np.argmin(hit)])
        rec['feats'][len(rec['feats'])] = dict(hvec=f['hvec'], angvec=f['angvec'], rel_s=f['rel_s'], h=f2['h'], ang=f2['ang'], iou=s['iou'],
                                               fine_t=fine_t, fine_agt=fine_agt, lr=int((fine_t * (dt / float(FEAT_SCALE))) / dt))
        return f

    E.compute_metrics, E.compute_coll_feat, E.plot_scenario_distrib = cm, feat, (lambda *a, **k: None)
    R.adv_losses.check_single_veh_coll = E.check_single_veh_coll = C.check_single_veh_coll = single
    R.adv_losses.check_pairwise_veh_coll, R.nutils.check_on_layer = pair, layer
    csvs = {}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, 'cluster.pkl'), 'wb') as f:
                pickle.dump(km, f)
            with open(os.path.join(tmp, 'labels.txt'), 'w') as f:
                f.write(', '.join(CLUSTER_NAMES) + '\n')
            out = os.path.join(tmp, 'out')
            os.makedirs(out)
            with contextlib.redirect_stdout(io.StringIO()):
                E.quant_eval(scenarios, os.path.join(tmp, 'cluster.pkl'), os.path.join(tmp, 'labels.txt'), env, out)
            for fn in sorted(os.listdir(out)):
                if fn.endswith('.csv'):
                    csvs[fn] = open(os.path.join(out, fn)).read()
        # the dictionaries: run the accumulation once more the way quant_eval does (it keeps them local)
        metrics, cnt, tot = {}, {}, {}
        saved = dict(rec['scenes'])
        with contextlib.redirect_stdout(io.StringIO()):
            for cat in CATEGORIES:
                for scene in scenarios[cat]:
                    metrics, cnt, tot, _ = cm(scene, env, 0, metrics, cnt, tot)
                    if cat != 'adv_failed':
                        cnt, tot = R.scenario_gen.log_freq_stat(cnt, tot, 'sol_success', int(cat == 'adv_sol_success'), 1)
        for k, v in saved.items():                        # keep the first run's records (same values, first timing)
            rec['scenes'][k] = v
    finally:
        E.compute_metrics, E.compute_coll_feat, E.plot_scenario_distrib = orig['cm'], orig['feat'], orig['plot']
        R.adv_losses.check_single_veh_coll, E.check_single_veh_coll, C.check_single_veh_coll = orig['single'], orig['esingle'], orig['csingle']
        R.adv_losses.check_pairwise_veh_coll, R.nutils.check_on_layer = orig['pair'], orig['layer']
    rates = E.compute_success_rates(scenarios)
    return scenarios, rec, (metrics, cnt, tot), csvs, km, feats, init, rates


def g18_adv_eval(R):
    scenarios, rec, (metrics, cnt, tot), csvs, km, feats, init, rates = run_reference(R)
    out = {}
    names = [s['name'] for cat in CATEGORIES for s in scenarios[cat]]
    out['names'] = np.asarray(names)
    out['categories'] = np.asarray([cat for cat in CATEGORIES for _ in scenarios[cat]])
    crash = [s for cat in CATEGORIES[:2] for s in scenarios[cat]]
    assert len(crash) == len(rec['feats'])
    info = {}
    for cat in CATEGORIES:
        for scene in scenarios[cat]:
            name, r = scene['name'], rec['scenes'][scene['name']]
            p = name + '/'
            fut = scene['fut_adv'].numpy()
            n, T = fut.shape[0], fut.shape[1]
            seq = dict(scene['eval_metrics'])
            out[p + 'seq_keys'] = np.asarray(list(seq.keys()))
            out[p + 'seq_vals'] = np.asarray([float(v) for v in seq.values()], dtype=np.float64)
            times, did = r['single']['times'], bool(r['single']['coll'].any())
            CT, coll_agt = int(np.amin(times)), int(np.argmin(times)) + 1
            atk = coll_agt if did else int(scene['attack_agt'])
            n_others = n - 1 - (1 if atk != 0 else 0)
            for k, v in (('coll_t', CT), ('coll_agt', coll_agt), ('atk_agt', atk), ('did_collide', int(did)), ('n_others', n_others)):
                out[p + k] = np.asarray(v, dtype=np.int64)
            out[p + 'iou_coarse'] = r['single']['iou']
            margins = [np.nanmin(np.abs(r['single']['iou'] - IOU_THRESH))]
            pr = r['pair']
            out[p + 'num_coll_veh'] = np.asarray(pr['num_coll'] if pr else -1, dtype=np.int64)
            out[p + 'num_traj_veh'] = np.asarray(pr['num_traj'] if pr else -1, dtype=np.int64)
            out[p + 'pair_marks'] = np.asarray(pr['marks'] if pr else np.zeros((0,)), dtype=np.int64)
            out[p + 'iou_pairs'] = pr['iou'] if pr else np.zeros((0, 0))
            if pr and pr['iou'].size:
                assert not np.isnan(pr['iou']).any(), 'a NaN pose inside the pairwise window: the reference cannot evaluate that'
                margins.append(np.abs(pr['iou'] - IOU_THRESH).min())
            ly = r['layer']
            env_coll = np.full((n,), -1, dtype=np.int64)
            frac = np.zeros((n, 0))
            if ly:
                valid = ~np.isnan(fut[:, :CT].sum(-1))
                frac = np.full((n, CT), np.nan)
                frac[valid] = ly['frac']
                with np.errstate(invalid='ignore'):
                    env_coll = (np.nan_to_num(frac, nan=1.0).astype(np.float32) < np.float32(1.0 - 0.05)).any(1).astype(np.int64)
                assert np.abs(ly['frac'] - 0.95).min() > 2.0 / (ly['L'] * ly['W']), 'tie condition: drivable fraction near 0.95 in ' + name
                half = np.abs(ly['ratio'] - np.floor(ly['ratio']) - 0.5)
                assert half.min() > 1e-3, 'tie condition: grid ratio near a half-integer in ' + name
                others = [a for a in range(1, n) if a != atk]
                assert int(env_coll[atk]) == seq['env_coll_atk']
                if others:
                    assert abs(float(env_coll[others].sum()) / len(others) - seq['env_coll_others']) < 1e-12
            out[p + 'env_coll'] = env_coll
            out[p + 'env_frac'] = frac
            out[p + 'env_L'] = np.asarray(ly['L'] if ly else -1, dtype=np.int64)
            out[p + 'env_W'] = np.asarray(ly['W'] if ly else -1, dtype=np.int64)
            out[p + 'env_ratio'] = ly['ratio'] if ly else np.full((2,), np.nan)
            for k, v in r['counts'].items():
                out[p + 'counts/' + k] = np.asarray(v, dtype=np.int64)
            if scene in crash:
                f = rec['feats'][[id(c) for c in crash].index(id(scene))]
                out[p + 'feat_hvec'], out[p + 'feat_angvec'] = np.asarray(f['hvec'], dtype=np.float64), np.asarray(f['angvec'], dtype=np.float64)
                for k in ('rel_s', 'h', 'ang'):
                    out[p + 'feat_' + k] = np.asarray(f[k], dtype=np.float64)
                for k, src in (('fine_t', 'fine_t'), ('fine_agt', 'fine_agt'), ('lr_coll_t', 'lr')):
                    out[p + k] = np.asarray(f[src], dtype=np.int64)
                out[p + 'iou_fine'] = f['iou']
                margins.append(np.nanmin(np.abs(f['iou'] - IOU_THRESH)))
                out['labels/' + name] = np.asarray(int(scene['label_idx']), dtype=np.int64)
                # the label must not hang on a near-tie between two centres
                x = np.asarray(f['angvec'] + f['hvec'])
                d = np.sort(((km.cluster_centers_ - x[None]) ** 2).sum(1))
                assert d[1] - d[0] > 1e-9, 'tie condition: ' + name + ' is equally close to two centres'
            margin = min(margins)
            assert margin > TIE_MARGIN, 'tie condition: %s has an IoU within %g of the threshold' % (name, margin)
            info[name] = dict(CT=CT, coll_agt=coll_agt, atk=atk, did=did, n=n, T=T, seq=seq, pair=pr, env=env_coll, r=r,
                              feat=rec['feats'][[id(c) for c in crash].index(id(scene))] if scene in crash else None, scene=scene)
            print('%-16s did %d CT %2d agt %2d atk %2d veh %s env %s L %s W %s margin %.4f %.2gs' % (
                name, did, CT, coll_agt, atk, (pr or {}).get('num_coll'), env_coll.tolist(), ly and ly['L'], ly and ly['W'], margin, r['seconds']))
    check_cases(info)
    out['metric_keys'] = np.asarray(list(metrics.keys()))
    out['metric_mean'] = np.asarray([np.mean(v) for v in metrics.values()], dtype=np.float64)
    out['metric_count'] = np.asarray([len(v) for v in metrics.values()], dtype=np.int64)
    out['freq_keys'] = np.asarray(list(cnt.keys()))
    out['freq_cnt'] = np.asarray([cnt[k] for k in cnt], dtype=np.int64)
    out['freq_total'] = np.asarray([tot[k] for k in cnt], dtype=np.int64)
    out['success_rates'] = np.asarray([rates[0], rates[1], rates[0] * rates[1]], dtype=np.float64)
    out['csv_names'] = np.asarray(sorted(csvs))
    for fn, text in csvs.items():
        out['csv/' + fn] = np.asarray(text)
    out['cluster_label_names'] = np.asarray(CLUSTER_NAMES)
    out['km/feats'], out['km/init'] = feats, init
    out['km/centers'], out['km/labels'] = km.cluster_centers_.astype(np.float64), km.labels_.astype(np.int64)
    out['km/inertia'], out['km/n_iter'] = np.asarray(km.inertia_, dtype=np.float64), np.asarray(km.n_iter_, dtype=np.int64)
    margin = lloyd_margins(feats, init, int(km.n_iter_))
    assert margin > 1e-9, 'tie condition: a k-means point is equally close to two centres'
    out['km/margin'] = np.asarray(margin, dtype=np.float64)
    print('k-means: n_iter %d inertia %.6f margin %.3g labels %s' % (km.n_iter_, km.inertia_, margin, km.labels_.tolist()))
    save_deterministic('g18_adv_eval.npz', out)


def check_cases(info):
    """The properties the scene set exists for, from the reference's outputs."""
    g = lambda n: info[n]
    first = lambda iou: [int(np.argmax(r > IOU_THRESH)) if (r > IOU_THRESH).any() else -1 for r in np.nan_to_num(iou, nan=0.0)]
    mid = g('sc_0000_mid')
    assert mid['did'] and 3 <= mid['CT'] <= 9 and mid['n'] == 19 and mid['T'] == 12 and mid['coll_agt'] == mid['scene']['attack_agt']
    fp = first(mid['pair']['iou'])                                        # pairs in (i, j > i) order over [0, CT)
    idx = lambda i, j, m=18: i * (2 * m - i - 1) // 2 + (j - i - 1)       # others' rows i < j
    assert fp[idx(6, 7)] >= 0 and mid['pair']['marks'][6] and mid['pair']['num_coll'] == 1, 'agents 7, 8 overlap before CT'
    late = all_pair_late(mid)
    assert late, 'agents 9, 10 overlap only at or after CT'
    assert mid['env'][12] == 1 and mid['env'][mid['atk']] == 0 and 0 < mid['seq']['env_coll_others'] < 1
    assert np.isnan(mid['scene']['fut_adv'][14, -1]).all() and not np.isnan(mid['scene']['fut_adv'][14, :mid['CT']]).any()
    assert 'fut_internal_ego' in mid['scene'] and np.isfinite(mid['seq']['match_plan_ang']) and mid['feat']['lr'] > 0
    s0 = g('sc_0001_step0')
    assert s0['did'] and s0['CT'] == 0 and s0['n'] == 2 and all(np.isnan(s0['seq'][k]) for k in ('veh_coll_rate', 'env_coll_atk', 'env_coll_others'))
    assert np.isnan(s0['seq']['adv_z_ll_other']) and np.isfinite(s0['seq']['adv_z_ll_atk']) and s0['feat']['lr'] == 0
    ea = g('sc_0002_early')
    assert ea['did'] and ea['CT'] in (1, 2) and np.isnan(ea['seq']['adv_atk_accel']) and ea['T'] == 8 and ea['n'] == 4
    assert ea['coll_agt'] != ea['scene']['attack_agt'] and ea['seq']['env_coll_atk'] == 1 and ea['seq']['env_coll_others'] == 0
    tie = g('sc_0003_tie')
    fc = first(tie['r']['single']['iou'])
    assert fc[1] == fc[2] == tie['CT'] and tie['coll_agt'] == 2 and tie['scene']['attack_agt'] == 3 and fc[0] != tie['CT']
    assert tie['seq']['env_coll_atk'] == 0 and tie['seq']['env_coll_others'] == 0 and 'fut_internal_ego' not in tie['scene']
    assert np.isnan(tie['seq']['match_plan_pos']) and np.isfinite(tie['seq']['adv_atk_accel'])
    off = g('sc_0004_offroad')
    assert off['did'] and off['CT'] > 2 and off['env'][2] == 1 and off['seq']['env_coll_atk'] == 0 and off['seq']['env_coll_others'] == 0.5
    none = g('sc_0005_none')
    assert not none['did'] and none['CT'] == 12 and none['atk'] == 2 and none['seq']['adv_collide'] == 0 and none['n'] == 4
    alone = g('sc_0006_alone')
    assert not alone['did'] and alone['CT'] == 8 and np.isnan(alone['seq']['env_coll_others']) and np.isnan(alone['seq']['adv_other_accel'])
    assert sorted(set(v['n'] - 1 for v in info.values())) == [1, 3, 4, 18] and sorted(set(v['T'] for v in info.values())) == [8, 12]


def all_pair_late(mid):
    """Agents 9 and 10 (others' rows 8, 9) never overlap inside [0, CT) but do at a later step (from the reference's IoU expression
    on the full horizon)."""
    fut, lw = mid['scene']['fut_adv'].numpy(), mid['scene']['veh_att'].numpy()
    from shapely.geometry import Polygon
    import datasets.nuscenes_utils as nutils
    hits = []
    for t in range(fut.shape[1]):
        pa, pb = Polygon(nutils.get_corners(fut[9, t], lw[9])), Polygon(nutils.get_corners(fut[10, t], lw[10]))
        hits.append(pa.intersection(pb).area / pa.union(pb).area > IOU_THRESH)
    return not any(hits[:mid['CT']]) and any(hits[mid['CT']:])


if __name__ == '__main__':
    torch.set_num_threads(8)
    write_scenarios()
    g18_adv_eval(import_eval_adv_gen())
