#!/usr/bin/env python3
"""Generate tests/golden/g20_dataset.npz and tests/golden/g20_scenarios/: the reference's own ``NuScenesDataset`` methods
(src/datasets/nuscenes_dataset.py ``post_process``, ``compile_scenarios``, ``__getitem__``) and its ``check_on_layer``, run in the
build container on the records of a hand-built tracks set.  The devkit, pyquaternion and torch_geometric imports are make_golden's
stand-ins (``np.int`` / ``np.float`` aliased); collation is ``Batch.from_data_list``.  The file is described in
tests/golden/README_g20.md.  The tracks (the INPUT) are stored in the fixture; the raster is rebuilt by ``fixture_env`` below,
which imports without the reference (the tests, GPU tests included, call it).

Usage:  python tests/golden/make_golden_dataset.py
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from strive_amd import synth                                                                  # noqa: E402
from strive_amd.graph import Batch                                                            # noqa: E402
from strive_amd.datasets import tracks as tracks_io                                           # noqa: E402

FIX = 'g20_dataset.npz'
SCEN_DIR = 'g20_scenarios'
NPAST, NFUT = 4, 12
CATEGORIES = ['car', 'truck']
CONFIGS = {'c0': dict(carpark=True, require_full_past=False, seq_interval=1),
           'c1': dict(carpark=False, require_full_past=True, seq_interval=3)}
FIELDS = ('past', 'past_gt', 'future', 'future_gt', 'lw', 'sem', 'past_vis', 'future_vis')
T_A, T_B, T_C = 24, 17, 19
OFF_XY = (29.0, 29.0)                         # centre of an off-road block of map 0 (roads: x or y in [40 k, 40 k + 18))
EDGE_L, EDGE_W, EDGE_H, EDGE_X = 4.5, 2.0, 0.3, 142.0     # the box that straddles the road edge y = 18 for the 0.3 threshold


# ------------------------------------------------------------------------------------------------
# inputs that need no reference
# ------------------------------------------------------------------------------------------------

def fixture_env(carpark):
    """``synth.make_raster(M=2)`` (map 0: 0.25 m pixels, a power of two; map 1: slightly off, so the float64 division matters) with
    layer 1 replaced by the car park; ``layer_map`` names it only when ``carpark``."""
    raster, dx = synth.make_raster(1024, 1024, M=2)
    raster, layer_map = synth.add_carpark_layer(raster, dx, layer=1)
    env = synth.SyntheticMapEnv(raster, dx)
    env.layer_map = dict(layer_map) if carpark else {k: v for k, v in layer_map.items() if k != 'carpark_area'}
    return env


def wrap(h):
    return (h + math.pi) % (2.0 * math.pi) - math.pi


def _agent(l, w, cat, frames, x, y, h):
    return {'l': l, 'w': w, 'k': cat, 'frames': list(frames), 'x': x, 'y': y, 'h': h}


def build_records(y_above, y_below):
    """{scene: (map name, T, [agents])}; an agent's x, y, h cover every frame of the scene, ``frames`` are the observed ones."""
    scenes = {}
    # ---- scene A, map 0: one agent per case ----
    T = T_A
    f = np.arange(T)
    on = lambda y0: np.full((T,), y0)                                                               # noqa: E731
    ego = _agent(4.084, 1.73, 'ego', f, 30.0 + 2.0 * f, on(9.0), 0.01 * np.sin(0.5 * f))
    ags = [ego]
    ags.append(_agent(4.5, 2.0, 'car', f, 140.0 - 1.5 * f, on(5.0), wrap(3.10 + 0.02 * f)))          # 1 frame 0 on, heading across +-pi
    ags.append(_agent(4.25, 1.875, 'truck', f[5:], 40.0 + 1.0 * f, on(12.0), 0.0 * f))               # 2 first seen mid-scene
    ags.append(_agent(4.75, 2.0, 'car', list(f[:4]) + [T - 1], 50.0 + 0.5 * f, on(14.0), 0.0 * f))   # 3 only lead: the last frame
    ags.append(_agent(4.0, 1.75, 'car', [7], 90.0 + 0.0 * f, on(4.0), 0.5 + 0.0 * f))                # 4 a single frame
    x5, y5 = 100.0 + 1.0 * f, on(10.0)
    x5[8], y5[8] = OFF_XY
    ags.append(_agent(4.5, 1.75, 'car', f, x5, y5, 0.02 * f))                                        # 5 off the road at frame 8
    ags.append(_agent(4.5, 2.0, 'truck', f, OFF_XY[0] + 0.1 * f, on(OFF_XY[1]), 0.0 * f))            # 6 never on the road
    x7 = np.where(f < 10, 66.0 + 0.05 * f, 80.0 + 1.0 * (f - 10))
    ags.append(_agent(4.0, 1.75, 'car', f, x7, on(5.0), 0.0 * f))                                    # 7 on the car park until frame 9
    y8, y9 = on(13.0), on(13.0)
    y8[6], y9[6] = y_above, y_below
    ags.append(_agent(EDGE_L, EDGE_W, 'car', f, on(EDGE_X), y8, on(EDGE_H)))                         # 8 frame 6 just above 0.3
    ags.append(_agent(EDGE_L, EDGE_W, 'car', f, on(EDGE_X + 7.0), y9, on(EDGE_H)))                  # 9 frame 6 just below 0.3
    scenes['scene-A'] = ('synthetic-0', T, ags)
    # ---- scene B, map 1: in its only window nobody but the ego qualifies ----
    T = T_B
    f = np.arange(T)
    ags = [_agent(4.084, 1.73, 'ego', f, 20.0 + 1.5 * f, np.full((T,), 5.0), 0.0 * f),
           _agent(4.5, 2.0, 'car', f[8:], 60.0 + 1.0 * f, np.full((T,), 4.0), 0.0 * f),
           _agent(5.5, 2.25, 'truck', f[5:], 90.0 - 1.0 * f, np.full((T,), 6.0), wrap(math.pi + 0.0 * f))]
    scenes['scene-B'] = ('synthetic-1', T, ags)
    # ---- scene C, map 0: 70 agents (more than a wavefront): scene A's visibility patterns repeated with offsets ----
    T = T_C
    f = np.arange(T)
    ags = [_agent(4.084, 1.73, 'ego', f, 20.0 + 2.0 * f, np.full((T,), 9.0), 0.0 * f)]
    for j in range(69):
        pat = j % 6
        x = 12.0 + 3.25 * j + (0.5 + 0.125 * (j % 4)) * f
        y = np.full((T,), 2.0 + 2.0 * (j % 8))
        h = 0.01 * (j % 5) * np.sin(0.3 * f)
        fr = f
        if pat == 1:
            fr = f[1 + j % 3:]
        elif pat == 2:
            fr = np.concatenate([f[:5], f[7:]])
        elif pat == 3:
            x[4], y[4] = OFF_XY[0] + 40.0 * (j % 3), OFF_XY[1]
        elif pat == 4:
            fr = f[:9 + j % 7]
        elif pat == 5 and j % 48 == 5:
            fr = [j % T]
        ags.append(_agent(4.0 + 0.125 * (j % 7), 1.75 + 0.0625 * (j % 4), CATEGORIES[j % 2], fr, x, y, wrap(h)))
    scenes['scene-C'] = ('synthetic-0', T, ags)
    return scenes


def records_to_tracks(scenes):
    tr = {'scene_name': [], 'scene_map': [], 'categories': list(CATEGORIES), 'frame_ptr': [0], 'ego_t': [], 'agent_ptr': [0], 'lw': [],
          'cat': [], 'obs_ptr': [0], 'obs_frame': [], 'obs': []}
    for si, (name, (mname, T, ags)) in enumerate(scenes.items()):
        tr['scene_name'].append(name)
        tr['scene_map'].append(mname)
        jit = np.rint(synth.counter_uniform((T,), 'g20/jit/%d' % si, -20000.0, 20000.0)).astype(np.int64)
        tr['ego_t'].extend((1532402927000000 + 30000000 * si + 500000 * np.arange(T, dtype=np.int64) + jit).tolist())
        tr['frame_ptr'].append(len(tr['ego_t']))
        for a in ags:
            tr['lw'].append([a['l'], a['w']])
            tr['cat'].append(0 if a['k'] == 'ego' else CATEGORIES.index(a['k']))
            for t in a['frames']:
                t = int(t)
                tr['obs_frame'].append(t)
                tr['obs'].append([a['x'][t], a['y'][t], a['h'][t], math.cos(a['h'][t]), math.sin(a['h'][t])])
            tr['obs_ptr'].append(len(tr['obs']))
        tr['agent_ptr'].append(len(tr['lw']))
    tr['lw'] = np.asarray(tr['lw'], dtype=np.float64)
    tr['obs'] = np.asarray(tr['obs'], dtype=np.float64)
    return tracks_io.check_tracks(tr)


def records_from_tracks(tr):
    """A tracks dict as the reference's ``scene2data`` records (what its ``compile_data`` hands to ``post_process``) and {scene: map name}."""
    data, s2m = {}, {}
    for s, scene in enumerate(tr['scene_name']):
        s2m[scene] = tr['scene_map'][s]
        ts = tr['ego_t'][tr['frame_ptr'][s]:tr['frame_ptr'][s + 1]]
        data[scene] = {}
        a0, a1 = int(tr['agent_ptr'][s]), int(tr['agent_ptr'][s + 1])
        for a in range(a0, a1):
            name = 'ego' if a == a0 else 'agt%04d' % (a - a0)
            rows = []
            for o in range(int(tr['obs_ptr'][a]), int(tr['obs_ptr'][a + 1])):
                x, y, h, hc, hs = [float(v) for v in tr['obs'][o]]
                rows.append({'x': x, 'y': y, 'h': h, 'hcos': hc, 'hsin': hs, 't': int(ts[tr['obs_frame'][o]]), 'samp_tok': ''})
            data[scene][name] = {'traj': rows, 'l': float(tr['lw'][a, 0]), 'w': float(tr['lw'][a, 1]),
                                 'k': 'ego' if a == a0 else tr['categories'][int(tr['cat'][a])]}
    return data, s2m


def write_scenarios(path):
    """Two scenario files in prepare_output_dict's format: three agents with ``sem`` and a NaN tail, two agents without ``sem``."""
    os.makedirs(path, exist_ok=True)

    def scene(n, T, nan_tail, with_sem, mname):
        f = np.arange(T)
        st = np.zeros((n, T, 6), dtype=np.float32)
        for a in range(n):
            h = (0.2 * a + 0.04 * f * (1 + a)).astype(np.float64) + (3.0 if a == 1 else 0.0)
            st[a, :, 0] = 40.0 + 12.0 * a + (1.0 + 0.5 * a) * f * np.cos(h[0])
            st[a, :, 1] = 6.0 + 2.0 * a + (1.0 + 0.5 * a) * f * np.sin(h[0])
            st[a, :, 2], st[a, :, 3] = np.cos(h), np.sin(h)
            st[a, :, 4], st[a, :, 5] = 2.0 + a, 0.08 * (1 + a)
        fut = st[:, NPAST:, :4].copy()
        if nan_tail:
            fut[n - 1, -3:] = np.nan
        d = {'N': n, 'dt': 0.5, 'map': mname, 'lw': [[4.5 + 0.25 * a, 2.0] for a in range(n)], 'past': st[:, :NPAST].tolist(),
             'fut_init': fut.tolist(), 'fut_adv': fut.tolist(), 'attack_agt': 1, 'attack_t': 3}
        if with_sem:
            d['sem'] = [[1, 0] if a % 2 == 0 else [0, 1] for a in range(n)]
        return d

    for name, d in (('sc_0000_sem', scene(3, 18, True, True, 'synthetic-0')), ('sc_0001_plain', scene(2, 19, False, False, 'synthetic-1'))):
        with open(os.path.join(path, name + '.json'), 'w') as fh:
            json.dump(d, fh)


# ------------------------------------------------------------------------------------------------
# the reference's run
# ------------------------------------------------------------------------------------------------

def ref_dataset(R, mod, env, cfg):
    ds = object.__new__(mod.NuScenesDataset)
    ds.map_env, ds.map_list = env, env.map_list
    ds.dt, ds.noise_std = 0.5, 0.0
    ds.npast, ds.nfuture, ds.seq_len = NPAST, NFUT, NPAST + NFUT
    ds.seq_interval, ds.require_full_past, ds.use_challenge_splits = cfg['seq_interval'], cfg['require_full_past'], False
    ds.categories = list(CATEGORIES)
    iden = torch.eye(len(CATEGORIES), dtype=torch.int)
    ds.cat2vec = {c: iden[i] for i, c in enumerate(CATEGORIES)}
    ds.vec2cat = {tuple(iden[i].tolist()): c for i, c in enumerate(CATEGORIES)}
    ni = R.dutils.NUSC_NORM_STATS[tuple(sorted(CATEGORIES))]
    ds.normalizer = R.dutils.MeanStdNormalizer(
        torch.Tensor([ni['lscale'][0], ni['lscale'][0], ni['h'][0], ni['h'][0], ni['s'][0], ni['hdot'][0]]),
        torch.Tensor([ni['lscale'][1], ni['lscale'][1], ni['h'][1], ni['h'][1], ni['s'][1], ni['hdot'][1]]))
    ds.veh_att_normalizer = R.dutils.MeanStdNormalizer(torch.Tensor([ni['l'][0], ni['w'][0]]), torch.Tensor([ni['l'][1], ni['w'][1]]))
    return ds


def store_windows(out, p, ds, scene_names):
    """Every window through the reference's __getitem__, collated."""
    ds.data_len = len(ds.seq_map)
    items = [ds[i] for i in range(len(ds))]
    for d, _ in items:                                               # without noise the observed states are the ground truth
        assert torch.equal(torch.nan_to_num(d.past), torch.nan_to_num(d.past_gt)) and torch.equal(torch.nan_to_num(d.future), torch.nan_to_num(d.future_gt))
    b = Batch.from_data_list([d for d, _ in items])
    out[p + 'seq_scene'] = np.asarray([scene_names.index(s) for s, _ in ds.seq_map], dtype=np.int32)
    out[p + 'seq_start'] = np.asarray([i for _, i in ds.seq_map], dtype=np.int32)
    out[p + 'map_idx'] = np.asarray([m for _, m in items], dtype=np.int64)
    out[p + 'ptr'] = b.ptr.numpy()
    out[p + 'batch'] = b.batch.numpy()
    out[p + 'edge_index'] = b.edge_index.numpy()
    for k in FIELDS:
        assert b[k].dtype == torch.float32, k
        out[p + k] = b[k].numpy()
    return b


def store_info(out, p, info, order, T_of):
    """scene2info as flat tables in the tracks' agent order; dropped agents are NaN rows with kept = 0."""
    traj, accel, vis, kept = [], [], [], []
    for scene, names in order:
        T = T_of[scene]
        for n in names:
            if n in info[scene]:
                e = info[scene][n]
                traj.append(np.asarray(e['traj'], dtype=np.float64))
                accel.append(np.asarray(e['accel'], dtype=np.float64) if 'accel' in e else np.full((T, 2), np.nan))
                vis.append(np.asarray(e['is_vis']).astype(np.int32))
                kept.append(1)
            else:
                traj.append(np.full((T, 6), np.nan))
                accel.append(np.full((T, 2), np.nan))
                vis.append(np.zeros((T,), dtype=np.int32))
                kept.append(0)
    out[p + 'traj'], out[p + 'accel'] = np.concatenate(traj), np.concatenate(accel)
    out[p + 'is_vis'], out[p + 'kept'] = np.concatenate(vis), np.asarray(kept, dtype=np.int32)


def edge_fraction(R, env, y):
    cars = torch.tensor([[EDGE_X, y, math.cos(EDGE_H), math.sin(EDGE_H)]], dtype=torch.float64)
    lw = torch.tensor([[EDGE_L, EDGE_W]], dtype=torch.float64)
    return float(R.nutils.check_on_layer(env.nusc_raster[:, 0], env.nusc_dx, cars, lw, torch.zeros((1,), dtype=torch.long))[0])


def main():
    import importlib
    import make_golden as mg
    R = mg.import_reference()
    import types
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules['tqdm'] = types.SimpleNamespace(tqdm=lambda x, *a, **k: x)
    mod = importlib.import_module('datasets.nuscenes_dataset')
    mod.tqdm = lambda x, *a, **k: x
    out = {}

    # the two positions of the edge box whose drivable fractions enclose 0.3 most tightly (steps of 1/64 m)
    env = fixture_env(True)
    fr = [(y, edge_fraction(R, env, y)) for y in 17.0 + np.arange(0, 192) / 64.0]
    y_above, f_above = min([(y, v) for y, v in fr if v >= 0.3], key=lambda p: p[1])
    y_below, f_below = max([(y, v) for y, v in fr if v < 0.3], key=lambda p: p[1])
    print('edge box: y %.6f -> %.6f (kept), y %.6f -> %.6f (dropped)' % (y_above, f_above, y_below, f_below))
    assert 0.3 <= f_above < 0.32 and 0.28 < f_below < 0.3
    out['edge_y'], out['edge_frac'] = np.asarray([y_above, y_below]), np.asarray([f_above, f_below])

    scenes = build_records(y_above, y_below)
    tr = records_to_tracks(scenes)
    for k in tracks_io.KEYS:
        out['tracks/' + k] = np.asarray(tr[k], dtype=np.str_) if k in ('scene_name', 'scene_map', 'categories') else tr[k]
    data, s2m = records_from_tracks(tr)
    order = [(s, list(data[s].keys())) for s in data]
    T_of = {s: int(tr['frame_ptr'][i + 1] - tr['frame_ptr'][i]) for i, s in enumerate(tr['scene_name'])}

    for cname, cfg in CONFIGS.items():
        env = fixture_env(cfg['carpark'])
        ds = ref_dataset(R, mod, env, cfg)
        ds.scene2map = {s: (m, env.map_list.index(m)) for s, m in s2m.items()}
        info, seq = ds.post_process(data)
        ds.data, ds.seq_map = info, seq
        store_info(out, cname + '/', info, order, T_of)
        b = store_windows(out, cname + '/', ds, list(tr['scene_name']))
        print('%s: %d windows, %d nodes, kept %d of %d agents' % (cname, len(seq), int(b.ptr[-1]), int(out[cname + '/kept'].sum()), len(out[cname + '/kept'])))
        check_cases(cname, cfg, out, tr, info)

    # the scenario route
    sdir = os.path.join(HERE, SCEN_DIR)
    write_scenarios(sdir)
    env = fixture_env(True)
    ds = ref_dataset(R, mod, env, CONFIGS['c0'])
    info, seq, s2m_s = ds.compile_scenarios(sdir)
    ds.data, ds.seq_map, ds.scene2map = info, seq, s2m_s
    names = list(info.keys())
    store_info(out, 'sc/', info, [(s, list(info[s].keys())) for s in names], {s: info[s]['ego']['traj'].shape[0] for s in names})
    b = store_windows(out, 'sc/', ds, names)
    out['sc/scene_name'] = np.asarray(names, dtype=np.str_)
    out['sc/numpy_version'] = np.asarray(np.__version__, dtype=np.str_)        # whose fp32 arctan2 gave sc/*'s heading rates
    print('sc: %d windows, %d nodes' % (len(seq), int(b.ptr[-1])))

    mg_save = __import__('make_golden_traffic_eval').save_deterministic
    mg_save(FIX, out)


def check_cases(cname, cfg, out, tr, info):
    """The properties the hand-built set exists for, from the reference's outputs."""
    A = info['scene-A']
    agt = lambda j: A.get('agt%04d' % j)                                                             # noqa: E731
    vis = lambda j: np.asarray(agt(j)['is_vis']).astype(int)                                        # noqa: E731
    assert vis(1).all(), 'agent 1 is seen from frame 0'
    h = tr['obs'][tr['obs_ptr'][1]:tr['obs_ptr'][2], 2]
    assert (np.abs(np.diff(h)) > 6.0).any(), 'agent 1 crosses +-pi'
    assert np.abs(agt(1)['traj'][:, 5]).max() < 0.1, 'and its heading rate does not see the jump'
    assert not vis(2)[:5].any() and vis(2)[5:].all() and np.isfinite(agt(2)['traj'][5, 4]), 'agent 2: forward difference at its first frame'
    assert vis(3)[:4].all() and not vis(3)[4:].any(), 'agent 3: the lead on the last frame is ignored'
    assert np.isnan(agt(3)['traj'][-1]).all()
    assert agt(4) is not None and not vis(4).any() and np.isnan(agt(4)['traj'][:, :4]).all(), 'agent 4: kept, never visible'
    assert vis(5)[:8].all() and not vis(5)[8] and vis(5)[9:].all(), 'agent 5: the off-road frame is a gap'
    assert agt(6) is None, 'agent 6 is dropped'
    if cfg['carpark']:
        assert not vis(7)[:10].any() and vis(7)[10:].all(), 'agent 7: car-park frames are dropped'
    else:
        assert vis(7).all()
    assert vis(8).all() and not vis(9)[6] and vis(9)[7], 'agents 8 / 9: either side of 0.3'
    p = cname + '/'
    n = np.diff(out[p + 'ptr'])
    sc = out[p + 'seq_scene']
    assert (n[sc == 1] == 1).all() and (sc == 1).any(), 'scene B: only the ego qualifies'
    print('%s: nodes per window %s, dropped agents %s' % (cname, n.tolist(), np.nonzero(out[p + 'kept'] == 0)[0].tolist()))
    assert n[sc == 2].max() > 64 or cfg['require_full_past'], 'scene C: more selected agents than a wavefront'
    assert len(set(out[p + 'map_idx'].tolist())) == 2, 'two maps'


if __name__ == '__main__':
    main()
