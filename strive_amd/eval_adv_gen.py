"""Quantitative evaluation of generated scenarios (reference src/eval_adv_gen.py --eval_quant): adversarial / solution / total
success rates and, per scenario and pooled, the collision rate among the non-ego vehicles before the crash, the off-road rate
of the attacker and of the others, their accelerations, the log-likelihood of the attack latents under the prior, how well the
internal planner fit matched the planner, and the collision-type label of every crash -- same function names, argument order,
dictionary keys and CSV files.

The reference evaluates one scene at a time with shapely polygon loops per agent pair and step.  Here ``quant_eval`` puts up
to ``batch_scenes`` consecutive scenes with the same number of steps through ONE launch of ``strive_scenario_eval_metrics``
(strive_amd/csrc/eval_metrics.hip; one workgroup per scene, float64 on the fp32 inputs) and labels the crashes with ONE
``strive_kmeans_step`` against fixed centres.  The kernel returns per-scene sums and frame counts; the pooled means are
total / count (utils/scenario_gen.py, ``PooledMetric``).

    python -m strive_amd.eval_adv_gen --scenarios DIR --eval_quant --cluster_path P --cluster_labels TXT --map_world synthetic --out OUT
"""
import csv
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .eval_common import LIN_MAX, i32, lin_table, pack_env, scene_jsons
from .utils.scenario_gen import log_metric_sum, log_freq_stat

OUT_I = ('adv_collide', 'coll_t', 'coll_agt', 'atk_agt', 'num_coll_veh', 'num_traj_veh', 'env_coll_atk', 'env_coll_others', 'n_others',
         'env_L', 'env_W', 'atk_accel_cnt', 'other_accel_cnt', 'll_other_cnt', 'fit_cnt', 'feat_status', 'fine_t', 'fine_agt', 'lr_coll_t',
         'env_frames')
OUT_D = ('atk_accel_sum', 'atk_accel_max', 'atk_accel_fwd_sum', 'atk_accel_fwd_max', 'atk_accel_lat_sum', 'atk_accel_lat_max',
         'other_accel_sum', 'other_accel_max', 'other_accel_fwd_sum', 'other_accel_fwd_max', 'other_accel_lat_sum', 'other_accel_lat_max',
         'll_atk', 'll_other_sum', 'fit_pos_sum', 'fit_ang_rad_sum', 'fit_ang_deg_sum', 'hvec_x', 'hvec_y', 'angvec_x', 'angvec_y', 'h',
         'ang', 'rel_s', 'env_mean_l', 'env_mean_w')
I = {k: i for i, k in enumerate(OUT_I)}
D = {k: i for i, k in enumerate(OUT_D)}
SEQ_KEYS = ('adv_collide', 'veh_coll_rate', 'env_coll_atk', 'env_coll_others', 'adv_atk_accel', 'adv_atk_accel_fwd', 'adv_atk_accel_lat',
            'adv_other_accel', 'adv_other_accel_fwd', 'adv_other_accel_lat', 'adv_z_ll_atk', 'adv_z_ll_other', 'match_plan_pos',
            'match_plan_ang', 'match_plan_ang_rad')                 # + sol_success, set by quant_eval: the reference's 16 keys
MAX_OTHERS = 63
RES_NAMES = ['adv_sol_success', 'sol_failed', 'adv_failed']
STATUS_TEXT = {1: 'only the ego is in the scene', 2: 'agent offsets, attack_agt or the map index are out of range',
               3: 'more than %d non-ego agents' % MAX_OTHERS, 4: 'the drivable-area sampling grid exceeds %d samples per axis' % LIN_MAX}


def read_adv_scenes(scene_path):
    """Every ``*.json`` scenario of a directory, sorted by name, with the reference's keys (src/eval_adv_gen.py:74-114): ``name,
    map, dt, sem, veh_att, past, fut_adv, fut_init`` and, when the file has them, ``fut_sol, fut_internal_ego, attack_t,
    attack_agt, z_adv, z_sol, z_prior_mean, z_prior_var``."""
    scenes = []
    for name, jd in scene_jsons(scene_path):
        if jd is None:
            print('Failed to load! Skipping')
            continue
        sc = {'name': name, 'map': jd['map'], 'dt': jd['dt']}
        for key, src in (('sem', 'sem'), ('veh_att', 'lw'), ('past', 'past'), ('fut_adv', 'fut_adv'), ('fut_init', 'fut_init')):
            sc[key] = torch.tensor(jd[src])
        for key in ('fut_sol', 'fut_internal_ego'):
            if key in jd:
                sc[key] = torch.tensor(jd[key])
        for key in ('attack_t', 'attack_agt'):
            if key in jd:
                sc[key] = jd[key]
        for key in ('z_adv', 'z_sol'):
            if key in jd:
                sc[key] = torch.tensor(jd[key])
        if 'z_prior' in jd:
            sc['z_prior_mean'] = torch.tensor(jd['z_prior']['mean'])
            sc['z_prior_var'] = torch.tensor(jd['z_prior']['var'])
        scenes.append(sc)
    return scenes


def scenario_eval_metrics(fut, ptr, lw, atk_agt, dt, z=None, mu=None, var=None, plan_fit=None, has_fit=None, map_env=None, mapix=None,
                          want_feat=None, lib=None):
    """The raw kernel: fut (NA,T,4) every scene's ``fut_adv`` with the ego first (NaN = unobserved), ptr (B+1) offsets, lw (NA,2),
    atk_agt (B), dt (B) or a number, z / mu / var (NA,D) or None together, plan_fit (B,T,4) + has_fit (B) or None, map_env + mapix
    (B) or None (no environment terms), want_feat (B) or None -> (out_i (B,20) int32 [OUT_I], out_d (B,26) float64 [OUT_D], status
    (B) int32) on ``fut``'s device.  Rows of scenes with a non-zero status (STATUS_TEXT) are not written: -1 / NaN."""
    lib = ops._lib_for(fut) if lib is None else lib
    dev = fut.device
    fut = fut.detach().to(torch.float32).contiguous()
    NA, T = int(fut.shape[0]), int(fut.shape[1])
    ptr = i32(ptr, dev)
    B = int(ptr.numel()) - 1
    if fut.dim() != 3 or fut.shape[2] != 4 or B < 0:
        raise ValueError('scenario_eval_metrics expects fut (NA,T,4) and ptr (B+1)')
    per_scene = lambda v, fill: torch.full((B,), fill, dtype=torch.int32, device=dev) if v is None else i32(v, dev, B)
    lw = lw.detach().to(device=dev, dtype=torch.float32).reshape(NA, 2).contiguous()
    atk_agt, want_feat = per_scene(atk_agt, 1), per_scene(want_feat, 0)
    dt = torch.as_tensor(dt, dtype=torch.float64).to(dev).expand(B).contiguous() if not torch.is_tensor(dt) or dt.dim() == 0 \
        else dt.to(device=dev, dtype=torch.float64).reshape(B).contiguous()
    if (z is None) != (mu is None) or (z is None) != (var is None):
        raise ValueError('z, mu and var are given together or not at all')
    Dz = 0
    if z is not None:
        Dz = int(z.shape[-1])
        z, mu, var = [v.detach().to(device=dev, dtype=torch.float32).reshape(NA, Dz).contiguous() for v in (z, mu, var)]
    if plan_fit is None:
        plan_fit, has_fit = torch.zeros((max(B, 1), T, 4), dtype=torch.float32, device=dev), None
    plan_fit = plan_fit.detach().to(device=dev, dtype=torch.float32).reshape(-1, T, 4).contiguous()
    has_fit = per_scene(has_fit, 0)
    out_i = torch.full((B, len(OUT_I)), -1, dtype=torch.int32, device=dev)
    out_d = torch.full((B, len(OUT_D)), float('nan'), dtype=torch.float64, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    if NA == 0:                                        # never hand a NULL pointer to the library
        fut = torch.zeros((1, T, 4), dtype=torch.float32, device=dev)
        lw = torch.ones((1, 2), dtype=torch.float32, device=dev)
        if z is not None:
            z, mu, var = [torch.ones((1, Dz), dtype=torch.float32, device=dev) for _ in range(3)]
    if B == 0:
        return out_i, out_d, status
    map_ref, lin, mapix_t = None, None, None
    if map_env is not None:
        map_ref = ops._map_pack(pack_env(map_env), dev).ref()
        lin = lin_table(dev)
        mapix_t = per_scene(mapix, 0)
    lib.call('strive_scenario_eval_metrics', L.ptr(fut), L.ptr(ptr), L.ptr(lw), L.ptr(atk_agt), L.ptr(dt), L.ptr(z), L.ptr(mu), L.ptr(var),
             Dz, L.ptr(plan_fit), L.ptr(has_fit), map_ref, L.ptr(mapix_t), L.ptr(lin), LIN_MAX, L.ptr(want_feat), B, NA, T,
             L.ptr(out_i), L.ptr(out_d), L.ptr(status), L.stream_ptr(fut))
    return out_i, out_d, status


def kmeans_step(feats, centers, lib=None):
    """One Lloyd step (``strive_kmeans_step``): feats (N,F) and centers (k,F) float64 on one device -> (labels (N) int32, mind (N),
    sums (k,F), counts (k) int32, inertia (1))."""
    lib = ops._lib_for(feats, centers) if lib is None else lib
    feats = feats.detach().to(torch.float64).contiguous()
    dev = feats.device
    centers = centers.detach().to(device=dev, dtype=torch.float64).contiguous()
    N, F, k = int(feats.shape[0]), int(feats.shape[1]), int(centers.shape[0])
    if feats.dim() != 2 or centers.dim() != 2 or int(centers.shape[1]) != F or N < 1:
        raise ValueError('kmeans_step expects feats (N,F) with N >= 1 and centers (k,F)')
    labels = torch.empty((N,), dtype=torch.int32, device=dev)
    mind = torch.empty((N,), dtype=torch.float64, device=dev)
    sums = torch.empty((k, F), dtype=torch.float64, device=dev)
    counts = torch.empty((k,), dtype=torch.int32, device=dev)
    inertia = torch.empty((1,), dtype=torch.float64, device=dev)
    lib.call('strive_kmeans_step', L.ptr(feats), L.ptr(centers), N, F, k, L.ptr(labels), L.ptr(mind), L.ptr(sums), L.ptr(counts),
             L.ptr(inertia), L.stream_ptr(feats))
    return labels, mind, sums, counts, inertia


# ------------------------------------------------------------------------------------------------
# batching
# ------------------------------------------------------------------------------------------------

def _stack(scenes, device, with_latents=True):
    """The kernel's inputs for scenes with one number of steps."""
    T = int(scenes[0]['fut_adv'].shape[1])
    counts = [int(s['fut_adv'].shape[0]) for s in scenes]
    fut = torch.cat([s['fut_adv'][:, :, :4].to(torch.float32) for s in scenes]).to(device)
    lw = torch.cat([s['veh_att'].to(torch.float32) for s in scenes]).to(device)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    atk = [int(s.get('attack_agt', 1)) for s in scenes]
    dt = torch.tensor([float(s['dt']) for s in scenes], dtype=torch.float64)
    z = mu = var = None
    if with_latents:
        z = torch.cat([s['z_adv'] for s in scenes]).to(device)
        mu = torch.cat([s['z_prior_mean'] for s in scenes]).to(device)
        var = torch.cat([s['z_prior_var'] for s in scenes]).to(device)
    has_fit = [int('fut_internal_ego' in s) for s in scenes]
    fit = torch.stack([s['fut_internal_ego'][:, :4].to(torch.float32) if 'fut_internal_ego' in s else torch.zeros((T, 4)) for s in scenes])
    return dict(fut=fut, ptr=ptr, lw=lw, atk_agt=atk, dt=dt, z=z, mu=mu, var=var, plan_fit=fit.to(device), has_fit=has_fit)


def group_by_steps(scenes, batch_scenes):
    """Consecutive groups of at most ``batch_scenes`` scene indices with one number of future steps (and one latent size)."""
    if batch_scenes < 1:
        raise ValueError('batch_scenes must be at least 1')
    shape = lambda s: (int(s['fut_adv'].shape[1]), int(s['z_adv'].shape[-1]) if 'z_adv' in s else 0)
    groups, cur = [], []
    for i, s in enumerate(scenes):
        if cur and (len(cur) >= batch_scenes or shape(s) != shape(scenes[cur[0]])):
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    return groups


def _check_status(status, scenes):
    for st, s in zip(status.tolist(), scenes):
        if st != 0:
            raise ValueError('scenario %s cannot be evaluated: %s' % (s.get('name', '?'), STATUS_TEXT.get(st, 'status %d' % st)))


def _feat_dict(name, oi, od, with_rel_s):
    if int(oi[I['feat_status']]) != 0:
        raise ValueError('scenario %s: the ego touches no other agent at any x5 up-sampled step, so it has no collision features '
                         '(the reference fails here too: np.amin of an empty array)' % name)
    feat = {'hvec': [float(od[D['hvec_x']]), float(od[D['hvec_y']])], 'angvec': [float(od[D['angvec_x']]), float(od[D['angvec_y']])]}
    if with_rel_s:
        feat['rel_s'] = float(od[D['rel_s']])
    else:
        feat['h'], feat['ang'] = float(od[D['h']]), float(od[D['ang']])
    return feat


def compute_coll_feat(lw, scene_traj, dt):
    """Collision features of ONE scene (reference src/eval_adv_gen.py:116-168; the kernel with B = 1): lw (NA,2), scene_traj
    (NA,T,4) with the ego first -> ``{'hvec', 'angvec', 'rel_s'}``."""
    NA = int(scene_traj.shape[0])
    oi, od, st = scenario_eval_metrics(scene_traj[:, :, :4], [0, NA], lw, [min(1, NA - 1)], float(dt), want_feat=[1])
    _check_status(st, [{}])
    return _feat_dict('?', oi[0].cpu().numpy(), od[0].cpu().numpy(), True)


def compute_accels(pos_traj, h_traj, dt):
    """Total, forward and lateral acceleration magnitudes of one trajectory (reference src/eval_adv_gen.py:323-337): pos_traj
    (T,2), h_traj (T,2) -> three (T-2) tensors.  Host glue for callers of the reference's helper; the evaluation itself forms
    these series inside the kernel."""
    vel = (pos_traj[1:] - pos_traj[:-1]) / dt
    s = torch.norm(vel, dim=-1)
    unit = h_traj / torch.norm(h_traj, dim=-1, keepdim=True)
    vel = s.unsqueeze(1) * unit[:-1]
    fwd = torch.abs((s[1:] - s[:-1]) / dt)
    acc = (vel[1:] - vel[:-1]) / dt
    lat_dir = torch.cat([-unit[:-2, 1:2], unit[:-2, 0:1]], dim=1)
    lat = torch.abs(torch.sum(acc * lat_dir, dim=-1))
    return torch.norm(acc, dim=-1), fwd, lat


def compute_success_rates(scenarios):
    """(adversarial success rate, solution success rate) (reference src/eval_adv_gen.py:515-520)."""
    tot_scenes = float(sum([len(cur_scenes) for _, cur_scenes in scenarios.items()]))
    n_adv_succ = len(scenarios['adv_sol_success']) + len(scenarios['sol_failed'])
    return n_adv_succ / tot_scenes, len(scenarios['adv_sol_success']) / float(n_adv_succ)


def _log_scene(oi, od, metrics, freq_metrics_cnt, freq_metrics_total, has_map):
    """One scene's kernel rows (host) into the running dictionaries, in the reference's order (:381-511)."""
    nan = float('nan')
    seq = dict()
    did, CT = int(oi[I['adv_collide']]), int(oi[I['coll_t']])
    freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'adv_collide', did, 1)
    seq['adv_collide'] = did
    n_others = int(oi[I['n_others']])
    if CT > 0:
        ncv, ntv = int(oi[I['num_coll_veh']]), int(oi[I['num_traj_veh']])
        freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'veh_coll_rate', ncv, ntv)
        seq['veh_coll_rate'] = float(ncv) / float(ntv)
        if not has_map:
            raise ValueError('compute_metrics needs a map environment for the off-road terms')
        atk_env = int(oi[I['env_coll_atk']])
        freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'env_coll_atk', atk_env, 1)
        seq['env_coll_atk'] = atk_env
        if n_others > 0:
            oth = int(oi[I['env_coll_others']])
            freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'env_coll_others', oth, n_others)
            seq['env_coll_others'] = float(oth) / n_others
        else:
            seq['env_coll_others'] = nan
    else:
        seq['veh_coll_rate'] = seq['env_coll_atk'] = seq['env_coll_others'] = nan
    for who, cnt_col in (('atk', 'atk_accel_cnt'), ('other', 'other_accel_cnt')):
        cnt = int(oi[I[cnt_col]])
        for suffix in ('accel', 'accel_fwd', 'accel_lat'):
            key = 'adv_%s_%s' % (who, suffix)
            if cnt > 0:
                total = float(od[D['%s_%s_sum' % (who, suffix)]])
                metrics = log_metric_sum(metrics, key, total, cnt)
                seq[key] = total / cnt
            else:
                seq[key] = nan
    metrics = log_metric_sum(metrics, 'adv_z_ll_atk', float(od[D['ll_atk']]), 1)
    seq['adv_z_ll_atk'] = float(od[D['ll_atk']])
    if n_others > 0:
        metrics = log_metric_sum(metrics, 'adv_z_ll_other', float(od[D['ll_other_sum']]), n_others)
        seq['adv_z_ll_other'] = float(od[D['ll_other_sum']]) / n_others
    else:
        seq['adv_z_ll_other'] = nan
    fit = int(oi[I['fit_cnt']])
    if fit >= 0:
        for key, col in (('match_plan_pos', 'fit_pos_sum'), ('match_plan_ang', 'fit_ang_deg_sum'), ('match_plan_ang_rad', 'fit_ang_rad_sum')):
            metrics = log_metric_sum(metrics, key, float(od[D[col]]), fit)
            seq[key] = float(od[D[col]]) / fit if fit > 0 else nan       # (the mean of an empty tensor is NaN in the reference too)
    else:
        seq['match_plan_pos'] = seq['match_plan_ang'] = seq['match_plan_ang_rad'] = nan
    return metrics, freq_metrics_cnt, freq_metrics_total, seq


def _eval_group(scenes, map_env, map_idx, want_feat, device):
    args = _stack(scenes, device)
    oi, od, st = scenario_eval_metrics(map_env=map_env, mapix=map_idx, want_feat=want_feat, **args)
    _check_status(st.cpu(), scenes)
    return oi.cpu().numpy(), od.cpu().numpy()


def compute_metrics(scene, map_env, map_idx, metrics, freq_metrics_cnt, freq_metrics_total):
    """Metrics of ONE scene (reference src/eval_adv_gen.py:339-513; the kernel with B = 1) on the device of ``map_env``'s raster:
    adds to ``metrics`` (pooled totals and counts) and to the frequency pair and returns ``(metrics, freq_metrics_cnt,
    freq_metrics_total, seq_metrics)`` with the reference's 15 per-scene keys (``quant_eval`` adds ``sol_success``), NaN where the
    reference puts NaN."""
    oi, od = _eval_group([scene], map_env, [int(map_idx)], [0], map_env.nusc_raster.device)
    return _log_scene(oi[0], od[0], metrics, freq_metrics_cnt, freq_metrics_total, True)


# ------------------------------------------------------------------------------------------------
# clustering labels
# ------------------------------------------------------------------------------------------------

class FixedClustering(object):
    """Cluster centres to label scenes with: ``cluster_centers_`` (k,F) float64 and, when known, ``labels_`` of the fit."""

    def __init__(self, centers, labels=None):
        self.cluster_centers_ = np.ascontiguousarray(np.asarray(centers, dtype=np.float64))
        self.labels_ = None if labels is None else np.asarray(labels)


def load_clustering(cluster_path):
    """``cluster_path``: an object with ``cluster_centers_``, the ``cluster.npz`` of strive_amd.cluster_scenarios, or a pickle of
    such an object (the reference's ``cluster.pkl`` loads only where scikit-learn can unpickle it)."""
    if hasattr(cluster_path, 'cluster_centers_'):
        return cluster_path
    if str(cluster_path).endswith('.npz'):
        with np.load(cluster_path, allow_pickle=False) as f:
            return FixedClustering(f['centers'], f['labels'] if 'labels' in f else None)
    import pickle
    with open(cluster_path, 'rb') as f:
        obj = pickle.load(f)
    if not hasattr(obj, 'cluster_centers_'):
        raise ValueError('%s holds no clustering (no cluster_centers_)' % cluster_path)
    return obj


def predict_clusters(clustering, feats, device):
    """Nearest centre of every feature row: one ``strive_kmeans_step`` with the centres held fixed."""
    centers = torch.as_tensor(np.asarray(clustering.cluster_centers_, dtype=np.float64))
    labels = kmeans_step(torch.as_tensor(np.asarray(feats, dtype=np.float64)).to(device), centers.to(device))[0]
    return labels.cpu().numpy().astype(np.int64)


def assign_cluster(scene_list, clustering, cluster_labels, csv_out_path=None, batch_scenes=256, device='cuda:0', _rows=None):
    """Label every scene of ``scene_list`` with its collision type (reference src/eval_adv_gen.py:208-236): the features come
    from batched kernel calls (``want_feat`` only: no map, no latents), the labels from ``clustering``'s centres.  Sets ``label``
    and ``label_idx`` in place, writes ``csv_out_path`` and returns the list of feature dicts."""
    print('Collecting scene features...')
    feat_list = []
    if _rows is None:
        _rows = []
        for group in group_by_steps(scene_list, int(batch_scenes)):
            scenes = [scene_list[i] for i in group]
            args = _stack(scenes, device, with_latents=False)
            oi, od, st = scenario_eval_metrics(want_feat=[1] * len(scenes), **args)
            _check_status(st.cpu(), scenes)
            _rows += list(zip(oi.cpu().numpy(), od.cpu().numpy()))
    for scene, (oi, od) in zip(scene_list, _rows):
        feat_list.append(_feat_dict(scene['name'], oi, od, True))
    if not feat_list:
        return feat_list
    angvec = np.array([feat['angvec'] for feat in feat_list])
    hvec = np.array([feat['hvec'] for feat in feat_list])
    scene_labels = predict_clusters(clustering, np.concatenate([angvec, hvec], axis=1), device)
    for si, scene in enumerate(scene_list):
        scene['label'] = cluster_labels[scene_labels[si]]
        scene['label_idx'] = scene_labels[si]
    if csv_out_path is not None:
        with open(csv_out_path, 'w') as f:
            csvwrite = csv.writer(f)
            csvwrite.writerow(['scene', 'cluster_idx', 'cluster_name'])
            for sidx, scene in enumerate(scene_list):
                csvwrite.writerow([scene['name'], scene_labels[sidx], scene['label']])
    return feat_list


def quant_eval(scenarios, cluster_path, cluster_labels, map_env, out_path, batch_scenes=256, device='cuda:0'):
    """The reference's quantitative evaluation (src/eval_adv_gen.py:238-320), batched: ``adv_sol_success``, ``sol_failed`` and
    ``adv_failed`` in that order, up to ``batch_scenes`` consecutive scenes with one number of steps per kernel call, collision
    features for the first two categories only.  Writes ``<category>_labels.csv``, ``eval_per_seq_{adv_sol,all_adv,all_scenes}.csv``
    and ``eval_total_*.csv`` with the reference's headers and row order (``scene_distrib.png`` is not drawn) and returns
    ``(metrics, freq_metrics_cnt, freq_metrics_total)`` (the reference returns nothing).  ``cluster_labels`` is the path of the
    comma-separated label file or the list itself.  A crash scenario without a x5 up-sampled contact raises ValueError."""
    os.makedirs(out_path, exist_ok=True)
    device = torch.device(device)
    clustering = load_clustering(cluster_path)
    if isinstance(cluster_labels, str):
        with open(cluster_labels, 'r') as f:
            cluster_labels = f.readlines()[0].split(',')
    cluster_labels = [label.strip() for label in cluster_labels]
    if map_env.nusc_raster.device != device:
        map_env.nusc_raster, map_env.nusc_dx = map_env.nusc_raster.to(device), map_env.nusc_dx.to(device)

    # every scene through the kernel once: metrics and (for the crashes) features
    rows = {}
    for resname in RES_NAMES:
        cur = scenarios[resname]
        rows[resname] = []
        for group in group_by_steps(cur, int(batch_scenes)):
            scenes = [cur[i] for i in group]
            map_idx = [map_env.map_list.index(s['map']) for s in scenes]
            oi, od = _eval_group(scenes, map_env, map_idx, [int(resname != 'adv_failed')] * len(scenes), device)
            rows[resname] += list(zip(oi, od))

    for coll_sname in ['adv_sol_success', 'sol_failed']:
        if len(scenarios[coll_sname]) == 0:
            continue
        assign_cluster(scenarios[coll_sname], clustering, cluster_labels, os.path.join(out_path, coll_sname + '_labels.csv'),
                       device=device, _rows=rows[coll_sname])

    adv_success_rate, sol_success_rate = compute_success_rates(scenarios)
    tot_success_rate = adv_success_rate * sol_success_rate
    metrics, freq_metrics_cnt, freq_metrics_total = {}, {}, {}
    for residx, resname in enumerate(RES_NAMES):
        for scene, (oi, od) in zip(scenarios[resname], rows[resname]):
            metrics, freq_metrics_cnt, freq_metrics_total, seq_metrics = _log_scene(oi, od, metrics, freq_metrics_cnt, freq_metrics_total, True)
            if resname in ['adv_sol_success', 'sol_failed']:
                sol_success = resname == 'adv_sol_success'
                freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'sol_success', int(sol_success), 1)
                seq_metrics['sol_success'] = int(sol_success)
            else:
                seq_metrics['sol_success'] = np.nan
            scene['eval_metrics'] = seq_metrics
        eval_name = {'adv_sol_success': 'adv_sol', 'sol_failed': 'all_adv', 'adv_failed': 'all_scenes'}[resname]
        per_seq_metrics = sorted(list(scenarios['adv_sol_success'][0]['eval_metrics'].keys()))
        with open(os.path.join(out_path, 'eval_per_seq_' + eval_name + '.csv'), 'w') as f:
            csvwrite = csv.writer(f)
            csvwrite.writerow(['name'] + per_seq_metrics)
            for ridx in range(residx + 1):
                for scene in scenarios[RES_NAMES[ridx]]:
                    csvwrite.writerow([scene['name']] + [scene['eval_metrics'][k] for k in per_seq_metrics])
        with open(os.path.join(out_path, 'eval_total_' + eval_name + '.csv'), 'w') as f:
            csvwrite = csv.writer(f)
            csvwrite.writerow(['adv_success', 'sol_success', 'tot_success'] + per_seq_metrics)
            data = [adv_success_rate, sol_success_rate, tot_success_rate]
            for k in per_seq_metrics:
                if k in metrics:
                    data.append(metrics[k].mean())
                if k in freq_metrics_cnt:
                    data.append(float(freq_metrics_cnt[k]) / freq_metrics_total[k])
                if k not in metrics and k not in freq_metrics_cnt:
                    data.append('')
            csvwrite.writerow(data)
    return metrics, freq_metrics_cnt, freq_metrics_total


def qual_eval(*args, **kwargs):
    raise NotImplementedError('qual_eval renders scenes with matplotlib and the nuScenes map API; rendering is not part of strive_amd')


def viz_scenario(*args, **kwargs):
    raise NotImplementedError('viz_scenario renders scenes with matplotlib and the nuScenes map API; rendering is not part of strive_amd')


class SyntheticMapWorld(object):
    """Map environment of ``--map_world synthetic``: the raster of strive_amd.synth.make_raster under the names the synthetic
    scenes carry (``synthetic-0`` ...)."""

    def __init__(self, nmaps=1):
        from . import synth
        self.nusc_raster, self.nusc_dx = synth.make_raster(M=nmaps)
        self.map_list = ['synthetic-%d' % i for i in range(nmaps)]


def eval_adv_gen(cfg, map_env):
    """Read ``adv_failed``, ``adv_sol_success`` and ``sol_failed`` under ``cfg['scenarios']`` and run the quantitative evaluation
    into ``<out>/eval_quant`` (reference src/eval_adv_gen.py:642-689)."""
    if not os.path.exists(cfg['scenarios']):
        raise SystemExit('Could not find scenario_dir %s!' % cfg['scenarios'])
    scenarios = {k: [] for k in ['adv_failed', 'adv_sol_success', 'sol_failed']}
    for resname in scenarios:
        res_path = os.path.join(cfg['scenarios'], resname)
        if os.path.exists(res_path):
            print('Reading in adversarial scenarios from %s...' % res_path)
            scenarios[resname] += read_adv_scenes(res_path)
    for k, v in scenarios.items():
        print('%s : %d' % (k, len(v)))
    res = None
    if cfg['eval_quant']:
        res = quant_eval(scenarios, cfg['cluster_path'], cfg['cluster_labels'], map_env, os.path.join(cfg['out'], 'eval_quant'),
                         batch_scenes=cfg['batch_scenes'], device=cfg['device'])
    if cfg['eval_qual']:
        qual_eval()
    return scenarios, res


def get_parser():
    import argparse
    p = argparse.ArgumentParser(description='Evaluation of generated scenarios')
    p.add_argument('--out', type=str, default='./out/eval_adv_gen_out', help='output directory')
    p.add_argument('--scenarios', type=str, required=True, help='directory with adv_failed, adv_sol_success and sol_failed')
    p.add_argument('--cluster_path', type=str, default='./data/clustering/cluster.npz', help='clustering to label the crashes with')
    p.add_argument('--cluster_labels', type=str, default='./data/clustering/cluster_labels.txt', help='comma-separated cluster names')
    p.add_argument('--eval_quant', action='store_true', help='quantitative evaluation')
    p.add_argument('--eval_qual', action='store_true', help='qualitative evaluation (rendering; not available)')
    p.add_argument('--map_world', type=str, default=None, choices=['synthetic'], help='map environment with the drivable raster')
    p.add_argument('--maps', type=str, default=None, help='a maps file (datasets/maps.py) with the maps the scenes name, instead of --map_world')
    p.add_argument('--batch_scenes', type=int, default=256, help='scenes per kernel call')
    p.add_argument('--device', type=str, default='cuda:0')
    return p


def main(argv=None):
    cfg = vars(get_parser().parse_args(argv))
    from .eval_traffic_tracks import maps_file_env, one_map_source, scenario_map_names
    one_map_source(cfg, 'map_world')
    if cfg['map_world'] is None and cfg['maps'] is None:
        raise SystemExit('eval_adv_gen: the nuScenes devkit and data are not available here; a map environment with the drivable '
                         'raster must be supplied from Python (quant_eval(scenarios, cluster_path, cluster_labels, map_env, ...)), or '
                         'use --map_world synthetic')
    os.makedirs(cfg['out'], exist_ok=True)
    if cfg['maps'] is not None:
        needed = scenario_map_names(*[os.path.join(cfg['scenarios'], r) for r in ('adv_failed', 'adv_sol_success', 'sol_failed')])
        return eval_adv_gen(cfg, maps_file_env(cfg['maps'], needed, cfg['device']))
    return eval_adv_gen(cfg, SyntheticMapWorld())


if __name__ == '__main__':
    main()
