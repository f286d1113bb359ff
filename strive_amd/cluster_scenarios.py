"""Collision-type clustering of generated scenarios (reference src/cluster_scenarios.py): k-means on the attacker's direction and
heading in the ego's frame at the first x5 up-sampled contact.

The features of all scenes come from batched launches of ``strive_scenario_eval_metrics`` (``want_feat`` only: no map, no
latents); ``fit_kmeans`` runs Lloyd iterations with ``strive_kmeans_step`` on the device (assignment, per-cluster sums and counts,
inertia) and the centre update and stopping rule on the host in float64.

    python -m strive_amd.cluster_scenarios --scenario_dirs DIR [DIR ...] --k 10 --out OUT
"""
import os

import numpy as np
import torch

from . import eval_adv_gen as EA
from .datasets.utils import read_adv_scenes


def compute_coll_feat(lw, scene_traj, dt, device=None):
    """Collision features of ONE scene (reference src/cluster_scenarios.py:83-121; the kernel with B = 1): ``{'h', 'hvec', 'ang',
    'angvec'}``."""
    NA = int(scene_traj.shape[0])
    traj = scene_traj[:, :, :4] if device is None else scene_traj[:, :, :4].to(device)
    oi, od, st = EA.scenario_eval_metrics(traj, [0, NA], lw, [min(1, NA - 1)], float(dt), want_feat=[1])
    EA._check_status(st.cpu(), [{}])
    return EA._feat_dict('?', oi[0].cpu().numpy(), od[0].cpu().numpy(), False)


def kmeans_plusplus(feats, k, rs):
    """k-means++ seeding on the host: the first centre uniformly, every further one with probability proportional to the squared
    distance to the nearest centre chosen so far.  NOT scikit-learn's seeding (which draws several candidates per centre and
    consumes its random stream differently): ``random_state=0`` of the reference is not reproduced."""
    feats = np.asarray(feats, dtype=np.float64)
    N = feats.shape[0]
    centers = [feats[rs.randint(N)]]
    d2 = ((feats - centers[0]) ** 2).sum(1)
    for _ in range(1, k):
        tot = d2.sum()
        idx = int(np.searchsorted(np.cumsum(d2), rs.random_sample() * tot)) if tot > 0 else rs.randint(N)
        centers.append(feats[min(idx, N - 1)])
        d2 = np.minimum(d2, ((feats - centers[-1]) ** 2).sum(1))
    return np.stack(centers)


def fit_kmeans(feats, k, init=None, seed=0, max_iter=300, tol=1e-4, device='cuda:0'):
    """Lloyd's k-means on feats (N,F), F <= 8, k <= 64 -> ``(centers (k,F), labels (N), inertia, n_iter)``, float64.  Every iteration
    is one ``strive_kmeans_step`` (labels, per-cluster sums and counts) and ``centers = sums / counts`` on the host.  It stops when
    the labels do not change, or when the squared centre shift is <= ``tol * mean(var(feats, axis=0))`` -- scikit-learn's rule
    (then one more assignment against the final centres, as scikit-learn does); the inertia belongs to the returned centres and
    labels.  ``init`` (k,F) gives the starting centres; with ``init=None`` they come from ``kmeans_plusplus`` with
    ``numpy.random.RandomState(seed)``, which is not scikit-learn's seeding.  A cluster that empties raises ValueError
    (scikit-learn relocates it)."""
    x_host = np.ascontiguousarray(np.asarray(feats, dtype=np.float64))
    if x_host.ndim != 2 or x_host.shape[0] < k or k < 1:
        raise ValueError('fit_kmeans needs feats (N,F) with N >= k >= 1')
    centers = kmeans_plusplus(x_host, k, np.random.RandomState(seed)) if init is None else np.array(init, dtype=np.float64)
    if centers.shape != (k, x_host.shape[1]):
        raise ValueError('init must be (k,F)')
    x = torch.from_numpy(x_host).to(device)
    tol_abs = float(tol) * float(np.mean(np.var(x_host, axis=0)))
    labels_old, strict, n_iter = None, False, 0
    for i in range(int(max_iter)):
        labels, _, sums, counts, _ = EA.kmeans_step(x, torch.from_numpy(centers).to(device))
        labels, sums, counts = labels.cpu().numpy(), sums.cpu().numpy(), counts.cpu().numpy()
        if (counts == 0).any():
            raise ValueError('cluster %d emptied at iteration %d (relocation is not implemented): choose other starting centres or a '
                             'smaller k' % (int(np.argmin(counts)), i))
        new = sums / counts[:, None]
        shift = float(((new - centers) ** 2).sum())
        centers = new
        n_iter = i + 1
        if labels_old is not None and np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol_abs:
            break
        labels_old = labels
    labels, _, _, _, inertia = EA.kmeans_step(x, torch.from_numpy(centers).to(device))
    return centers, labels.cpu().numpy().astype(np.int64), float(inertia.cpu()[0]), n_iter


def scene_features(scene_list, batch_scenes=256, device='cuda:0'):
    """(N,4) float64 ``[angvec, hvec]`` of every scene, through batched kernel calls."""
    rows = []
    adapted = [dict(name=s['name'], dt=s['dt'], veh_att=s['veh_att'], fut_adv=s['scene_fut']) for s in scene_list]
    for group in EA.group_by_steps(adapted, int(batch_scenes)):
        scenes = [adapted[i] for i in group]
        oi, od, st = EA.scenario_eval_metrics(want_feat=[1] * len(scenes), **EA._stack(scenes, device, with_latents=False))
        EA._check_status(st.cpu(), scenes)
        for s, i_row, d_row in zip(scenes, oi.cpu().numpy(), od.cpu().numpy()):
            f = EA._feat_dict(s['name'], i_row, d_row, False)
            rows.append(f['angvec'] + f['hvec'])
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def cluster_scenarios(scenario_dirs, out_path, k, viz=False, init=None, seed=0, batch_scenes=256, device='cuda:0'):
    """Read the scenarios of ``scenario_dirs``, cluster their collision features into ``k`` types and write
    ``<out_path>/cluster.npz`` (``centers`` (k,4), ``labels`` (N), ``names`` ``%04d_<scene name>``, ``feats`` (N,4)), which
    ``eval_adv_gen --cluster_path`` reads.  Returns ``(centers, labels, inertia, n_iter)``.  (The reference pickles the
    scikit-learn object and draws cluster_k%d.jpg; rendering is not part of strive_amd.)"""
    if viz:
        raise NotImplementedError('viz renders every scene with matplotlib; rendering is not part of strive_amd')
    scene_list = []
    for scene_dir in scenario_dirs:
        print('Reading in adversarial scenarios from %s...' % scene_dir.rstrip('/').split('/')[-1])
        scene_list += read_adv_scenes(scene_dir)
    print('Collecting scene features...')
    names = [('%04d_' % si) + scene['name'] for si, scene in enumerate(scene_list)]
    feats = scene_features(scene_list, batch_scenes, device)
    print(feats.shape)
    print('Clustering using k=%d clusters...' % k)
    centers, labels, inertia, n_iter = fit_kmeans(feats, k, init=init, seed=seed, device=device)
    os.makedirs(out_path, exist_ok=True)
    np.savez(os.path.join(out_path, 'cluster.npz'), centers=centers, labels=labels, names=np.asarray(names), feats=feats)
    return centers, labels, inertia, n_iter


def get_parser():
    import argparse
    p = argparse.ArgumentParser(description='Collision scenario clustering')
    p.add_argument('--out', type=str, default='./out/clustering_out', help='output directory')
    p.add_argument('--scenario_dirs', nargs='+', type=str, required=True, help='directories to load scenarios from')
    p.add_argument('--k', type=int, default=10, help='number of clusters')
    p.add_argument('--seed', type=int, default=0, help='seed of the k-means++ starting centres')
    p.add_argument('--viz', action='store_true', help='render every collision (not available)')
    p.add_argument('--device', type=str, default='cuda:0')
    return p


def main(argv=None):
    cfg = get_parser().parse_args(argv)
    return cluster_scenarios(cfg.scenario_dirs, cfg.out, cfg.k, cfg.viz, seed=cfg.seed, device=cfg.device)


if __name__ == '__main__':
    main()
