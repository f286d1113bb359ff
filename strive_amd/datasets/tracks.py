"""The devkit-free record file ("tracks"): one ``.npz`` with exactly what the reference's ``compile_data``
hands to ``post_process`` (reference src/datasets/nuscenes_dataset.py:350-414), all scenes flattened into ragged arrays.

  scene_name (S) str, scene_map (S) str        scene and map names
  frame_ptr (S+1) int64, ego_t (F) int64       a scene's timeline in microseconds
  agent_ptr (S+1) int64                        a scene's agents; the first is the ego, the others in order of first appearance
  lw (A,2) float64, cat (A) int32              length and width; index into ``categories`` (the ego's is ignored)
  categories (K) str                           category names ('car', 'truck', ...)
  obs_ptr (A+1) int64                          an agent's observations
  obs_frame (O) int32                          index on the scene's timeline (the reference's ego_t_map)
  obs (O,5) float64                            x, y, h, hcos, hsin, already flipped for Singapore as compile_data does
"""
import numpy as np

KEYS = ('scene_name', 'scene_map', 'frame_ptr', 'ego_t', 'agent_ptr', 'lw', 'cat', 'categories', 'obs_ptr', 'obs_frame', 'obs')


def _monotone(name, p, first, last):
    p = np.asarray(p)
    if p.ndim != 1 or p.shape[0] < 1 or int(p[0]) != first or int(p[-1]) != last or np.any(np.diff(p) < 0):
        raise ValueError('tracks: %s must rise from %d to %d' % (name, first, last))


def check_tracks(tr):
    """Shapes and monotonicity of a tracks dict; returns it with canonical dtypes."""
    for k in KEYS:
        if k not in tr:
            raise ValueError('tracks: missing array %r' % k)
    out = {'scene_name': [str(s) for s in np.asarray(tr['scene_name']).tolist()],
           'scene_map': [str(s) for s in np.asarray(tr['scene_map']).tolist()],
           'categories': [str(s) for s in np.asarray(tr['categories']).tolist()],
           'frame_ptr': np.asarray(tr['frame_ptr'], dtype=np.int64), 'ego_t': np.asarray(tr['ego_t'], dtype=np.int64),
           'agent_ptr': np.asarray(tr['agent_ptr'], dtype=np.int64), 'lw': np.asarray(tr['lw'], dtype=np.float64),
           'cat': np.asarray(tr['cat'], dtype=np.int32), 'obs_ptr': np.asarray(tr['obs_ptr'], dtype=np.int64),
           'obs_frame': np.asarray(tr['obs_frame'], dtype=np.int32), 'obs': np.asarray(tr['obs'], dtype=np.float64)}
    S = len(out['scene_name'])
    if len(out['scene_map']) != S or len(set(out['scene_name'])) != S:
        raise ValueError('tracks: scene_name and scene_map must have one (unique) entry per scene')
    A, O, F = out['lw'].shape[0], out['obs'].shape[0], out['ego_t'].shape[0]
    if out['lw'].shape != (A, 2) or out['cat'].shape != (A,) or out['obs'].shape != (O, 5) or out['obs_frame'].shape != (O,):
        raise ValueError('tracks: lw (A,2), cat (A), obs (O,5), obs_frame (O) expected')
    for name, p, n, last in (('frame_ptr', out['frame_ptr'], S, F), ('agent_ptr', out['agent_ptr'], S, A), ('obs_ptr', out['obs_ptr'], A, O)):
        if p.shape != (n + 1,):
            raise ValueError('tracks: %s has %d entries, expected %d' % (name, p.shape[0], n + 1))
        _monotone(name, p, 0, last)
    if np.any(np.diff(out['agent_ptr']) < 1):
        raise ValueError('tracks: every scene needs its ego')
    T = np.diff(out['frame_ptr'])
    if np.any(T < 2):
        raise ValueError('tracks: every scene needs at least two frames')
    for s in range(S):
        if np.any(np.diff(out['ego_t'][out['frame_ptr'][s]:out['frame_ptr'][s + 1]]) <= 0):
            raise ValueError('tracks: timeline of scene %d does not rise' % s)
    scene_of = np.repeat(np.arange(S), np.diff(out['agent_ptr']))
    agent_of = np.repeat(np.arange(A), np.diff(out['obs_ptr']))
    if O and (np.any(out['obs_frame'] < 0) or np.any(out['obs_frame'] >= T[scene_of[agent_of]])):
        raise ValueError('tracks: obs_frame outside its scene')
    same = agent_of[1:] == agent_of[:-1]
    if O > 1 and np.any(np.diff(out['obs_frame'])[same] <= 0):
        raise ValueError('tracks: the observations of an agent must rise in time')
    ego = out['agent_ptr'][:-1]
    n_ego = np.diff(out['obs_ptr'])[ego]
    if np.any(n_ego != T):
        raise ValueError('tracks: the ego is observed in every frame of its scene')
    K = len(out['categories'])
    others = np.ones((A,), dtype=bool)
    others[ego] = False
    if np.any(out['cat'][others] < 0) or np.any(out['cat'][others] >= K):
        raise ValueError('tracks: cat outside categories')
    if not np.all(np.isfinite(out['obs'])) or not np.all(np.isfinite(out['lw'])):
        raise ValueError('tracks: obs and lw must be finite')
    return out


def save_tracks(path, tr):
    tr = check_tracks(tr)
    arrs = dict(tr)
    for k in ('scene_name', 'scene_map', 'categories'):
        arrs[k] = np.asarray(tr[k], dtype=np.str_)
    np.savez_compressed(path, **arrs)


def load_tracks(path):
    with np.load(path, allow_pickle=False) as z:
        return check_tracks({k: z[k] for k in z.files})
