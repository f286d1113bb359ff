"""Test infrastructure of tests/test_render.py (and of tests/golden/make_golden_render.py, which imports the case builders from here
so that there is one copy): the inputs of the g24 fixture, and the renderer's stated rule (include/strive_hip.h
strive_render_pictures) restated in float64 numpy on the same fp32 inputs, with the distance of every sub-sample to the nearest
primitive boundary."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
G18 = os.path.join(HERE, 'golden', 'g18_scenarios')
NAN = float('nan')


# ------------------------------------------------------------------------------------------------------------------------
# g24 inputs
# ------------------------------------------------------------------------------------------------------------------------

def _tracks(NA, T, key, nan_lead=(), nan_gap=()):
    """(NA, T, 4) tracks in a 64-pixel crop frame: gentle arcs, unit headings."""
    g = torch.Generator().manual_seed(key)
    start = torch.rand((NA, 2), generator=g) * 40 + 8
    ang = torch.rand((NA,), generator=g) * 6.28
    turn = (torch.rand((NA,), generator=g) - 0.5) * 0.2
    out = torch.zeros((NA, T, 4))
    for n in range(NA):
        p, a = start[n].clone(), float(ang[n])
        for t in range(T):
            out[n, t] = torch.tensor([float(p[0]), float(p[1]), float(np.cos(a)), float(np.sin(a))])
            p = p + 2.5 * torch.tensor([np.cos(a), np.sin(a)], dtype=torch.float32)
            a += float(turn[n])
    for n, k in nan_lead:
        out[n, :k] = NAN
    for n, a, b in nan_gap:
        out[n, a:b] = NAN
    return out


def direct_cases():
    """name -> keyword arguments of the reference's viz_map_crop (after x and out_path)."""
    lw3 = torch.tensor([[7.0, 3.0], [6.0, 2.5], [9.5, 3.5]])
    k3 = _tracks(3, 8, 1, nan_lead=[(1, 2)], nan_gap=[(2, 3, 5)])
    k4 = torch.stack([_tracks(2, 6, 10 + s, nan_lead=[(0, 1)] if s == 1 else ()) for s in range(3)], dim=1)       # (2, 3, 6, 4)
    lw2 = lw3[:2]
    return {
        'traj3_default': dict(car_kin=k3, car_lw=lw3, viz_traj=True),
        'traj3_styled_gt': dict(car_kin=k3, car_lw=lw3, gt_kin=_tracks(3, 8, 2, nan_gap=[(0, 2, 4)]), viz_traj=True,
                                car_colors=['orangered', 'lawngreen', 'cornflowerblue'], car_alpha=[1.0, 0.5, 0.25],
                                traj_linewidth=[2.5, 3.5, 1.0], traj_markers=[False, True, False], traj_markersize=[10.0, 15.0, 4.0]),
        'traj4_ns3': dict(car_kin=k4, car_lw=lw2, gt_kin=k4[:, 0], viz_traj=True, traj_markers=[False, False]),
        'cars3': dict(car_kin=k3, car_lw=lw3, viz_traj=False, car_alpha=[1.0, 0.9, 0.8]),
        'cars4_ns3': dict(car_kin=k4, car_lw=lw2, viz_traj=False, car_colors=['gold', 'coral']),
        'one_agent': dict(car_kin=k3[:1], car_lw=lw3[:1], viz_traj=True, traj_markers=[False]),
    }


def dir_scenes():
    """name -> scene dict of strive_amd.datasets.utils.read_adv_scenes (the reference's src/datasets/utils.py keys)."""
    from strive_amd.datasets.utils import read_adv_scenes
    sc = {}
    for cat, want in (('adv_sol_success', ('sc_0000_mid', 'sc_0002_early')), ('adv_failed', ('sc_0006_alone',))):
        for s in read_adv_scenes(os.path.join(G18, cat)):
            if s['name'] in want:
                sc[s['name']] = s
    lead = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sc['sc_0002_early'].items()}
    lead['scene_past'][2, :2] = NAN                       # a NaN lead-in
    lead['scene_fut'][3, 3:5] = NAN                       # a NaN gap mid-track
    lead['name'] = 'nan_lead_gap'
    sc['nan_lead_gap'] = lead
    return sc          # (a scene of one agent has bounds of zero width there: the reference divides by zero)


def adv_scenes():
    """name -> scene dict of strive_amd.eval_adv_gen.read_adv_scenes (the reference's src/eval_adv_gen.py keys)."""
    from strive_amd.eval_adv_gen import read_adv_scenes
    sc = {}
    for cat, want in (('adv_sol_success', ('sc_0002_early', 'sc_0003_tie')), ('adv_failed', ('sc_0006_alone',))):
        for s in read_adv_scenes(os.path.join(G18, cat)):
            if s['name'] in want:
                sc[s['name']] = s
    early = sc['sc_0002_early']
    early['fut_sol'] = early['fut_adv'].clone()
    early['fut_sol'][0, :, 1] += torch.linspace(0, 3, early['fut_adv'].size(1))
    early['past'][early['attack_agt'], :2] = NAN          # the attacker's first observed step is step 2
    del sc['sc_0003_tie']['attack_agt'], sc['sc_0003_tie']['attack_t']        # the defaults: agent 0, the middle step
    solo = {k: (v[:1].clone() if torch.is_tensor(v) and k != 'sem' else v) for k, v in sc['sc_0006_alone'].items() if k[:2] != 'z_'}
    del solo['attack_agt']                                # one agent: the ego is its own attacker and is drawn twice
    solo['name'] = 'one_agent'
    sc['one_agent'] = solo
    return sc                                             # sc_0006_alone: the attacker is the last agent, no fut_sol


# ------------------------------------------------------------------------------------------------------------------------
# the stated rule, float64
# ------------------------------------------------------------------------------------------------------------------------
CAR, POLYLINE, DISC = 0, 1, 2


def _samples(L):
    """(L, L, 16) x and y of the sub-samples of pixel (row, col): x = col + (k + 1/2)/4, y = L - 1 - row + (j + 1/2)/4."""
    o = (np.arange(4) + 0.5) / 4
    col = np.arange(L, dtype=np.float64)
    x = np.broadcast_to(col[None, :, None, None] + o[None, None, None, :], (L, L, 4, 4))
    y = np.broadcast_to((L - 1 - col)[:, None, None, None] + o[None, None, :, None], (L, L, 4, 4))
    return x.reshape(L, L, 16), y.reshape(L, L, 16)


def _seg_dist(x, y, a, b):
    ex, ey = b[0] - a[0], b[1] - a[1]
    qx, qy = x - a[0], y - a[1]
    len2 = ex * ex + ey * ey
    t = np.clip((qx * ex + qy * ey) / len2, 0.0, 1.0) if len2 > 0 else np.zeros_like(x)
    return np.hypot(qx - t * ex, qy - t * ey)


def render_ref(prims, verts, L, background):
    """One picture by the stated rule in float64.  prims (n, 16) float32 records (strive_hip.h), verts (NV, 2) float32, background
    (L, L, 3) float -> (bytes (L, L, 3) uint8, margin (L, L): the smallest distance, over the pixel's sub-samples and the primitives,
    from a sub-sample to a boundary that decides an inside test)."""
    x, y = _samples(L)
    c = np.array(background, dtype=np.float64).copy()
    margin = np.full((L, L), np.inf)
    P = np.asarray(prims, dtype=np.float32)
    V = np.asarray(verts, dtype=np.float32).astype(np.float64)

    def blend(inside, rgb, alpha):
        cov = inside.sum(axis=2) / 16.0
        a = (alpha * cov)[:, :, None]
        c[:] = c + a * (np.asarray(rgb, dtype=np.float64)[None, None, :] - c)

    for p in P:
        kind = int(p[0:1].view(np.int32)[0])
        q = p.astype(np.float64)
        rgb, alpha = q[7:10], q[10]
        if kind == CAR:
            if np.isnan(q[1:7]).any() or np.isnan(q[11:13]).any():
                continue
            n = np.hypot(q[3], q[4])
            ux, uy = (q[3] / n, q[4] / n) if n > 0 else (1.0, 0.0)
            hl, hw, he, hs = 0.5 * q[5], 0.5 * q[6], 0.5 * q[11], 0.5 * q[12]
            dx, dy = x - q[1], y - q[2]
            u, v = dx * ux + dy * uy, dy * ux - dx * uy
            au, av = np.abs(u), np.abs(v)
            blend((au <= hl) & (av <= hw), rgb, alpha)
            blend((au <= hl + he) & (av <= hw + he) & ~((au < hl - he) & (av < hw - he)), (0, 0, 0), alpha)
            blend((u >= -hs) & (u <= hl + hs) & (av <= hs), (0, 0, 0), alpha)
            d = np.minimum.reduce([np.abs(au - hl), np.abs(av - hw), np.abs(au - hl - he), np.abs(av - hw - he), np.abs(au - hl + he),
                                   np.abs(av - hw + he), np.abs(u + hs), np.abs(u - hl - hs), np.abs(av - hs)])
            near = (au <= abs(hl) + abs(he) + abs(hs) + 1e-3) & (av <= abs(hw) + abs(he) + abs(hs) + 1e-3)       # a boundary ends at the outer box
            margin = np.minimum(margin, np.where(near, d, np.inf).min(axis=2))
        elif kind == DISC:
            if np.isnan(q[[1, 2, 5]]).any():
                continue
            r = 0.5 * q[5]
            dist = np.hypot(x - q[1], y - q[2])
            blend((dist <= r) & (r >= 0), rgb, alpha)
            margin = np.minimum(margin, np.abs(dist - r).min(axis=2))
        elif kind == POLYLINE:
            vb, ve = [int(i) for i in p[13:15].view(np.int32)]
            pts = V[vb:ve]
            if pts.shape[0] < 2 or np.isnan(pts).any() or np.isnan(q[11]):
                continue
            r = 0.5 * q[11]
            dist = np.minimum.reduce([_seg_dist(x, y, pts[i], pts[i + 1]) for i in range(pts.shape[0] - 1)])
            blend((dist <= r) & (r >= 0), rgb, alpha)
            margin = np.minimum(margin, np.abs(dist - r).min(axis=2))
    return np.clip(np.rint(255.0 * c), 0, 255).astype(np.uint8), margin


def composite_map(crop, rgb, alphas):
    """White, then c += (v_i alpha_i)(col_i - c) in fp32 over the layers of ``crop`` (C, L, L) uint8 (index [i, l, w]) -> the
    background (L, L, 3) float32 of a picture: picture[row, col] shows crop[:, col, L - 1 - row]."""
    C, L, _ = crop.shape
    v = np.ascontiguousarray(np.transpose(np.asarray(crop), (0, 2, 1))[:, ::-1, :]).astype(np.float32)     # [i, row, col]
    c = np.ones((L, L, 3), dtype=np.float32)
    for i in range(C):
        a = (v[i] * np.float32(alphas[i]))[:, :, None]
        c = c + a * (np.asarray(rgb[i], dtype=np.float32)[None, None, :] - c)
    return c


def to_bytes(c):
    return np.clip(np.rint(np.float32(255.0) * c.astype(np.float32)), 0, 255).astype(np.uint8)


# ---- random primitive tables (seeds fixed so that the restatement alone leaves out < 2 % of a picture's pixels) ----

def rec(kind, rgb=(0, 0, 0), alpha=1.0):
    r = np.zeros((16,), dtype=np.float32)
    r[0:1].view(np.int32)[0] = kind
    r[7:10] = rgb
    r[10] = alpha
    return r


def car(cx, cy, hx, hy, l, w, rgb, alpha, se=1.3, sl=1.7):
    r = rec(CAR, rgb, alpha)
    r[1:7] = (cx, cy, hx, hy, l, w)
    r[11], r[12] = se, sl
    return r


def disc(cx, cy, d, rgb, alpha):
    r = rec(DISC, rgb, alpha)
    r[1], r[2], r[5] = cx, cy, d
    return r


def polyline(vb, ve, width, rgb, alpha):
    r = rec(POLYLINE, rgb, alpha)
    r[11] = width
    r[13:15].view(np.int32)[:] = (vb, ve)
    return r


RESEED = {}          # (L, n) -> offset, where the plain seed puts more than 2 % of the pixels on a boundary (none does)


def case_seed(L, n):
    return 1000 * L + n + RESEED.get((L, n), 0)


def random_prims(n, L0, seed):
    """n primitives of all three kinds around an L-pixel picture (some across the border, some outside) + their vertex table."""
    L = L0
    g = np.random.RandomState(seed)
    prims, verts = [], []
    nv = 0
    L = L * min(1.0, 40.0 / max(n, 1))                   # many primitives: smaller ones, so that the length of boundary in the picture stays
    span = lambda: g.rand(2) * (L0 + 8) - 4
    for i in range(n):
        rgb, alpha = g.rand(3), g.rand() * 0.9 + 0.1
        cx, cy = span()
        kind = i % 3
        if kind == CAR:
            a = g.rand() * 6.28
            s = 0.5 + g.rand() * 2
            prims.append(car(cx, cy, s * np.cos(a), s * np.sin(a), 1 + g.rand() * max(2.0, L / 3), 0.5 + g.rand() * max(1.0, L / 6), rgb, alpha))
        elif kind == DISC:
            prims.append(disc(cx, cy, 0.3 + g.rand() * max(1.0, L / 5), rgb, alpha))
        else:
            k = 2 + int(g.rand() * 5)
            pts = np.cumsum(np.concatenate([[[cx, cy]], (g.rand(k - 1, 2) - 0.5) * max(3.0, L / 2)]), axis=0)
            verts.append(pts.astype(np.float32))
            prims.append(polyline(nv, nv + k, 0.4 + g.rand() * 3, rgb, alpha))
            nv += k
    P = np.stack(prims) if prims else np.zeros((0, 16), dtype=np.float32)
    V = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.float32)
    return P, V
