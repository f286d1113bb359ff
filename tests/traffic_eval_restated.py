"""float64 numpy restatement of strive_traffic_eval_metrics (strive_amd/csrc/eval_metrics.hip), formula by formula and in the kernel's order
of summation (reference src/losses/traffic_model.py:120-164, 297-364, 366-419, 465-545; src/datasets/nuscenes_utils.py:266-298,
416-428; src/datasets/utils.py:75-90).  Test infrastructure only; nothing here is loaded by the product."""
import numpy as np

from adv_eval_restated import pose_iou, drivable_count

IOU_THRESH = 0.02
NT = 256                          # threads of the workgroup: the order in which partial sums are added
f32 = np.float32


def unnorm(v, mean, std):
    """MeanStdNormalizer.unnormalize in fp32: (v * std) + mean, each operation rounded."""
    v = np.asarray(v, dtype=f32)
    d = v.shape[-1]
    return ((v * np.asarray(std, dtype=f32)[:d]).astype(f32) + np.asarray(mean, dtype=f32)[:d]).astype(f32)


def errs(g, p):
    """(position error, heading error in degrees) of two fp32 poses, float64."""
    g, p = np.asarray(g, dtype=np.float64), np.asarray(p, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ex, ey = g[0] - p[0], g[1] - p[1]
        pos = np.sqrt(ex * ex + ey * ey)
        gn, qn = np.sqrt(g[2] * g[2] + g[3] * g[3]), np.sqrt(p[2] * p[2] + p[3] * p[3])
        dot = (g[2] / gn) * (p[2] / qn) + (g[3] / gn) * (p[3] / qn)
        raw = dot
        dot = -1.0 if dot < -1.0 else (1.0 if dot > 1.0 else dot)
        deg = np.arccos(dot) * (180.0 / 3.14159265358979323846)
    return float(pos), float(deg), float(raw)


def nan_min(vals):
    m = np.inf
    for v in vals:
        m = (m + v) if (m != m or v != v) else (v if v < m else m)
    return float(m)


def grid(pred_u, lw_u, ptr, dx_all, ego_only):
    """(L, W, rows, ratio_l, ratio_w) as traffic_eval_grid_kernel forms them: thread t adds count * size of the items t, t + 256,
    ... in that order, one thread adds the 256 partial sums in thread order."""
    NA = pred_u.shape[0]
    items = [int(a) for a in ptr[:-1]] if ego_only else list(range(NA))
    cnt, sl, sw = np.zeros(NT, dtype=np.int64), np.zeros(NT), np.zeros(NT)
    for k, a in enumerate(items):
        c = int((~np.isnan(pred_u[a]).any(-1)).sum())
        if c > 0:
            t = k % NT
            cnt[t] += c
            sl[t] += float(c) * float(lw_u[a, 0])
            sw[t] += float(c) * float(lw_u[a, 1])
    tot, tl, tw = 0, 0.0, 0.0
    for t in range(NT):
        tot += int(cnt[t])
        tl += sl[t]
        tw += sw[t]
    sdx = 0.0
    for v in np.asarray(dx_all, dtype=np.float64).reshape(-1):
        sdx += float(v)
    mdx = sdx / float(np.asarray(dx_all).size)
    if tot == 0:
        return 0, 0, 0, float('nan'), float('nan')
    rl, rw = (tl / float(tot)) / mdx, (tw / float(tot)) / mdx
    return int(np.rint(rl)), int(np.rint(rw)), tot, rl, rw


def metrics(pred, gt, vis, ptr, lw, smean, sstd, amean, astd, raster=None, dx=None, mapix=None, ego_only=True, grid_lw=None,
            err=False, disp=False, veh=False, env=False):
    """All four groups on NORMALISED inputs -> dict of arrays shaped like the kernel's outputs, plus ``abs/<key>`` (the sum of the
    absolute values of the terms of every summed quantity), ``dot`` (the unclamped heading dot products behind ang_err / the ego's
    angle errors), ``iou`` (every IoU formed, NaN = skipped) and ``frac`` (count / (L W) of every valid frame examined)."""
    pred_u = unnorm(pred, smean, sstd)
    lw_u = unnorm(lw, amean, astd)
    NA, NS, T = pred_u.shape[:3]
    ptr = [int(v) for v in ptr]
    B = len(ptr) - 1
    out = {}
    if gt is not None:
        gt_u = unnorm(np.asarray(gt)[..., :4], smean, sstd)
        Tg = gt_u.shape[1]
    if err:
        assert T == Tg
        pe, ae, dots = np.full((NA, Tg), np.nan), np.full((NA, Tg), np.nan), np.full((NA, Tg), np.nan)
        for a in range(NA):
            for t in range(Tg):
                if float(vis[a, t]) == 1.0:
                    pe[a, t], ae[a, t], dots[a, t] = errs(gt_u[a, t], pred_u[a, 0, t])
        out['pos_err'], out['ang_err'], out['dot/err'] = pe, ae, dots
    if disp:
        Tc = min(T, Tg)
        d = np.full((B, 5), np.nan)
        ab = np.zeros((B, 5))
        dots = np.full((B, NS, Tc), np.nan)
        for b in range(B):
            a0 = ptr[b]
            ade, fde, aade, afde = [], [], [], []
            for s in range(NS):
                sd, sa, pos, deg = 0.0, 0.0, 0.0, 0.0
                for t in range(Tc):
                    pos, deg, dots[b, s, t] = errs(gt_u[a0, t], pred_u[a0, s, t])
                    sd += pos
                    sa += deg
                ade.append(sd / float(Tc))
                fde.append(pos)
                aade.append(sa / float(Tc))
                afde.append(deg)
            d[b, :4] = [nan_min(ade), nan_min(fde), nan_min(aade), nan_min(afde)]
            part, e = np.zeros(NT), 0
            p = pred_u[a0].astype(np.float64)
            for s in range(NS):
                for s2 in range(NS):
                    for t in range(Tc):
                        if s2 > s:
                            ex, ey = p[s, t, 0] - p[s2, t, 0], p[s, t, 1] - p[s2, t, 1]
                            part[e % NT] += np.sqrt(ex * ex + ey * ey)
                        e += 1
            tot = 0.0
            for t in range(NT):
                tot += part[t]
            with np.errstate(invalid='ignore', divide='ignore'):
                d[b, 4] = np.float64(2.0 * tot) / np.float64(float(NS) * float(NS - 1) * float(Tc))
        out['disp'], out['dot/disp'] = d, dots
    if veh:
        did = np.zeros((NA, NS), dtype=np.int32)
        ious = []
        for b in range(B):
            for i in range(ptr[b], ptr[b + 1]):
                for s in range(NS):
                    for j in range(i + 1, ptr[b + 1]):
                        for t in range(T):
                            v = pose_iou(pred_u[i, s, t], lw_u[i], pred_u[j, s, t], lw_u[j])
                            ious.append(v)
                            if v > IOU_THRESH:
                                did[i, s] = 1
        out['did_collide_veh'], out['iou'] = did, np.asarray(ious, dtype=np.float64)
    if env:
        L, W, rows, rl, rw = grid(pred_u, lw_u, ptr, dx, ego_only)
        if grid_lw is not None:
            L, W, rows = int(grid_lw[0]), int(grid_lw[1]), 1
        out['grid_i'], out['grid_d'] = np.asarray([L, W, rows], dtype=np.int32), np.asarray([rl, rw])
        did = np.zeros((B if ego_only else NA, NS), dtype=np.int32)
        fracs = []
        thresh = f32(1.0 - 0.05)
        for b in range(B):
            m = int(mapix[b])
            for a in ([ptr[b]] if ego_only else range(ptr[b], ptr[b + 1])):
                for s in range(NS):
                    for t in range(T):
                        if rows == 0 or np.isnan(pred_u[a, s, t]).any():
                            continue
                        on = drivable_count(np.asarray(raster[m, 0]), np.asarray(dx[m]), pred_u[a, s, t], lw_u[a], L, W)
                        fracs.append(on / float(L * W))
                        if f32(on) / f32(L * W) < thresh:
                            did[b if ego_only else a, s] = 1
        out['did_collide_map'], out['frac'] = did, np.asarray(fracs, dtype=np.float64)
    return out
