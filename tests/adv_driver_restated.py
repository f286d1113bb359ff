"""float64 numpy restatement of strive_feasibility_screen and strive_ego_verdicts (strive_amd/csrc/eval_metrics.hip), formula by formula
(reference src/utils/scenario_gen.py:30-107; src/adv_scenario_gen.py:176-226; src/datasets/nuscenes_utils.py:266-332;
src/losses/adv_gen_nusc.py:517-565; src/utils/adv_gen_optim.py:214-235; src/utils/sol_optim.py:126-165).  Both also return what a test
needs to know how far every decision was from its threshold.  Test infrastructure only; nothing here is loaded by the product."""
import numpy as np

from adv_eval_restated import pose_iou, drivable_count
from traffic_eval_restated import IOU_THRESH, unnorm

f32, f64 = np.float32, np.float64
LINE_MAX = 65536


def mean_dx(dx_all):
    s = 0.0
    for v in np.asarray(dx_all, dtype=f64).reshape(-1):
        s += float(v)
    return s / float(np.asarray(dx_all).size)


def line_weights(n):
    """torch.linspace(0, 1, n) in fp32, element by element: step = 1 / (n - 1); the first half counts up from 0, the second down from 1."""
    if n < 2:
        return np.zeros(n, dtype=f32)
    i = np.arange(n)
    step = f32(1.0) / f32(n - 1)
    up = (step * i.astype(f32)).astype(f32)
    down = (f32(1.0) - (step * (n - 1 - i).astype(f32)).astype(f32)).astype(f32)
    return np.where(i < n // 2, up, down).astype(f32)


def line_zero(raster0, dx, start, end, n):
    """(samples of the line on a 0 pixel, does a sample leave the raster): start (1 - w) + end w in fp32, fp64 divide, round half even."""
    H, W = raster0.shape
    w = line_weights(n)
    w1 = (f32(1.0) - w).astype(f32)
    pix = []
    for c in range(2):
        g = ((f32(start[c]) * w1).astype(f32) + (f32(end[c]) * w).astype(f32)).astype(f32)
        pix.append(np.rint(g.astype(f64) / float(dx[c])))
    inside = (pix[0] >= 0) & (pix[0] < W) & (pix[1] >= 0) & (pix[1] < H)
    px, py = pix[0][inside].astype(np.int64), pix[1][inside].astype(np.int64)
    return int((raster0[py, px] == 0).sum()), bool((~inside).any())


def max_step(p):
    """Largest displacement between consecutive steps of p (..., T, >=2) fp32, in float64; NaN wins; NaN without a pair of steps."""
    p = np.asarray(p, dtype=f64)
    if p.shape[-2] < 2:
        return float('nan')
    dx, dy = p[..., 1:, 0] - p[..., :-1, 0], p[..., 1:, 1] - p[..., :-1, 1]
    v = np.sqrt(dx * dx + dy * dy)
    return float('nan') if np.isnan(v).any() else float(v.max())


def agent_best(eg, ag, t0, thresh, infront_min):
    """One non-ego agent against the ego, both (NS,FT,4) fp32 unnormalised: (dist, step, samp, within, the distances after the mask
    (NS,FT'), the distances before it, the cosines or None)."""
    e, a = eg.astype(f64), ag.astype(f64)
    dx, dy = a[..., 0] - e[..., 0], a[..., 1] - e[..., 1]
    d = np.sqrt(dx * dx + dy * dy)
    raw, cos = d[:, t0:], None
    if infront_min is not None:
        with np.errstate(invalid='ignore', divide='ignore'):
            cos = (dx / d) * e[..., 2] + (dy / d) * e[..., 3]
        d = np.where(cos >= infront_min, d, np.inf)
        cos = cos[:, t0:]
    d = d[:, t0:]
    per_step, samp = d.min(axis=0), d.argmin(axis=0)            # (the first sample on a tie)
    k = int(per_step.argmin())                                   # (the first step on a tie; 0 if every step is masked)
    return float(per_step[k]), k + t0, int(samp[k]), bool((d < thresh).any()), d, raw, cos


def screen(samples, ptr, mapix, smean, sstd, raster, dx, thresh, t0=0, agent_vel=0.0, ego_vel=0.0, infront_min=None, check_sep=True,
           planner_rule=0, allowed=None, gt=None):
    """All scenes on NORMALISED samples (NA,NS,FT,4) -> dict of arrays shaped like the kernel's outputs with the wrapper's fill values
    (a refused scene keeps them), plus ``margin``: how far the decisions were from their thresholds.  thresh, vel: every agent's
    closest approach and largest speed (and the ego's, under a planner rule) against their thresholds, relative.  cos: the cosine
    against infront_min, absolute, of every (sample, step) that decides an agent's closest approach: those no further away, before
    the mask, than the closest approach plus 1e-3 of it (all of them for an agent that is masked throughout).  half: |agent - ego| /
    mean(dx) against a half-integer, absolute, of the lines within one sample of the scene's longest (sep_n is their maximum).  gap: the relative gap between the smallest and the second smallest distinct value
    where a minimum was taken (over the steps, and over the samples of the chosen step)."""
    u = unnorm(samples, smean, sstd)
    NA = u.shape[0]
    ptr = [int(v) for v in ptr]
    B = len(ptr) - 1
    out = {'feasible': np.zeros(NA, dtype=np.int32), 'within': np.zeros(NA, dtype=np.int32), 'step': np.full(NA, -1, dtype=np.int32),
           'best_samp': np.full(NA, -1, dtype=np.int32), 'sep_zero': np.zeros(NA, dtype=np.int32), 'dist': np.full(NA, np.inf),
           'max_vel': np.full(NA, np.nan), 'out_i': np.zeros((B, 8), dtype=np.int32), 'out_d': np.full((B, 3), np.nan),
           'status': np.zeros(B, dtype=np.int32)}
    margin = {'thresh': np.inf, 'vel': np.inf, 'cos': np.inf, 'half': np.inf, 'gap': np.inf}
    gu = None if gt is None else unnorm(np.asarray(gt)[..., :4], smean, sstd)
    mdx = mean_dx(dx)

    def rel(v, ref):
        v = np.asarray(v, dtype=f64)
        v = v[np.isfinite(v)]
        return np.inf if not v.size or ref == 0 else float(np.abs(v - ref).min() / abs(ref))

    def gap(v):
        v = np.unique(np.asarray(v, dtype=f64)[np.isfinite(v)])
        return np.inf if v.size < 2 else float((v[1] - v[0]) / v[1])

    for b in range(B):
        lo, hi = ptr[b], ptr[b + 1]
        n, m = hi - lo, int(mapix[b])
        if lo < 0 or n <= 0 or hi > NA:
            out['status'][b] = 2
            continue
        if m < 0 or m >= raster.shape[0]:
            out['status'][b] = 3
            continue
        if not np.isfinite(u[lo:hi]).all():
            out['status'][b] = 5
            continue
        eg = u[lo]
        best, lines, sep_n, qs = [], [], 0, []
        for j in range(1, n):
            dist, step, samp, within, d, raw, cos = agent_best(eg, u[lo + j], t0, thresh, infront_min)
            start, end = u[lo + j, samp, step, :2], eg[samp, step, :2]
            ddx, ddy = float(start[0]) - float(end[0]), float(start[1]) - float(end[1])
            q = np.sqrt(ddx * ddx + ddy * ddy) / mdx
            sep_n = max(sep_n, int(np.rint(q)) if q <= LINE_MAX else LINE_MAX + 1)
            best.append((dist, step, samp, within, max_step(u[lo + j])))
            lines.append((start, end))
            margin['thresh'] = min(margin['thresh'], rel([dist], thresh))
            margin['vel'] = min(margin['vel'], rel([best[-1][4]], agent_vel))
            qs.append(q)
            margin['gap'] = min(margin['gap'], gap(d.min(axis=0)), gap(d[:, step - t0]))
            if cos is not None:
                decides = np.isfinite(cos) & (raw <= dist * (1.0 + 1e-3))
                if decides.any():
                    margin['cos'] = min(margin['cos'], float(np.abs(cos[decides] - infront_min).min()))
        margin['half'] = min([margin['half']] + [abs(q - np.floor(q) - 0.5) for q in qs if q >= max(qs) - 1.0])
        if sep_n > LINE_MAX:
            out['status'][b] = 6
            continue
        zeros = [line_zero(np.asarray(raster[m, 0]), np.asarray(dx[m]), s, e, sep_n) if check_sep else (0, False) for s, e in lines]
        if any(z[1] for z in zeros):
            out['status'][b] = 6
            continue
        n_within = n_any = n_feas = 0
        ha, ht, hd = -1, -1, np.inf
        for j in range(1, n):
            dist, step, samp, within, vel = best[j - 1]
            any_ = within and zeros[j - 1][0] == 0 and vel > agent_vel
            feas = any_ and (allowed is None or int(allowed[lo + j]) != 0)
            n_within, n_any, n_feas = n_within + int(within), n_any + int(any_), n_feas + int(feas)
            if feas and dist < hd:
                ha, ht, hd = j, step, dist
            a = lo + j
            out['feasible'][a], out['within'][a], out['step'][a], out['best_samp'][a] = int(feas), int(within), step, samp
            out['sep_zero'][a], out['dist'][a], out['max_vel'][a] = zeros[j - 1][0], dist, vel
        ev = max_step(eg)
        gv = float('nan') if gu is None else max_step(gu[lo])
        ego_v = gv if planner_rule == 1 else ev
        slow = planner_rule != 0 and ego_v < ego_vel
        if planner_rule != 0:
            margin['vel'] = min(margin['vel'], rel([ego_v], ego_vel))
        verdict = 1 if slow else 2 if n == 1 else 3 if n_any == 0 else 4 if n_feas == 0 else 0
        out['out_i'][b] = [n - 1, n_within, n_any, n_feas, ha, ht, sep_n, verdict]
        out['out_d'][b] = [ev, gv, hd]
    out['margin'] = margin
    return out


def ego(traj, ptr, lw, atk, smean, sstd, amean, astd, raster=None, dx=None, mapix=None, lin_max=128):
    """All scenes on NORMALISED inputs (traj (NA,T,4)) -> dict of arrays shaped like the kernel's outputs with the wrapper's fill
    values, plus ``iou`` (every IoU formed up to an agent's first hit, NaN = skipped) and ``frac`` (count / (L W) of every valid ego
    frame).  raster None: no drivable test."""
    tu, lwu = unnorm(traj, smean, sstd), unnorm(lw, amean, astd)
    NA, T = tu.shape[:2]
    ptr = [int(v) for v in ptr]
    B = len(ptr) - 1
    want_env = raster is not None
    out = {'hit': np.zeros(NA, dtype=np.int32), 'coll_t': np.full(NA, T, dtype=np.int32), 'out_i': np.zeros((B, 8), dtype=np.int32),
           'grid_d': np.full((B, 2), np.nan), 'status': np.zeros(B, dtype=np.int32)}
    ious, fracs = [], []
    thresh = f32(1.0 - 0.05)
    for b in range(B):
        lo, hi = ptr[b], ptr[b + 1]
        n = hi - lo
        a = -1 if atk is None else int(atk[b])
        if lo < 0 or n <= 0 or hi > NA or (a != -1 and not 1 <= a < n):
            out['status'][b] = 2
            continue
        if want_env and not 0 <= int(mapix[b]) < raster.shape[0]:
            out['status'][b] = 3
            continue
        L = W = rows = 0
        ratio = [np.nan, np.nan]
        if want_env:
            rows = int((~np.isnan(tu[lo]).any(-1)).sum())
            if rows > 0:
                mdx = mean_dx(dx)
                ratio = [((float(rows) * float(lwu[lo, c])) / float(rows)) / mdx for c in range(2)]
                L, W = int(np.rint(ratio[0])), int(np.rint(ratio[1]))
                if not (1 <= L <= lin_max and 1 <= W <= lin_max):
                    out['status'][b] = 4
                    continue
        for j in range(lo + 1, hi):
            for t in range(T):
                v = pose_iou(tu[lo, t], lwu[lo], tu[j, t], lwu[j])
                ious.append(v)
                if v > IOU_THRESH:
                    out['hit'][j], out['coll_t'][j] = 1, t
                    break
        env = 0
        if want_env and rows > 0:
            m = int(mapix[b])
            for t in range(T):
                if np.isnan(tu[lo, t]).any():
                    continue
                on = drivable_count(np.asarray(raster[m, 0]), np.asarray(dx[m]), tu[lo, t], lwu[lo], L, W)
                fracs.append(on / float(L * W))
                env |= int(f32(on) / f32(L * W) < thresh)
        n_hit = int(out['hit'][lo + 1:hi].sum())
        first = int(out['coll_t'][lo + 1:hi].min()) if n > 1 else T
        out['hit'][lo], out['coll_t'][lo] = int(n_hit > 0), first
        out['out_i'][b] = [n - 1, n_hit, -1 if a == -1 else int(out['hit'][lo + a]), first, env if want_env else -1, L, W, rows]
        out['grid_d'][b] = ratio
    out['iou'], out['frac'] = np.asarray(ious, dtype=f64), np.asarray(fracs, dtype=f64)
    return out
