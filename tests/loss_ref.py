"""Float64 reference of the optimisation-time collision losses, and the input recipes of tests/test_loss_edges.py.

Test infrastructure only.  Everything here takes the fp32 INPUTS the kernels of strive_amd/csrc/losses.hip get (trajectories,
the product's fp32 circle offsets ``cent_x``, radii and penalty distances) and evaluates the operation in float64 with plain torch /
numpy: no kernel, no oracle class.  Decisions (hit, first arg-min, behind test, soft-min masks) are taken on the float64 values; the
tests assert beforehand that none of them is within a stated margin of its boundary ("undecided"), so that fp32 arithmetic cannot
legitimately decide differently.
"""
import math

import numpy as np
import torch

from oracle import losses as olosses

NCIRC = 5
K_TOL = 16.0                 # kernel error <= K_TOL * max(oracle-fp32 error, 2^-23 * max|reference|)
EPS32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------
# input recipes
# ------------------------------------------------------------------------------------------------

def recipe(n, seed, origin, T=4):
    r = np.random.default_rng(seed)
    L = r.uniform(3.8, 5.5, n); W = r.uniform(1.7, 2.2, n)
    cols = int(np.ceil(np.sqrt(n)))
    gx = (np.arange(n) % cols) * 3.0; gy = (np.arange(n) // cols) * 3.0
    p0 = np.stack([gx, gy], 1) + r.uniform(-1, 1, (n, 2)) + origin
    v = r.uniform(-2, 2, (n, 2))
    a0 = r.uniform(0, 2 * np.pi, n); da = r.uniform(-0.2, 0.2, (n, T))
    pos = p0[:, None] + v[:, None] * np.arange(T)[None, :, None]
    ang = a0[:, None] + np.cumsum(da, 1)
    traj = np.concatenate([pos, np.cos(ang)[..., None], np.sin(ang)[..., None]], -1).astype(np.float32)
    return traj, np.stack([L, W], 1).astype(np.float32)      # (n,T,4) unnormalised, (n,2) length/width


# (n, origin) -> (undecided margin m, seed, colliding ordered slots over the 12 fine steps); buffer 0.3, one scene of n agents
RECIPE_ROWS = {
    (2, 0): (1e-4, 3, 16),
    (16, 0): (1e-4, 1, 576),
    (17, 0): (1e-4, 1, 530),
    (33, 0): (1e-4, 1, 1220),
    (65, 0): (1e-4, 3, 2646),
    (16, 2000): (4e-3, 7, 340),
    (17, 2000): (4e-3, 63, 362),
}
RECIPE_BUFFER = 0.3


def recipe_row(n, origin, T=4):
    """(traj (n,T,4), lw (n,2), ptr, margin) of one row of RECIPE_ROWS as torch tensors"""
    m, seed, _ = RECIPE_ROWS[(n, origin)]
    traj, lw = recipe(n, seed, float(origin), T)
    return torch.from_numpy(traj), torch.from_numpy(lw), torch.tensor([0, n], dtype=torch.long), m


def ragged(sizes, seeds, T=4, origin=0.0):
    """scenes concatenated: scene b from recipe(sizes[b], seeds[b]) shifted by 400 * b metres in x"""
    trajs, lws = [], []
    for b, (n, s) in enumerate(zip(sizes, seeds)):
        tr, lw = recipe(n, s, origin, T)
        tr = tr.astype(np.float64)
        tr[:, :, 0] += 400.0 * b
        trajs.append(tr.astype(np.float32))
        lws.append(lw)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.long)
    return torch.from_numpy(np.concatenate(trajs)), torch.from_numpy(np.concatenate(lws)), ptr


# seeds of the ragged batches (margin 1e-4, buffer 0.3): every scene reuses the seed of its row where one exists
RAGGED = {
    'r_1_17_2': ([1, 17, 2], [5, 1, 3]),
    'r_16_16': ([16, 16], [1, 7]),
}


def veh_constants(lw):
    """(cent_x (NA,5), rad (NA,)) in fp32 exactly as the product forms them (losses/adv_gen_nusc.py VehCollLoss)"""
    from strive_amd.losses.adv_gen_nusc import _linspace5
    lw = lw.float()
    rad = (lw[:, 1] / 2.).contiguous()
    cent = _linspace5(-(lw[:, 0] / 2.) + rad, (lw[:, 0] / 2.) - rad).contiguous()
    return cent, rad


def env_pdist(lw):
    """fp32 penalty distances of the environment term as the product forms them (EnvCollLoss)"""
    lw = lw.float()
    return torch.sqrt((lw[:, 0] ** 2 / 4.0) + (lw[:, 1] ** 2 / 4.0))


# ------------------------------------------------------------------------------------------------
# pieces
# ------------------------------------------------------------------------------------------------

def safe_norm(v):
    """|v| over the last dim in float64 with gradient 0 (not NaN) at v = 0"""
    d2 = (v * v).sum(-1)
    pos = d2 > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))


def interp_traj(traj, scale=3):
    """F.interpolate(mode='linear') by ``scale`` with the heading renormalised, in the dtype of ``traj`` (float64 here); the oracle's
    function is dtype-generic"""
    return olosses.interp_traj(traj, scale)


def slot_agents(ptr):
    """(slot_i, slot_j): agents of every ordered in-scene slot, slot = pair_off[i] + (j - ptr[scene(i)])"""
    si, sj = [], []
    p = [int(v) for v in ptr]
    for b in range(len(p) - 1):
        n = p[b + 1] - p[b]
        ii = np.repeat(np.arange(n), n) + p[b]
        jj = np.tile(np.arange(n), n) + p[b]
        si.append(ii)
        sj.append(jj)
    if not si:
        return torch.zeros((0,), dtype=torch.long), torch.zeros((0,), dtype=torch.long)
    return torch.from_numpy(np.concatenate(si)), torch.from_numpy(np.concatenate(sj))


class VehRef(object):
    """pen (T,P) float64 (differentiable w.r.t. the ``fine`` it was built from), hit (T,P) bool (i != j and dmin <= pd), amin (T,P)
    first index among the exact minima of the 25 distances, dmin, gap (second smallest minus smallest), pd (P,) float64 of the fp32
    value the kernel forms, slot_i / slot_j (P,)"""


def veh_ref(fine, cent_x, rad, buffer, ptr):
    """fine (NA,TO,4): float64 tensor (may require grad) holding fp32 values; cent_x (NA,5), rad (NA,) fp32"""
    out = VehRef()
    si, sj = slot_agents(ptr)
    out.slot_i, out.slot_j = si, sj
    TO = fine.shape[1]
    pd32 = (rad.float()[si] + rad.float()[sj]) + torch.tensor(buffer, dtype=torch.float32)     # fp32((r_i + r_j) + buffer)
    out.pd = pd32.double()
    c = cent_x.double()
    cen = fine[:, :, None, :2] + fine[:, :, None, 2:4] * c[:, None, :, None]                   # (NA,TO,5,2)
    pens, amins, dmins, gaps = [], [], [], []
    p = [int(v) for v in ptr]
    for b in range(len(p) - 1):
        lo, hi = p[b], p[b + 1]
        n = hi - lo
        if n == 0:
            continue
        cb = cen[lo:hi].transpose(0, 1)                                                          # (TO,n,5,2)
        diff = cb[:, :, None, :, None, :] - cb[:, None, :, None, :, :]                            # (TO,n,n,5,5,2)
        d = safe_norm(diff).reshape(TO, n * n, NCIRC * NCIRC)
        dn = d.detach().numpy()
        am = np.argmin(dn, axis=-1)                                                              # first index among the exact minima
        srt = np.sort(dn, axis=-1)
        amt = torch.from_numpy(am)
        dm = torch.gather(d, 2, amt.unsqueeze(-1)).squeeze(-1)
        pens.append(dm)
        amins.append(amt)
        gaps.append(torch.from_numpy(srt[..., 1] - srt[..., 0]))
    if pens:
        dmin = torch.cat(pens, 1)
        out.amin = torch.cat(amins, 1)
        out.gap = torch.cat(gaps, 1)
    else:
        dmin = torch.zeros((TO, 0), dtype=torch.float64)
        out.amin = torch.zeros((TO, 0), dtype=torch.long)
        out.gap = torch.zeros((TO, 0), dtype=torch.float64)
    out.dmin = dmin
    out.pen = 1.0 - dmin / out.pd.view(1, -1)
    out.hit = (dmin.detach() <= out.pd.view(1, -1)) & (si != sj).view(1, -1)               # (NaN compares false)
    return out


def veh_undecided(vr, m):
    """(#hit-undecided, #argmin-undecided) slots of a VehRef at margin m"""
    off = (vr.slot_i != vr.slot_j).view(1, -1)
    dm = vr.dmin.detach()
    und_hit = ((dm - vr.pd.view(1, -1)).abs() < m) & off
    und_arg = vr.hit & (vr.gap < m)
    return int(und_hit.sum()), int(und_arg.sum())


def pair_valid(ptr, single_veh_idx=None):
    si, sj = slot_agents(ptr)
    v = si != sj
    if single_veh_idx is not None:
        NA = int(ptr[-1])
        sel = torch.zeros((NA,), dtype=torch.bool)
        sel[ptr[:-1] + single_veh_idx] = True
        v = v & (sel[si] | sel[sj])
    return v


def masked_mean(v, m):
    cnt = int(m.sum())
    return (torch.where(m, v, torch.zeros_like(v)).sum() / max(cnt, 1)), cnt


def env_ref(fine, env_agent, pt, pdist, row_alive=None):
    """penalties 1 - |c - p| / r of the rows (e, t) with a collision point; pt (NE*TO,2) fp32 DATA (NaN = none); -> (pen (NE*TO,),
    valid (NE*TO,))"""
    NE = len(env_agent)
    TO = fine.shape[1]
    p = pt.double().view(NE, TO, 2)
    valid = ~torch.isnan(p.sum(-1))
    if row_alive is not None:
        valid = valid & row_alive.view(-1, 1)
    c = fine[env_agent][:, :, :2]
    d = safe_norm(c - torch.where(valid.unsqueeze(-1), p, torch.zeros_like(p)))
    pen = 1.0 - d / pdist.double().view(NE, 1)
    return pen.reshape(-1), valid.reshape(-1)


def prior_nll_rows(z, mu, var):
    """-log N(z; mu, var) summed over the latent dim"""
    return (torch.log(torch.sqrt(var)) + 0.5 * math.log(2.0 * math.pi) + (z - mu) ** 2 / (2.0 * var)).sum(-1)


# ------------------------------------------------------------------------------------------------
# objectives
# ------------------------------------------------------------------------------------------------

def avoid_ref(w, traj, lw, ptr, buffer, z, mu, var, init_z, pt=None, env_agent=None, single_veh_idx=None):
    """AvoidCollLoss as oracle/losses.py composes it, in float64 on fp32 inputs.  ``pt``: the collision points of the env rows on
    the product's fine trajectory, as data.  z (NZ,D) or (NZ,1,D).  Returns a dict of float64 scalars / counts and the
    gradients d_traj, d_z."""
    tr = traj.double().clone().requires_grad_(True)
    zz = z.double().clone().requires_grad_(True)
    cent, rad = veh_constants(lw)
    fine = interp_traj(tr, 3)
    res = {'VEH': 0.0, 'VEH_N': 0, 'ENV': 0.0, 'ENV_N': 0, 'PRIOR': 0.0, 'INIT': 0.0}
    loss = torch.zeros((), dtype=torch.float64)
    if w['coll_veh'] > 0.0:
        vr = veh_ref(fine, cent, rad, buffer, ptr)
        mean, cnt = masked_mean(vr.pen, vr.hit & pair_valid(ptr, single_veh_idx).view(1, -1))
        loss = loss + w['coll_veh'] * mean
        res['VEH'], res['VEH_N'], res['veh'] = float(mean.detach()), cnt, vr
    if w['coll_env'] > 0.0:
        NA = traj.shape[0]
        ea = torch.arange(NA) if env_agent is None else env_agent.long()
        pen, valid = env_ref(fine, ea, pt, env_pdist(lw)[ea])
        mean, cnt = masked_mean(pen, valid)
        loss = loss + w['coll_env'] * mean
        res['ENV'], res['ENV_N'] = float(mean.detach()), cnt
    if w['motion_prior'] > 0.0:
        m_, v_ = mu.double(), var.double()
        if zz.dim() == 3:
            m_, v_ = m_.unsqueeze(1), v_.unsqueeze(1)
        p = prior_nll_rows(zz, m_, v_).mean()
        loss = loss + w['motion_prior'] * p
        res['PRIOR'] = float(p.detach())
    if w['init_z'] > 0.0:
        i = torch.sum((init_z.double() - zz) ** 2, dim=1).mean()         # (singleton form: dim 1 has one entry, the mean is over B*D)
        loss = loss + w['init_z'] * i
        res['INIT'] = float(i.detach())
    res['LOSS'] = float(loss.detach())
    if loss.requires_grad:
        loss.backward()
    res['d_traj'] = tr.grad if tr.grad is not None else torch.zeros_like(tr)
    res['d_z'] = zz.grad if zz.grad is not None else torch.zeros_like(zz)
    return res


def adv_ref(w, traj, tgt, lw, ptr, buffer, z, mu, var, init_z, t0=0, infront=None, attack_agt_idx=None, pt=None):
    """AdvGenLoss as oracle/losses.py composes it, in float64 on fp32 inputs (agent 0 of every scene is the ego; one latent row
    per non-ego agent).  Reports soft (NE,NT), rew, sel, min_agt / min_t, dots (for the behind precondition), every term and count
    and the gradients."""
    tr = traj.double().clone().requires_grad_(True)
    tg = tgt.double().clone().requires_grad_(True)
    zz = z.double().clone().requires_grad_(True)
    p = [int(v) for v in ptr]
    B, NA = len(p) - 1, p[-1]
    ego = torch.zeros((NA,), dtype=torch.bool)
    ego[ptr[:-1]] = True
    ne_idx = torch.nonzero(~ego).flatten()
    NE = ne_idx.numel()
    seg = torch.repeat_interleave(torch.arange(B), (ptr[1:] - ptr[:-1]) - 1)
    ne_ptr = [p[b] - b for b in range(B + 1)]
    T = traj.shape[1]
    NT = T - t0
    res = {}
    # crash term
    atk = tr[ne_idx][:, t0:, :2]
    tge = tg[seg][:, t0:]
    dvec = atk - tge[:, :, :2]
    dist = safe_norm(dvec)
    masked = torch.zeros((NE, NT), dtype=torch.bool)
    sel = 0
    res['dots'] = None
    if infront is not None:
        dd, dn = dvec.detach(), dist.detach()
        dots = (dd / dn.unsqueeze(-1) * tge[:, :, 2:4].detach()).sum(-1)          # NaN at d = 0: not behind
        behind = dots < infront
        always = behind.all(dim=1, keepdim=True).expand(NE, NT)
        if bool(always.all()):
            sel = 1
            always = torch.zeros_like(always)
        masked = masked | always
        res['dots'] = dots
    if attack_agt_idx is not None:
        am = torch.zeros((NA,), dtype=torch.bool)
        am[attack_agt_idx] = True
        masked = masked | ~am[ne_idx].view(-1, 1)
    soft = torch.zeros((NE, NT), dtype=torch.float64)
    crash = []
    min_agt, min_t, top2 = [], [], []
    for b in range(B):
        a0, a1 = ne_ptr[b], ne_ptr[b + 1]
        d = dist[a0:a1].reshape(-1)
        mk = masked[a0:a1].reshape(-1)
        if d.numel() == 0 or bool(mk.all()):
            s = torch.zeros_like(d)
        else:
            mx = (-d.detach()[~mk]).max()
            e = torch.where(mk, torch.zeros_like(d), torch.exp(torch.where(mk, torch.zeros_like(d), -d - mx)))
            s = e / e.sum()
        crash.append((s * d ** 2).sum())
        if d.numel():
            sd = s.detach()
            k = int(np.argmax(sd.numpy()))
            min_agt.append(k // NT + 1)
            min_t.append(k % NT + t0)
            srt = np.sort(sd.numpy())[::-1]
            top2.append((float(srt[0]), float(srt[1]) if srt.size > 1 else 0.0))
        else:
            min_agt.append(None); min_t.append(None); top2.append((0.0, 0.0))
        soft[a0:a1] = s.detach().view(-1, NT)
    crash = torch.stack(crash) if crash else torch.zeros((0,), dtype=torch.float64)
    rew = 1.0 - soft.detach().sum(1)
    res.update(soft=soft.detach(), rew=rew, sel=sel, min_agt=min_agt, min_t=min_t, top2=top2, crash_scene=crash.detach())
    cent, rad = veh_constants(lw)
    fine = interp_traj(tr, 3)
    loss = torch.zeros((), dtype=torch.float64)
    res.update(VEH=0.0, VEH_N=0, PLAN=0.0, PLAN_N=0, ENV=0.0, ENV_N=0, PRIOR=0.0, INIT=0.0, CRASH=0.0)
    if w.get('init_z', 0.0) > 0.0:
        coeff = rew * w['init_z'] + (1.0 - rew) * w['init_z_atk']
        i = (((init_z.double() - zz) ** 2).sum(1) * coeff).sum()
        loss = loss + i
        res['INIT'] = float(i.detach())
    if w.get('motion_prior', 0.0) > 0.0:
        coeff = rew * w['motion_prior'] + (1.0 - rew) * w['motion_prior_atk']
        pr = (prior_nll_rows(zz, mu.double(), var.double()) * coeff).mean() if NE else torch.zeros((), dtype=torch.float64)
        loss = loss + pr
        res['PRIOR'] = float(pr.detach())
    if w.get('coll_veh', 0.0) > 0.0 or w.get('coll_veh_plan', 0.0) > 0.0:
        vr = veh_ref(fine, cent, rad, buffer, ptr)
        res['veh'] = vr
        si, sj = vr.slot_i, vr.slot_j
        valid = (si != sj).view(1, -1)
        with_ego = (ego[si] | ego[sj]).view(1, -1)
        if w.get('coll_veh', 0.0) > 0.0:
            mean, cnt = masked_mean(vr.pen, vr.hit & valid & ~with_ego)
            loss = loss + w['coll_veh'] * mean
            res['VEH'], res['VEH_N'] = float(mean.detach()), cnt
        if w.get('coll_veh_plan', 0.0) > 0.0:
            ne_row = torch.cumsum((~ego).long(), 0) - 1
            other = torch.where(ego[si], sj, si)                        # the non-ego member of an ego-involving slot
            pw = torch.where(ego[other], torch.ones((), dtype=torch.float64), rew[ne_row[other].clamp(min=0)]) if NE else \
                torch.ones((si.numel(),), dtype=torch.float64)
            mean, cnt = masked_mean(vr.pen * pw.view(1, -1), vr.hit & valid & with_ego)
            loss = loss + w['coll_veh_plan'] * mean
            res['PLAN'], res['PLAN_N'] = float(mean.detach()), cnt
    if w.get('coll_env', 0.0) > 0.0 and NE:
        pen, valid = env_ref(fine, ne_idx, pt, env_pdist(lw)[ne_idx])
        mean, cnt = masked_mean(pen, valid)
        loss = loss + w['coll_env'] * mean
        res['ENV'], res['ENV_N'] = float(mean.detach()), cnt
    if w.get('adv_crash', 0.0) > 0.0 and B:
        cm = crash.mean()
        loss = loss + w['adv_crash'] * cm
        res['CRASH'] = float(cm.detach())
    res['LOSS'] = float(loss.detach())
    if loss.requires_grad:
        loss.backward()
    for k, t in (('d_traj', tr), ('d_tgt', tg), ('d_z', zz)):
        res[k] = t.grad if t.grad is not None else torch.zeros_like(t)
    return res


# ------------------------------------------------------------------------------------------------
# tolerance scheme
# ------------------------------------------------------------------------------------------------

def _f64(a):
    if torch.is_tensor(a):
        return a.detach().cpu().double().numpy()
    return np.asarray(a, dtype=np.float64)


def bound(ref, orc32):
    """max(e32, floor): e32 = largest |oracle fp32 - reference|, floor = 2^-23 * max|reference|"""
    r, o = _f64(ref), _f64(orc32)
    assert r.shape == o.shape, 'oracle %s vs reference %s' % (o.shape, r.shape)
    e32 = float(np.max(np.abs(r - o))) if r.size else 0.0
    floor = EPS32 * (float(np.max(np.abs(r))) if r.size else 0.0)
    return max(e32, floor)


RATIOS = []          # (case, backend, quantity, ratio) of every check_ratio call of the process


def check_ratio(case, backend, what, got, ref, orc32, mask=None):
    """assert |got - ref| <= K_TOL * max(e32, floor), record the ratio"""
    g, r, o = _f64(got), _f64(ref), _f64(orc32)
    if mask is not None:
        mk = _f64(mask).astype(bool)
        g, r, o = g[mk], r[mk], o[mk]
    assert g.shape == r.shape, '%s: got %s, reference %s' % (what, g.shape, r.shape)
    assert np.all(np.isfinite(g)), '%s %s: non-finite values from the kernel' % (case, what)
    b = bound(r, o)
    err = float(np.max(np.abs(g - r))) if r.size else 0.0
    ratio = err / b if b > 0.0 else (0.0 if err == 0.0 else float('inf'))
    RATIOS.append((case, backend, what, ratio))
    print('RATIO %s | %s | %s | err %.3e | bound %.3e | ratio %.3f' % (case, backend, what, err, b, ratio))
    assert ratio <= K_TOL, '%s %s [%s]: kernel error %.3e is %.1f x max(e32, floor) = %.3e (limit %g)' % (case, what, backend, err, ratio, b, K_TOL)
    return ratio
