"""The kernels of strive_amd/csrc/losses.hip at their edges against the float64 reference of tests/loss_ref.py.

Every case runs through one body twice: on the host emulation (tests/hipemu, ``ops._lib_for`` patched, scratch and torch.empty
poisoned) and on the MI355X with the product's library (marked gpu).

Tolerance: for every compared quantity q, |kernel - reference| <= 16 * max(e32, 2^-23 * max|reference|), e32 = the largest
difference between oracle/losses.py run in fp32 and the reference on the same inputs (16 is the factor tests/test_map_cnn_layers.py
uses for fp32 steps against torch fp32's own error).  Counts, hit, amin, sel, min_agt, min_t and everything called exact are
compared for equality.  Decisions are unambiguous by construction: every case first asserts ON THE REFERENCE ALONE that no slot
is "undecided" (|dmin - pd| < m, or colliding with its second-smallest distance within m of the smallest; no behind-test dot
within 1e-3 of its threshold); the seeds that meet this are recorded in loss_ref.py.  Every check prints a ``RATIO`` line (run
with -s); the observed ratios are in profiles/r22_loss_edge_ratios.md.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from util import poisoned_workspace, nan_empty
from strive_amd import _lib as L, synth
from oracle import losses as olosses

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

AO = dict(LOSS=0, VEH=1, ENV=2, PRIOR=3, INIT=4, VEH_N=5, ENV_N=6)
DO = dict(LOSS=0, VEH=1, PLAN=2, ENV=3, PRIOR=4, INIT=5, CRASH=6, VEH_N=7, PLAN_N=8, ENV_N=9, SEL=10)


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


def on_both(*cases, slow=()):
    """parametrize (case, backend): every case on the emulation and, marked gpu, on the MI355X; ``slow`` = ids of the cases that
    take too long on the emulation for the default set"""
    ps = []
    for c in cases:
        cid = '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)
        ps.append(pytest.param(c, 'emu', id=cid + '-emu', marks=[pytest.mark.slow] if cid in slow else []))
        ps.append(pytest.param(c, 'gpu', id=cid + '-gpu', marks=pytest.mark.gpu))
    return pytest.mark.parametrize('case,backend', ps)


class Backend(object):
    """library + device of one run; direct calls of the vehicle-penalty kernels (amin is not visible through the Python API)"""

    def __init__(self, backend, request, monkeypatch):
        from strive_amd import ops
        self.name, self.ops = backend, ops
        if backend == 'emu':
            self.lib = request.getfixturevalue('emu')
            self.dev = 'cpu'
            lib = self.lib
            monkeypatch.setattr(ops, '_lib_for', lambda *tensors: lib)
            monkeypatch.setattr(ops, '_ws_cache', {})                           # fresh scratch buffers ...
            monkeypatch.setattr(ops, '_workspace', poisoned_workspace(ops))    # ... that start as NaN bytes
            monkeypatch.setattr(torch, 'empty', nan_empty())                   # and so does everything allocated uninitialised
        else:
            assert torch.cuda.is_available(), 'gpu cases need the MI355X'
            self.lib = L.get_lib()
            self.dev = 'cuda:0'

    def veh_setup(self, lw, ptr):
        cent, rad = R.veh_constants(lw)
        info = self.ops.SceneInfo(ptr, self.dev)
        return info, info.pack(1), cent.to(self.dev), rad.to(self.dev)

    def veh_fwd(self, fine, lw, ptr, buffer):
        """strive_veh_coll_fwd (cull = 0) on a fine-level trajectory (device tensor) -> pen, hit, amin (TO,P)"""
        info, sc, cent, rad = self.veh_setup(lw, ptr)
        TO = fine.shape[1]
        pen = torch.full((TO, info.P), float('nan'), device=self.dev)
        hit = torch.full((TO, info.P), 0xFF, dtype=torch.uint8, device=self.dev)
        amin = torch.full((TO, info.P), 0xFF, dtype=torch.uint8, device=self.dev)
        self.lib.call('strive_veh_coll_fwd', sc.ref(), L.ptr(info.pair_off), info.P, L.ptr(fine), TO, L.ptr(cent), L.ptr(rad),
                      C.c_float(buffer), L.ptr(pen), L.ptr(hit), L.ptr(amin), L.stream_ptr(fine))
        return pen, hit, amin

    def veh_bwd(self, fine, lw, ptr, buffer, d_pen, amin):
        info, sc, cent, rad = self.veh_setup(lw, ptr)
        d_fine = torch.zeros_like(fine)
        self.lib.call('strive_veh_coll_bwd', sc.ref(), L.ptr(info.pair_off), info.P, L.ptr(fine), fine.shape[1], L.ptr(cent),
                      L.ptr(rad), C.c_float(buffer), L.ptr(d_pen.contiguous()), L.ptr(amin), L.ptr(d_fine), L.stream_ptr(fine))
        return d_fine


def flat_env(H=64):
    raster = torch.zeros((1, 4, H, H), dtype=torch.uint8)
    raster[:, 0] = 1
    return synth.SyntheticMapEnv(raster, torch.tensor([[0.25, 0.25]], dtype=torch.float64))


def textured_env(M=1):
    raster, dx = synth.make_raster(1024, 1024, M=M)
    return synth.SyntheticMapEnv(raster, dx)


def dev_env(env, dev):
    return synth.SyntheticMapEnv(env.nusc_raster.clone(), env.nusc_dx.clone()).to(dev)


class given_coll_points(object):
    """oracle/losses.py takes its collision points from oracle.mapenv; inside this context it takes ``pt`` instead -- the points
    the product computed on its own fine trajectory, as data (the collision-point kernel has its own tests)"""

    def __init__(self, pt):
        self.pt = None if pt is None else pt.detach().cpu().float()

    def __enter__(self):
        self.orig = olosses.coll_point
        if self.pt is not None:
            olosses.coll_point = lambda raster, dx, flat, att, mix: self.pt.clone()
        return self

    def __exit__(self, *exc):
        olosses.coll_point = self.orig
        return False


def latents(n, D, key):
    z = synth.f32(synth.counter_uniform((n, D), key + '/z', -1.0, 1.0))
    mu = synth.f32(synth.counter_uniform((n, D), key + '/m', -0.5, 0.5))
    var = synth.f32(synth.counter_uniform((n, D), key + '/v', 0.3, 2.0))
    init = synth.f32(synth.counter_uniform((n, D), key + '/i', -1.0, 1.0))
    return z, mu, var, init


def assert_decided(vr, m, what):
    uh, ua = R.veh_undecided(vr, m)
    assert uh == 0 and ua == 0, '%s: precondition on the REFERENCE: %d hit-undecided and %d argmin-undecided slots at margin %g ' \
        '(not a kernel failure: pick another seed)' % (what, uh, ua, m)


def veh_case(case):
    """(traj (n,T,4), lw, ptr, margin) of a recipe row (n, origin) or of a ragged batch"""
    if isinstance(case, str):
        sizes, seeds = R.RAGGED[case]
        traj, lw, ptr = R.ragged(sizes, seeds)
        return traj, lw, ptr, 1e-4
    return R.recipe_row(*case)


def oracle_veh32(fine32, lw, ptr, buffer, d_pen):
    """oracle VehColl in fp32 -> pen (T,P) in slot layout, its gradient for d_pen"""
    si, sj = R.slot_agents(ptr)
    tc = fine32.clone().requires_grad_(True)
    dense, _ = olosses.VehColl(lw, ptr=ptr, buffer_dist=buffer)(tc, return_raw=True)
    pen = dense[:, si, sj]
    (pen * d_pen).sum().backward()
    return pen.detach(), tc.grad


# ================================================================================================
# A. strive_veh_coll_fwd / bwd alone
# ================================================================================================

ROWS = [(2, 0), (16, 0), (17, 0), (33, 0), (65, 0), (16, 2000), (17, 2000), 'r_1_17_2', 'r_16_16']


@on_both(*ROWS)
def test_a_veh_coll_against_float64(case, backend, request, monkeypatch):
    """pen behind hit, hit and amin (exact), d_traj for a counter-generated d_pen: one pass of the VG = 16 lanes (2, 16), two and
    more with a partial last one (17, 33, 65), ragged scenes with a singleton, coordinates of 2000 m"""
    be = Backend(backend, request, monkeypatch)
    traj, lw, ptr, m = veh_case(case)
    with torch.no_grad():
        fine32 = olosses.interp_traj(traj, 3).contiguous()
    buf = R.RECIPE_BUFFER
    cent, rad = R.veh_constants(lw)
    f64 = fine32.double().requires_grad_(True)
    vr = R.veh_ref(f64, cent, rad, buf, ptr)
    assert_decided(vr, m, str(case))
    if not isinstance(case, str):
        assert int(vr.hit.sum()) == R.RECIPE_ROWS[case][2]
    TO, P = vr.hit.shape
    d_pen = synth.f32(synth.counter_uniform((TO, P), 'edges/a/%s' % (case,), 0.1, 1.0)) * vr.hit
    (vr.pen * d_pen.double()).sum().backward()
    open32, og32 = oracle_veh32(fine32, lw, ptr, buf, d_pen)
    fd = fine32.to(be.dev)
    pen, hit, amin = be.veh_fwd(fd, lw, ptr, buf)
    assert torch.equal(hit.cpu().bool(), vr.hit) and int(hit.max()) <= 1, 'hit differs from the reference'
    assert torch.equal(amin.cpu().long()[vr.hit], vr.amin[vr.hit]), 'amin differs from the reference'
    tag = 'A %s' % (case,)
    R.check_ratio(tag, backend, 'pen', pen.cpu(), vr.pen, open32, mask=vr.hit)
    d_fine = be.veh_bwd(fd, lw, ptr, buf, d_pen.to(be.dev), amin)
    R.check_ratio(tag, backend, 'd_traj', d_fine.cpu(), f64.grad, og32)
    if case == 'r_1_17_2':
        assert float(d_fine[0].abs().max()) == 0.0, 'the singleton scene has no slot besides itself'


# ================================================================================================
# B. exact geometry
# ================================================================================================

def _exact_scenes():
    """two-agent scenes, L = 5, W = 2 (cent_x = -1.5 .. 1.5), one fine step; every product of the arithmetic is exact in fp32"""
    up = float(np.nextafter(np.float32(2.5), np.float32(np.inf)))
    poses = {
        'side': ((0, 0, 1, 0), (0, 2.5, 1, 0)),
        'side_off': ((0, 0, 1, 0), (0, up, 1, 0)),
        'nose_tail': ((0, 0, 1, 0), (5.25, 0, 1, 0)),
        'coincident': ((1, 2, 1, 0), (1, 2, 1, 0)),
        't_bone': ((0, 0, 1, 0), (3.0, 0.25, 0, 1)),
    }
    names = list(poses)
    fine = torch.tensor([p for k in names for p in poses[k]], dtype=torch.float32).view(-1, 1, 4)
    lw = torch.tensor([[5.0, 2.0]] * (2 * len(names)))
    ptr = torch.arange(0, 2 * len(names) + 1, 2)
    return names, fine, lw, ptr


@on_both('exact')
def test_b_exact_geometry(case, backend, request, monkeypatch):
    be = Backend(backend, request, monkeypatch)
    names, fine, lw, ptr = _exact_scenes()
    buf = 0.5
    cent, rad = R.veh_constants(lw)
    assert cent[0].tolist() == [-1.5, -0.75, 0.0, 0.75, 1.5]
    f64 = fine.double().requires_grad_(True)
    vr = R.veh_ref(f64, cent, rad, buf, ptr)
    assert float(vr.pd[1]) == 2.5
    fd = fine.to(be.dev)
    pen, hit, amin = be.veh_fwd(fd, lw, ptr, buf)
    pen, hit, amin = pen.cpu()[0], hit.cpu()[0], amin.cpu()[0]
    s = {k: 4 * i for i, k in enumerate(names)}              # slots of scene k: s+1 = (first, second), s+2 = (second, first)
    assert torch.equal(hit.bool(), vr.hit[0]) and torch.equal(amin.long()[vr.hit[0]], vr.amin[0][vr.hit[0]])
    # side by side: five tied minima -> first index; dmin == pd exactly -> colliding, penalty exactly 0
    assert int(vr.amin[0, s['side'] + 1]) == 0
    assert hit[s['side'] + 1] == 1 and amin[s['side'] + 1] == 0 and hit[s['side'] + 2] == 1 and amin[s['side'] + 2] == 0
    assert float(pen[s['side'] + 1]) == 0.0
    assert hit[s['side_off'] + 1] == 0 and hit[s['side_off'] + 2] == 0, 'one ulp past the penalty distance must not collide'
    # nose to tail: one minimum, circle 4 of the first against circle 0 of the second
    assert hit[s['nose_tail'] + 1] == 1 and amin[s['nose_tail'] + 1] == 20 and amin[s['nose_tail'] + 2] == 4
    assert float(pen[s['nose_tail'] + 1]) == float(np.float32(1.0) - np.float32(2.25) / np.float32(2.5))
    # coincident
    assert hit[s['coincident'] + 1] == 1 and amin[s['coincident'] + 1] == 0 and float(pen[s['coincident'] + 1]) == 1.0
    assert hit[s['t_bone'] + 1] == 1 and int(amin[s['t_bone'] + 1]) == int(vr.amin[0, s['t_bone'] + 1]) == 22
    R.check_ratio('B exact', backend, 'pen', pen, vr.pen[0], vr.pen[0].detach(), mask=vr.hit[0])
    # gradient of the (first, second) slots only: the lever arm is that of the chosen circle pair
    d_pen = torch.zeros((1, vr.hit.shape[1]))
    for k in names:
        d_pen[0, s[k] + 1] = 1.0
    d_pen = d_pen * vr.hit
    (vr.pen * d_pen.double()).sum().backward()
    g = be.veh_bwd(fd, lw, ptr, buf, d_pen.to(be.dev), be.veh_fwd(fd, lw, ptr, buf)[2]).cpu()[:, 0]
    assert bool(torch.isfinite(g).all())
    R.check_ratio('B exact', backend, 'd_traj', g, f64.grad[:, 0], f64.grad[:, 0])
    a, b = 2 * names.index('side'), 2 * names.index('side') + 1
    assert float(g[a, 0]) == 0.0 and float(g[a, 2]) == 0.0 and float(g[a, 1]) > 0.0
    assert float(g[a, 3]) == float(np.float32(g[a, 1].item()) * np.float32(-1.5)), 'circle pair (0, 0): lever arm cent_x[0]'
    assert float(g[b, 3]) == float(np.float32(g[b, 1].item()) * np.float32(-1.5)) and float(g[b, 1]) == -float(g[a, 1])
    c = 2 * names.index('coincident')
    assert float(g[c:c + 2].abs().max()) == 0.0, 'd = 0: the gradient is exactly zero'
    c = 2 * names.index('side_off')
    assert float(g[c:c + 2].abs().max()) == 0.0


@on_both('nan_pose')
def test_b_nan_pose_equals_the_agent_moved_away(case, backend, request, monkeypatch):
    """a NaN pose of one agent at one fine step: no slot of that agent at that step collides; everything else is bit-identical to
    the same call with the agent 1 km away"""
    be = Backend(backend, request, monkeypatch)
    traj, lw, ptr, m = R.recipe_row(17, 0)
    with torch.no_grad():
        fine = olosses.interp_traj(traj, 3).contiguous()
    ag, t = 5, 4
    f_nan, f_far = fine.clone(), fine.clone()
    f_nan[ag, t] = float('nan')
    f_far[ag, t, 0] += 1000.0
    buf = R.RECIPE_BUFFER
    si, sj = R.slot_agents(ptr)
    touched = (si == ag) | (sj == ag)
    res = []
    for f in (f_nan, f_far):
        fd = f.to(be.dev)
        pen, hit, amin = be.veh_fwd(fd, lw, ptr, buf)
        res.append((fd, pen, hit, amin))
    hit_n, hit_f = res[0][2].cpu(), res[1][2].cpu()
    assert int(hit_n[t][touched].sum()) == 0 and int(hit_f[t][touched].sum()) == 0
    assert torch.equal(hit_n, hit_f) and int(hit_n.sum()) > 100
    hb = hit_n.bool()
    assert torch.equal(res[0][1].cpu()[hb], res[1][1].cpu()[hb]) and torch.equal(res[0][3].cpu()[hb], res[1][3].cpu()[hb])
    d_pen = synth.f32(synth.counter_uniform(tuple(hb.shape), 'edges/b/nan', 0.1, 1.0)) * hb
    g = [be.veh_bwd(fd, lw, ptr, buf, d_pen.to(be.dev), amin).cpu() for fd, _, _, amin in res]
    assert bool(torch.isfinite(g[0]).all()) and torch.equal(g[0], g[1])
    assert float(g[0][ag, t].abs().max()) == 0.0


# ================================================================================================
# fused AvoidCollLoss: helper
# ================================================================================================

def run_avoid(be, w, traj, lw, ptr, buffer, env, mapix, z, mu, var, init, single=None, all_pairs=False):
    """the fused call through the product's module -> (out (8,) cpu, d_traj, d_z, module)"""
    from strive_amd.losses.adv_gen_nusc import AvoidCollLoss
    dev = be.dev
    kw = dict(veh_coll_buffer=buffer)
    if not all_pairs:
        kw['ptr'] = ptr
    if single is not None:
        kw['single_veh_idx'] = single
    fn = AvoidCollLoss(w, lw.to(dev), mapix.to(dev), dev_env(env, dev), init.to(dev), **kw)
    tr = traj.clone().to(dev).requires_grad_(True)
    zz = z.clone().to(dev).requires_grad_(True)
    loss, out = be.ops.avoid_coll_loss(tr, zz, mu.to(dev), var.to(dev), fn._setup())
    loss.backward()
    assert float(loss.detach()) == float(out[0])
    d_z = zz.grad.cpu() if zz.grad is not None else torch.zeros_like(z)
    return out.cpu(), tr.grad.cpu(), d_z, fn


def oracle_avoid32(w, traj, lw, ptr, buffer, env, mapix, z, mu, var, init, pt, single=None):
    tr = traj.clone().requires_grad_(True)
    zz = z.clone().requires_grad_(True)
    with given_coll_points(pt):
        fn = olosses.AvoidColl(w, lw, mapix, env, init, veh_coll_buffer=buffer, single_veh_idx=single, ptr=ptr)
        out = fn(tr, zz, (mu, var))
    if torch.is_tensor(out['loss']) and out['loss'].requires_grad:
        out['loss'].backward()
    res = {'LOSS': float(out['loss'].detach()) if torch.is_tensor(out['loss']) else float(out['loss']), 'd_traj': tr.grad if tr.grad is not None else torch.zeros_like(tr),
           'd_z': zz.grad if zz.grad is not None else torch.zeros_like(zz)}
    for k, name in (('VEH', 'coll_veh_loss'), ('ENV', 'coll_env_loss'), ('PRIOR', 'motion_prior_loss'), ('INIT', 'init_loss')):
        res[k] = float(out[name].detach().mean()) if name in out else 0.0
    return res


def env_points(be, fn, traj, env_agent, lw):
    """the collision points of the environment rows on the product's own fine trajectory (the bits the fused call computes)"""
    dev = be.dev
    with torch.no_grad():
        fine = be.ops.interp_traj(traj.to(dev), 3)
    rows = fine[env_agent.to(dev)]
    NE, TO, _ = rows.shape
    gl, gw = fn.env_coll_loss._grid_size(NE, TO)
    att = lw[env_agent].to(dev).view(NE, 1, 2).expand(NE, TO, 2).reshape(NE * TO, 2)
    mix = fn.env_coll_loss.mapixes.view(NE, 1).expand(NE, TO).reshape(NE * TO)
    pt, _ = be.ops.coll_point(fn.env_coll_loss.map_env, rows.reshape(NE * TO, 4), att, mix, gl, gw)
    return pt.cpu()


def check_avoid(tag, be, out, d_traj, d_z, ref, orc, terms):
    for k in ('VEH_N', 'ENV_N'):
        assert float(out[AO[k]]) == float(ref[k]), '%s: count %s is %g, the reference has %d' % (tag, k, float(out[AO[k]]), ref[k])
    for k in terms + ['LOSS']:
        R.check_ratio(tag, be.name, k, out[AO[k]], ref[k], orc[k])
    R.check_ratio(tag, be.name, 'd_traj', d_traj, ref['d_traj'], orc['d_traj'])
    if 'PRIOR' in terms or 'INIT' in terms:
        R.check_ratio(tag, be.name, 'd_z', d_z.reshape(ref['d_z'].shape), ref['d_z'], orc['d_z'])
    assert bool((out[7:] == 0).all())


W_VEH = {'coll_veh': 1.5, 'coll_env': 0.0, 'motion_prior': 0.0, 'init_z': 0.0}
W_ENV = {'coll_veh': 0.0, 'coll_env': 0.75, 'motion_prior': 0.0, 'init_z': 0.0}
W_ALL = {'coll_veh': 1.5, 'coll_env': 0.75, 'motion_prior': 0.02, 'init_z': 0.3}


# ================================================================================================
# C. the cull
# ================================================================================================

MARGINS = (-4e-3, -2e-3, 2e-3, 4e-3, 0.5, 3.0)
N_ANG = 37
BOUNDARY_SEED = 11


def boundary_pairs(origin, T=4):
    """222 two-agent scenes in line along a heading: centre distance = pd + reach_i + reach_j + margin (formed in float64, poses
    rounded to fp32 once), frames constant in time"""
    r = np.random.default_rng(BOUNDARY_SEED)
    n = len(MARGINS) * N_ANG
    Ls = r.uniform(3.5, 12.0, (n, 2)).astype(np.float32)
    Ws = r.uniform(1.6, 2.9, (n, 2)).astype(np.float32)
    lw = torch.from_numpy(np.stack([Ls, Ws], -1).reshape(2 * n, 2))
    cent, rad = R.veh_constants(lw)
    reach = cent.abs().max(1)[0].double().view(n, 2)
    pd = ((rad.view(n, 2)[:, 0] + rad.view(n, 2)[:, 1]) + torch.tensor(0.3)).double()
    ang = np.tile(np.arange(N_ANG) * (2 * np.pi / N_ANG) + 0.01, len(MARGINS))
    mar = np.repeat(np.array(MARGINS), N_ANG)
    dist = pd.numpy() + reach[:, 0].numpy() + reach[:, 1].numpy() + mar
    base = origin + r.uniform(-20, 20, (n, 2))
    hx, hy = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)        # the fp32 heading the kernel gets
    nrm = np.sqrt(hx.astype(np.float64) ** 2 + hy.astype(np.float64) ** 2)
    pj = base + np.stack([hx, hy], 1) / nrm[:, None] * dist[:, None]
    poses = np.zeros((n, 2, 4))
    poses[:, 0, :2], poses[:, 1, :2] = base, pj
    poses[:, :, 2], poses[:, :, 3] = hx[:, None], hy[:, None]
    traj = torch.from_numpy(poses.reshape(2 * n, 1, 4).astype(np.float32)).expand(2 * n, T, 4).contiguous()
    return traj, lw, torch.arange(0, 2 * n + 1, 2), torch.from_numpy(mar)


@on_both(0, 2000, 3000)
def test_c_cull_boundary_pairs(case, backend, request, monkeypatch):
    """pairs within millimetres of the cull distance, and clearly past it: no colliding pair may be culled, the count is the
    reference's.  Undecided margin: 4 ulp of the coordinates (a circle-centre difference carries at most 1 ulp of each pose
    coordinate), never below 1e-4; the nominal margins are 2e-3 and more."""
    be = Backend(backend, request, monkeypatch)
    origin = float(case)
    traj, lw, ptr, mar = boundary_pairs(origin)
    m = max(1e-4, 4.0 * float(np.spacing(np.float32(origin + 40.0))))
    NA = traj.shape[0]
    z, mu, var, init = latents(NA, 4, 'edges/c')
    env, mapix = flat_env(), torch.zeros((NA,), dtype=torch.long)
    ref = R.avoid_ref(W_VEH, traj, lw, ptr, 0.3, z, mu, var, init)
    vr = ref['veh']
    uh, _ = R.veh_undecided(vr, m)
    assert uh == 0, 'precondition on the REFERENCE: %d undecided pairs at margin %g' % (uh, m)
    want_hit = (mar < 0).repeat_interleave(4).view(1, -1) & (vr.slot_i != vr.slot_j).view(1, -1)
    assert torch.equal(vr.hit, want_hit.expand_as(vr.hit)), 'the pairs with a negative margin collide, the others do not'
    orc = oracle_avoid32(W_VEH, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init, None)
    out, d_traj, d_z, _ = run_avoid(be, W_VEH, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init)
    check_avoid('C boundary %d' % case, be, out, d_traj, d_z, ref, orc, ['VEH'])


def assembled_veh_term(be, traj, lw, ptr, buffer, w_veh, valid):
    """AO_VEH_N, AO_VEH and d_traj of the vehicle term put together in the test from the product's own pieces WITHOUT the cull:
    interp_traj -> strive_veh_coll_fwd -> strive_veh_coll_bwd with d_pen = g on hit & valid, g as veh_coll_bwd_kernel<true> forms gs"""
    import math
    dev = be.dev
    tr = traj.clone().to(dev).requires_grad_(True)
    fine = be.ops.interp_traj(tr, 3)
    fd = fine.detach().contiguous()
    pen, hit, amin = be.veh_fwd(fd, lw, ptr, buffer)
    mask = hit.bool() & valid.to(dev).view(1, -1)
    cnt = int(mask.sum())
    mean = np.float32(math.fsum(pen[mask].double().cpu().tolist()) / max(cnt, 1))
    g = np.float32(1.0 * float(np.float32(w_veh)) / max(cnt, 1))              # (float)((double)d_loss * (double)w / max(c, 1))
    d_pen = mask.to(torch.float32) * float(g)
    d_fine = be.veh_bwd(fd, lw, ptr, buffer, d_pen, amin)
    fine.backward(d_fine)
    return cnt, float(mean), tr.grad.cpu()


@on_both(*ROWS, '16_16_all_pairs')
def test_c_culled_equals_unculled(case, backend, request, monkeypatch):
    """the fused call (cull = 1) against the same quantities assembled without the cull, product against product: count equal,
    mean and gradient bit-identical"""
    be = Backend(backend, request, monkeypatch)
    all_pairs = case == '16_16_all_pairs'
    traj, lw, ptr, m = veh_case('r_16_16' if all_pairs else case)
    NA = traj.shape[0]
    z, mu, var, init = latents(NA, 4, 'edges/c2')
    env, mapix = flat_env(), torch.zeros((NA,), dtype=torch.long)
    out, d_traj, _, _ = run_avoid(be, W_VEH, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init, all_pairs=all_pairs)
    use_ptr = torch.tensor([0, NA]) if all_pairs else ptr
    cnt, mean, g = assembled_veh_term(be, traj, lw, use_ptr, 0.3, W_VEH['coll_veh'], R.pair_valid(use_ptr))
    assert cnt > 0 and float(out[AO['VEH_N']]) == float(cnt)
    assert float(out[AO['VEH']]) == mean, 'mean: fused %.9g, assembled %.9g' % (float(out[AO['VEH']]), mean)
    assert torch.equal(d_traj, g), 'gradient differs in %d entries, worst %.3g' % (int((d_traj != g).sum()), float((d_traj - g).abs().max()))
    if all_pairs:
        # one scene of 32 whose halves are 400 m apart: most slots take the cull branch; the count is the two scenes' counts added
        per_scene, _, _, _ = run_avoid(be, W_VEH, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init)
        ref = R.avoid_ref(W_VEH, traj, lw, ptr, 0.3, z, mu, var, init)
        assert_decided(ref['veh'], m, case)
        assert float(out[AO['VEH_N']]) == float(per_scene[AO['VEH_N']]) == float(ref['VEH_N'])
        orc = oracle_avoid32(W_VEH, traj, lw, None, 0.3, env, mapix, z, mu, var, init, None)
        check_avoid('C all-pairs', be, out, d_traj, torch.zeros_like(z), ref, orc, ['VEH'])


# ================================================================================================
# D. loss_partial_kernel strides, latent sizes, the empty case
# ================================================================================================

@on_both((33, 4, 'veh'), (65, 32, 'all'), (17, 1, 'all'), (17, 33, 'all'), (17, 64, 'all'))
def test_d_partial_sums_and_latent_sizes(case, backend, request, monkeypatch):
    """P = 1089 (not a multiple of 256) over 7 workgroups for 60 slot chunks; 65 agents with all four weights; latent sizes 1, 33
    and 64: means, counts, d_traj and d_z"""
    be = Backend(backend, request, monkeypatch)
    n, D, which = case
    traj, lw, ptr, m = R.recipe_row(n, 0)
    w = W_VEH if which == 'veh' else W_ALL
    z, mu, var, init = latents(n, D, 'edges/d%d' % D)
    env, mapix = textured_env(), torch.zeros((n,), dtype=torch.long)
    if which == 'all':
        traj = traj.clone()
        traj[:, :, :2] += 60.0                   # onto the raster (the precondition below is asserted on the translated scene)
    out, d_traj, d_z, fn = run_avoid(be, w, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init)
    pt = env_points(be, fn, traj, torch.arange(n), lw) if w['coll_env'] > 0 else None
    ref = R.avoid_ref(w, traj, lw, ptr, 0.3, z, mu, var, init, pt=pt)
    assert_decided(ref['veh'], m, str(case))
    if which == 'all':
        assert ref['ENV_N'] > 3 and ref['VEH_N'] > 3
    orc = oracle_avoid32(w, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init, pt)
    check_avoid('D %s' % (case,), be, out, d_traj, d_z, ref, orc, ['VEH'] if which == 'veh' else ['VEH', 'ENV', 'PRIOR', 'INIT'])


@on_both('empty')
def test_d_nothing_collides(case, backend, request, monkeypatch):
    """agents 40 m apart on a uniform drivable raster: every collision mean and count exactly 0, d_traj exactly 0, the loss is the
    latent terms"""
    be = Backend(backend, request, monkeypatch)
    n, D = 16, 32
    traj, lw = R.recipe(n, 1, 0.0)
    traj = torch.from_numpy(traj).clone()
    grid = torch.stack([torch.arange(n) % 4, torch.arange(n) // 4], 1).float() * 40.0 + 50.0
    traj[:, :, :2] = grid.view(n, 1, 2) + (traj[:, :, :2] - traj[:, :1, :2]) * 0.5
    lw = torch.from_numpy(lw)
    ptr = torch.tensor([0, n])
    z, mu, var, init = latents(n, D, 'edges/d0')
    raster = torch.zeros((1, 4, 1024, 1024), dtype=torch.uint8)
    raster[:, 0] = 1
    env = synth.SyntheticMapEnv(raster, torch.tensor([[0.25, 0.25]], dtype=torch.float64))
    mapix = torch.zeros((n,), dtype=torch.long)
    out, d_traj, d_z, fn = run_avoid(be, W_ALL, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init)
    pt = env_points(be, fn, traj, torch.arange(n), lw)
    assert bool(torch.isnan(pt).all()), 'the case must have no collision point'
    ref = R.avoid_ref(W_ALL, traj, lw, ptr, 0.3, z, mu, var, init, pt=pt)
    orc = oracle_avoid32(W_ALL, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init, pt)
    assert ref['VEH_N'] == 0 and ref['ENV_N'] == 0
    for k in ('VEH', 'ENV', 'VEH_N', 'ENV_N'):
        assert float(out[AO[k]]) == 0.0
    assert float(d_traj.abs().max()) == 0.0 and bool(torch.isfinite(d_traj).all())
    want = np.float32(np.float64(np.float32(W_ALL['motion_prior'])) * np.float64(out[AO['PRIOR']]) +
                      np.float64(np.float32(W_ALL['init_z'])) * np.float64(out[AO['INIT']]))
    assert abs(float(out[AO['LOSS']]) - float(want)) <= 2.0 * float(np.spacing(np.float32(want))), 'the loss is the latent terms'
    check_avoid('D empty', be, out, d_traj, d_z, ref, orc, ['PRIOR', 'INIT'])


# ================================================================================================
# E. the environment term
# ================================================================================================

@on_both('1_4_2', '3_5_single')
def test_e_environment_term(case, backend, request, monkeypatch):
    """AO_ENV, AO_ENV_N (exact) and d_traj with only coll_env on, over a textured raster with two maps; all agents, and the
    solution loop's form (first agent of each scene only).  The collision points are data (taken from ops.coll_point on the
    product's fine trajectory), which removes the fp32-sum-against-float64-mean noise of the collision point from the comparison."""
    from test_emu_kernels import _loss_case
    be = Backend(backend, request, monkeypatch)
    single = 0 if case == '3_5_single' else None
    sizes = [3, 5] if single is not None else [1, 4, 2]
    batch, map_idx, env, traj, lw = _loss_case(sizes, 'edges/e/' + case + ('/6' if single is not None else ''))     # (a key whose first agents go off-road)
    ptr = batch.ptr
    NA, B = traj.shape[0], len(sizes)
    mapix = map_idx[batch.batch]
    NZ = B if single is not None else NA
    z, mu, var, init = latents(NZ, 8, 'edges/e')
    if single is not None:
        z, init = z.view(NZ, 1, 8), init.view(NZ, 1, 8)
    out, d_traj, d_z, fn = run_avoid(be, W_ENV, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init, single=single)
    env_agent = ptr[:-1] + single if single is not None else torch.arange(NA)
    pt = env_points(be, fn, traj, env_agent, lw)
    ref = R.avoid_ref(W_ENV, traj, lw, ptr, 0.3, z, mu, var, init, pt=pt, env_agent=env_agent, single_veh_idx=single)
    assert ref['ENV_N'] > 3, 'the case must have environment collisions'
    orc = oracle_avoid32(W_ENV, traj, lw, ptr, 0.3, env, mapix, z, mu, var, init, pt, single=single)
    check_avoid('E %s' % case, be, out, d_traj, d_z, ref, orc, ['ENV'])


# ================================================================================================
# G. interp_traj at T = 1 and T = 2
# ================================================================================================

@on_both(1, 2, 5)
def test_g_interp_traj_short(case, backend, request, monkeypatch):
    be = Backend(backend, request, monkeypatch)
    T, N = case, 9
    x = synth.f32(synth.counter_uniform((N, T, 4), 'edges/g/x%d' % T, -30.0, 30.0))
    ang = synth.counter_uniform((N, 1), 'edges/g/a%d' % T, 0.0, 6.28) + np.cumsum(synth.counter_uniform((N, T), 'edges/g/d%d' % T, -0.5, 0.5), 1)
    ang = torch.as_tensor(np.asarray(ang))          # consecutive headings at most 0.5 rad apart: never antiparallel
    x[:, :, 2], x[:, :, 3] = torch.cos(ang).float(), torch.sin(ang).float()
    d_out = synth.f32(synth.counter_normal((N, 3 * T, 4), 'edges/g/g%d' % T))
    x64 = x.double().requires_grad_(True)
    want = R.interp_traj(x64, 3)
    want.backward(d_out.double())
    x32 = x.clone().requires_grad_(True)
    o32 = olosses.interp_traj(x32, 3)
    o32.backward(d_out)
    xd = x.clone().to(be.dev).requires_grad_(True)
    got = be.ops.interp_traj(xd, 3)
    got.backward(d_out.to(be.dev))
    assert tuple(got.shape) == (N, 3 * T, 4)
    R.check_ratio('G T=%d' % T, backend, 'fine', got.detach().cpu(), want.detach(), o32.detach())
    R.check_ratio('G T=%d' % T, backend, 'd_traj', xd.grad.cpu(), x64.grad, x32.grad)


# ================================================================================================
# F. adv_crash / adv_crash_bwd and the AdvGenLoss composition
# ================================================================================================

W_CRASH = {'coll_veh': 0.0, 'coll_veh_plan': 0.0, 'coll_env': 0.0, 'init_z': 0.5, 'init_z_atk': 0.05, 'motion_prior': 1.0,
           'motion_prior_atk': 0.005, 'adv_crash': 2.0}
W_ADV = {'coll_veh': 20.0, 'coll_veh_plan': 20.0, 'coll_env': 20.0, 'init_z': 0.5, 'init_z_atk': 0.05, 'motion_prior': 1.0,
         'motion_prior_atk': 0.005, 'adv_crash': 2.0}


def adv_module(be, w, lw, ptr, buffer, env, mapix, init, t0, infront):
    from strive_amd.losses.adv_gen_nusc import AdvGenLoss
    dev = be.dev
    return AdvGenLoss(w, lw.to(dev), mapix.to(dev), dev_env(env, dev), init.to(dev), ptr, veh_coll_buffer=buffer,
                      crash_loss_min_time=t0, crash_loss_min_infront=infront)


def run_adv(be, fn, traj, tgt, z, mu, var, atk=None, alive=None, fused=True):
    """the product's AdvGenLoss: the module's forward (loss, min_agt / min_t, gradients) and, for the fused form, out / soft / rew"""
    dev = be.dev
    tr = traj.clone().to(dev).requires_grad_(True)
    tg = tgt.clone().to(dev).requires_grad_(True)
    zz = z.clone().to(dev).requires_grad_(True)
    al = None if alive is None else alive.to(dev)
    assert fn._fusable(tr, tg, zz, (mu, var)) == fused
    o = fn(tr, tg, zz, (mu.to(dev), var.to(dev)), return_mins=True, attack_agt_idx=atk, scene_alive=al)
    o['loss'].backward()
    res = {'loss': float(o['loss'].detach()), 'min_agt': list(o['min_agt']), 'min_t': list(o['min_t']), 'd_traj': tr.grad.cpu(),
           'd_tgt': tg.grad.cpu() if tg.grad is not None else torch.zeros_like(tgt), 'd_z': zz.grad.cpu()}
    if fused:
        assert fn._fused is not None, 'the fused call was not taken'
        with torch.no_grad():
            ala = None if al is None else al.to(torch.uint8).contiguous()
            tgz = tg.detach() if al is None else torch.where(al.bool().view(-1, 1, 1), tg.detach(), torch.zeros_like(tg))
            _, out, soft, rew = be.ops.adv_gen_loss(tr.detach(), tgz, zz.detach(), mu.to(dev), var.to(dev), fn._setup(),
                                                    attack_agt_idx=atk, scene_alive=ala)
        res.update(out=out.cpu(), soft=soft.cpu(), rew=rew.cpu())
        assert float(out[0]) == res['loss']
    return res


def oracle_adv32(w, traj, tgt, lw, ptr, buffer, env, mapix, z, mu, var, init, t0, infront, atk, pt):
    """oracle/losses.py AdvGen in fp32 (collision points given), plus its soft-min weights restated with its own operators"""
    tr = traj.clone().requires_grad_(True)
    tg = tgt.clone().requires_grad_(True)
    zz = z.clone().requires_grad_(True)
    with given_coll_points(pt):
        fn = olosses.AdvGen(w, lw, mapix, env, init, ptr, veh_coll_buffer=buffer, crash_loss_min_time=t0, crash_loss_min_infront=infront)
        o = fn(tr, tg, zz, (mu, var), return_mins=True, attack_agt_idx=atk)
    o['loss'].backward()
    res = {'LOSS': float(o['loss'].detach()), 'd_traj': tr.grad, 'd_tgt': tg.grad if tg.grad is not None else torch.zeros_like(tgt),
           'd_z': zz.grad, 'CRASH': float(o['adv_crash_loss'].detach().mean()), 'INIT': float(o['init_loss'].detach()) if 'init_loss' in o else 0.0,
           'PRIOR': float(o['motion_prior_loss'].detach().mean()) if 'motion_prior_loss' in o else 0.0}
    for k, name in (('VEH', 'coll_veh_loss'), ('PLAN', 'coll_veh_plan_loss'), ('ENV', 'coll_env_loss')):
        res[k] = float(o[name].detach().mean()) if name in o else 0.0
    # soft-min weights in fp32 (AdvGen keeps them internal): the same lines on the same inputs
    with torch.no_grad():
        B, NT = tgt.shape[0], traj.shape[1] - t0
        a = traj[~fn.ego_mask][:, t0:]
        g = tgt[:, t0:, :4]
        ge = torch.cat([g[b:b + 1].expand(int(fn.sizes[b]) - 1, -1, -1) for b in range(B)], dim=0)
        din = torch.norm(a[:, :, :2] - ge[:, :, :2], dim=-1)
        if infront is not None:
            behind = olosses.check_behind(a, g, ptr, infront)
            always = (behind.sum(1, keepdim=True) == behind.shape[1]).expand_as(behind)
            if bool(always.all()):
                always = torch.zeros_like(always)
            din = torch.where(always, torch.full_like(din, float('inf')), din)
        if atk is not None:
            am = torch.zeros(traj.shape[0], dtype=torch.bool)
            am[atk] = True
            din = torch.where(~am[~fn.ego_mask].unsqueeze(1).expand_as(din), torch.full_like(din, float('inf')), din)
        soft = []
        for b in range(B):
            sm = F.softmin(din[fn.nonego_ptr[b]:fn.nonego_ptr[b + 1]].reshape(-1), dim=0)
            soft.append(torch.zeros_like(sm) if sm.numel() and bool(torch.isnan(sm[0])) else sm)
        res['soft'] = torch.cat(soft).view(-1, NT)
        res['rew'] = 1.0 - res['soft'].sum(1)
    return res


def check_adv(tag, be, got, ref, orc, terms, exact_case=False):
    out = got['out']
    for k in ('VEH_N', 'PLAN_N', 'ENV_N'):
        assert float(out[DO[k]]) == float(ref[k]), '%s: count %s is %g, the reference has %d' % (tag, k, float(out[DO[k]]), ref[k])
    assert float(out[DO['SEL']]) == float(ref['sel'])
    assert bool((out[11:] == 0).all())
    if ref['dots'] is not None and not exact_case:
        assert not bool(((ref['dots'] - ref['infront']).abs() < 1e-3).any()), 'precondition on the REFERENCE: a behind test within 1e-3'
    for k in terms + ['CRASH', 'LOSS']:
        R.check_ratio(tag, be.name, k, out[DO[k]], ref[k], orc[k])
    R.check_ratio(tag, be.name, 'soft', got['soft'], ref['soft'], orc['soft'])
    R.check_ratio(tag, be.name, 'rew', got['rew'], ref['rew'], orc['rew'])
    for k in ('d_traj', 'd_tgt', 'd_z'):
        R.check_ratio(tag, be.name, k, got[k], ref[k], orc[k])
    for b, (s0, s1) in enumerate(ref['top2']):
        if s0 > 0.0 and (s0 - s1) > 1e-4 * s0:                      # (precondition of the arg-max comparison)
            assert got['min_agt'][b] == ref['min_agt'][b] and got['min_t'][b] == ref['min_t'][b], 'soft-min arg-max of scene %d' % b


def adv_reference(w, traj, tgt, lw, ptr, buffer, z, mu, var, init, t0, infront, atk=None, pt=None):
    ref = R.adv_ref(w, traj, tgt, lw, ptr, buffer, z, mu, var, init, t0=t0, infront=infront, attack_agt_idx=atk, pt=pt)
    ref['infront'] = infront
    return ref


def crash_scenes(sizes, seeds, T, origin=60.0):
    """recipe scenes (no shift between them: scenes only meet inside their own blocks) whose first agent is the ego; the target is
    the ego's frames shifted by (1.5, 0.5)"""
    trajs, lws = [], []
    for n, s in zip(sizes, seeds):
        tr, lw = R.recipe(n, s, origin, T)
        trajs.append(tr)
        lws.append(lw)
    traj, lw = torch.from_numpy(np.concatenate(trajs)), torch.from_numpy(np.concatenate(lws))
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.long)
    tgt = traj[ptr[:-1]].clone()
    tgt[:, :, 0] += 1.5
    tgt[:, :, 1] += 0.5
    return traj, tgt, lw, ptr


# id -> (scene sizes with the ego, seeds, T, t0, infront); E = (n - 1) * (T - t0) entries per scene
CRASH_SIZES = {
    'e1': ([2], [3], 4, 3, None),                       # one entry
    'e256': ([17], [1], 16, 0, 0.0),                    # one full pass of the 256 threads
    'e16_e272': ([2, 18], [3, 2], 16, 0, -0.5),         # 272: the first size past one pass, beside a one-attacker scene
    'e1024': ([65], [3], 16, 0, None),                  # ADV_MAXE and the 64 rows of the behind table
}


@on_both(*CRASH_SIZES)
def test_f_crash_sizes(case, backend, request, monkeypatch):
    be = Backend(backend, request, monkeypatch)
    sizes, seeds, T, t0, infront = CRASH_SIZES[case]
    traj, tgt, lw, ptr = crash_scenes(sizes, seeds, T)
    NA, B = traj.shape[0], len(sizes)
    z, mu, var, init = latents(NA - B, 32, 'edges/f/' + case)
    env, mapix = flat_env(), torch.zeros((NA,), dtype=torch.long)
    fn = adv_module(be, W_CRASH, lw, ptr, 0.3, env, mapix, init, t0, infront)
    got = run_adv(be, fn, traj, tgt, z, mu, var)
    ref = adv_reference(W_CRASH, traj, tgt, lw, ptr, 0.3, z, mu, var, init, t0, infront)
    orc = oracle_adv32(W_CRASH, traj, tgt, lw, ptr, 0.3, env, mapix, z, mu, var, init, t0, infront, None, None)
    check_adv('F size %s' % case, be, got, ref, orc, ['PRIOR', 'INIT'])


@on_both('n65', 'nt17')
def test_f_scenes_past_the_crash_tables_take_the_unfused_path(case, backend, request, monkeypatch):
    """65 non-ego agents, and 64 with 17 crash time samples: _fusable is false, forward_terms gives the reference's objective and
    gradients all the same; the fused entry point itself refuses the size with its message and writes nothing"""
    from strive_amd._lib import StriveHipError
    be = Backend(backend, request, monkeypatch)
    n, T = (66, 16) if case == 'n65' else (65, 17)
    traj, tgt, lw, ptr = crash_scenes([n], [3], T)
    z, mu, var, init = latents(n - 1, 8, 'edges/f/' + case)
    env, mapix = flat_env(), torch.zeros((n,), dtype=torch.long)
    fn = adv_module(be, W_CRASH, lw, ptr, 0.3, env, mapix, init, 0, None)
    got = run_adv(be, fn, traj, tgt, z, mu, var, fused=False)
    ref = adv_reference(W_CRASH, traj, tgt, lw, ptr, 0.3, z, mu, var, init, 0, None)
    orc = oracle_adv32(W_CRASH, traj, tgt, lw, ptr, 0.3, env, mapix, z, mu, var, init, 0, None, None, None)
    tag = 'F unfused %s' % case
    R.check_ratio(tag, backend, 'LOSS', got['loss'], ref['LOSS'], orc['LOSS'])
    for k in ('d_traj', 'd_tgt', 'd_z'):
        R.check_ratio(tag, backend, k, got[k], ref[k], orc[k])
    assert got['min_agt'] == ref['min_agt'] and got['min_t'] == ref['min_t']
    # the entry point itself
    dev = be.dev
    setup = fn._setup()
    st, _keep, nbytes = setup.struct_for(T, 8, None, None)
    assert nbytes > 0
    bufs = [torch.full((int(nbytes),), 0x5A, dtype=torch.uint8, device=dev), torch.full((n - 1, T), 7.0, device=dev),
            torch.full((n - 1,), 7.0, device=dev)]
    out = torch.full((16,), 7.0, device=dev)
    pk = be.ops._map_pack(setup.map_env, torch.device(dev))
    td, gd = traj.to(dev), tgt.to(dev)
    zd, md, vd = z.to(dev), mu.to(dev), var.to(dev)
    with pytest.raises(StriveHipError, match='scene too large for the crash kernel'):
        be.lib.call('strive_adv_gen_fwd', setup.sc.ref(), pk.ref(), C.byref(st), L.ptr(td), L.ptr(gd), T, L.ptr(zd), L.ptr(md),
                    L.ptr(vd), L.ptr(out), L.ptr(bufs[1]), L.ptr(bufs[2]), L.ptr(bufs[0]), nbytes, L.stream_ptr(td))
    assert bool((bufs[0] == 0x5A).all()) and bool((bufs[1] == 7.0).all()) and bool((bufs[2] == 7.0).all())


def placed(tgt_xy, attackers, T=4, heading=(1.0, 0.0)):
    """scenes of an ego and explicitly placed static attackers: attackers[b] = list of (x, y) offsets from scene b's target;
    the target is static with the given heading, the ego sits 1.5 m behind it"""
    rows, lws, sizes, tgts = [], [], [], []
    r = np.random.default_rng(5)
    for (tx, ty), atks in zip(tgt_xy, attackers):
        sizes.append(1 + len(atks))
        tgts.append([tx, ty, heading[0], heading[1]])
        rows.append([tx - 1.5, ty - 0.5, heading[0], heading[1]])
        for ax, ay in atks:
            a = r.uniform(0, 2 * np.pi)
            rows.append([tx + ax, ty + ay, np.cos(a), np.sin(a)])
    NA = len(rows)
    traj = torch.tensor(rows, dtype=torch.float32).view(NA, 1, 4).expand(NA, T, 4).contiguous()
    tgt = torch.tensor(tgts, dtype=torch.float32).view(-1, 1, 4).expand(-1, T, 4).contiguous()
    lw = torch.from_numpy(np.stack([r.uniform(3.8, 5.5, NA), r.uniform(1.7, 2.2, NA)], 1).astype(np.float32))
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.long)
    return traj, tgt, lw, ptr


# id -> (targets, attackers per scene as offsets from the target, infront, exact case?)
BEHIND = {
    # straight to the side of a target heading (1, 0): dot = 0 exactly and 0 < 0.0 is false -> NOT behind, it carries the soft-min
    'side_is_not_behind': ([(80.0, 80.0)], [[(0.0, 3.0), (-2.0, 0.25)]], 0.0, True),
    'none_masked': ([(80.0, 80.0), (120.0, 90.0)], [[(2.0, 3.0), (-4.0, 1.0)], [(3.0, -2.0)]], None, False),
    'mixed': ([(80.0, 80.0), (120.0, 90.0)], [[(2.0, 3.0), (-4.0, 1.0)], [(3.0, -2.0), (-3.0, 0.5), (1.0, 6.0)]], -0.5, False),
    'all_behind_everywhere': ([(80.0, 80.0), (120.0, 90.0)], [[(-2.0, 0.5), (-4.0, 1.0)], [(-3.0, -0.5)]], 0.0, False),
    'all_behind_in_one_scene': ([(80.0, 80.0), (120.0, 90.0)], [[(-2.0, 0.5), (-4.0, 1.0)], [(3.0, -0.5), (-3.0, 1.0)]], 0.0, False),
    # soft-min range
    'far_500m': ([(80.0, 80.0)], [[(500.0, 30.0), (-510.0, 4.0), (3.0, 520.0)]], None, False),
    'all_equal': ([(80.0, 80.0)], [[(5.0, 0.0), (0.0, 5.0), (-5.0, 0.0), (0.0, -5.0), (3.0, 4.0)]], None, False),
    'on_the_target': ([(80.0, 80.0)], [[(0.0, 0.0), (4.0, 1.0)]], 0.0, True),
}


@on_both(*BEHIND)
def test_f_behind_mask_and_softmin_range(case, backend, request, monkeypatch):
    be = Backend(backend, request, monkeypatch)
    tgt_xy, attackers, infront, exact = BEHIND[case]
    traj, tgt, lw, ptr = placed(tgt_xy, attackers)
    NA, B = traj.shape[0], len(tgt_xy)
    z, mu, var, init = latents(NA - B, 32, 'edges/f/' + case)
    env, mapix = flat_env(), torch.zeros((NA,), dtype=torch.long)
    t0 = 1
    fn = adv_module(be, W_CRASH, lw, ptr, 0.3, env, mapix, init, t0, infront)
    got = run_adv(be, fn, traj, tgt, z, mu, var)
    ref = adv_reference(W_CRASH, traj, tgt, lw, ptr, 0.3, z, mu, var, init, t0, infront)
    orc = oracle_adv32(W_CRASH, traj, tgt, lw, ptr, 0.3, env, mapix, z, mu, var, init, t0, infront, None, None)
    assert bool(torch.isfinite(got['soft']).all()) and bool(torch.isfinite(got['d_traj']).all())
    if case == 'side_is_not_behind':
        assert float(ref['dots'][0, 0]) == 0.0 and float(got['soft'][0].sum()) > 0.0 and float(got['soft'][1].sum()) == 0.0
    if case == 'all_behind_everywhere':
        assert ref['sel'] == 1 and float(got['out'][DO['SEL']]) == 1.0 and float(got['soft'].sum()) > 1.9
    if case == 'all_behind_in_one_scene':
        assert ref['sel'] == 0 and float(got['out'][DO['SEL']]) == 0.0
        assert float(got['soft'][:2].abs().max()) == 0.0 and bool((got['rew'][:2] == 1.0).all())
    if case == 'far_500m':
        assert float(got['soft'].sum()) > 0.99, 'exp(-500) underflows without the max subtraction'
    if case == 'all_equal':
        assert bool((got['soft'] == got['soft'][0, 0]).all())
    if case == 'on_the_target':
        assert float(got['soft'][0].sum()) > 0.9 and float(got['d_traj'][1].abs().max()) == 0.0, 'd = 0: weight about 1, gradient 0'
    check_adv('F %s' % case, be, got, ref, orc, ['PRIOR', 'INIT'], exact_case=exact)


COMPOSE_SIZES, COMPOSE_SEEDS = [3, 5, 4], [2, 4, 6]


def compose_case(sizes=COMPOSE_SIZES, seeds=COMPOSE_SEEDS):
    traj, tgt, lw, ptr = crash_scenes(sizes, seeds, 4)
    NA, B = traj.shape[0], len(sizes)
    z, mu, var, init = latents(NA - B, 32, 'edges/f/compose')
    return traj, tgt, lw, ptr, z, mu, var, init


@on_both('selection', 'dead_scene')
def test_f_composition(case, backend, request, monkeypatch):
    """every term on (planner pairs with re-weights, environment term over a textured raster): an attacker selection that leaves
    scene 1 without candidates; scene_alive with scene 1 dead = the reference on the batch rebuilt without it"""
    be = Backend(backend, request, monkeypatch)
    traj, tgt, lw, ptr, z, mu, var, init = compose_case()
    NA, B = traj.shape[0], len(COMPOSE_SIZES)
    env, mapix = textured_env(), torch.zeros((NA,), dtype=torch.long)
    t0, infront = 1, -0.5
    fn = adv_module(be, W_ADV, lw, ptr, 0.3, env, mapix, init, t0, infront)
    ego = torch.zeros((NA,), dtype=torch.bool)
    ego[ptr[:-1]] = True
    ne_idx = torch.nonzero(~ego).flatten()
    pt = env_points(be, fn, traj, ne_idx, lw)
    if case == 'selection':
        atk = torch.tensor([int(ptr[0]) + 1, int(ptr[2]) + 2])
        got = run_adv(be, fn, traj, tgt, z, mu, var, atk=atk)
        ref = adv_reference(W_ADV, traj, tgt, lw, ptr, 0.3, z, mu, var, init, t0, infront, atk=atk, pt=pt)
        orc = oracle_adv32(W_ADV, traj, tgt, lw, ptr, 0.3, env, mapix, z, mu, var, init, t0, infront, atk, pt)
        assert_decided(ref['veh'], 1e-4, case)
        assert float(ref['crash_scene'][1]) == 0.0 and ref['VEH_N'] > 0 and ref['PLAN_N'] > 0 and ref['ENV_N'] > 0
        check_adv('F compose selection', be, got, ref, orc, ['VEH', 'PLAN', 'ENV', 'PRIOR', 'INIT'])
        return
    alive = torch.tensor([1, 0, 1], dtype=torch.uint8)
    got = run_adv(be, fn, traj, tgt, z, mu, var, alive=alive)
    # the batch rebuilt without scene 1
    keep = torch.cat([torch.arange(int(ptr[0]), int(ptr[1])), torch.arange(int(ptr[2]), int(ptr[3]))])
    ne_keep = torch.tensor([i for i, a in enumerate(ne_idx.tolist()) if a in set(keep.tolist())])
    ptr2 = torch.tensor([0, COMPOSE_SIZES[0], COMPOSE_SIZES[0] + COMPOSE_SIZES[2]])
    TO = 12
    pt2 = pt.view(-1, TO, 2)[ne_keep].reshape(-1, 2)
    args = (traj[keep], tgt[[0, 2]], lw[keep], ptr2, 0.3)
    ref = adv_reference(W_ADV, *args, z[ne_keep], mu[ne_keep], var[ne_keep], init[ne_keep], t0, infront, pt=pt2)
    orc = oracle_adv32(W_ADV, *args, env, mapix[keep], z[ne_keep], mu[ne_keep], var[ne_keep], init[ne_keep], t0, infront, None, pt2)
    assert_decided(ref['veh'], 1e-4, case)
    assert ref['VEH_N'] > 0 and ref['PLAN_N'] > 0 and ref['ENV_N'] > 0
    dead = torch.arange(int(ptr[1]), int(ptr[2]))
    assert float(got['d_traj'][dead].abs().max()) == 0.0 and float(got['d_tgt'][1].abs().max()) == 0.0
    ne_dead = torch.tensor([i for i in range(ne_idx.numel()) if i not in set(ne_keep.tolist())])
    assert float(got['d_z'][ne_dead].abs().max()) == 0.0 and float(got['soft'][ne_dead].abs().max()) == 0.0
    sub = dict(got, d_traj=got['d_traj'][keep], d_tgt=got['d_tgt'][[0, 2]], d_z=got['d_z'][ne_keep], soft=got['soft'][ne_keep],
               rew=got['rew'][ne_keep], min_agt=[got['min_agt'][0], got['min_agt'][2]], min_t=[got['min_t'][0], got['min_t'][2]])
    check_adv('F compose dead scene', be, sub, ref, orc, ['VEH', 'PLAN', 'ENV', 'PRIOR', 'INIT'])
