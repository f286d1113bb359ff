"""The adv_scenario_gen driver (strive_amd/adv_scenario_gen_tracks.py -> strive_feasibility_screen, strive_ego_verdicts,
strive_amd/csrc/eval_metrics.hip): its two kernels against the per-scene path they stand for, its queue, and its epoch on injected
stages and, on the MI355X, end to end.  The per-scene path: ``determine_feasibility_nusc``
(reference src/utils/scenario_gen.py:30-107), ``check_line_layer`` (reference src/datasets/nuscenes_utils.py:300-332),
``compute_adv_gen_success`` (reference src/utils/adv_gen_optim.py:214-235), ``compute_sol_success`` (reference
src/utils/sol_optim.py:126-165) and the queue of reference src/adv_scenario_gen.py:176-256.

References: fixture g23 (tests/golden/g23_adv_driver.npz, README_g23.md), which is the reference's own run -- its
``determine_feasibility_nusc`` per scene (feas/*), its two success functions per scene (ego/*) and its ``run_one_epoch`` on the
injected stages below for both planners (run/*); the package's torch functions of the same names; and the float64 restatement
tests/adv_driver_restated.py.  The builders of g23's inputs live here (``FEAS_CASES``, ``EGO_CASES``, ``RunLoader`` and the injected
stages) and need no reference; tests/golden/make_golden_adv_driver.py imports them.

Bounds.  Both sides start from the SAME fp32 unnormalised values; the reference and the torch functions continue in fp32 (the
operations counted below are the reference's: src/utils/scenario_gen.py:68, :103, src/adv_scenario_gen.py:180, :190,
src/datasets/nuscenes_utils.py ``check_on_layer``'s ``torch.mean(lw) / torch.mean(dx)``), the kernels in float64.
eps32 = 2^-23, eps64 = 2^-52.
  flags, counts, steps, samples, sep_n, sep_zero, verdicts, statuses: equal.  The inputs keep every decision away from its threshold
      (asserted on the restatement's float64 values): distances and speeds relatively 1e-3 from their thresholds, cosines 1e-3 from
      infront_min, |agent - ego| / mean(dx) 1e-3 from a half-integer, minima relatively 1e-5 from the runner-up unless they are exact
      duplicates, IoUs 1e-3 from 0.02, drivable fractions two samples from 0.95, grid ratios 1e-3 from a half-integer.
  dist, max_vel, the ego speeds: |a - b| in fp32 is two subtractions (eps32 / 2 each, relative to the difference), two squares, one
      addition and one square root (eps32 / 2 each, halved by the root): below 2.5 eps32 relative; 4 eps32 is asserted.
  grid ratios: the mean over R equal fp32 sizes (R / 2 eps32 worst case) and one division: (2 + R / 2) eps32 relative.
Against the restatement and, on the MI355X, against the host emulation: integers equal, doubles within 16 eps64 relative.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import adv_driver_restated as RS
from strive_amd import _lib as L
from strive_amd import ops
from strive_amd import synth
from strive_amd import adv_scenario_gen_tracks as AG
from strive_amd.constants import state_norm_tensors, att_norm_tensors
from strive_amd.datasets import nuscenes_utils as nutils
from strive_amd.utils.adv_gen_optim import compute_adv_gen_success
from strive_amd.utils.scenario_gen import determine_feasibility_nusc
from strive_amd.utils.sol_optim import compute_sol_success

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
DEV = 'cuda:0'
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
RATIOS = {}
SIZES = [1, 2, 17, 65, 257]                       # ego only; one agent; several agents per wave; past one wave's lanes; past 256
SCREEN_INT = ('feasible', 'within', 'step', 'best_samp', 'sep_zero', 'out_i', 'status')
SCREEN_DBL = ('dist', 'max_vel', 'out_d')
EGO_INT = ('hit', 'coll_t', 'out_i', 'status')
# determine_feasibility_nusc's parameters and the ego rule: every combination the tests use
PARAMS = {
    'plain': dict(thresh=10.0, t0=0, agent_vel=0.0, infront_min=None, check_sep=True, planner_name=None, ego_vel=0.0),
    'front': dict(thresh=12.5, t0=4, agent_vel=0.3, infront_min=0.0, check_sep=True, planner_name='hardcode', ego_vel=1.0),
    'last': dict(thresh=15.0, t0=-1, agent_vel=0.3, infront_min=0.2, check_sep=True, planner_name='ego', ego_vel=3.5),
    'nosep': dict(thresh=10.0, t0=0, agent_vel=0.0, infront_min=None, check_sep=False, planner_name='ego', ego_vel=1.0),
}


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


@pytest.fixture()
def emu_ops(emu):
    orig = (ops._lib_for, L.get_lib)
    ops._lib_for = lambda *tensors: emu           # CPU tensors + the emulated library: test infrastructure only
    L.get_lib = lambda: emu
    yield emu
    ops._lib_for, L.get_lib = orig


def check(key, got, want, bound, what):
    """NaN-ness and infinities equal; |got - want| <= bound elementwise elsewhere; the worst error / bound is printed and recorded."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(want))
    assert got.shape == want.shape, '%s %s: shape %s vs %s' % (what, key, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s %s: NaN pattern differs' % (what, key)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and np.array_equal(np.isinf(got), inf), '%s %s: infinities differ' % (what, key)
    ok = np.isfinite(want)
    if not ok.any():
        return
    err = np.abs(got[ok] - want[ok])
    ratio = np.where(bound[ok] > 0, err / np.where(bound[ok] > 0, bound[ok], 1.0), np.where(err == 0, 0.0, np.inf))
    r = float(ratio.max())
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print('%s %-14s largest error %.3g, error / bound %.3g' % (what, key, float(err.max()), r))
    assert r <= 1.0, '%s %s: error / bound %.3g' % (what, key, r)


def teardown_module(module):
    print('error / bound: %s' % json.dumps(RATIOS, indent=1, sort_keys=True))
    if os.environ.get('STRIVE_WRITE_RATIOS') and RATIOS:
        with open(os.path.join(REPO, 'profiles', os.environ['STRIVE_WRITE_RATIOS']), 'w') as f:
            f.write('# Screening and ego verdicts (`strive_feasibility_screen`, `strive_ego_verdicts`): largest observed error / bound\n\n')
            f.write('| quantity | largest error / bound |\n|---|---|\n')
            for k in sorted(RATIOS):
                f.write('| %s | %.3g |\n' % (k, RATIOS[k]))


# ------------------------------------------------------------------------------------------------
# inputs, shared and never modified
# ------------------------------------------------------------------------------------------------

_CACHE = {}
NS_, FT_, TG_ = 20, 12, 12
# the counter streams of the scattered scenes: the first ones whose scenes keep every decision of every PARAMS entry (and every IoU)
# away from its threshold, as the tests assert
SCREEN_KEY = {65: 'd', 257: 'k68'}
EGO_KEY = {(17, 12): 'c', (65, 12): 'c', (257, 12): 'b'}


class StubModel(object):
    """What the two calls read of a model: its two normalisers."""

    def __init__(self):
        from strive_amd.datasets.utils import MeanStdNormalizer
        self.nrm, self.att = MeanStdNormalizer(*state_norm_tensors()), MeanStdNormalizer(*att_norm_tensors())

    def get_normalizer(self):
        return self.nrm

    def get_att_normalizer(self):
        return self.att


def model():
    if 'model' not in _CACHE:
        _CACHE['model'] = StubModel()
    return _CACHE['model']


def maps():
    if 'maps' not in _CACHE:
        _CACHE['maps'] = synth.make_raster(M=2)
    return _CACHE['maps']


def env(device='cpu'):
    if ('env', device) not in _CACHE:
        raster, dx = maps()
        _CACHE[('env', device)] = synth.SyntheticMapEnv(raster.clone(), dx.clone()).to(device)
    return _CACHE[('env', device)]


class _Graph(object):
    def __init__(self, ptr, lw=None, future_gt=None):
        self.ptr = torch.as_tensor(ptr, dtype=torch.long)
        self.lw, self.future_gt = lw, future_gt

    @property
    def batch(self):
        return torch.repeat_interleave(torch.arange(len(self.ptr) - 1), self.ptr[1:] - self.ptr[:-1])


def normalise(world):
    smean, sstd = state_norm_tensors()
    return ((synth.f32(world) - smean[:4]) / sstd[:4]).contiguous()


def screen_scene(n, NS=NS_, FT=FT_, key=None, y0=89.0, speed=1.5):
    """Samples (n,NS,FT,4) and gt (n,TG_,4), NORMALISED, of one scene: the ego drives along a horizontal road band of either map
    (y0 = 89 m) with its samples fanning out; the others are scattered over roads and blocks around it, some parked, with their own
    fans.  Built in: agent 1 stays behind the ego at every step, agent 2 never moves, sample 1 duplicates sample 0 exactly."""
    key = SCREEN_KEY.get(n, 'a') if key is None else key
    ck = (n, NS, FT, key, y0, speed)
    if ck not in _CACHE:
        k = 'g23/screen/%d/%d/%d/%s' % (n, NS, FT, key)
        u = lambda shape, name, lo=0.0, hi=1.0: synth.counter_uniform(shape, k + name, lo, hi)       # noqa: E731
        t = np.arange(FT)[None, None, :]
        half = min(18.0 + 2.5 * np.sqrt(n), 70.0)
        p0 = np.concatenate([[[120.0, y0]], np.stack([120.0 + u((n - 1,), '/x', -half, half + 10.0), y0 + u((n - 1,), '/y', -half, half)], -1)])
        ang = u((n,), '/h', 0.0, 2.0 * np.pi)
        ang[0] = 0.0
        spd = u((n,), '/v', 0.4, 3.0)
        spd[0] = speed
        if n > 1:
            p0[1], ang[1], spd[1] = [112.0, y0 + 0.5], 0.0, 0.8 * speed                              # behind the ego and falling back
        if n > 2:
            p0[2], spd[2] = [126.4, y0 + 3.5], 0.0                                                   # parked beside the ego's path
        fan = 1.0 + 0.08 * (np.arange(NS)[None, :, None] % 7) * u((n, 1, 1), '/fan', 0.5, 1.0)        # the sample's speed factor
        swerve = 0.02 * (np.arange(NS)[None, :, None] // 7) * t ** 1.5                               # and its lateral drift
        if n > 1:
            fan[1], swerve = fan[0], np.broadcast_to(swerve, (n, NS, FT)).copy()
        along = spd[:, None, None] * fan * t
        hx, hy = np.cos(ang)[:, None, None], np.sin(ang)[:, None, None]
        lat = np.broadcast_to(swerve, (n, NS, FT)) * (spd[:, None, None] > 0)
        w = np.zeros((n, NS, FT, 4))
        w[..., 0] = p0[:, 0, None, None] + along * hx - lat * hy
        w[..., 1] = p0[:, 1, None, None] + along * hy + lat * hx
        w[..., 2], w[..., 3] = hx, hy
        if NS > 1:
            w[:, 1] = w[:, 0]                                                                        # an exact tie: the first wins
        g = np.zeros((n, TG_, 4))
        g[..., 0] = p0[:, 0, None] + spd[:, None] * np.arange(TG_)[None, :] * hx[:, 0]
        g[..., 1] = p0[:, 1, None] + spd[:, None] * np.arange(TG_)[None, :] * hy[:, 0]
        g[..., 2], g[..., 3] = hx[:, 0], hy[:, 0]
        _CACHE[ck] = (normalise(w), normalise(g))
    return _CACHE[ck]


def cat_scenes(scenes):
    ptr = np.cumsum([0] + [int(s[0].shape[0]) for s in scenes]).tolist()
    return torch.cat([s[0] for s in scenes]), torch.cat([s[1] for s in scenes]), ptr


def params(name, FT=FT_):
    p = dict(PARAMS[name])
    p['t0'] = p['t0'] % FT
    return p


def run_screen(lib, smp, gt, ptr, map_idx, p, device='cpu', allowed=None, **kw):
    out = AG.screen_batch(smp.to(device), model(), _Graph(ptr, future_gt=gt.to(device)), env(device), torch.as_tensor(map_idx).to(device),
                          p['thresh'], p['t0'], p['agent_vel'], p['infront_min'], p['check_sep'], p['planner_name'], p['ego_vel'],
                          allowed=None if allowed is None else torch.as_tensor(allowed).to(device), lib=lib, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def restated_screen(smp, gt, ptr, map_idx, p, allowed=None):
    sm, ss = [t.numpy() for t in state_norm_tensors()]
    raster, dx = maps()
    return RS.screen(smp.numpy(), ptr, map_idx, sm, ss, raster.numpy(), dx.numpy(), p['thresh'], p['t0'], p['agent_vel'], p['ego_vel'],
                     p['infront_min'], p['check_sep'], AG.PLANNER_RULE[p['planner_name']], allowed=allowed,
                     gt=gt.numpy() if p['planner_name'] == 'ego' else None)


def restated_screen_scene(n, name, m):
    key = ('rs', n, name, m)
    if key not in _CACHE:
        smp, gt = screen_scene(n)
        _CACHE[key] = restated_screen(smp, gt, [0, n], [m], params(name))
    return _CACHE[key]


def assert_screen_margins(r, what):
    m = r['margin']
    assert m['thresh'] > 1e-3 and m['vel'] > 1e-3 and m['cos'] > 1e-3 and m['half'] > 1e-3 and m['gap'] > 1e-5, '%s: %r' % (what, m)


def check_screen64(got, want, what):
    """Two evaluations of the same float64 formulas: discrete outputs equal, continuous ones within 16 eps64 relative."""
    for k in SCREEN_INT:
        assert np.array_equal(got[k], want[k]), '%s %s' % (what, k)
    for k in SCREEN_DBL:
        fin = np.where(np.isfinite(want[k]), np.abs(want[k]), 0.0)
        check('f64/' + k, got[k], want[k], 16 * EPS64 * fin, what)


def ego_scene(n, T, key=None, y0=89.0, truck=False):
    """(traj (n,1,T,4), lw (n,2)) NORMALISED of one scene: the ego drives 6 m per step along a road band (y0 = 89 m; 110 m is off the
    road between the crossings); the others are scattered densely along its path, any heading.  Built in: agent 1 loses its second
    half to NaN, agent 2 is NaN throughout, agent 3 stands where the ego arrives at the last step (a hit at T - 1 only)."""
    key = EGO_KEY.get((n, T), 'a') if key is None else key
    ck = ('ego', n, T, key, y0, truck)
    if ck not in _CACHE:
        k = 'g23/ego/%d/%d/%s' % (n, T, key)
        tr = np.zeros((n, T, 4))
        reach = 6.0 * (T - 1)
        tr[:, :, 0] = 100.0 + synth.counter_uniform((n, 1), k + '/x', -5.0, reach + 5.0) + 0.3 * np.arange(T)[None, :]
        tr[:, :, 1] = y0 + synth.counter_uniform((n, 1), k + '/y', -1.0, 1.0) * (2.0 + n / 8.0)
        ang = synth.counter_uniform((n, 1), k + '/h') * 2.0 * np.pi
        tr[:, :, 2], tr[:, :, 3] = np.cos(ang), np.sin(ang)
        tr[0, :, 0], tr[0, :, 1], tr[0, :, 2], tr[0, :, 3] = 100.0 + 6.0 * np.arange(T), y0, 1.0, 0.0
        lw = np.asarray([[4.5, 2.0], [4.0, 1.75], [8.0, 2.5], [5.0, 2.25]])[(synth.counter_uniform((n,), k + '/lw') * 4).astype(int)]
        lw[0] = [8.0, 2.5] if truck else [4.5, 2.0]
        if n > 3 and T > 1:
            tr[1, T // 2:] = np.nan
            tr[2] = np.nan
            tr[3, :, 0], tr[3, :, 1], tr[3, :, 2], tr[3, :, 3] = 100.0 + reach + 0.25, y0 + 0.5, 1.0, 0.0
            lw[3] = [4.0, 1.75]
        amean, astd = att_norm_tensors()
        _CACHE[ck] = (normalise(tr).unsqueeze(1).contiguous(), (synth.f32(lw) - amean) / astd)
    return _CACHE[ck]


def run_ego(lib, traj, lw, ptr, atk=None, map_idx=None, device='cpu', **kw):
    out = AG.ego_verdicts(traj.to(device), model(), _Graph(ptr, lw=lw.to(device)), None if atk is None else torch.as_tensor(atk).to(device),
                          env(device) if map_idx is not None else None, None if map_idx is None else torch.as_tensor(map_idx).to(device),
                          lib=lib, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def restated_ego(traj, lw, ptr, atk=None, map_idx=None, **kw):
    sm, ss = [t.numpy() for t in state_norm_tensors()]
    am, as_ = [t.numpy() for t in att_norm_tensors()]
    raster, dx = maps()
    return RS.ego(traj[:, 0].numpy(), ptr, lw.numpy(), atk, sm, ss, am, as_, raster.numpy() if map_idx is not None else None, dx.numpy(),
                  map_idx, **kw)


EGO_SHAPES = [(1, 12), (2, 1), (17, 12), (65, 12), (257, 12), (17, 70)]        # (the last: more steps than one wave has lanes)


def ego_case(n, T):
    """(traj, lw, atk, map index) of one shape: an attacker wherever there is another agent, the truck scene on map 1."""
    traj, lw = ego_scene(n, T, truck=n == 65)
    return traj, lw, (None if n == 1 else [min(3, n - 1)]), [1 if n == 65 else 0]


def restated_ego_shape(n, T):
    key = ('re', n, T)
    if key not in _CACHE:
        traj, lw, atk, mi = ego_case(n, T)
        _CACHE[key] = restated_ego(traj, lw, [0, n], atk, mi)
    return _CACHE[key]


def assert_ego_margins(r, what):
    v = r['iou'][~np.isnan(r['iou'])]
    assert not v.size or np.abs(v - RS.IOU_THRESH).min() > 1e-3, what
    for b in range(r['out_i'].shape[0]):
        cells = int(r['out_i'][b, 5]) * int(r['out_i'][b, 6])
        if cells:
            assert np.abs(r['grid_d'][b] - np.floor(r['grid_d'][b]) - 0.5).min() > 1e-3, what
    if r['frac'].size:
        assert np.abs(r['frac'] - 0.95).min() > 2.0 / 45, what          # (no grid of these tests has more than 45 samples)


def check_ego64(got, want, what):
    for k in EGO_INT:
        assert np.array_equal(got[k], want[k]), '%s %s' % (what, k)
    check('f64/grid_d', got['grid_d'], want['grid_d'], 16 * EPS64 * np.abs(np.nan_to_num(want['grid_d'], nan=0.0)), what)


def sentinels(spec, device='cpu'):
    return {k: torch.full(shape, -7, dtype=dtype, device=device) for k, (shape, dtype) in spec.items()}


def screen_sentinels(NA, B, device='cpu'):
    spec = {k: ((NA,), torch.int32) for k in ('feasible', 'within', 'step', 'best_samp', 'sep_zero')}
    spec.update({'dist': ((NA,), torch.float64), 'max_vel': ((NA,), torch.float64), 'out_i': ((B, 8), torch.int32),
                 'out_d': ((B, 3), torch.float64), 'status': ((B,), torch.int32)})
    return sentinels(spec, device)


def ego_sentinels(NA, B, device='cpu'):
    return sentinels({'hit': ((NA,), torch.int32), 'coll_t': ((NA,), torch.int32), 'out_i': ((B, 8), torch.int32),
                      'grid_d': ((B, 2), torch.float64), 'status': ((B,), torch.int32)}, device)


def near_pair():
    """One agent 0.054 m from a standing ego, less than mean(dx) / 2: its line has no samples (n = 0) and cannot be blocked."""
    w = np.zeros((2, 1, 2, 4))
    w[0, 0, :, :2], w[1, 0, :, :2] = [50.0, 9.0], [50.05, 9.02]
    w[1, 0, 1, 0] += 0.5                                                 # (it moves, after step 0)
    w[..., 2] = 1.0
    return normalise(w), normalise(np.zeros((2, TG_, 4)))


def FEAS_CASES():
    """[(samples, gt, map index)]: the scenes of fixture g23's ``feas/s<k>``, each screened alone by the reference under every entry
    of PARAMS.  0-4: the scattered scenes of SIZES, NS 20 (17 agents on map 1); 5: 17 agents, NS 1; 6, 7: the two scenes whose own
    sep_n differ; 8: the pair closer than mean(dx) / 2."""
    short, long_ = two_line_lengths()
    return ([screen_scene(n) + (1 if n == 17 else 0,) for n in SIZES] + [screen_scene(17, NS=1) + (0,)]
            + [short + (0,), long_ + (0,), near_pair() + (0,)])


def EGO_CASES():
    """[(traj, lw, local attacker or None, map index)]: the scenes of fixture g23's ``ego/s<k>``.  0-5: EGO_SHAPES (65: the truck
    scene, on map 1); 6: 17 agents with the ego off the road."""
    cases = []
    for n, T in EGO_SHAPES:
        traj, lw, atk, mi = ego_case(n, T)
        cases.append((traj, lw, None if atk is None else atk[0], mi[0]))
    traj, lw = ego_scene(17, 12, y0=110.0)
    return cases + [(traj, lw, 4, 0)]


def g23():
    if 'g23' not in _CACHE:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_adv_driver.npz')) as z:
            _CACHE['g23'] = {k: z[k] for k in z.files}
    return _CACHE['g23']


# ------------------------------------------------------------------------------------------------
# host emulation against the reference's own run (fixture g23, tests/golden/README_g23.md)
# ------------------------------------------------------------------------------------------------

def check_screen_against_g23(lib, k, name, device='cpu'):
    """The kernel on scene k alone against ``determine_feasibility_nusc`` as the reference ran it.  Flags, steps, sep_n and the
    per-line counts of samples on a 0 pixel are equal; dist, max_vel and the ego speeds are within 4 eps32 relative (the module
    docstring's count of the reference's fp32 operations after the shared fp32 unnormalisation)."""
    smp, gt, m = FEAS_CASES()[k]
    n, FT = int(smp.shape[0]), int(smp.shape[2])
    p = params(name, FT)
    G, pre, what = g23(), 'feas/s%d/%s/' % (k, name), 'g23 feas/s%d %s' % (k, name)
    out = run_screen(lib, smp, gt, [0, n], [m], p, device=device)
    assert out['status'].tolist() == [0], what
    ev, gv = G[pre + 'ego_vel']
    check('g23/ego_vel', out['out_d'][0, :2], [ev, gv if p['planner_name'] == 'ego' else np.nan], 4 * EPS32 * np.asarray([ev, gv]), what)
    slow = {None: False, 'ego': gv < p['ego_vel'], 'hardcode': ev < p['ego_vel']}[p['planner_name']]
    o = out['out_i'][0]
    if bool(G[pre + 'none']):
        assert n == 1 and o.tolist() == [0, 0, 0, 0, -1, -1, 0, 1 if slow else 2], what
        return
    feas, step, dist = G[pre + 'feasible'], G[pre + 'step'], G[pre + 'dist'].astype(np.float64)
    assert np.array_equal(out['feasible'][1:], feas.astype(np.int32)), what
    assert np.array_equal(out['step'][1:], step), what
    assert np.array_equal(out['within'][1:], (dist < p['thresh']).astype(np.int32)), what
    check('g23/dist', out['dist'][1:], dist, 4 * EPS32 * np.where(np.isfinite(dist), dist, 0.0), what)
    vel = G[pre + 'max_vel'].astype(np.float64)
    check('g23/max_vel', out['max_vel'][1:], vel, 4 * EPS32 * vel, what)
    nf = int(feas.sum())
    assert o[0] == n - 1 and o[1] == int((dist < p['thresh']).sum()) and o[2] == o[3] == nf, what
    assert o[7] == (1 if slow else 3 if nf == 0 else 0), what
    if nf:
        masked = np.where(feas.astype(bool), dist, np.inf)
        assert o[4] == int(masked.argmin()) + 1 and o[5] == int(step[o[4] - 1]), what
        check('g23/dist', out['out_d'][0, 2], masked.min(), 4 * EPS32 * masked.min(), what)
    if p['check_sep']:
        assert o[6] == int(G[pre + 'sep_n']), what
        assert np.array_equal(out['sep_zero'][1:], G[pre + 'sep_zero']), what
        ratio = G[pre + 'ratio']                     # (the tie condition on the reference's values: the lines that decide sep_n)
        ratio = ratio[ratio >= ratio.max() - 1.0]
        assert np.abs(ratio - np.floor(ratio) - 0.5).min() > 1e-3 and rel_away(dist, p['thresh']) > 1e-3, what
    assert p['agent_vel'] == 0 or rel_away(vel, p['agent_vel']) > 1e-3, what


def rel_away(values, threshold):
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(np.abs(v - threshold).min() / abs(threshold)) if v.size else np.inf


@pytest.mark.parametrize('name', sorted(PARAMS))
@pytest.mark.parametrize('k', range(9))
def test_screen_against_the_reference_run(emu, k, name):
    check_screen_against_g23(emu, k, name)


def test_the_reference_blocks_the_short_line_only_in_a_joint_call():
    """What the reference's ``check_line_layer`` gave for the two-sep_n pair: free when each scene is screened alone (feas/s6, s7),
    the short scene's line blocked when both lines go through ONE call (feas/joint) -- the case test_sep_n_is_per_scene runs."""
    G = g23()
    assert G['feas/s6/plain/sep_zero'].tolist() == [0] and G['feas/s7/plain/sep_zero'].tolist() == [0]
    assert (int(G['feas/s6/plain/sep_n']), int(G['feas/s7/plain/sep_n']), int(G['feas/joint/sep_n'])) == (6, 80, 80)
    assert G['feas/joint/blocked'].tolist() == [1, 0]
    assert int(G['feas/s8/plain/sep_n']) == 0 and G['feas/s8/plain/feasible'].tolist() == [1], 'n = 0: no samples, not blocked'


def check_ego_against_g23(lib, k, device='cpu'):
    """Both ``ego_verdicts`` calls on scene k alone against ``compute_adv_gen_success`` / ``compute_sol_success`` as the reference ran
    them: flags, first steps, verdicts and the grid are equal; the grid ratios within (2 + R / 2) eps32 relative."""
    traj, lw, atk, m = EGO_CASES()[k]
    n, T = int(traj.shape[0]), int(traj.shape[2])
    G, pre, what = g23(), 'ego/s%d/' % k, 'g23 ego/s%d' % k
    iou = G[pre + 'iou']
    iou = iou[~np.isnan(iou)]
    assert not iou.size or np.abs(iou - RS.IOU_THRESH).min() > 1e-3, what
    L_, W_ = int(G[pre + 'L']), int(G[pre + 'W'])
    assert np.abs(G[pre + 'frac'].astype(np.float64) - 0.95).min() > 2.0 / (L_ * W_) and np.abs(G[pre + 'ratio'] - np.floor(G[pre + 'ratio']) - 0.5).min() > 1e-3
    adv = run_ego(lib, traj, lw, [0, n], None if atk is None else [atk], device=device)
    sol = run_ego(lib, traj, lw, [0, n], None, [m], device=device)
    assert adv['status'].tolist() == [0] and sol['status'].tolist() == [0], what
    hit, coll_t = G[pre + 'hit'].astype(np.int32), G[pre + 'coll_t']
    for r in (adv, sol):
        assert np.array_equal(r['hit'][1:], hit) and r['out_i'][0, 0] == n - 1 and r['out_i'][0, 1] == int(hit.sum()), what
        assert np.array_equal(r['coll_t'][1:][hit == 1], coll_t[hit == 1]) and (r['coll_t'][1:][hit == 0] == T).all(), what
    assert adv['out_i'][0, 2] == int(G[pre + 'adv']), what
    o = sol['out_i'][0]
    assert bool(o[1] == 0 and o[4] == 0) == bool(G[pre + 'sol']) and (o[5], o[6]) == (L_, W_), what
    assert o[4] == int((G[pre + 'frac'] < np.float32(0.95)).any()) and o[7] == G[pre + 'frac'].size, what
    check('g23/grid_ratio', sol['grid_d'][0], G[pre + 'ratio'], (2.0 + T / 2.0) * EPS32 * np.abs(G[pre + 'ratio']), what)


@pytest.mark.parametrize('k', range(7))
def test_ego_verdicts_against_the_reference_run(emu, k):
    check_ego_against_g23(emu, k)


def test_the_reference_run_holds_the_required_cases():
    G = g23()
    assert [int(G['ego/s%d/L' % k]) for k in range(7)] == [18, 18, 18, 32, 18, 18, 18], 'the truck scene has its own grid'
    assert int(G['ego/s2/coll_t'][2]) == 11 and G['ego/s2/hit'][2] == 1 and G['ego/s2/hit'][1] == 0, 'a hit at the last step; all-NaN'
    assert int(G['ego/s6/sol']) == 0 and (G['ego/s6/frac'] < 0.95).any(), 'the ego off the road'
    assert G['ego/s0/hit'].size == 0 and int(G['ego/s0/adv']) == -1


# ------------------------------------------------------------------------------------------------
# host emulation: strive_feasibility_screen
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(PARAMS))
@pytest.mark.parametrize('n', SIZES)
def test_screen_matches_restatement(emu, n, name):
    smp, gt = screen_scene(n)
    m = 1 if n == 17 else 0
    want = restated_screen_scene(n, name, m)
    assert_screen_margins(want, 'n=%d %s' % (n, name))
    check_screen64(run_screen(emu, smp, gt, [0, n], [m], params(name)), want, 'restated n=%d %s' % (n, name))
    assert want['status'].tolist() == [0]
    if n >= 17 and name == 'plain':                         # the scenes show every rule at work
        o = want['out_i'][0]
        assert 0 < o[3] < o[1] < o[0] and want['sep_zero'][1:].any() and not want['sep_zero'][1:].all()
        assert want['within'][2] == 1 and want['feasible'][2] == 0 and want['max_vel'][2] == 0.0, 'the parked agent is near and refused'
    if n >= 2:
        assert want['best_samp'][1] != 1, 'sample 1 duplicates sample 0: the first wins'
    if n >= 2 and name in ('front', 'last'):
        assert np.isinf(want['dist'][1]) and want['step'][1] == params(name)['t0'] and want['best_samp'][1] == 0, 'behind the ego at every step'


@pytest.mark.parametrize('name', sorted(PARAMS))
def test_screen_matches_the_per_scene_torch_path(emu, name):
    """determine_feasibility_nusc on each scene alone, as the reference's loop calls it, against ONE call on the five scenes."""
    p = params(name)
    scenes = [screen_scene(n) for n in SIZES]
    smp, gt, ptr = cat_scenes(scenes)
    mi = [0, 1, 1, 0, 0]
    out = run_screen(emu, smp, gt, ptr, mi, p)
    assert not out['status'].any()
    for n in SIZES:
        assert_screen_margins(restated_screen_scene(n, name, 1 if n == 17 else 0), 'n=%d %s' % (n, name))
    nrm = model().get_normalizer()
    for b, n in enumerate(SIZES):
        lo, hi = ptr[b], ptr[b + 1]
        feas, step, dist = determine_feasibility_nusc(smp[lo:hi], nrm, p['thresh'], p['t0'], p['agent_vel'], p['infront_min'], p['check_sep'],
                                                      env(), torch.tensor([mi[b]]))
        what = '%s scene %d' % (name, b)
        eg = nrm.unnormalize(smp[lo])
        ev = torch.norm(eg[:, 1:, :2] - eg[:, :-1, :2], dim=-1).max().item()
        gg = nrm.unnormalize(gt[lo])
        gv = torch.norm(gg[1:, :2] - gg[:-1, :2], dim=-1).max().item()
        check('ego_vel', out['out_d'][b, :2], [ev, gv if p['planner_name'] == 'ego' else np.nan], 4 * EPS32 * ev, what)
        slow = {None: False, 'ego': gv < p['ego_vel'], 'hardcode': ev < p['ego_vel']}[p['planner_name']]
        if feas is None:
            assert out['out_i'][b].tolist() == [0, 0, 0, 0, -1, -1, 0, 1 if slow else 2]
            continue
        assert np.array_equal(out['feasible'][lo + 1:hi], feas.numpy().astype(np.int32)), what
        assert np.array_equal(out['step'][lo + 1:hi], step.numpy()), what
        assert np.array_equal(out['within'][lo + 1:hi], (dist.numpy() < p['thresh']).astype(np.int32)), what
        check('dist', out['dist'][lo + 1:hi], dist.numpy(), 4 * EPS32 * np.where(np.isfinite(dist.numpy()), dist.numpy(), 0.0), what)
        o = out['out_i'][b]
        nf = int(feas.sum())
        assert o[0] == n - 1 and o[2] == o[3] == nf and o[7] == (1 if slow else 3 if nf == 0 else 0), what
        if nf:
            masked = torch.where(feas, dist, torch.full_like(dist, float('inf')))
            assert o[4] == int(masked.argmin()) + 1 and o[5] == int(step[o[4] - 1]), what
            check('dist', out['out_d'][b, 2], float(masked.min()), 4 * EPS32 * float(masked.min()), what)
        if p['check_sep']:                                   # the lines of this scene, as check_line_layer draws them for this scene
            u = nrm.unnormalize(smp[lo:hi])
            ar = torch.arange(1, n)
            samp, st = torch.as_tensor(out['best_samp'][lo + 1:hi]).long(), torch.as_tensor(out['step'][lo + 1:hi]).long()
            blocked = nutils.check_line_layer(env().nusc_raster[:, 0], env().nusc_dx, u[ar, samp, st][:, :2], u[0][samp, st][:, :2],
                                              torch.tensor([mi[b]]).expand(n - 1))
            assert np.array_equal(out['sep_zero'][lo + 1:hi] > 0, blocked.numpy()), what


def test_allowed_mask_and_verdict_four(emu):
    """adv_attack_with: only the agents of the category stay feasible; none of them -> verdict 4, with the other counts unchanged."""
    smp, gt = screen_scene(17)
    p = params('plain')
    free = run_screen(emu, smp, gt, [0, 17], [0], p)
    feas = np.nonzero(free['feasible'])[0]
    assert feas.size >= 2
    allowed = np.zeros(17, dtype=np.int32)
    allowed[feas[1]] = 1
    one = run_screen(emu, smp, gt, [0, 17], [0], p, allowed=allowed)
    assert np.nonzero(one['feasible'])[0].tolist() == [feas[1]] and one['out_i'][0].tolist()[:5] == [16, free['out_i'][0, 1], feas.size, 1, feas[1]]
    assert one['out_i'][0, 7] == 0 and one['out_d'][0, 2] == free['dist'][feas[1]]
    check_screen64(one, restated_screen(smp, gt, [0, 17], [0], p, allowed=allowed), 'allowed')
    none = run_screen(emu, smp, gt, [0, 17], [0], p, allowed=np.zeros(17, dtype=np.int32))
    assert none['out_i'][0].tolist() == [16, free['out_i'][0, 1], feas.size, 0, -1, -1, free['out_i'][0, 6], 4] and np.isinf(none['out_d'][0, 2])
    for k in ('within', 'step', 'best_samp', 'sep_zero', 'dist', 'max_vel'):
        assert none[k].tobytes() == free[k].tobytes()


def two_line_lengths():
    """Two one-agent scenes on map 0 whose own sep_n differ.  Both agents face the ego across the corner of a block: the line of the
    short scene (5 samples) steps over the corner, the same line at the long scene's sep_n would land on it."""
    raster, dx = maps()
    r0, d = raster[0, 0].numpy(), float(dx[0, 0])
    smean, sstd = state_norm_tensors()

    def scene(ego_xy, agent_xy):
        w = np.zeros((2, 1, 2, 4))
        w[0, 0, :, :2], w[1, 0, :, :2] = ego_xy, agent_xy
        w[1, 0, 1, 0] += 0.5                                             # (it moves)
        w[..., 2] = 1.0
        return normalise(w), normalise(np.zeros((2, TG_, 4)))
    # the block corner of map 0 at (18 m, 18 m): pixels 72.. are off the road on both axes
    assert r0[72, 72] == 0 and r0[71, 72] == 1 and r0[72, 71] == 1 and d == 0.25
    short = scene([17.425, 18.425], [18.425, 17.425])                 # |line| = 1.41 m -> 6 samples; 0.45 .. 0.55 of it is off the road
    long_ = scene([40.0, 9.0], [60.0, 9.0])                           # along the road band: 80 samples, all on the road
    return short, long_


def test_sep_n_is_per_scene(emu):
    """check_line_layer takes its number of samples from the longest line of ONE call, and the reference calls it per scene: a scene's
    lines are sampled at its own sep_n whatever else is in the batch (a kernel with one line length per call gets the pair wrong)."""
    short, long_ = two_line_lengths()
    p = params('plain')
    smp, gt, ptr = cat_scenes([short, long_])
    both = run_screen(emu, smp, gt, ptr, [0, 0], p)
    alone = run_screen(emu, short[0], short[1], [0, 2], [0], p)
    assert both['out_i'][:, 6].tolist() == [6, 80] and alone['out_i'][0, 6] == 6
    for k in SCREEN_INT[:5] + SCREEN_DBL[:2]:
        assert alone[k].tobytes() == both[k][:2].tobytes(), k
    assert alone['out_i'].tobytes() == both['out_i'][:1].tobytes() and alone['out_d'].tobytes() == both['out_d'][:1].tobytes()
    # the torch glue on each scene alone, and on both at once
    nrm = model().get_normalizer()
    u = nrm.unnormalize(smp)
    layer, dx = env().nusc_raster[:, 0], env().nusc_dx
    own = [bool(nutils.check_line_layer(layer, dx, u[a, 0, 0:1, :2], u[a - 1, 0, 0:1, :2], torch.tensor([0]))[0]) for a in (1, 3)]
    joint = nutils.check_line_layer(layer, dx, u[[1, 3], 0, 0, :2], u[[0, 2], 0, 0, :2], torch.tensor([0, 0])).tolist()
    assert (both['sep_zero'][[1, 3]] > 0).tolist() == own == [False, False] and joint == [True, False]
    assert both['feasible'].tolist() == [0, 1, 0, 0] and both['out_i'][:, 7].tolist() == [0, 3]


@pytest.mark.parametrize('n', [0, 1, 2, 3, 64, 65])
def test_sep_zero_equals_the_torch_glue_sum(emu, n):
    """Random lines of exactly n samples, one per scene, across roads and blocks of both maps: sep_zero is check_line_layer's sum."""
    B = 24
    k = 'g23/lines/%d' % n
    raster, dx = maps()
    mdx = float(dx.mean())
    ang = synth.counter_uniform((B,), k + '/a', 0.0, 2.0 * np.pi)
    length = (n + synth.counter_uniform((B,), k + '/l', -0.4, 0.4)) * mdx if n else synth.counter_uniform((B,), k + '/l', 0.02, 0.4) * mdx
    agent = synth.counter_uniform((B, 2), k + '/s', 40.0, 200.0)
    ego = agent + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    w = np.zeros((2 * B, 1, 2, 4))
    w[0::2, 0, 1, :2], w[1::2, 0, 1, :2] = ego, agent                        # step 1 is the only one that counts (t0 = 1)
    w[0::2, 0, 0, :2], w[1::2, 0, 0, :2] = ego + 0.4, agent - 0.3
    w[..., 2] = 1.0
    smp = normalise(w)
    mi = (np.arange(B) % 2).tolist()
    p = dict(params('plain'), thresh=1000.0, t0=1)
    out = run_screen(emu, smp, normalise(np.zeros((2 * B, TG_, 4))), list(range(0, 2 * B + 1, 2)), mi, p)
    assert not out['status'].any() and out['step'][1::2].tolist() == [1] * B and out['out_i'][:, 6].tolist() == [n] * B
    u = model().get_normalizer().unnormalize(smp)
    a, e = u[1::2, 0, 1, :2], u[0::2, 0, 1, :2]
    lw_ = torch.linspace(0.0, 1.0, n).view(1, n, 1)
    pts = a.view(B, 1, 2) * (1.0 - lw_) + e.view(B, 1, 2) * lw_
    pix = torch.round(pts / dx[torch.tensor(mi)].view(B, 1, 2)).long()
    zero = torch.sum(raster[:, 0][torch.tensor(mi).view(B, 1).expand(B, n), pix[..., 1], pix[..., 0]] == 0, dim=-1)
    assert np.array_equal(out['sep_zero'][1::2], zero.numpy()) and (n < 2 or 0 < int((zero > 0).sum()) < B)
    assert np.array_equal(out['feasible'][1::2], (zero == 0).numpy().astype(np.int32))


def check_screen_batch_independence(lib, device):
    """A scene alone and inside a batch, in another place and among other neighbours: the same bytes."""
    p = params('front')
    scenes = [screen_scene(n) for n in SIZES]
    smp, gt, ptr = cat_scenes(scenes)
    mi = [0, 1, 1, 0, 0]
    full = run_screen(lib, smp, gt, ptr, mi, p, device)
    again = run_screen(lib, smp, gt, ptr, mi, p, device)
    assert all(full[k].tobytes() == again[k].tobytes() for k in full), 'two runs give the same bytes'
    for b in (0, 2, 4):
        one = run_screen(lib, scenes[b][0], scenes[b][1], [0, SIZES[b]], [mi[b]], p, device)
        lo, hi = ptr[b], ptr[b + 1]
        for k in SCREEN_INT[:5] + SCREEN_DBL[:2]:
            assert one[k].tobytes() == full[k][lo:hi].tobytes(), (b, k)
        assert one['out_i'].tobytes() == full['out_i'][b:b + 1].tobytes() and one['out_d'].tobytes() == full['out_d'][b:b + 1].tobytes()
    return full


def test_screen_outputs_do_not_depend_on_the_batch(emu):
    check_screen_batch_independence(emu, 'cpu')


def test_screen_status_codes_leave_outputs_untouched(emu):
    p = params('plain')
    scenes = [screen_scene(n) for n in (2, 17, 2, 17)]
    smp, gt, ptr = cat_scenes(scenes)
    NA = ptr[-1]
    good = run_screen(emu, smp, gt, ptr, [0, 0, 0, 0], p)

    def untouched(out, b, lo, hi):
        return all((out[k][lo:hi] == -7).all() for k in SCREEN_INT[:5] + SCREEN_DBL[:2]) and (out['out_i'][b] == -7).all() and (out['out_d'][b] == -7).all()

    def served(out, b, lo, hi):
        return all(out[k][lo + 1:hi].tobytes() == good[k][lo + 1:hi].tobytes() for k in SCREEN_INT[:5] + SCREEN_DBL[:2]) and \
            out['out_i'][b].tobytes() == good['out_i'][b].tobytes() and all(out[k][lo] == -7 for k in SCREEN_INT[:5] + SCREEN_DBL[:2])
    # 3: the map index; 2: a scene that ends past the last agent, one that ends before it starts
    out = run_screen(emu, smp, gt, ptr, [0, 2, -1, 0], p, out=screen_sentinels(NA, 4))
    assert out['status'].tolist() == [0, 3, 3, 0] and untouched(out, 1, 2, 19) and untouched(out, 2, 19, 21) and served(out, 0, 0, 2) and served(out, 3, 21, 38)
    out = run_screen(emu, smp, gt, [0, 2, 99, 21, NA], [0, 0, 0, 0], p, out=screen_sentinels(NA, 4))
    assert out['status'].tolist() == [0, 2, 2, 0] and untouched(out, 1, 2, 21) and served(out, 3, 21, 38)
    # 5: one non-finite value anywhere in the scene's samples (here a heading of its last agent)
    for v in (float('nan'), float('inf')):
        bad = smp.clone()
        bad[18, 7, 3, 3] = v
        out = run_screen(emu, bad, gt, ptr, [0, 0, 0, 0], p, out=screen_sentinels(NA, 4))
        assert out['status'].tolist() == [0, 5, 0, 0] and untouched(out, 1, 2, 19) and served(out, 2, 19, 21)
    # 6: a line that leaves the raster (an agent beyond the map's edge at 256 m) -- torch would raise there
    far = smp.clone()
    smean, sstd = state_norm_tensors()
    far[20, :, :, 0] = (300.0 - smean[0]) / sstd[0]
    out = run_screen(emu, far, gt, ptr, [0, 0, 0, 0], p, out=screen_sentinels(NA, 4))
    assert out['status'].tolist() == [0, 0, 6, 0] and untouched(out, 2, 19, 21) and served(out, 1, 2, 19)
    with pytest.raises(IndexError):
        determine_feasibility_nusc(far[19:21], model().get_normalizer(), p['thresh'], map_env=env(), map_idx=torch.tensor([0]))
    assert run_screen(emu, far, gt, ptr, [0, 0, 0, 0], dict(p, check_sep=False))['status'].tolist() == [0, 0, 0, 0], 'no line is drawn'
    with pytest.raises(ValueError, match='status 6'):
        AG.check_status(out['status'], AG.SCREEN_STATUS_TEXT, 'strive_feasibility_screen')


def test_screen_refuses_bad_arguments(emu):
    smp, gt = screen_scene(2)
    for bad in (dict(infront_min=1.5), dict(infront_min=-1.01), dict(t0=FT_), dict(t0=-1)):
        with pytest.raises(L.StriveHipError):
            run_screen(emu, smp, gt, [0, 2], [0], dict(params('plain'), **bad))
    with pytest.raises(L.StriveHipError):
        run_screen(emu, smp[:, :, :1], gt, [0, 2], [0], params('plain'))            # one step: no displacement to take a maximum of


# ------------------------------------------------------------------------------------------------
# host emulation: strive_ego_verdicts
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,T', EGO_SHAPES)
def test_ego_verdicts_match_restatement(emu, n, T):
    traj, lw, atk, mi = ego_case(n, T)
    want = restated_ego_shape(n, T)
    assert_ego_margins(want, 'n=%d T=%d' % (n, T))
    check_ego64(run_ego(emu, traj, lw, [0, n], atk, mi), want, 'restated n=%d T=%d' % (n, T))
    o = want['out_i'][0]
    assert want['status'].tolist() == [0] and o[0] == n - 1 and o[4] == 0 and o[7] == T
    assert (o[5], o[6]) == ((32, 10) if n == 65 else (18, 8)), 'the truck scene and the car scenes have their own grids'
    if n > 3 and T > 1:
        assert want['hit'][3] == 1 and want['coll_t'][3] == T - 1 and o[2] == 1, 'a hit at the last step only'
        assert want['hit'][2] == 0 and want['coll_t'][2] == T, 'an agent that is NaN throughout never hits'
        assert 1 < o[1] < n - 1 and o[3] < T - 1
    # without the drivable test and without an attacker: the same flags, -1 for what was not asked
    plain = run_ego(emu, traj, lw, [0, n])
    assert plain['hit'].tobytes() == want['hit'].tobytes() and plain['coll_t'].tobytes() == want['coll_t'].tobytes()
    assert plain['out_i'][0].tolist() == [o[0], o[1], -1, o[3], -1, 0, 0, 0] and np.isnan(plain['grid_d']).all()


def test_ego_verdicts_match_the_per_scene_torch_path(emu_ops):
    """compute_adv_gen_success and compute_sol_success on each scene alone against ONE call each on the batch."""
    scenes = [ego_scene(1, 12), ego_scene(2, 1), ego_scene(17, 12), ego_scene(17, 12, y0=110.0), ego_scene(65, 12, truck=True),
              ego_scene(3, 12, y0=9.0)]
    scenes[1] = (scenes[1][0].expand(2, 1, 12, 4).contiguous(), scenes[1][1])
    free = scenes[5][0].clone()
    free[1:, :, :, 1] += 30.0 / state_norm_tensors()[1][1]                       # the others of the last scene: 30 m aside
    scenes[5] = (free, scenes[5][1])
    traj, lw = torch.cat([s[0] for s in scenes]), torch.cat([s[1] for s in scenes])
    sizes = [int(s[0].shape[0]) for s in scenes]
    ptr = np.cumsum([0] + sizes).tolist()
    atk = [-1, 1, 3, 4, 3, 2]
    mi = torch.tensor([0, 1, 0, 0, 1, 0])
    adv = AG.ego_verdicts(traj, model(), _Graph(ptr, lw=lw), torch.tensor(atk))
    sol = AG.ego_verdicts(traj, model(), _Graph(ptr, lw=lw), None, env(), mi)
    assert not adv['status'].any() and not sol['status'].any()
    assert_ego_margins(restated_ego(traj, lw, ptr, atk, mi.tolist()), 'the six scenes')
    want_adv, want_sol = [], []
    for b, n in enumerate(sizes):
        lo, hi = ptr[b], ptr[b + 1]
        g = _Graph([0, n], lw=lw[lo:hi])
        want_adv.append(-1 if atk[b] < 0 else int(compute_adv_gen_success(traj[lo:hi], model(), g, atk[b])))
        want_sol.append(bool(compute_sol_success(traj[lo:hi], model(), g, env(), mi[b:b + 1])))
    assert adv['out_i'][:, 2].tolist() == want_adv == [-1, 1, 1, 0, 1, 0]
    got_sol = ((sol['out_i'][:, 1] == 0) & (sol['out_i'][:, 4] == 0)).tolist()
    assert got_sol == want_sol == [True, False, False, False, False, True]
    assert sol['out_i'][:, 4].tolist() == [0, 0, 0, 1, 0, 0], 'the ego of scene 3 leaves the road'
    assert sol['out_i'][:, 5:7].tolist() == [[18, 8], [18, 8], [18, 8], [18, 8], [32, 10], [18, 8]]
    # the grid ratio against check_on_layer's own: the mean over the ego's R valid rows in fp32, divided by mean(dx) in float64
    dx = env().nusc_dx
    for b in range(len(sizes)):
        lwu = model().get_att_normalizer().unnormalize(lw[ptr[b]:ptr[b] + 1]).expand(12, 2)
        ref = (torch.mean(lwu, dim=0).double() / torch.mean(dx)).numpy()
        check('grid_ratio', sol['grid_d'][b].numpy(), ref, (2.0 + 12 / 2.0) * EPS32 * np.abs(ref), 'scene %d' % b)


def check_ego_batch_independence(lib, device):
    cases = [ego_case(n, 12) for n in (1, 17, 65, 257)]
    traj, lw = torch.cat([c[0] for c in cases]), torch.cat([c[1] for c in cases])
    ptr = np.cumsum([0, 1, 17, 65, 257]).tolist()
    atk, mi = [-1, 3, 3, 3], [0, 0, 1, 0]
    full = run_ego(lib, traj, lw, ptr, atk, mi, device)
    again = run_ego(lib, traj, lw, ptr, atk, mi, device)
    assert all(full[k].tobytes() == again[k].tobytes() for k in full), 'two runs give the same bytes'
    for b, (t1, l1, a1, m1) in enumerate(cases):
        one = run_ego(lib, t1, l1, [0, int(t1.shape[0])], a1, m1, device)
        lo, hi = ptr[b], ptr[b + 1]
        assert one['hit'].tobytes() == full['hit'][lo:hi].tobytes() and one['coll_t'].tobytes() == full['coll_t'][lo:hi].tobytes(), b
        assert one['out_i'].tobytes() == full['out_i'][b:b + 1].tobytes() and one['grid_d'].tobytes() == full['grid_d'][b:b + 1].tobytes(), b
    return full


def test_ego_outputs_do_not_depend_on_the_batch(emu):
    check_ego_batch_independence(emu, 'cpu')


def test_ego_status_codes_leave_outputs_untouched(emu):
    cases = [ego_case(n, 12) for n in (2, 17, 2, 17)]
    traj, lw = torch.cat([c[0] for c in cases]), torch.cat([c[1] for c in cases])
    ptr, NA = [0, 2, 19, 21, 38], 38
    good = run_ego(emu, traj, lw, ptr, [1, 3, -1, 3], [0, 0, 0, 0])
    assert not good['status'].any()

    def untouched(out, b, lo, hi):
        return (out['hit'][lo:hi] == -7).all() and (out['coll_t'][lo:hi] == -7).all() and (out['out_i'][b] == -7).all() and (out['grid_d'][b] == -7).all()

    def served(out, b, lo, hi):
        return out['hit'][lo:hi].tobytes() == good['hit'][lo:hi].tobytes() and out['out_i'][b].tobytes() == good['out_i'][b].tobytes()
    out = run_ego(emu, traj, lw, ptr, [1, 3, -1, 3], [0, 2, -1, 0], out=ego_sentinels(NA, 4))
    assert out['status'].tolist() == [0, 3, 3, 0] and untouched(out, 1, 2, 19) and untouched(out, 2, 19, 21) and served(out, 0, 0, 2) and served(out, 3, 21, 38)
    out = run_ego(emu, traj, lw, [0, 2, 99, 21, NA], [1, -1, -1, 3], [0, 0, 0, 0], out=ego_sentinels(NA, 4))
    assert out['status'].tolist() == [0, 2, 2, 0] and untouched(out, 1, 2, 21) and served(out, 3, 21, 38)
    # an attacker index that is the ego, past the scene, or below -1
    out = run_ego(emu, traj, lw, ptr, [0, 17, -2, 16], [0, 0, 0, 0], out=ego_sentinels(NA, 4))
    assert out['status'].tolist() == [2, 2, 2, 0] and untouched(out, 0, 0, 2) and untouched(out, 1, 2, 19) and out['out_i'][3, 2] == good['hit'][21 + 16]
    # 4: the ego's grid is larger than the linspace table allows; the other scenes are served
    out = run_ego(emu, traj, lw, ptr, [1, 3, -1, 3], [0, 0, 0, 0], out=ego_sentinels(NA, 4), lin_max=17)
    assert out['status'].tolist() == [4, 4, 4, 4] and untouched(out, 0, 0, 2)
    big = lw.clone()
    amean, astd = att_norm_tensors()
    big[2] = (torch.tensor([40.0, 2.0]) - amean) / astd
    out = run_ego(emu, traj, big, ptr, [1, 3, -1, 3], [0, 0, 0, 0], out=ego_sentinels(NA, 4))
    assert out['status'].tolist() == [0, 4, 0, 0] and untouched(out, 1, 2, 19) and served(out, 2, 19, 21)
    assert run_ego(emu, traj, big, ptr, [1, 3, -1, 3])['status'].tolist() == [0, 0, 0, 0], 'no grid is formed without the drivable test'


# ------------------------------------------------------------------------------------------------
# the queue of feasible scenes
# ------------------------------------------------------------------------------------------------

def row(n_others, n_any, n_feasible, slow=False):
    verdict = 1 if slow else 2 if n_others == 0 else 3 if n_any == 0 else 4 if n_feasible == 0 else 0
    return [n_others, n_any, n_any, n_feasible, -1, -1, 0, verdict]


def drive(batcher, scenes):
    lines, batches = [], []
    for i, (r, count) in enumerate(scenes):
        for kind, v in batcher.push(r, count, i == len(scenes) - 1):
            (lines if kind == 'log' else batches).append(v)
    return lines, batches


def test_batcher_logs_and_batches_as_the_reference_loop():
    Bt = AG.FeasibilityBatcher
    scenes = [(row(4, 2, 2), 5), (row(0, 0, 0), 1), (row(3, 0, 0), 4), (row(5, 1, 1, slow=True), 6), (row(6, 3, 0), 7), (row(7, 2, 1), 8),
              (row(2, 1, 1), 3), (row(3, 0, 0), 4)]
    lines, batches = drive(Bt(12, 'ego'), scenes)
    assert batches == [[0, 5], [6]], 'a batch closes mid-stream at 13 >= 12 agents; the skipped last scene flushes the queue'
    assert lines == [Bt.FEASIBLE, Bt.CURRENT % 5, Bt.ONLY_EGO, Bt.NONE_NEAR, Bt.SLOW['ego'], Bt.NO_CATEGORY, Bt.FEASIBLE, Bt.CURRENT % 13, Bt.FORMED,
                     Bt.FEASIBLE, Bt.CURRENT % 3, Bt.NONE_NEAR, Bt.FORMED]
    assert Bt.SLOW['ego'] == 'Ego vehicle not moving more than velocity threshold, skipping...' and Bt.FORMED == 'Formed batch! Starting optimization...'


def test_batcher_last_scene_quirk():
    """(sic) On the loader's last scene a skip does not ``continue``: a slow ego with a feasible attacker is queued."""
    Bt = AG.FeasibilityBatcher
    lines, batches = drive(Bt(100, 'hardcode'), [(row(4, 2, 2, slow=True), 5), (row(4, 2, 2, slow=True), 5)])
    assert batches == [[1]] and lines == [Bt.SLOW['hardcode'], Bt.SLOW['hardcode'], Bt.FEASIBLE, Bt.CURRENT % 5, Bt.FORMED]
    # a slow, ego-only last scene logs both lines and forms nothing from an empty queue
    lines, batches = drive(Bt(100, 'ego'), [(row(0, 0, 0, slow=True), 1)])
    assert batches == [] and lines == [Bt.SLOW['ego'], Bt.ONLY_EGO]
    # a last scene without an attacker of the category still flushes
    lines, batches = drive(Bt(100, 'ego'), [(row(4, 2, 2), 5), (row(4, 2, 0), 5)])
    assert batches == [[0]] and lines == [Bt.FEASIBLE, Bt.CURRENT % 5, Bt.NO_CATEGORY, Bt.FORMED]
    # a single scene as large as the batch closes it at once; an empty stream does nothing
    assert drive(Bt(4, 'ego'), [(row(4, 2, 2), 5), (row(4, 2, 2), 5), (row(1, 1, 1), 2)])[1] == [[0], [1], [2]]
    assert drive(Bt(4, 'ego'), []) == ([], [])
    with pytest.raises(ValueError):
        Bt(4, 'replay')


def test_batcher_on_the_screening_of_a_batch(emu):
    """From the kernel's rows: the five scenes of SIZES under the 'last' rule (the ego's gt speed 1.5 m per step is below 3.5)."""
    smp, gt, ptr = cat_scenes([screen_scene(n) for n in SIZES])
    out = run_screen(emu, smp, gt, ptr, [0, 1, 1, 0, 0], params('last'))
    assert out['out_i'][:, 7].tolist() == [1] * 5 and out['out_i'][4, 3] > 0
    Bt = AG.FeasibilityBatcher
    lines, batches = drive(Bt(32, 'ego'), [(out['out_i'][b], SIZES[b]) for b in range(5)])
    assert batches == [[4]] and lines == [Bt.SLOW['ego']] * 5 + [Bt.FEASIBLE, Bt.CURRENT % 257, Bt.FORMED]


# ------------------------------------------------------------------------------------------------
# the epoch on injected stages
# ------------------------------------------------------------------------------------------------

class InjModel(StubModel):
    """A model whose embed / decode_embedding are plain functions of the batch: the stages around them are injected."""
    dt, FT, Z = 0.5, 12, 4

    def embed(self, scene_graph, map_idx, map_env):
        z = scene_graph.past_gt[:, :, 0].contiguous()[:, :self.Z] * 0.1
        return {'posterior_out': (z, z * 0.0 + 1.0), 'prior_out': (z * 0.5, z * 0.0 + 2.0), 'map_feat': z.clone()}

    def decode_embedding(self, z, embed_info, scene_graph, map_idx, map_env, nfuture=None):
        fut = scene_graph.future_gt[:, :, :4].clone()
        fut[:, :, 0] += 0.01 * z[:, :1]
        return {'future_pred': fut}


def inj_sample(scene_graph, map_idx, map_env, NS, include_mean=True):
    """NS futures per agent that depend on the agent's own rows alone, so a scene's samples do not depend on its chunk."""
    fut = scene_graph.future_gt[:, :, :4]
    fut = torch.where(torch.isnan(fut), scene_graph.past_gt[:, -1:, :4].expand_as(fut), fut)          # an unseen frame: where it was last seen
    fut = torch.where(torch.isnan(fut), normalise(np.asarray([128.0, 128.0, 1.0, 0.0])).to(fut).expand_as(fut), fut)
    smp = fut.unsqueeze(1).repeat(1, NS, 1, 1)
    smp[:, :, :, 1] += 0.02 * torch.arange(NS, dtype=fut.dtype, device=fut.device).view(1, NS, 1) * scene_graph.lw[:, :1].unsqueeze(-1)
    return {'future_pred': smp}


def inj_init(z, init_traj, vis, lr, weights, model_, scene_graph, map_env, map_idx, iters, embed_info, prior):
    return z + 0.001 * iters, init_traj.clone(), {}


class InjPlanner(object):
    """Drives the ego where the data has it, half a metre aside."""

    def __init__(self, map_env, cfg):
        pass

    def reset(self, state, veh_att, batch, B, map_idx):
        self.state, self.batch, self.B = state, batch, B

    def rollout(self, agent_obs, agent_t, agent_ptr, planner_t, control_all=False):
        ego = torch.stack([self.state[(self.batch == b).nonzero()[0, 0]] for b in range(self.B)])[:, :4].double()
        out = ego.unsqueeze(1).repeat(1, len(planner_t), 1)
        out[:, :, 0] += 2.0 * torch.arange(1, len(planner_t) + 1, dtype=torch.float64, device=out.device).view(1, -1) * out[:, :, 2]
        out[:, :, 1] += 0.5
        return out


def inj_adv(cur_z, lr, weights, model_, scene_graph, map_env, map_idx, num_iters, embed_info, planner_name, tgt_prior, other_prior, t0,
            infront, planner=None, planner_viz_out=None):
    """The attacker is agent 1 of each scene; in scenes with an odd number of agents it is put onto the ego's path."""
    fut = scene_graph.future_gt[:, :, :4].clone()
    ptr = scene_graph.ptr.cpu().numpy()
    for b in range(len(ptr) - 1):
        if (ptr[b + 1] - ptr[b]) % 2 == 1:
            fut[ptr[b] + 1] = fut[ptr[b]]
    dec = {'future_pred': fut + 0.001}
    return cur_z + 0.5, fut.unsqueeze(1), dec, ptr[:-1] + 1, np.full(len(ptr) - 1, 5)


def inj_sol(cur_z, final_result_traj, future_len, lr, weights, model_, scene_graph, map_env, map_idx, num_iters, embed_info, tgt_prior,
            other_prior):
    """The ego leaves sideways, free of the attacker: by 6 m in the even scenes of the batch, by 25 m, off the road, in the odd ones."""
    sol = final_result_traj.clone()
    smean, sstd = state_norm_tensors()
    for b, a in enumerate(scene_graph.ptr[:-1].tolist()):
        sol[a, 0, :, 1] += (6.0 + 19.0 * (b % 2)) / sstd[1]
    return cur_z - 0.25, sol, {}


INJ = {'sample_batched': inj_sample, 'run_init_optim': inj_init, 'planner': InjPlanner, 'run_adv_gen_optim': inj_adv,
       'run_find_solution_optim': inj_sol}


# ---- the loaders of fixture g23's run/ego and run/hardcode: the reference's own run_one_epoch on the injected stages above ----

RUN_PT, RUN_FT = 4, 12
RUN_ARGS = dict(feasibility_thresh=15.5, feasibility_time=2, feasibility_vel=0.5, feasibility_infront_min=None, feasibility_check_sep=True,
                num_iters=1, lr=0.05, adv_attack_with='car')
RUN_BATCH_SIZE = 6
# kind -> (ego speed in m per step, [(dx, dy, speed, category)] of the others, map).  The ego starts at (60.6, 89) on the road band
# y in [80, 98) of map 0 and drives along x; the others drive along x too, each at its own speed (no two steps are equally near).
RUN_SCENES = {
    'three': (2.0, [(8.0, 3.5, 1.9, 0), (-10.0, -3.5, 1.8, 0)], 0),          # odd: the injected attacker reaches the ego
    'four': (2.0, [(8.0, 3.5, 1.9, 0), (-10.0, -3.5, 1.8, 0), (14.0, 3.5, 1.7, 1)], 0),    # even: the adversarial stage fails
    'five': (2.0, [(8.0, 3.5, 1.9, 0), (-10.0, -3.5, 1.8, 0), (14.0, 3.5, 1.7, 1), (-16.0, 3.5, 1.6, 0)], 0),
    'alone': (2.0, [], 1),                                                  # only the ego
    'far': (2.0, [(40.0, 3.5, 1.9, 0), (-45.0, -3.5, 1.8, 0)], 0),           # nobody within 15.5 m
    'slow': (0.1, [(8.0, 3.5, 1.9, 0), (-10.0, -3.5, 1.8, 0)], 0),           # the ego hardly moves; an attacker is there
    'trucks': (2.0, [(8.0, 3.5, 1.9, 1), (-10.0, -3.5, 1.8, 1)], 0),         # feasible attackers, none of them a car
    'strip': (2.0, [(0.0, 13.0, 1.9, 0)], 0),                                # one agent 13 m aside, across the block edge at y = 98
    'parked': (2.0, [(8.0, 3.5, 1.9, 0), (10.0, 0.5, 0.0, 0)], 0),           # a parked car where the injected planner drives
}
RUN_KINDS = {
    # the last scene is skipped and flushes the queue
    'ego': ['three', 'alone', 'four', 'far', 'slow', 'trucks', 'three', 'parked', 'five', 'three', 'strip', 'three', 'far'],
    # (sic) the last scene's ego is too slow, and it is queued all the same
    'hardcode': ['three', 'alone', 'four', 'far', 'slow', 'trucks', 'three', 'parked', 'five', 'three', 'strip', 'slow'],
}


def run_scene(kind):
    """One scene of the run/* loaders as (single-scene Batch, map_idx (1) long)."""
    from strive_amd.graph import Data, Batch, clique_edge_index
    ego_v, others, m = RUN_SCENES[kind]
    n = 1 + len(others)
    steps = np.arange(RUN_PT + RUN_FT) - (RUN_PT - 1)                        # 0 at the last past step
    st = np.zeros((n, RUN_PT + RUN_FT, 6))
    sem, lw = np.zeros((n, 2)), np.zeros((n, 2))
    for a, (dx_, dy_, v, cat) in enumerate([(0.0, 0.0, ego_v, 0)] + others):
        st[a, :, 0], st[a, :, 1], st[a, :, 2], st[a, :, 4] = 60.6 + dx_ + v * steps, 89.0 + dy_, 1.0, v / 0.5
        sem[a, cat] = 1.0
        lw[a] = (8.0, 2.5) if cat else (4.5, 2.0)
    smean, sstd = state_norm_tensors()
    amean, astd = att_norm_tensors()
    state_t = (synth.f32(st) - smean) / sstd
    fut = state_t[:, RUN_PT:].contiguous()
    data = Data(x=torch.empty((n,)), pos=torch.empty((n,)), edge_index=clique_edge_index(n), past=state_t[:, :RUN_PT].contiguous(),
                past_gt=state_t[:, :RUN_PT].clone(), sem=synth.f32(sem), lw=(synth.f32(lw) - amean) / astd, past_vis=torch.ones((n, RUN_PT)),
                future=fut, future_gt=fut.clone(), future_vis=torch.ones((n, RUN_FT)))
    return Batch.from_data_list([data]), torch.tensor([m], dtype=torch.long)


class _RunDataset(object):
    dt = 0.5
    categories = ['car', 'truck']
    vec2cat = {(1, 0): 'car', (0, 1): 'truck'}


class RunLoader(list):
    """The single scenes of run/<planner>, as a batch-size-1 loader yields them."""
    dataset = _RunDataset()

    def __init__(self, planner_name):
        super().__init__(run_scene(kind) for kind in RUN_KINDS[planner_name])


def run_lines(lines, out):
    """Log lines as fixture g23 keeps them: the output directory written as OUT, the timing line dropped."""
    return [ln.replace(out, 'OUT') for ln in lines if not ln.startswith('Optimized sequence in ')]


def listing(out):
    root = os.path.join(out, 'scenario_results')
    return sorted((d, fn) for d in os.listdir(root) for fn in os.listdir(os.path.join(root, d)))


def strip(lines, out):
    return ['Optimized sequence' if ln.startswith('Optimized sequence in ') else ln.replace(out, 'OUT') for ln in lines]


def inj_dataset(device='cpu'):
    raster, dx = synth.make_raster(M=2)
    menv = synth.SyntheticMapEnv(raster, dx).to(device)
    from strive_amd.datasets.nuscenes_dataset import NuScenesDataset
    return NuScenesDataset(synth.make_tracks(n_scenes=3, n_agents=6, T=21, M=2), menv, npast=4, nfuture=12, seq_interval=2, device=device), menv


def run_inj_epoch(loader, menv, out, planner_name, device='cpu', batch_size=10, **kw):
    args = dict(planner_name=planner_name, feasibility_thresh=15.5, feasibility_time=2, feasibility_vel=0.5, feasibility_infront_min=None,
                feasibility_check_sep=True, num_iters=1, save=True, keep_results=True, stage_fns=INJ, dt=0.5, init_iters=(2, 3))
    args.update(kw)
    with open(out + '.txt', 'w') as log:
        written, kept = AG.run_one_epoch(loader, batch_size, InjModel(), menv, device, out, {}, log=log, **args)
    return written, kept, strip(open(out + '.txt').read().splitlines(), out)


@pytest.mark.parametrize('planner_name', ['ego', 'hardcode'])
def test_epoch_on_injected_stages(emu_ops, tmp_path, capsys, planner_name):
    """Chunked screening against scene-by-scene screening, a scene_source against a plain iterable: the same batches, log lines and
    files; every file is prepare_output_dict's full key set; every directory is what the per-scene success functions say."""
    from strive_amd.refine_traffic_tracks import scene_source
    ds, menv = inj_dataset()
    src = scene_source(ds, shuffle=True, generator=torch.Generator().manual_seed(5))
    runs = {}
    for name, loader, chunk in (('chunked', src, 64), ('single', src, 1), ('iterable', list(src), 16)):
        runs[name] = run_inj_epoch(loader, menv, str(tmp_path / name), planner_name, screen_agents=chunk) + (str(tmp_path / name),)
    capsys.readouterr()
    a = runs['chunked']
    assert sum(a[0].values()) == len(listing(a[3])) >= 3 and len([d for d in a[0] if a[0][d]]) >= 2, a[0]
    assert AG.FeasibilityBatcher.FORMED in a[2] and any(ln.endswith('skipping...') for ln in a[2])
    for name in ('single', 'iterable'):
        b = runs[name]
        assert a[0] == b[0] and a[2] == b[2] and listing(a[3]) == listing(b[3]), name
        assert [r['positions'] for r in a[1]] == [r['positions'] for r in b[1]]
        for d, fn in listing(a[3]):
            assert open(os.path.join(a[3], 'scenario_results', d, fn)).read() == open(os.path.join(b[3], 'scenario_results', d, fn)).read(), fn
    m = InjModel()
    for r in a[1]:
        scenes, ptr = r['scene_graph'].to_data_list(), r['scene_graph'].ptr.tolist()
        k = 0
        for b, pos in enumerate(r['positions']):
            one = _Graph([0, ptr[b + 1] - ptr[b]], lw=r['scene_graph'].lw[ptr[b]:ptr[b + 1]])
            adv = compute_adv_gen_success(r['final_result_traj'][ptr[b]:ptr[b + 1]], m, one, r['attack_agt'][b])
            sol = False
            if adv:
                sp = r['sol_scene_graph'].ptr.tolist()
                sol = compute_sol_success(r['sol_result_traj'][sp[k]:sp[k + 1]][:, 0:1], m, one, menv, r['sol_map_idx'][k:k + 1])
                k += 1
            assert (adv, sol) == (r['adv_succeeded'][b], r['sol_succeeded'][b])
            d = 'adv_failed' if not adv else ('adv_sol_success' if sol else 'sol_failed')
            with open(os.path.join(a[3], 'scenario_results', d, 'scene_%04d.json' % pos)) as f:
                got = json.load(f)
            assert list(got)[:8] == ['N', 'dt', 'map', 'lw', 'sem', 'past', 'fut_init', 'fut_adv'] and got['attack_agt'] == 1 and got['attack_t'] == 5
            assert ('fut_sol' in got) == ('z_sol' in got) == adv and set(got['z_prior']) == {'mean', 'var'} and len(got['fut_internal_ego']) == 12
            assert got['map'] == menv.map_list[int(r['map_idx'][b])] and got['N'] == ptr[b + 1] - ptr[b] == len(got['z_adv'])


def check_epoch_against_g23(planner_name, out, device='cpu'):
    """The driver on the loader of run/<planner> with the injected stages against the reference's own ``run_one_epoch`` on the same
    loader and stages: the batches, every log line (the timing line apart), every directory, file name and JSON value."""
    G, p = g23(), 'run/%s/' % planner_name
    loader = RunLoader(planner_name)
    if device != 'cpu':
        loader[:] = [(g.to(device), mi.to(device)) for g, mi in loader]
    raster, dx = maps()
    menv = synth.SyntheticMapEnv(raster.clone(), dx.clone()).to(device)
    with open(out + '.txt', 'w') as log:
        written, kept = AG.run_one_epoch(loader, RUN_BATCH_SIZE, InjModel(), menv, device, out, {}, planner_name=planner_name, log=log,
                                         save=True, keep_results=True, stage_fns=INJ, screen_agents=1, **RUN_ARGS)
    lines = run_lines(open(out + '.txt').read().splitlines(), out)
    want = [str(ln) for ln in G[p + 'lines']]
    assert lines == want, '\n'.join('%r | %r' % (a, b) for a, b in zip(lines, want) if a != b)
    sizes = [1 + len(RUN_SCENES[k][1]) for k in RUN_KINDS[planner_name]]
    assert [[sizes[i] for i in r['positions']] for r in kept] == json.loads(str(G[p + 'batches']))
    assert listing(out) == sorted(zip([str(d) for d in G[p + 'dirs']], [str(f) for f in G[p + 'files']]))
    assert {d for d, _ in listing(out)} == set(AG.RESULT_DIRS), 'all three result directories occur'
    for d, fn, text in zip(G[p + 'dirs'], G[p + 'files'], G[p + 'json']):
        with open(os.path.join(out, 'scenario_results', str(d), str(fn))) as f:
            got = json.load(f)
        ref = json.loads(str(text))
        assert list(got) == list(ref), fn
        for key in ref:
            if device == 'cpu':
                assert got[key] == ref[key], (fn, key)
            else:                                  # fp32 values of the same formulas from another device's torch: 4 eps32 relative
                flat = lambda v: np.asarray(list(v.values()) if isinstance(v, dict) else v, dtype=np.float64) if not isinstance(v, str) else v   # noqa: E731
                a, b = flat(got[key]), flat(ref[key])
                assert (a == b) if isinstance(b, str) else np.allclose(a, b, rtol=4 * EPS32, atol=4 * EPS32 * 256.0, equal_nan=True), (fn, key)
    removed = 'Planner already caused collision after init, removing from batch...'
    assert (removed in lines) == (planner_name == 'hardcode'), 'the scene with the parked car is removed after the init stage'
    return lines


@pytest.mark.parametrize('planner_name', ['ego', 'hardcode'])
def test_epoch_against_the_reference_run(emu_ops, tmp_path, capsys, planner_name):
    lines = check_epoch_against_g23(planner_name, str(tmp_path / planner_name))
    capsys.readouterr()
    Bt = AG.FeasibilityBatcher
    assert lines.count(Bt.NO_CATEGORY) == 1, 'adv_attack_with filters one scene out'
    events = [ln for ln in lines if ln in (Bt.SLOW[planner_name], Bt.NONE_NEAR, Bt.FEASIBLE, Bt.FORMED)]
    if planner_name == 'ego':
        assert events[-2:] == [Bt.NONE_NEAR, Bt.FORMED], 'the skipped last scene flushes the queue'
    else:
        assert events[-3:] == [Bt.SLOW['hardcode'], Bt.FEASIBLE, Bt.FORMED], '(sic) the slow last scene is queued'


@pytest.mark.parametrize('planner_name', ['ego', 'hardcode'])
def test_batcher_against_the_reference_lines(emu, planner_name):
    """The queue alone, fed with the kernel's rows of the run/<planner> scenes: its lines are the reference's lines of that kind."""
    Bt = AG.FeasibilityBatcher
    loader = RunLoader(planner_name)
    batcher, lines, batches = Bt(RUN_BATCH_SIZE, planner_name), [], []
    a = RUN_ARGS
    for i, (g, mi) in enumerate(loader):
        smp = inj_sample(g, mi, None, 20)['future_pred']
        allowed = (g.sem[:, 0] == 1).to(torch.int32)
        out = AG.screen_batch(smp, model(), g, env(), mi, a['feasibility_thresh'], a['feasibility_time'], 0.0, a['feasibility_infront_min'],
                              a['feasibility_check_sep'], planner_name, a['feasibility_vel'], allowed, lib=emu)
        assert out['status'].tolist() == [0]
        for kind, v in batcher.push(out['out_i'][0].numpy(), int(g.past.shape[0]), i == len(loader) - 1):
            (lines if kind == 'log' else batches).append(v)
    own = (Bt.SLOW[planner_name], Bt.ONLY_EGO, Bt.NONE_NEAR, Bt.NO_CATEGORY, Bt.FEASIBLE, Bt.FORMED)
    want = [str(ln) for ln in g23()['run/%s/lines' % planner_name] if str(ln) in own or str(ln).startswith('Current batch NA: ')]
    assert lines == want and batches == [[0, 2], [6, 7], [8, 9], [11]]
    assert all(line in lines for line in own), 'every skip line occurs'


def test_copies_to_the_host_do_not_depend_on_the_number_of_scenes(emu_ops, tmp_path, monkeypatch, capsys):
    """``.cpu()`` calls of an epoch: one per screening chunk, whatever the chunk holds; per batch the same number at B = 1 and at
    B = 5: one per ego_verdicts call and one for the files (and the injected adversarial stage's own, of its ptr)."""
    ds, menv = inj_dataset()
    calls = [0]
    orig, orig_batch = torch.Tensor.cpu, AG._optimise_batch

    def counted(self, *a, **k):
        calls[0] += 1
        return orig(self, *a, **k)
    from strive_amd.refine_traffic_tracks import SceneSource
    orig_gather, inside = SceneSource.gather, [0]

    def gather(self, positions):                           # (the dataset's own copies are not the driver's)
        c0 = calls[0]
        res = orig_gather(self, positions)
        inside[0] += calls[0] - c0
        return res
    monkeypatch.setattr(SceneSource, 'gather', gather)
    seen = {}
    for name, chunk in ((1, 1), (5, 1000)):
        # one scene per batch; then as many agents as the first five feasible scenes hold
        batch_size = 1 if name == 1 else sum(na for _, _, _, na in seen[1][0][:5])
        per_batch = []

        def batch(*a, **k):
            c0 = calls[0]
            res = orig_batch(*a, **k)
            c1 = calls[0]
            per_batch.append((len(res['positions']), any(res['adv_succeeded']), c1 - c0, int(res['scene_graph'].past.shape[0])))
            return res
        monkeypatch.setattr(AG, '_optimise_batch', batch)
        monkeypatch.setattr(torch.Tensor, 'cpu', counted)
        c0, g0 = calls[0], inside[0]
        run_inj_epoch(scene_source_of(ds), menv, str(tmp_path / str(name)), 'ego', batch_size=batch_size, screen_agents=chunk)
        total = calls[0] - c0 - (inside[0] - g0)
        monkeypatch.setattr(torch.Tensor, 'cpu', orig)
        seen[name] = (per_batch, total - sum(b[2] for b in per_batch))
    capsys.readouterr()
    five = seen[5]
    assert [b[0] for b in seen[1][0]] == [1] * 8 and [b[0] for b in five[0]] == [5, 3]
    assert seen[1][1] == len(ds) == 9 and five[1] == 1, 'one read-back per screening chunk'
    with_sol = {b[2] for b in seen[1][0] if b[1]}
    assert len(with_sol) == 1 and {b[2] for b in seen[1][0] if not b[1]} == {with_sol.pop() - 1}, seen[1][0]
    # with a solution stage: the two verdict calls, the files, and the injected stage's own copy -- at B = 1 and at B = 5
    assert five[0][0][1] and five[0][0][2] == max(b[2] for b in seen[1][0]) == 4, seen


def scene_source_of(ds):
    from strive_amd.refine_traffic_tracks import scene_source
    return scene_source(ds)


# ------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------

def test_both_config_files_and_viz(tmp_path):
    golden_dir = os.path.join(REPO, 'tests', 'golden')
    cfg, ignored = AG.parse_cfg(['--config', os.path.join(golden_dir, 'g23_adv_gen_rule_based.cfg')])
    assert ignored == ['data_dir', 'data_version', 'split', 'val_size', 'num_workers', 'viz']
    want = dict(out='./out/adv_gen_rule_based_out', seq_interval=10, shuffle=False, batch_size=1, ckpt='./model_ckpt/traffic_model.pth',
                feasibility_check_sep=True, planner='hardcode', planner_cfg='default', viz=False, save=True, num_iters=200, lr=0.05,
                init_loss_motion_prior_ext=0.01, init_loss_match_ext=10.0, loss_coll_veh=20.0, loss_coll_veh_plan=20.0, loss_coll_env=20.0,
                loss_init_z=0.5, loss_init_z_atk=0.05, loss_motion_prior=1.0, loss_motion_prior_atk=0.005, loss_motion_prior_ext=0.0001,
                loss_match_ext=10.0, loss_adv_crash=2.0, sol_future_len=16, sol_loss_motion_prior=0.005, sol_loss_coll_veh=10.0,
                sol_loss_coll_env=10.0, sol_loss_motion_prior_ext=0.001, sol_loss_match_ext=10.0, feasibility_thresh=10.0, feasibility_time=4,
                feasibility_vel=0.5, feasibility_infront_min=0.0, adv_attack_with=None, screen_agents=AG.DEFAULT_SCREEN_AGENTS,
                on_planner_error='raise')
    assert {k: cfg[k] for k in want} == want
    cfg, ignored = AG.parse_cfg(['--config', os.path.join(golden_dir, 'g23_adv_gen_replay.cfg'), '--num_iters', '7', '--planner', 'hardcode'])
    assert (cfg['out'], cfg['num_iters'], cfg['planner'], cfg['init_loss_motion_prior_ext']) == ('./out/adv_gen_replay_out', 7, 'hardcode', 0.1)
    assert AG.parse_cfg(['--config', os.path.join(golden_dir, 'g23_adv_gen_replay.cfg')])[0]['planner'] == 'ego'
    # the reference's defaults (:33-106) without a file
    cfg, ignored = AG.parse_cfg([])
    assert ignored == [] and (cfg['planner'], cfg['num_iters'], cfg['feasibility_check_sep'], cfg['sol_loss_init_z'], cfg['batch_size']) == ('ego', 300, False, 0.0, 4)
    with pytest.raises(NotImplementedError, match='rendering'):
        AG.parse_cfg(['--viz'])
    with pytest.raises(NotImplementedError):
        AG.run_one_epoch([], 4, InjModel(), env(), 'cpu', str(tmp_path / 'v'), {}, planner_name='ego', viz=True, dt=0.5)
    assert not os.path.exists(str(tmp_path / 'v'))
    with pytest.raises(ValueError):
        AG.parse_cfg(['--planner', 'replay'])
    with pytest.raises(SystemExit, match='Must pass in model weights'):
        AG.main(['--out', str(tmp_path / 'o')])


# ------------------------------------------------------------------------------------------------
# MI355X
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_gpu_screen_matches_emulation_and_restatement(emu, n):
    smp, gt = screen_scene(n)
    m = 1 if n == 17 else 0
    for name in ('plain', 'front'):
        got = run_screen(None, smp, gt, [0, n], [m], params(name), DEV)
        check_screen64(got, run_screen(emu, smp, gt, [0, n], [m], params(name)), 'gpu vs emu n=%d %s' % (n, name))
        check_screen64(got, restated_screen_scene(n, name, m), 'gpu vs restated n=%d %s' % (n, name))


@pytest.mark.gpu
def test_gpu_screen_alone_against_batched_and_line_lengths(emu):
    full = check_screen_batch_independence(None, DEV)
    scenes = [screen_scene(n) for n in SIZES]
    smp, gt, ptr = cat_scenes(scenes)
    check_screen64(full, run_screen(emu, smp, gt, ptr, [0, 1, 1, 0, 0], params('front')), 'gpu vs emu, batch')
    short, long_ = two_line_lengths()
    smp, gt, ptr = cat_scenes([short, long_])
    both = run_screen(None, smp, gt, ptr, [0, 0], params('plain'), DEV)
    assert both['out_i'][:, 6].tolist() == [6, 80] and both['sep_zero'].tolist() == [0, 0, 0, 0] and both['feasible'].tolist() == [0, 1, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('n,T', EGO_SHAPES)
def test_gpu_ego_verdicts_match_emulation_and_restatement(emu, n, T):
    traj, lw, atk, mi = ego_case(n, T)
    got = run_ego(None, traj, lw, [0, n], atk, mi, DEV)
    check_ego64(got, run_ego(emu, traj, lw, [0, n], atk, mi), 'gpu vs emu n=%d T=%d' % (n, T))
    check_ego64(got, restated_ego_shape(n, T), 'gpu vs restated n=%d T=%d' % (n, T))


@pytest.mark.gpu
def test_gpu_ego_alone_against_batched(emu):
    full = check_ego_batch_independence(None, DEV)
    cases = [ego_case(n, 12) for n in (1, 17, 65, 257)]
    traj, lw = torch.cat([c[0] for c in cases]), torch.cat([c[1] for c in cases])
    check_ego64(full, run_ego(emu, traj, lw, np.cumsum([0, 1, 17, 65, 257]).tolist(), [-1, 3, 3, 3], [0, 0, 1, 0]), 'gpu vs emu, batch')


def check_end_to_end(planner_name, device, tmp_path):
    """The command line on a synthetic tracks file with the real stages (3 iterations, init fits of 2): every written file loads
    through read_adv_scenes, and its directory is what compute_adv_gen_success / compute_sol_success say per scene."""
    from strive_amd.datasets import tracks as tracks_io
    from strive_amd.datasets.utils import read_adv_scenes
    from strive_amd.utils import torch as UT
    from util import product_model
    path = str(tmp_path / 'tracks.npz')
    tracks_io.save_tracks(path, synth.make_tracks(n_scenes=2, n_agents=5, T=20))
    m, sd = product_model()
    if planner_name == 'hardcode':
        m.load_state_dict(synth.lane_keeping_weights(sd))
    ckpt = str(tmp_path / 'ckpt.pth')
    UT.save_state(ckpt, m, torch.optim.Adam(m.parameters(), lr=1e-3), cur_epoch=2)
    out = str(tmp_path / 'out')
    cfg = os.path.join(REPO, 'tests', 'golden', 'g23_adv_gen_rule_based.cfg' if planner_name == 'hardcode' else 'g23_adv_gen_replay.cfg')
    orig = AG.run_one_epoch
    AG.run_one_epoch = lambda *a, **k: orig(*a, **dict(k, init_iters=(2, 2)))
    try:
        written, kept = AG.main(['--config', cfg, '--tracks', path, '--ckpt', ckpt, '--out', out, '--num_iters', '3', '--seq_interval', '3',
                                 '--batch_size', '8', '--seed', '7', '--feasibility_thresh', '40', '--feasibility_vel', '0.05', '--device', device,
                                 '--on_planner_error', 'drop'], keep_results=True)
    finally:
        AG.run_one_epoch = orig
    lines = open(os.path.join(out, 'adv_gen_log.txt')).read().splitlines()
    assert lines[0].startswith('Args: ') and any(ln.startswith('Ignoring config keys') and 'viz' in ln for ln in lines)
    files = listing(out)
    assert len(files) == sum(written.values()) >= 2 and AG.FeasibilityBatcher.FORMED in lines
    raster, dx = synth.make_raster()
    menv = synth.SyntheticMapEnv(raster, dx).to(device)
    m = m.to(device)
    judged = 0
    for r in kept:
        ptr = r['scene_graph'].ptr.tolist()
        k = 0
        for b, pos in enumerate(r['positions']):
            one = _Graph([0, ptr[b + 1] - ptr[b]], lw=r['scene_graph'].lw[ptr[b]:ptr[b + 1]])
            adv = compute_adv_gen_success(r['final_result_traj'][ptr[b]:ptr[b + 1]], m, one, r['attack_agt'][b]) if b not in r['dropped'] else False
            sol = False
            if r['adv_succeeded'][b]:
                sp = r['sol_scene_graph'].ptr.tolist()
                sol = compute_sol_success(r['sol_result_traj'][sp[k]:sp[k + 1]][:, 0:1], m, one, menv, r['sol_map_idx'][k:k + 1])
                k += 1
            if b in r['dropped']:
                assert not any(fn == 'scene_%04d.json' % pos for _, fn in files)
                continue
            assert (bool(adv), bool(sol)) == (r['adv_succeeded'][b], r['sol_succeeded'][b])
            assert ('adv_failed' if not adv else ('adv_sol_success' if sol else 'sol_failed'), 'scene_%04d.json' % pos) in files
            judged += 1
    assert judged == len(files)
    for d in {d for d, _ in files}:
        got = read_adv_scenes(os.path.join(out, 'scenario_results', d))
        assert len(got) == sum(1 for d2, _ in files if d2 == d) and all(sc['scene_fut'].shape[1:] == (12, 4) and 'attack_t' in sc for sc in got)


@pytest.mark.gpu
@pytest.mark.parametrize('planner_name', ['ego', 'hardcode'])
def test_gpu_driver_end_to_end(tmp_path, capsys, planner_name):
    check_end_to_end(planner_name, DEV, tmp_path)
    capsys.readouterr()


@pytest.mark.gpu
def test_gpu_epoch_on_injected_stages(tmp_path, capsys):
    """The injected epoch on the device: the same lines and files as on the host emulation's side of the suite would give for a
    scene_source against a plain iterable."""
    from strive_amd.refine_traffic_tracks import scene_source
    ds, menv = inj_dataset(DEV)
    src = scene_source(ds, shuffle=True, generator=torch.Generator().manual_seed(5))
    a = run_inj_epoch(src, menv, str(tmp_path / 'a'), 'hardcode', DEV, screen_agents=64)
    b = run_inj_epoch(list(src), menv, str(tmp_path / 'b'), 'hardcode', DEV, screen_agents=1)
    capsys.readouterr()
    assert a[0] == b[0] and a[2] == b[2] and listing(str(tmp_path / 'a')) == listing(str(tmp_path / 'b')) and sum(a[0].values()) >= 3
    for d, fn in listing(str(tmp_path / 'a')):
        assert open(os.path.join(str(tmp_path / 'a'), 'scenario_results', d, fn)).read() == open(os.path.join(str(tmp_path / 'b'), 'scenario_results', d, fn)).read()


@pytest.mark.gpu
@pytest.mark.parametrize('k', range(9))
def test_gpu_screen_against_the_reference_run(k):
    for name in sorted(PARAMS):
        check_screen_against_g23(None, k, name, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('k', range(7))
def test_gpu_ego_verdicts_against_the_reference_run(k):
    check_ego_against_g23(None, k, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('planner_name', ['ego', 'hardcode'])
def test_gpu_epoch_against_the_reference_run(tmp_path, capsys, planner_name):
    check_epoch_against_g23(planner_name, str(tmp_path / planner_name), DEV)
    capsys.readouterr()
