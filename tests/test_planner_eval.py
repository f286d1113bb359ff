"""Batched planner evaluation (strive_amd/eval_planner.py -> strive_planner_eval_metrics, strive_amd/csrc/eval_metrics.hip) against the
reference's src/eval_planner.py (fixture g17, tests/golden/make_golden_planner_eval.py) and against a float64 numpy restatement.

Tolerances (derived, not fitted).  Coordinates are metres on the 256 m synthetic world, dt = 0.5 s.

  * Integers and booleans (did_collide, coll_time, coll_agt, coll_idx, frame count) are EQUAL: the fixture's tie condition keeps
    every IoU of the reference more than 1e-3 away from the 0.02 threshold, and the kernel's IoU (float64 clip of fp32 / float64
    poses) differs from the reference's (exact area of fp32-rounded corners) by ~1e-6.
  * coll_vel = |(p1 - p0) / dt - (a1 - a0) / dt|.  The other agents' poses are fp32; the reference forms (a1 - a0) / dt in fp32, the
    kernel in float64.  One fp32 subtraction of coordinates up to C and one division: <= 2 eps32 C / dt per component; two
    components and the norm bring it to ``4 * eps32 * C / dt`` absolute, plus ``4 * eps32`` relative for the fp32 roundings of
    the result chain.  (eps32 = 2^-23, C = max |coordinate| of the scene.)
  * The acceleration terms use the plan only, so the same expression applies with eps64 -- also in replay mode, where the
    reference holds the plan as an fp32 tensor (torch.tensor of the JSON) and runs its chain in fp32 while the kernel widens the
    same values to float64: the recorded trajectories have dyadic speeds, and the measured error stays inside the eps64 bound
    (largest error / bound 0.75, profiles/r16_planner_eval_ratios.md).  No bound is widened.
  * GPU against the emulator (and the emulator against the numpy restatement): same formulas, float64; only fused contraction
    and libm's atan2 / cos / sin differ: ``16 * eps64`` relative to the expected value, in every column (measured: largest
    error / bound 0.068, profiles/r16_planner_eval_ratios.md).
  * Full driver on the GPU: the device planner's plan is within PLAN_ATOL = 1e-9 of the fixture (tests/test_planner.py).  A
    perturbation d of every plan coordinate moves a speed by <= 4 d / dt, an acceleration frame by <= 8 d / dt^2 from the second
    difference plus <= 8 S d / dt from the renormalised headings scaling speeds up to S (S = 20 m/s bounds every plan here).
"""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch

import make_golden_planner_eval as mgp
from util import golden
from strive_amd import _lib as L
from strive_amd import ops
from strive_amd import eval_planner as EP
from strive_amd.constants import state_norm_tensors, att_norm_tensors
from strive_amd.datasets.utils import MeanStdNormalizer
from strive_amd.planners.planner import PlannerConfig
from strive_amd.planners.hardcode_goalcond_nusc import CONFIG_DICT
from strive_amd.utils.scenario_gen import log_metric, log_freq_stat, print_metrics, PooledMetric

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

FIX = 'g17_planner_eval.npz'
DT = mgp.DT
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
PLAN_ATOL = 1e-9
SPEED_MAX = 20.0
DEV = 'cuda:0'
DISCRETE = ('coll_time', 'coll_agt', 'coll_idx', 'accel_count')      # per scene in run_planner_eval's details_out
RATIOS = {}                       # largest error / bound seen per quantity (printed; profiles/r16_planner_eval_ratios.md)


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


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------

_SCENES = {}


def fixture_scenes():
    """{evaluation name: dict(others (n,T,4) fp32, lw_ego (2), lw_others (n,2), T)} of the g17 scenes, built once."""
    if not _SCENES:
        for sc in EP.read_adv_scenes(mgp.SCEN_DIR):
            _SCENES['adv_' + sc['name']] = dict(others=sc['adv_fut'], lw_ego=sc['veh_att'][0], lw_others=sc['veh_att'][1:],
                                                veh_att=sc['veh_att'], T=int(sc['adv_fut'].shape[1]))
        sn, an = MeanStdNormalizer(*state_norm_tensors()), MeanStdNormalizer(*att_norm_tensors())
        for i, (g, _) in enumerate(mgp.regular_inputs()[1]):
            if g.past_gt.size(0) > 1:
                att = an.unnormalize(g.lw)
                _SCENES['regular_seq_%05d' % i] = dict(others=sn.unnormalize(g.future_gt[1:, :, :4]), lw_ego=att[0], lw_others=att[1:],
                                                       veh_att=att, T=int(g.future_gt.shape[1]))
    return _SCENES


def stack(names, plans, device='cpu'):
    sc = fixture_scenes()
    others = torch.cat([sc[n]['others'] for n in names]).to(device)
    ptr = np.concatenate([[0], np.cumsum([sc[n]['others'].shape[0] for n in names])])
    lw_ego = torch.stack([sc[n]['lw_ego'] for n in names]).to(device)
    lw_others = torch.cat([sc[n]['lw_others'] for n in names]).to(device)
    plan = torch.stack([torch.as_tensor(p).double() for p in plans]).to(device)
    return plan, others, ptr, lw_ego, lw_others


def run_kernel(lib, plan, others, ptr, lw_ego, lw_others, dt=DT, scale=3):
    oi, od, st = EP.planner_eval_metrics(plan, others, ptr, lw_ego, lw_others, dt, scale=scale, lib=lib)
    return oi.cpu().numpy(), od.cpu().numpy(), st.cpu().numpy()


def note(key, err, bound):
    r = float(err) / float(bound)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    return r


def check_scene_against_fixture(g, mode, name, oi, od, extra_vel=0.0, extra_acc=0.0):
    p = '%s/%s/' % (mode, name)
    assert [int(v) for v in oi] == [int(g[p + k]) for k in ('did_collide', 'coll_time', 'coll_agt', 'coll_idx', 'accel_count')], p
    sc = fixture_scenes()[name]
    C = max(float(np.nanmax(np.abs(sc['others'][..., :2].numpy()))), float(np.abs(g[p + 'plan'][:, :2]).max()))
    want = float(g[p + 'coll_vel'])
    if int(oi[0]):
        if np.isnan(want):
            assert np.isnan(od[0])
        else:
            bound = 4 * EPS32 * C / DT + 4 * EPS32 * abs(want) + extra_vel
            r = note('%s coll_vel' % mode, abs(od[0] - want), bound)
            print('%s coll_vel %.9g want %.9g err/bound %.3g' % (p, od[0], want, r))
            assert r <= 1.0, p
    else:
        assert np.isnan(od[0]) and np.isnan(want)
    for col, key in ((1, 'mean_accel'), (3, 'mean_accel_fwd'), (5, 'mean_accel_lat')):
        want = float(g[p + key])
        if int(oi[4]) == 0:
            assert np.isnan(want), p
            continue
        got = od[col] / int(oi[4])
        bound = 4 * EPS64 * C / DT + 4 * EPS64 * abs(want) + extra_acc
        r = note('%s %s' % (mode, key), abs(got - want), bound)
        print('%s%s %.9g want %.9g err/bound %.3g' % (p, key, got, want, r))
        assert abs(got - want) <= bound, p


# ------------------------------------------------------------------------------------------------
# float64 numpy restatement (reference src/eval_planner.py:114-218 + src/losses/adv_gen_nusc.py:517-565, 625-644)
# ------------------------------------------------------------------------------------------------

def np_corners(pose, lw):
    hl, hw = 0.5 * float(lw[0]), 0.5 * float(lw[1])
    h = np.arctan2(float(pose[3]), float(pose[2]))
    c, s = np.cos(h), np.sin(h)
    return [(lx * c - ly * s + float(pose[0]), lx * s + ly * c + float(pose[1])) for lx, ly in ((-hl, -hw), (hl, -hw), (hl, hw), (-hl, hw))]


def np_area(p):
    return 0.5 * abs(sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p))))


def np_iou(a, b):
    poly = list(a)
    for e in range(4):
        if not poly:
            break
        ex, ey = b[e]
        dx, dy = b[(e + 1) % 4][0] - ex, b[(e + 1) % 4][1] - ey
        out = []
        for i in range(len(poly)):
            p, q = poly[i], poly[(i + 1) % len(poly)]
            si = dx * (p[1] - ey) - dy * (p[0] - ex)
            sj = dx * (q[1] - ey) - dy * (q[0] - ex)
            if si >= 0:
                out.append(p)
            if (si >= 0) != (sj >= 0):
                t = si / (si - sj)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
    inter = np_area(poly) if len(poly) >= 3 else 0.0
    return inter / (np_area(a) + np_area(b) - inter)


def np_interp(x, scale, dtype):
    """F.interpolate(mode='linear', align_corners=False) along axis -2 in ``dtype`` + heading renormalisation."""
    x = np.asarray(x, dtype=dtype)
    T = x.shape[-2]
    j = np.arange(T * scale).astype(dtype)
    src = np.maximum(dtype(1.0 / scale) * (j + dtype(0.5)) - dtype(0.5), dtype(0.0)).astype(dtype)
    i0 = np.minimum(np.floor(src).astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    w1 = (src - i0.astype(dtype)).astype(dtype)
    w0 = (dtype(1.0) - w1).astype(dtype)
    with np.errstate(invalid='ignore'):
        u = (w0[:, None] * x[..., i0, :]).astype(dtype) + (w1[:, None] * x[..., i1, :]).astype(dtype)
        nrm = np.sqrt(u[..., 2] * u[..., 2] + u[..., 3] * u[..., 3]).astype(dtype)
        u[..., 2] /= nrm
        u[..., 3] /= nrm
    return u


def np_metrics(plan, others, lw_ego, lw_others, dt, scale):
    """-> (ints [did, time, agt, idx, count], floats [vel, sum, max, sum, max, sum, max], smallest |IoU - 0.02|)"""
    plan = np.asarray(plan, dtype=np.float64)
    others = np.asarray(others, dtype=np.float32)
    T, n = plan.shape[0], others.shape[0]
    fp, fo = np_interp(plan, scale, np.float64), np_interp(others, scale, np.float32)
    times = np.full((n,), T * scale, dtype=np.int64)
    margin = np.inf
    ego = [np_corners(fp[j], lw_ego) for j in range(T * scale)]
    for a in range(n):
        for j in range(T * scale):
            if np.isnan(fo[a, j]).any():
                continue
            iou = np_iou(ego[j], np_corners(fo[a, j], lw_others[a]))
            margin = min(margin, abs(iou - 0.02))
            if iou > 0.02 and times[a] == T * scale:
                times[a] = j
    did = bool((times < T * scale).any())
    ct, ca = int(times.min()), int(times.argmin())
    idx = int((ct * (dt / float(scale))) / dt) if did else T - 1
    vel = np.nan
    if did:
        f1 = idx if idx > 0 else 1
        o = others.astype(np.float64)
        rel = (plan[f1, :2] - plan[f1 - 1, :2]) / dt - (o[ca, f1, :2] - o[ca, f1 - 1, :2]) / dt
        vel = float(np.sqrt(rel[0] * rel[0] + rel[1] * rel[1]))
    fl = [vel] + [0.0] * 6
    count = 0
    pos, head = plan[:idx + 1, :2], plan[:idx + 1, 2:]
    if pos.shape[0] > 2:
        v = (pos[1:] - pos[:-1]) / dt
        s = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2)
        uh = head / np.sqrt(head[:, 0:1] ** 2 + head[:, 1:2] ** 2)
        pv = s[:, None] * uh[:-1]
        fwd = np.abs((s[1:] - s[:-1]) / dt)
        acc = (pv[1:] - pv[:-1]) / dt
        lat = np.abs(acc[:, 0] * -uh[:-2, 1] + acc[:, 1] * uh[:-2, 0])
        accn = np.sqrt(acc[:, 0] ** 2 + acc[:, 1] ** 2)
        count = len(fwd)
        for c, series in enumerate((accn, fwd, lat)):
            tot = 0.0
            for x in series:
                tot += float(x)
            fl[1 + 2 * c], fl[2 + 2 * c] = tot, float(series.max())
    return [int(did), ct, ca if did else 0, idx, count], fl, margin


def synthetic_case(n, T, key):
    """One scene of ``n`` others around an ego driving along +x with a gentle turn and varying speed; others drift across its path
    at different times, one has a NaN head, one a NaN tail."""
    from strive_amd import synth
    t = 0.5 * (np.arange(T) + 1)
    sp = 6.0 + 1.5 * np.sin(0.7 * t)
    hh = 0.04 * t
    x = 100.0 + np.cumsum(sp * np.cos(hh) * 0.5)
    y = 120.0 + np.cumsum(sp * np.sin(hh) * 0.5)
    plan = np.stack([x, y, 1.3 * np.cos(hh), 1.3 * np.sin(hh)], -1)          # (un-normalised headings: the kernel renormalises)
    u = lambda shape, k, lo, hi: synth.counter_uniform(shape, '%s/%s' % (key, k), lo, hi)
    ox = 100.0 + u((n, 1), 'x', 0.0, 40.0) + u((n, 1), 'vx', -3.0, 6.0) * t[None]
    oy = 120.0 + u((n, 1), 'y', -14.0, 14.0) + u((n, 1), 'vy', -2.5, 2.5) * t[None]
    oh = u((n, 1), 'h', -3.1, 3.1) + 0.0 * t[None]
    others = np.stack([ox, oy, np.cos(oh), np.sin(oh)], -1).astype(np.float32)
    if n > 1 and T > 2:
        others[1, :1] = np.nan
        others[n // 2, T - 1:] = np.nan
    lw_o = np.stack([4.2 + 0.4 * u((n,), 'l', 0.0, 1.0), 1.9 + 0.2 * u((n,), 'w', 0.0, 1.0)], -1).astype(np.float32)
    return plan, others, np.asarray([4.5, 2.0], dtype=np.float32), lw_o


SHAPES = [(n, T, scale) for n in (1, 2, 17, 65) for T, scale in ((2, 1), (3, 3), (12, 3), (12, 1))]      # 65 x 12 x 3 = 2340 pairs > 256
_RESTATED = {}


def restated(n, T, scale):
    key = (n, T, scale)
    if key not in _RESTATED:
        case = synthetic_case(n, T, 'pe/%d/%d' % (n, T))
        _RESTATED[key] = (case, np_metrics(*case, DT, scale))
    return _RESTATED[key]


def close_to_restatement(od, want, what):
    """float64 and the same formulas on both sides: every float within ``16 * eps64`` RELATIVE of the expected value (equal where
    that is 0)."""
    for c in range(7):
        if np.isnan(want[c]):
            assert np.isnan(od[c]), (what, c)
            continue
        err, tol = abs(od[c] - want[c]), 16 * EPS64 * abs(want[c])
        if err > 0:
            r = note('%s col %d' % (what.split()[0], c), err, tol) if tol > 0 else float('inf')
            print('%s col %d: got %.17g want %.17g err %.3g err/(16 eps64 |want|) %.3g' % (what, c, od[c], want[c], err, r))
        assert err <= tol, (what, c, od[c], want[c], tol)


# ------------------------------------------------------------------------------------------------
# CPU: the kernel on the host emulation
# ------------------------------------------------------------------------------------------------

def test_fixture_tie_condition_and_cases():
    g = golden(FIX)
    for mode in ('plan', 'replay'):
        names = [str(n) for n in g[mode + '/names']]
        assert names == ['adv_' + s[0] for s in mgp.ADV_SCENES] + ['regular_seq_00000', 'regular_seq_00002', 'regular_seq_00003']
        for n in names:
            iou = g['%s/%s/iou' % (mode, n)]
            assert np.nanmin(np.abs(iou - 0.02)) > 1e-3, (mode, n)
            assert iou.shape == (fixture_scenes()[n]['others'].shape[0], 3 * fixture_scenes()[n]['T'])
    r = lambda n, k: g['replay/adv_%s/%s' % (n, k)]
    assert int(r('sc_0000_mid', 'did_collide')) and 3 <= int(r('sc_0000_mid', 'coll_idx')) <= 8 and r('sc_0000_mid', 'iou').shape[0] >= 17
    assert int(r('sc_0001_step0', 'coll_time')) == 0 and r('sc_0001_step0', 'iou').shape[0] == 1
    assert int(r('sc_0002_cidx1', 'coll_idx')) == 1 and int(r('sc_0002_cidx1', 'accel_count')) == 0
    assert int(r('sc_0003_last', 'did_collide')) and int(r('sc_0003_last', 'coll_idx')) == 11
    assert not int(r('sc_0004_none', 'did_collide'))
    hit = np.nan_to_num(r('sc_0005_pair', 'iou'), nan=0.0) > 0.02
    assert int(hit[1].argmax()) == int(hit[2].argmax()) == int(r('sc_0005_pair', 'coll_time')) and int(r('sc_0005_pair', 'coll_agt')) == 1
    assert np.isnan(r('sc_0006_nantail', 'iou')[2, -1]) and int(r('sc_0006_nantail', 'coll_agt')) == 2
    assert sorted(set(fixture_scenes()[n]['T'] for n in names)) == [8, 12]


@pytest.mark.parametrize('mode', ['plan', 'replay'])
def test_kernel_matches_reference_fixture(emu, mode):
    g = golden(FIX)
    names = [str(n) for n in g[mode + '/names']]
    for T in (12, 8):
        sel = [n for n in names if fixture_scenes()[n]['T'] == T]
        oi, od, st = run_kernel(emu, *stack(sel, [g['%s/%s/plan' % (mode, n)] for n in sel]))
        assert not st.any()
        for b, n in enumerate(sel):
            check_scene_against_fixture(g, mode, n, oi[b], od[b])
    print('error / bound: %r' % RATIOS)


def test_scene_outputs_do_not_depend_on_the_batch(emu):
    g = golden(FIX)
    names = [str(n) for n in g['plan/names'] if fixture_scenes()[str(n)]['T'] == 12][:7]
    assert len(names) == 7
    plans = [g['plan/%s/plan' % n] for n in names]
    oi7, od7, _ = run_kernel(emu, *stack(names, plans))
    oir, odr, _ = run_kernel(emu, *stack(names[::-1], plans[::-1]))
    for b, n in enumerate(names):
        oi1, od1, _ = run_kernel(emu, *stack([n], [plans[b]]))
        assert oi1[0].tobytes() == oi7[b].tobytes() == oir[6 - b].tobytes()
        assert od1[0].tobytes() == od7[b].tobytes() == odr[6 - b].tobytes()


@pytest.mark.parametrize('copy', [True, False])
def test_compute_metrics_matches_reference_dictionaries(emu_ops, copy):
    g = golden(FIX)
    for mode in ('plan', 'replay'):
        metrics, cnt, tot = {}, {}, {}
        per_scene = []
        for n in [str(v) for v in g[mode + '/names']]:
            sc = fixture_scenes()[n]
            plan = torch.from_numpy(g['%s/%s/plan' % (mode, n)])
            metrics, cnt, tot, cur = EP.compute_metrics(plan, sc['others'], sc['veh_att'], DT, metrics, cnt, tot, n.split('_')[0],
                                                        log_no_prefix_copy=copy)
            per_scene.append(cur)
            p = '%s/%s/' % (mode, n)
            assert cur['did_collide'] == int(g[p + 'did_collide'])
            assert ('coll_vel' in cur) == bool(cur['did_collide']) and ('mean_accel' in cur) == (int(g[p + 'accel_count']) > 0)
            assert set(cur) <= {'did_collide', 'coll_vel', 'mean_accel', 'mean_accel_fwd', 'mean_accel_lat'}
        want_keys = [str(k) for k in g[mode + '/metric_keys']]
        want_freq = [str(k) for k in g[mode + '/freq_keys']]
        if not copy:
            want_keys = [k for k in want_keys if not k.startswith('total_')]
            want_freq = [k for k in want_freq if not k.startswith('total_')]
        assert list(metrics.keys()) == want_keys and list(cnt.keys()) == list(tot.keys()) == want_freq
        for k in want_freq:
            i = [str(v) for v in g[mode + '/freq_keys']].index(k)
            assert (cnt[k], tot[k]) == (int(g[mode + '/freq_cnt'][i]), int(g[mode + '/freq_total'][i]))
        for k in want_keys:
            i = [str(v) for v in g[mode + '/metric_keys']].index(k)
            assert isinstance(metrics[k], PooledMetric) and metrics[k].count == int(g[mode + '/metric_count'][i])
            want = float(g[mode + '/metric_mean'][i])
            eps = EPS32 if k.endswith('coll_vel') else EPS64
            assert abs(metrics[k].mean() - want) <= 4 * eps * 256.0 / DT + 4 * eps * abs(want), (mode, k, metrics[k].mean(), want)


def test_metric_helpers():
    m = log_metric({}, 'a', np.array([1.0, 2.0, 6.0]))
    m = log_metric(m, 'a', np.array([3.0]))
    assert m['a'].count == 4 and m['a'].mean() == 3.0 and len(m['a']) == 4
    c, t = log_freq_stat({}, {}, 'f', 1, 1)
    c, t = log_freq_stat(c, t, 'f', 0, 1)
    lines = []
    print_metrics(m, c, t, log=lines.append)
    assert lines == ['a = 3.000000', 'f = 0.500000']


@pytest.fixture()
def replay_runs(emu_ops, tmp_path):
    runs = {}
    for bs in (1, 64):
        plans = []
        out = str(tmp_path / ('bs%d' % bs))
        runs[bs] = EP.run_planner_eval(None, None, None, DT, 'cpu', out, None, None, scenario_dir=mgp.SCEN_DIR, skip_regular=True,
                                       eval_replay_planner=True, batch_scenes=bs, details_out=plans) + (plans, out)
    return runs


def test_run_planner_eval_replay(replay_runs):
    g = golden(FIX)
    metrics, cnt, tot, names, seqs, plans, out = replay_runs[64]
    assert names == ['adv_' + s[0] for s in mgp.ADV_SCENES] == sorted(names)
    # pooled means: np.mean over the concatenated frames of all scenes (not a mean of per-scene means)
    for key, col in (('adv_accel', 'mean_accel'), ('adv_accel_fwd', 'mean_accel_fwd'), ('adv_accel_lat', 'mean_accel_lat')):
        cnts = np.array([int(g['replay/%s/accel_count' % n]) for n in names])
        means = np.array([float(g['replay/%s/%s' % (n, col)]) for n in names])
        pooled = float(np.nansum(means * cnts) / cnts.sum())
        assert metrics[key].count == int(cnts.sum()) == metrics['total_' + key[4:]].count
        tol = 4 * EPS64 * 256.0 / DT + 4 * EPS64 * abs(pooled)
        assert abs(metrics[key].mean() - pooled) <= tol
        i = [str(k) for k in g['replay/metric_keys']].index(key)           # the reference's own np.mean over the concatenated frames
        assert metrics[key].count == int(g['replay/metric_count'][i]) and abs(metrics[key].mean() - float(g['replay/metric_mean'][i])) <= tol
    assert len(set(cnts[cnts > 0])) > 1, 'scenes contribute different numbers of frames, so a mean of means would differ'
    assert cnt['adv_coll'] == sum(int(g['replay/%s/did_collide' % n]) for n in names) and tot['adv_coll'] == len(names)
    for n, cur, det in zip(names, seqs, plans):
        assert sorted(cur) == ['coll_vel', 'did_collide', 'mean_accel', 'mean_accel_fwd', 'mean_accel_lat']
        assert cur['did_collide'] == int(g['replay/%s/did_collide' % n])
        assert np.array_equal(det['plan'].numpy(), g['replay/%s/plan' % n].astype(np.float64))
        assert [det[k] for k in DISCRETE] == [int(g['replay/%s/%s' % (n, k)]) for k in DISCRETE], n
    # one call per scene and one call per group give the same results, bit for bit
    m1, c1, t1, names1, seqs1, plans1, _ = replay_runs[1]
    assert names1 == names and c1 == cnt and t1 == tot
    for a, b in zip(seqs, seqs1):
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    # (the pooled totals are summed scene by scene in both runs)
    assert {k: (v.total, v.count) for k, v in metrics.items()} == {k: (v.total, v.count) for k, v in m1.items()}
    rows = list(csv.reader(open(os.path.join(out, 'all_eval_results.csv'))))
    assert rows[0] == ['scene', 'coll_vel', 'did_collide', 'mean_accel', 'mean_accel_fwd', 'mean_accel_lat'] and rows[0][1:] == sorted(rows[0][1:])
    assert [r[0] for r in rows[1:]] == names and rows[5][1] == 'nan'


@pytest.mark.parametrize('n,T,scale', SHAPES)
def test_kernel_matches_restatement(emu, n, T, scale):
    (plan, others, lw_e, lw_o), (wi, wf, margin) = restated(n, T, scale)
    assert margin > 1e-9, 'a tie at the threshold: choose other poses'
    oi, od, st = run_kernel(emu, torch.from_numpy(plan)[None], torch.from_numpy(others), [0, n], torch.from_numpy(lw_e)[None],
                            torch.from_numpy(lw_o), scale=scale)
    assert int(st[0]) == 0 and [int(v) for v in oi[0]] == wi
    close_to_restatement(od[0], wf, 'restatement %d/%d/%d' % (n, T, scale))


def test_restated_shapes_cover_hits_misses_and_a_later_agent():
    res = [restated(*s)[1][0] for s in SHAPES]
    assert any(r[0] for r in res) and any(not r[0] for r in res) and any(r[2] > 0 for r in res)
    assert any(r[4] > 0 for r in res) and any(r[0] and r[4] == 0 for r in res)


def test_refusals_and_edge_cases(emu):
    (plan, others, lw_e, lw_o), _ = restated(2, 12, 3)
    pl, ot, le, lo = torch.from_numpy(plan)[None], torch.from_numpy(others), torch.from_numpy(lw_e)[None], torch.from_numpy(lw_o)
    with pytest.raises(L.StriveHipError, match='T must be at least 2'):
        run_kernel(emu, pl[:, :1], ot[:, :1], [0, 2], le, lo)
    with pytest.raises(L.StriveHipError, match='scale'):
        run_kernel(emu, pl, ot, [0, 2], le, lo, scale=0)
    oi = torch.zeros((1, 5), dtype=torch.int32)
    od = torch.zeros((1, 7), dtype=torch.float64)
    st = torch.zeros((1,), dtype=torch.int32)
    ptr = torch.tensor([0, 2], dtype=torch.int32)
    args = [L.ptr(pl.contiguous()), L.ptr(ot), L.ptr(ptr), L.ptr(le), L.ptr(lo), 1, 2, 12, 3, DT, L.ptr(oi), L.ptr(od), L.ptr(st), None]
    for k in (0, 1, 2, 3, 4, 10, 11, 12):
        bad = list(args)
        bad[k] = None
        with pytest.raises(L.StriveHipError, match='null argument'):
            emu.call('strive_planner_eval_metrics', *bad)
    # a scene without others: its status is set, its rows and the other scenes' outputs are untouched
    alone_i, alone_d, _ = run_kernel(emu, pl, ot, [0, 2], le, lo)
    oi3, od3, st3 = run_kernel(emu, pl.repeat(3, 1, 1), torch.cat([ot, ot]), [0, 2, 2, 4], le.repeat(3, 1), torch.cat([lo, lo]))
    assert st3.tolist() == [0, 1, 0] and (oi3[1] == -1).all() and np.isnan(od3[1]).all()
    for b in (0, 2):
        assert oi3[b].tobytes() == alone_i[0].tobytes() and od3[b].tobytes() == alone_d[0].tobytes()
    # offsets that leave ``others`` are refused per scene, nothing is read
    _, _, stb = run_kernel(emu, pl, ot, [0, 5], le, lo)
    assert stb.tolist() == [2]
    # a batch without any collision
    far = ot.clone()
    far[..., 0] += 150.0
    oin, odn, stn = run_kernel(emu, pl.repeat(2, 1, 1), torch.cat([far, far]), [0, 2, 4], le.repeat(2, 1), torch.cat([lo, lo]))
    assert not stn.any() and oin[:, 0].tolist() == [0, 0] and oin[:, 1].tolist() == [36, 36] and oin[:, 3].tolist() == [11, 11]
    assert oin[:, 4].tolist() == [10, 10] and np.isnan(odn[:, 0]).all() and np.isfinite(odn[:, 1:]).all()


def test_grouping_is_pure_host_logic():
    steps = [12, 12, 8, 8, 12, 12, 12, 12, 12, 12]
    maps = ['a', 'b', 'a', 'a', 'a', 'b', 'c', 'd', 'e', 'a']
    groups = EP.group_scenes(steps, maps, 64)
    assert groups == [[0, 1], [2, 3], [4, 5, 6, 7], [8, 9]]                  # T changes twice; the fifth map opens a group
    assert [i for grp in groups for i in grp] == list(range(10))
    assert EP.group_scenes(steps, maps, 1) == [[i] for i in range(10)]
    assert EP.group_scenes(steps, maps, 3) == [[0, 1], [2, 3], [4, 5, 6], [7, 8, 9]]
    assert EP.group_scenes([], [], 4) == []
    with pytest.raises(ValueError):
        EP.group_scenes(steps, maps, 0)


def test_cli_needs_a_lane_world(capsys):
    with pytest.raises(SystemExit, match='map environment with lane graphs must be supplied from Python'):
        EP.main(['--scenario_dir', mgp.SCEN_DIR, '--skip_regular'])
    args = EP.get_parser().parse_args(['--planner_smax', '20', '--planner_predsfacs', '0.5', '1.0', '--batch_scenes', '8'])
    assert args.planner_smax == 20.0 and args.planner_predsfacs == [0.5, 1.0] and args.planner_nsteps == 25 and args.batch_scenes == 8


# ------------------------------------------------------------------------------------------------
# MI355X
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_kernel_matches_emulator(emu):
    g = golden(FIX)
    hip = L.get_lib()
    cases = []
    for mode in ('plan', 'replay'):
        names = [str(n) for n in g[mode + '/names']]
        for T in (12, 8):
            sel = [n for n in names if fixture_scenes()[n]['T'] == T]
            cases.append((stack(sel, [g['%s/%s/plan' % (mode, n)] for n in sel]), 3, T))
    (plan, others, lw_e, lw_o), _ = restated(65, 12, 3)
    cases.append(((torch.from_numpy(plan)[None], torch.from_numpy(others), np.array([0, 65]), torch.from_numpy(lw_e)[None],
                   torch.from_numpy(lw_o)), 3, 12))
    for ci, ((plan, others, ptr, lw_e, lw_o), scale, T) in enumerate(cases):
        wi, wd, ws = run_kernel(emu, plan, others, ptr, lw_e, lw_o, scale=scale)
        gi, gd, gs = run_kernel(hip, plan.to(DEV), others.to(DEV), ptr, lw_e.to(DEV), lw_o.to(DEV), scale=scale)
        assert np.array_equal(gi, wi) and np.array_equal(gs, ws)
        for b in range(gd.shape[0]):
            close_to_restatement(gd[b], wd[b], 'gpu case %d scene %d' % (ci, b))
    print('error / bound: %r' % RATIOS)


@pytest.fixture(scope='module')
def gpu_runs(tmp_path_factory):
    lg, regular = mgp.regular_inputs()
    import make_golden as mg
    env = mg._LaneEnv(lg)
    sn, an = MeanStdNormalizer(*state_norm_tensors()), MeanStdNormalizer(*att_norm_tensors())
    runs = {}
    for bs in (64, 1):
        plans = []
        out = str(tmp_path_factory.mktemp('pe%d' % bs))
        runs[bs] = EP.run_planner_eval(PlannerConfig(**CONFIG_DICT['default']), regular, env, DT, DEV, out, sn, an, scenario_dir=mgp.SCEN_DIR,
                                       batch_scenes=bs, details_out=plans) + (plans,)
    return runs


G17_NAMES = ['adv_' + s[0] for s in mgp.ADV_SCENES] + ['regular_seq_00000', 'regular_seq_00002', 'regular_seq_00003']


@pytest.mark.gpu
@pytest.mark.parametrize('name', G17_NAMES)
def test_gpu_driver_matches_reference_fixture(gpu_runs, name):
    """One scene of the full driver (device planner + metrics kernel, batch_scenes 64) against the reference's own run.  (The
    fixture records the reference with its initial world widened to float64, the arithmetic of the numpy it was written for:
    make_golden_planner_eval._widen_initial_world.  Under numpy >= 2 its fp32 scalars move the 19-agent scene's plan by 2.67e-7 m.)"""
    g = golden(FIX)
    metrics, cnt, tot, names, seqs, plans = gpu_runs[64]
    assert names == G17_NAMES == [str(n) for n in g['plan/names']]
    extra_vel = 4 * PLAN_ATOL / DT
    extra_acc = PLAN_ATOL * (8 / (DT * DT) + 8 * SPEED_MAX / DT)
    i = names.index(name)
    cur, det, want = seqs[i], plans[i], g['plan/%s/plan' % name]
    plan = det['plan']
    print('%s: max |plan - reference| %.3g' % (name, float(np.abs(plan.numpy() - want).max())))
    np.testing.assert_allclose(plan.numpy(), want, rtol=0, atol=PLAN_ATOL)
    assert float(np.linalg.norm(np.diff(want[:, :2], axis=0), axis=1).max()) / DT < SPEED_MAX
    cntf = det['accel_count']
    oi = [cur['did_collide']] + [det[k] for k in DISCRETE]          # the driver's own discrete outputs, compared with the fixture's below
    od = [cur['coll_vel']] + [v for k in ('mean_accel', 'mean_accel_fwd', 'mean_accel_lat') for v in (cur[k] * max(cntf, 1), 0.0)]
    assert np.isnan(cur['mean_accel']) == (cntf == 0)
    check_scene_against_fixture(g, 'plan', name, oi, od, extra_vel=extra_vel, extra_acc=extra_acc)


@pytest.mark.gpu
def test_gpu_driver_dictionaries_match_reference_fixture(gpu_runs):
    g = golden(FIX)
    metrics, cnt, tot, names, seqs, plans = gpu_runs[64]
    assert [s['did_collide'] for s in seqs] == [int(g['plan/%s/did_collide' % n]) for n in names]
    assert list(metrics.keys()) == [str(k) for k in g['plan/metric_keys']]
    assert [metrics[k].count for k in metrics] == [int(v) for v in g['plan/metric_count']]
    assert [(cnt[k], tot[k]) for k in cnt] == list(zip(g['plan/freq_cnt'].tolist(), g['plan/freq_total'].tolist()))
    assert list(cnt.keys()) == [str(k) for k in g['plan/freq_keys']]


@pytest.mark.gpu
def test_gpu_driver_batch_sizes_agree_bitwise(gpu_runs):
    a, b = gpu_runs[64], gpu_runs[1]
    assert a[3] == b[3] and a[1] == b[1] and a[2] == b[2]
    for da, db in zip(a[5], b[5]):
        assert torch.equal(da['plan'], db['plan']) and [da[k] for k in DISCRETE] == [db[k] for k in DISCRETE]
    for sa, sb in zip(a[4], b[4]):
        assert json.dumps(sa, sort_keys=True) == json.dumps(sb, sort_keys=True)
