"""Batched scenario evaluation and collision clustering (strive_amd/eval_adv_gen.py, strive_amd/cluster_scenarios.py ->
strive_scenario_eval_metrics, strive_kmeans_step, strive_amd/csrc/eval_metrics.hip) against the reference's src/eval_adv_gen.py and
src/cluster_scenarios.py (fixture g18, tests/golden/make_golden_adv_eval.py) and against a float64 numpy restatement
(tests/adv_eval_restated.py).

Tolerances (derived, not fitted).  Coordinates are metres on the 256 m synthetic world, dt = 0.5 s, eps32 = 2^-23, eps64 = 2^-52,
C = max |coordinate| of the scene, S = 32 m/s bounds every speed of the fixture (the fastest agent moves 9.25 m/s, the fastest
lateral approach 5 m/s).  The reference runs its chains in fp32 on the fp32 inputs, the kernel in float64 on the same inputs, so
every bound is an upper bound of the REFERENCE's rounding error.

  * Integers, booleans and NaN-ness are EQUAL: the fixture's tie conditions keep every IoU more than 1e-3 from 0.02 (the kernel's
    float64 clip differs from the exact area of the fp32-rounded corners by ~1e-6), every drivable fraction more than two samples
    from 0.95, every grid ratio more than 1e-3 from a half-integer.  Rates of integers (veh_coll_rate, env_coll_*) are equal.
  * Accelerations: a velocity component is (p1 - p0) / dt: <= 2 eps32 C / dt; the speed, its product with the unit heading (2 eps32
    for the normalisation, scaled by S) and the second difference / dt double that twice: ``8 eps32 C / dt^2 + 8 eps32 S / dt``
    absolute per frame, plus ``8 eps32 |a|`` for the roundings of the result chain (norm, abs, dot with the lateral direction).  A
    mean over n frames is off by at most the largest frame error plus the fp32 summation, ``n eps32 |mean|``.
  * Log-likelihood of one row: ``(D + 8) eps32 sum_d |term_d|`` (D additions, 8 roundings inside a term: sqrt, log, subtraction,
    square, doubling, division, two subtractions).  The others' mean over n rows: the mean of the rows' bounds plus ``n eps32`` times
    the mean of sum_d |term_d|.
  * Planner fit, position: ``4 eps32 C`` absolute (two subtractions of coordinates, the norm) + ``(4 + n) eps32 |mean|``.  Angle in
    radians: the dot product of two fp32-normalised headings is off by <= 6 eps32 (2 per normalisation, 2 for products and sum);
    acos has the derivative 1 / sqrt(1 - x^2), so a frame with |x| <= 1 - 1e-3 is off by ``6 eps32 / sqrt(1 - x^2) + 4 eps32 |angle|``;
    nearer to +-1 the conditioning is unbounded and the frame is bounded by acos(1 - 6 eps32) <= ``sqrt(12 eps32)`` instead (the
    fixture's frames there have identical headings and an exact dot product of 1).  Mean: the mean of the frame bounds + ``n eps32
    |mean|``.  Degrees: the radian bound times 180 / pi plus ``2 eps32 |degrees|`` for the conversion.
  * Collision features: hvec is a sum of two products of fp32 unit-vector components (<= 4 eps32) of headings interpolated and
    renormalised in fp32 (<= 2 eps32 each): ``8 eps32``.  angvec is the rotated, normalised difference of two interpolated positions
    (3 eps32 C each) at distance r: ``16 eps32 C / r + 8 eps32``.  h = atan2(hvec): ``16 eps32 + 4 eps32 |h|``; ang = atan2(angvec):
    twice the angvec bound + ``4 eps32 |ang|``.  rel_s: ``4 eps32 C / dt + 4 eps32 |rel_s|`` (as coll_vel in test_planner_eval.py).
  * Pooled means (the dictionaries, eval_total_*.csv): the largest per-scene bound of that quantity + ``n eps32 |mean|``, n = pooled
    count (np.mean of fp32 values).
  * Kernel against the restatement, and the GPU against the emulator: same formulas, float64: ``16 eps64`` relative to the expected
    value; for sums relative to sum |terms| (the log-likelihood terms have both signs).  atan2 / acos / log of libm differ by an ulp.
  * k-means against scikit-learn: labels and n_iter equal (every point's two nearest centres differ by > 1e-9 in squared distance at
    every iteration); the features are unit vectors and every centre is a mean of at most N of them: centres within ``4 N eps64``,
    inertia within ``4 N eps64 inertia + 4 N eps64``.

Largest error / bound per quantity: printed by the tests; profiles/r17_adv_eval_ratios.md (written when STRIVE_WRITE_RATIOS is set).
"""
import csv
import io
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import adv_eval_restated as RS
import make_golden_adv_eval as mga
from util import golden
from strive_amd import _lib as L
from strive_amd import ops
from strive_amd import synth
from strive_amd import eval_adv_gen as EA
from strive_amd import cluster_scenarios as CS
from strive_amd.utils.scenario_gen import PooledMetric

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

FIX = 'g18_adv_eval.npz'
DT = mga.DT
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
SPEED_MAX = 32.0
DEV = 'cuda:0'
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
RATIOS = {}                       # largest error / bound seen per quantity
DISCRETE = ('adv_collide', 'coll_t', 'coll_agt', 'atk_agt', 'num_coll_veh', 'num_traj_veh', 'env_coll_atk', 'env_coll_others', 'n_others',
            'env_L', 'env_W')
ACCEL_KEYS = ['adv_%s_%s' % (w, s) for w in ('atk', 'other') for s in ('accel', 'accel_fwd', 'accel_lat')]


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


def note(key, err, bound):
    r = float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else float('inf'))
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    return r


def teardown_module(module):
    print('error / bound: %s' % json.dumps(RATIOS, indent=1, sort_keys=True))
    if os.environ.get('STRIVE_WRITE_RATIOS') and RATIOS:
        with open(os.path.join(REPO, 'profiles', os.environ['STRIVE_WRITE_RATIOS']), 'w') as f:
            f.write('| quantity | largest error / bound |\n|---|---|\n')
            for k in sorted(RATIOS):
                f.write('| %s | %.3g |\n' % (k, RATIOS[k]))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------

_CACHE = {}


def scenarios():
    """{category: [scene dicts]} of g18, read once (quant_eval writes into the dicts: tests that call it take a copy)."""
    if 'scen' not in _CACHE:
        _CACHE['scen'] = {c: EA.read_adv_scenes(os.path.join(mga.SCEN_DIR, c)) for c in mga.CATEGORIES}
    return _CACHE['scen']


def fresh_scenarios():
    return {c: [dict(s) for s in v] for c, v in scenarios().items()}


def all_scenes():
    return [(c, s) for c in mga.CATEGORIES for s in scenarios()[c]]


def map_env(device='cpu'):
    key = 'env/' + str(device)
    if key not in _CACHE:
        env = EA.SyntheticMapWorld()
        env.nusc_raster, env.nusc_dx = env.nusc_raster.to(device), env.nusc_dx.to(device)
        _CACHE[key] = env
    return _CACHE[key]


def run_scenes(lib, scenes, want_feat, device='cpu', with_map=True, with_latents=True):
    out = {}
    order = []
    T_of = lambda s: int(s['fut_adv'].shape[1])
    for T in sorted(set(T_of(s) for s in scenes), reverse=True):
        sel = [i for i, s in enumerate(scenes) if T_of(s) == T]
        args = EA._stack([scenes[i] for i in sel], device, with_latents=with_latents)
        oi, od, st = EA.scenario_eval_metrics(map_env=map_env(device) if with_map else None, mapix=[0] * len(sel) if with_map else None,
                                              want_feat=[want_feat[i] for i in sel], lib=lib, **args)
        assert not st.cpu().numpy().any()
        for k, i in enumerate(sel):
            out[i] = (oi[k].cpu().numpy(), od[k].cpu().numpy())
        order += sel
    return [out[i] for i in range(len(scenes))]


def restated_scene(scene, want_feat, with_map=True, with_latents=True):
    key = ('rs', scene['name'], want_feat, with_map, with_latents)
    if key not in _CACHE:
        env = map_env()
        lat = dict(z=scene['z_adv'].numpy(), mu=scene['z_prior_mean'].numpy(), var=scene['z_prior_var'].numpy()) if with_latents else {}
        fit = scene['fut_internal_ego'].numpy() if 'fut_internal_ego' in scene else None
        _CACHE[key] = RS.scene_metrics(scene['fut_adv'].numpy(), scene['veh_att'].numpy(), scene['attack_agt'], float(scene['dt']), fit=fit,
                                       raster=env.nusc_raster.numpy() if with_map else None, dx=env.nusc_dx.numpy(), want_feat=want_feat, **lat)
    return _CACHE[key]


def close_to_restatement(oi, od, want, what):
    """Integers equal; floats within 16 eps64 relative to the expected value, sums relative to the sum of |terms|."""
    for k, c in EA.I.items():
        assert int(oi[c]) == int(want['i'][k]), (what, k, int(oi[c]), want['i'][k])
    for k, c in EA.D.items():
        w = want['d'][k]
        if np.isnan(w):
            assert np.isnan(od[c]), (what, k, od[c])
            continue
        den = want['abs'].get(k, abs(w))
        den = abs(w) if np.isnan(den) else max(den, abs(w))
        err, tol = abs(od[c] - w), 16 * EPS64 * den
        if err > 0:
            r = note('restated ' + k, err, tol)
            print('%s %s: got %.17g want %.17g err %.3g err/bound %.3g' % (what, k, od[c], w, err, r))
        assert err <= tol, (what, k, od[c], w, tol)


# ------------------------------------------------------------------------------------------------
# bounds against the reference
# ------------------------------------------------------------------------------------------------

def scene_bounds(scene, g):
    """{seq_metrics key: bound} for one fixture scene, from the formulas of the module docstring."""
    n = scene['name']
    fut = scene['fut_adv'].numpy().astype(np.float64)
    C = float(np.nanmax(np.abs(fut[..., :2])))
    CT, atk = int(g[n + '/coll_t']), int(g[n + '/atk_agt'])
    others = [a for a in range(1, fut.shape[0]) if a != atk]
    seq = dict(zip([str(k) for k in g[n + '/seq_keys']], g[n + '/seq_vals'].tolist()))
    cnt = lambda k: int(g[n + '/counts/' + k]) if (n + '/counts/' + k) in g.files else 0
    b = {}
    for k in ACCEL_KEYS:
        if not np.isnan(seq[k]):
            b[k] = 8 * EPS32 * C / DT ** 2 + 8 * EPS32 * SPEED_MAX / DT + (8 + cnt(k)) * EPS32 * abs(seq[k])
    z, m, v = [scene[k].numpy().astype(np.float64) for k in ('z_adv', 'z_prior_mean', 'z_prior_var')]
    D = z.shape[1]
    ab = np.abs(-np.log(np.sqrt(v))) + RS.LOG_SQRT_2PI + (z - m) ** 2 / (2 * v)
    ab = ab.sum(1)
    b['adv_z_ll_atk'] = (D + 8) * EPS32 * ab[atk]
    if others:
        b['adv_z_ll_other'] = (D + 8 + len(others)) * EPS32 * float(np.mean(ab[others]))
    if 'fut_internal_ego' in scene:
        if CT > 0:
            q = scene['fut_internal_ego'].numpy().astype(np.float64)[:CT]
            e = fut[0, :CT]
            x = np.clip(np.sum(e[:, 2:] / np.linalg.norm(e[:, 2:], axis=1, keepdims=True) * q[:, 2:] / np.linalg.norm(q[:, 2:], axis=1, keepdims=True), axis=1),
                        -1.0, 1.0)
            ang = np.arccos(x)
            with np.errstate(divide='ignore'):
                frame = np.where(np.abs(x) <= 1 - 1e-3, 6 * EPS32 / np.sqrt(np.maximum(1 - x * x, 1e-300)) + 4 * EPS32 * ang, np.sqrt(12 * EPS32))
            b['match_plan_pos'] = 4 * EPS32 * C + (4 + CT) * EPS32 * abs(seq['match_plan_pos'])
            b['match_plan_ang_rad'] = float(frame.mean()) + CT * EPS32 * abs(seq['match_plan_ang_rad'])
            b['match_plan_ang'] = b['match_plan_ang_rad'] * 180.0 / np.pi + 2 * EPS32 * abs(seq['match_plan_ang'])
    return seq, b


def feat_bounds(scene, g):
    n = scene['name']
    fut = scene['fut_adv'].numpy().astype(np.float64)
    C = float(np.nanmax(np.abs(fut[..., :2])))
    ft, fa = int(g[n + '/fine_t']), int(g[n + '/fine_agt'])
    fine = RS.interp32(scene['fut_adv'].numpy(), RS.FEAT_SCALE).astype(np.float64)
    r = float(np.linalg.norm(fine[fa + 1, ft, :2] - fine[0, ft, :2]))
    av = 16 * EPS32 * C / r + 8 * EPS32
    return dict(hvec=8 * EPS32, angvec=av, h=16 * EPS32 + 4 * EPS32 * abs(float(g[n + '/feat_h'])), ang=2 * av + 4 * EPS32 * abs(float(g[n + '/feat_ang'])),
                rel_s=4 * EPS32 * C / DT + 4 * EPS32 * abs(float(g[n + '/feat_rel_s'])))


def check_value(key, got, want, bound, what):
    if np.isnan(want):
        assert np.isnan(got), (what, key, got)
        return
    assert not np.isnan(got), (what, key)
    if bound is None:
        assert got == want, (what, key, got, want)
        return
    r = note('reference ' + key, abs(got - want), bound)
    print('%s %s %.9g want %.9g err/bound %.3g' % (what, key, got, want, r))
    assert abs(got - want) <= bound, (what, key, got, want, bound)


def check_scene_against_fixture(g, cat, scene, oi, od):
    n = scene['name']
    I, D = EA.I, EA.D
    for k in ('did_collide', 'coll_t', 'coll_agt', 'atk_agt', 'n_others', 'num_coll_veh', 'num_traj_veh', 'env_L', 'env_W'):
        col = 'adv_collide' if k == 'did_collide' else k
        assert int(oi[I[col]]) == int(g[n + '/' + k]), (n, k)
    env = g[n + '/env_coll']
    atk = int(g[n + '/atk_agt'])
    others = [a for a in range(1, len(env)) if a != atk]
    assert int(oi[I['env_coll_atk']]) == int(env[atk]) and int(oi[I['env_coll_others']]) == (int(env[others].sum()) if int(env[0]) >= 0 else -1), n
    CT = int(g[n + '/coll_t'])
    if CT > 0:
        assert int(oi[I['env_frames']]) == int((~np.isnan(g[n + '/env_frac'])).sum())
        assert np.allclose([od[D['env_mean_l']] * 4, od[D['env_mean_w']] * 4], g[n + '/env_ratio'], rtol=0, atol=1e-5)
    cnt = lambda k: int(g[n + '/counts/' + k]) if (n + '/counts/' + k) in g.files else 0
    assert int(oi[I['atk_accel_cnt']]) == cnt('adv_atk_accel') == cnt('adv_atk_accel_lat') and int(oi[I['other_accel_cnt']]) == cnt('adv_other_accel')
    assert max(int(oi[I['ll_other_cnt']]), 0) == cnt('adv_z_ll_other') and max(int(oi[I['fit_cnt']]), 0) == cnt('match_plan_pos') == cnt('match_plan_ang')
    metrics, fc, ft, seq = EA._log_scene(oi, od, {}, {}, {}, True)
    want, bounds = scene_bounds(scene, g)
    assert list(seq.keys()) == [k for k in want if k != 'sol_success'] == list(EA.SEQ_KEYS)
    for k, v in seq.items():
        check_value(k, v, want[k], bounds.get(k), n)
    if cat != 'adv_failed':
        assert [int(oi[I[k]]) for k in ('feat_status', 'fine_t', 'fine_agt', 'lr_coll_t')] == [0] + [int(g[n + '/' + k]) for k in ('fine_t', 'fine_agt', 'lr_coll_t')]
        fb = feat_bounds(scene, g)
        for c, k in enumerate(('hvec_x', 'hvec_y')):
            check_value('hvec', od[D[k]], float(g[n + '/feat_hvec'][c]), fb['hvec'], n)
        for c, k in enumerate(('angvec_x', 'angvec_y')):
            check_value('angvec', od[D[k]], float(g[n + '/feat_angvec'][c]), fb['angvec'], n)
        for k in ('h', 'ang', 'rel_s'):
            check_value(k, od[D[k]], float(g[n + '/feat_' + k]), fb[k], n)
    else:
        assert int(oi[I['feat_status']]) == -1 and np.isnan(od[D['rel_s']])


# ------------------------------------------------------------------------------------------------
# CPU: the kernel on the host emulation
# ------------------------------------------------------------------------------------------------

def test_fixture_tie_conditions_and_cases():
    g = golden(FIX)
    names = [str(n) for n in g['names']]
    assert names == [s['name'] for s in mga.SCENES] and [str(c) for c in g['categories']] == [s['cat'] for s in mga.SCENES]
    for n in names:
        for k in ('iou_coarse', 'iou_pairs', 'iou_fine'):
            if n + '/' + k in g.files and g[n + '/' + k].size:
                assert np.nanmin(np.abs(g[n + '/' + k] - 0.02)) > 1e-3, (n, k)
        if int(g[n + '/env_L']) > 0:
            LW = int(g[n + '/env_L']) * int(g[n + '/env_W'])
            assert np.nanmin(np.abs(g[n + '/env_frac'] - 0.95)) > 2.0 / LW, n
            ratio = g[n + '/env_ratio']
            assert np.abs(ratio - np.floor(ratio) - 0.5).min() > 1e-3, n
    assert float(g['km/margin']) > 1e-9
    v = lambda n, k: g[n + '/' + k]
    seq = lambda n: dict(zip([str(k) for k in v(n, 'seq_keys')], v(n, 'seq_vals').tolist()))
    first = lambda iou: [int(np.argmax(r > 0.02)) if (r > 0.02).any() else -1 for r in np.nan_to_num(iou, nan=0.0)]
    mid = 'sc_0000_mid'                                                                    # a hit mid-horizon, 18 others, T 12
    assert int(v(mid, 'did_collide')) and 3 <= int(v(mid, 'coll_t')) <= 9 and v(mid, 'iou_coarse').shape == (18, 12)
    assert int(v(mid, 'num_coll_veh')) == 1 and v(mid, 'pair_marks')[6] == 1               # a non-ego pair before CT
    assert np.isnan(v(mid, 'iou_coarse')[13, -1]) and int(v(mid, 'coll_agt')) != 14        # NaN tail on a non-colliding agent
    assert v(mid, 'env_coll')[12] == 1 and v(mid, 'env_coll')[5] == 0 and int(v(mid, 'lr_coll_t')) > 0
    assert np.isfinite(seq(mid)['match_plan_pos'])
    s0 = 'sc_0001_step0'                                                                   # a hit at step 0, ego + attacker only
    assert int(v(s0, 'coll_t')) == 0 and np.isnan(seq(s0)['veh_coll_rate']) and int(v(s0, 'n_others')) == 0 and int(v(s0, 'lr_coll_t')) == 0
    ea = 'sc_0002_early'                                                                   # no attacker acceleration block, attacker off road
    assert int(v(ea, 'coll_t')) in (1, 2) and np.isnan(seq(ea)['adv_atk_accel']) and seq(ea)['env_coll_atk'] == 1 and v(ea, 'iou_coarse').shape == (3, 8)
    assert int(v(ea, 'coll_agt')) == 3 != scenarios()['adv_sol_success'][2]['attack_agt']
    tie = 'sc_0003_tie'                                                                    # two agents at the same step; nobody off road; no fit
    f = first(v(tie, 'iou_coarse'))
    assert f[1] == f[2] == int(v(tie, 'coll_t')) and int(v(tie, 'coll_agt')) == 2 and not v(tie, 'env_coll').any() and np.isnan(seq(tie)['match_plan_pos'])
    off = 'sc_0004_offroad'                                                                # another agent off road
    assert v(off, 'env_coll').tolist() == [0, 0, 1, 0] and seq(off)['env_coll_others'] == 0.5
    assert not int(v('sc_0005_none', 'did_collide')) and int(v('sc_0005_none', 'coll_t')) == 12
    assert not int(v('sc_0006_alone', 'did_collide')) and np.isnan(seq('sc_0006_alone')['env_coll_others'])
    # a pair that overlaps only at or after CT: agents 9, 10 of sc_0000_mid (restated over the whole horizon)
    sc = scenarios()['adv_sol_success'][0]
    fut, lw = sc['fut_adv'].numpy(), sc['veh_att'].numpy()
    hits = [RS.pose_iou(fut[9, t], lw[9], fut[10, t], lw[10]) > 0.02 for t in range(12)]
    CT = int(v(mid, 'coll_t'))
    assert not any(hits[:CT]) and any(hits[CT:]) and v(mid, 'pair_marks')[8] == 0


@pytest.mark.parametrize('batched', [False, True])
def test_kernel_matches_reference_fixture(emu, batched):
    g = golden(FIX)
    pairs = all_scenes()
    want_feat = [int(c != 'adv_failed') for c, _ in pairs]
    if batched:
        rows = run_scenes(emu, [s for _, s in pairs], want_feat)
    else:
        rows = [run_scenes(emu, [s], [w])[0] for (_, s), w in zip(pairs, want_feat)]
    for (cat, scene), (oi, od) in zip(pairs, rows):
        check_scene_against_fixture(g, cat, scene, oi, od)


def test_kernel_matches_restatement_on_the_fixture(emu):
    pairs = all_scenes()
    rows = run_scenes(emu, [s for _, s in pairs], [1] * len(pairs))
    for (cat, scene), (oi, od) in zip(pairs, rows):
        want = restated_scene(scene, True)
        assert want['margin_iou'] > 1e-3 and want['margin_frac'] > 2.0 and want['margin_grid'] > 1e-3
        close_to_restatement(oi, od, want, scene['name'])
    # no map, no latents: those columns absent, the others unchanged
    rows2 = run_scenes(emu, [s for _, s in pairs], [1] * len(pairs), with_map=False, with_latents=False)
    for (cat, scene), (oi, od), (oi_full, od_full) in zip(pairs, rows2, rows):
        close_to_restatement(oi, od, restated_scene(scene, True, with_map=False, with_latents=False), scene['name'] + ' bare')
        same = [EA.D[k] for k in EA.OUT_D if not k.startswith(('ll_', 'env_'))]
        assert od[same].tobytes() == od_full[same].tobytes()


def synthetic_case(nO, T, D, key):
    """Ego along +x on the road band y in [80, 98) with varying speed and a gentle turn; others drift across its path, one with a
    NaN head, one with a NaN tail; a planner fit; D latents."""
    t = 0.5 * (np.arange(T) + 1)
    sp = 6.0 + 1.5 * np.sin(0.7 * t)
    hh = 0.03 * t
    x = 100.0 + np.cumsum(sp * np.cos(hh) * 0.5)
    y = 88.0 + np.cumsum(sp * np.sin(hh) * 0.5)
    ego = np.stack([x, y, 1.3 * np.cos(hh), 1.3 * np.sin(hh)], -1)
    u = lambda shape, k, lo, hi: synth.counter_uniform(shape, '%s/%s' % (key, k), lo, hi)
    ox = 100.0 + u((nO, 1), 'x', 0.0, 45.0) + u((nO, 1), 'vx', -3.0, 6.0) * t[None]
    oy = 88.0 + u((nO, 1), 'y', -16.0, 16.0) + u((nO, 1), 'vy', -2.5, 2.5) * t[None]
    oh = u((nO, 1), 'h', -3.1, 3.1) + 0.02 * t[None]
    fut = np.concatenate([ego[None], np.stack([ox, oy, np.cos(oh), np.sin(oh)], -1)]).astype(np.float32)
    if nO > 2 and T > 3:
        fut[2, :1] = np.nan
        fut[1 + nO // 2, T - 1:] = np.nan
    lw = np.stack([4.2 + 0.4 * u((nO + 1,), 'l', 0.0, 1.0), 1.9 + 0.2 * u((nO + 1,), 'w', 0.0, 1.0)], -1).astype(np.float32)
    fit = fut[0].copy()
    fit[:, :2] += u((T, 2), 'fit', -0.5, 0.5).astype(np.float32)
    fh = hh + u((T,), 'fith', -0.2, 0.2)
    fit[:, 2], fit[:, 3] = np.cos(fh), np.sin(fh)
    z, mu = u((nO + 1, D), 'z', -2.0, 2.0).astype(np.float32), u((nO + 1, D), 'mu', -1.0, 1.0).astype(np.float32)
    var = u((nO + 1, D), 'var', 0.1, 2.0).astype(np.float32)
    return dict(name=key, dt=DT, fut_adv=torch.from_numpy(fut), veh_att=torch.from_numpy(lw), attack_agt=min(2, nO), fut_internal_ego=torch.from_numpy(fit),
                z_adv=torch.from_numpy(z), z_prior_mean=torch.from_numpy(mu), z_prior_var=torch.from_numpy(var))


# (others, T, latent size): 1 other; odd sizes; D = 1 and D = 64; 63 others = 1953 pairs and 63 x 5 T fine pairs > 256 work items
SHAPES = [(1, 2, 1), (2, 3, 64), (5, 12, 7), (18, 12, 32), (63, 4, 32)]


def restated_case(nO, T, D):
    sc = synthetic_case(nO, T, D, 'ae/%d/%d/%d' % (nO, T, D))
    return sc, restated_scene(sc, True)


@pytest.mark.parametrize('nO,T,D', SHAPES)
def test_kernel_matches_restatement(emu, nO, T, D):
    sc, want = restated_case(nO, T, D)
    assert want['margin_iou'] > 1e-9 and want['margin_frac'] > 1e-6 and want['margin_grid'] > 1e-6, 'a tie: choose other poses'
    oi, od = run_scenes(emu, [sc], [1])[0]
    close_to_restatement(oi, od, want, 'restatement %d/%d/%d' % (nO, T, D))


def test_restated_shapes_cover_the_branches():
    res = [restated_case(*s)[1]['i'] for s in SHAPES]
    assert any(r['adv_collide'] for r in res) and any(not r['adv_collide'] for r in res)
    assert any(r['num_coll_veh'] > 0 for r in res) and any(r['env_coll_others'] > 0 for r in res) and any(r['feat_status'] == 0 for r in res)
    assert any(r['other_accel_cnt'] > 0 for r in res) and any(r['atk_accel_cnt'] == 0 for r in res)


def test_scene_outputs_do_not_depend_on_the_batch(emu):
    scenes = [s for _, s in all_scenes() if s['fut_adv'].shape[1] == 12]
    assert len(scenes) == 4
    wf = [1] * len(scenes)
    fwd = run_scenes(emu, scenes, wf)
    rev = run_scenes(emu, scenes[::-1], wf)
    for b, s in enumerate(scenes):
        oi1, od1 = run_scenes(emu, [s], [1])[0]
        assert oi1.tobytes() == fwd[b][0].tobytes() == rev[len(scenes) - 1 - b][0].tobytes()
        assert od1.tobytes() == fwd[b][1].tobytes() == rev[len(scenes) - 1 - b][1].tobytes()


def test_status_codes_and_refusals(emu):
    sc = scenarios()['adv_sol_success'][3]                         # 5 agents, T 12
    fut, lw = sc['fut_adv'], sc['veh_att']
    run = lambda fut, ptr, lw, atk, **kw: [v.numpy() for v in EA.scenario_eval_metrics(fut, ptr, lw, atk, DT, lib=emu, **kw)]
    alone_i, alone_d, st = run(fut, [0, 5], lw, [3])
    assert st.tolist() == [0]
    # 1: ego only; its rows and the other scenes' outputs are untouched
    oi, od, st = run(torch.cat([fut, fut[:1], fut]), [0, 5, 6, 11], torch.cat([lw, lw[:1], lw]), [3, 0, 3])
    assert st.tolist() == [0, 1, 0] and (oi[1] == -1).all() and np.isnan(od[1]).all()
    for b in (0, 2):
        assert oi[b].tobytes() == alone_i[0].tobytes() and od[b].tobytes() == alone_d[0].tobytes()
    # 2: offsets that leave the arrays, an attack_agt outside the scene, a map index outside the map list
    assert run(fut, [0, 9], lw, [3])[2].tolist() == [2]
    assert run(fut, [0, 5], lw, [5])[2].tolist() == [2]
    assert run(fut, [0, 5], lw, [3], map_env=map_env(), mapix=[1])[2].tolist() == [2]
    # 3: more than 63 others (64 is refused, 63 runs: test_kernel_matches_restatement)
    many = fut[1:2].repeat(65, 1, 1)
    many[:, :, 1] += 4.0 * torch.arange(65).view(65, 1)
    oi, od, st = run(many, [0, 65], lw[:1].repeat(65, 1), [1])
    assert st.tolist() == [3] and (oi == -1).all()
    assert run(many[:64], [0, 64], lw[:1].repeat(64, 1), [1])[2].tolist() == [0]
    with pytest.raises(L.StriveHipError, match='T must be'):
        run(fut[:, :1], [0, 5], lw, [3])
    with pytest.raises(L.StriveHipError, match='latent size'):
        z = torch.ones((5, 65))
        run(fut, [0, 5], lw, [3], z=z, mu=z, var=z)
    with pytest.raises(ValueError, match='together'):
        run(fut, [0, 5], lw, [3], z=torch.ones((5, 4)))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    oi, od, st = torch.zeros((1, 20), dtype=torch.int32), torch.zeros((1, 26), dtype=torch.float64), torch.zeros((1,), dtype=torch.int32)
    f, dt = fut.contiguous(), torch.tensor([DT], dtype=torch.float64)
    args = [L.ptr(f), L.ptr(i32([0, 5])), L.ptr(lw), L.ptr(i32([3])), L.ptr(dt), None, None, None, 0, L.ptr(f[:1].contiguous()), L.ptr(i32([0])),
            None, None, None, 0, L.ptr(i32([0])), 1, 5, 12, L.ptr(oi), L.ptr(od), L.ptr(st), None]
    emu.call('strive_scenario_eval_metrics', *args)
    for k in (0, 1, 2, 3, 4, 9, 10, 15, 19, 20, 21):
        bad = list(args)
        bad[k] = None
        with pytest.raises(L.StriveHipError, match='null argument'):
            emu.call('strive_scenario_eval_metrics', *bad)
    bad = list(args)
    bad[5] = L.ptr(torch.ones((5, 4)))
    bad[8] = 4
    with pytest.raises(L.StriveHipError, match='together'):
        emu.call('strive_scenario_eval_metrics', *bad)
    # an empty batch and an empty agent list never hand the library a NULL
    oi, od, st = run(fut[:0], [0], lw[:0], [])
    assert oi.shape == (0, 20) and st.shape == (0,)
    assert run(fut[:0], [0, 0], lw[:0], [1])[2].tolist() == [2]


# ------------------------------------------------------------------------------------------------
# quant_eval, compute_metrics, the CLI
# ------------------------------------------------------------------------------------------------

def cluster_files(tmp_path):
    g = golden(FIX)
    path = str(tmp_path / 'cluster.npz')
    np.savez(path, centers=g['km/centers'], labels=g['km/labels'])
    labels = str(tmp_path / 'cluster_labels.txt')
    with open(labels, 'w') as f:
        f.write(', '.join(str(n) for n in g['cluster_label_names']) + '\n')
    return path, labels


def column_bound(key, scene_bound, want):
    """Bound of one CSV cell: None = equal."""
    if key in ('adv_collide', 'veh_coll_rate', 'env_coll_atk', 'env_coll_others', 'sol_success', 'adv_success', 'tot_success'):
        return None
    return scene_bound[key]


def check_quant_eval_outputs(g, out, res, scen):
    metrics, cnt, tot = res
    names = [str(n) for n in g['names']]
    by_name = {s['name']: s for c in mga.CATEGORIES for s in scen[c]}
    bounds = {n: scene_bounds(by_name[n], g)[1] for n in names}
    assert sorted(fn for fn in os.listdir(out) if fn.endswith('.csv')) == [str(n) for n in g['csv_names']]
    for fn in [str(n) for n in g['csv_names']]:
        got = list(csv.reader(open(os.path.join(out, fn))))
        want = list(csv.reader(io.StringIO(str(g['csv/' + fn]))))
        assert got[0] == want[0] and len(got) == len(want), fn
        if fn.endswith('_labels.csv'):
            assert got == want, fn
            continue
        for rg, rw in zip(got[1:], want[1:]):
            for key, a, b in zip(got[0], rg, rw):
                if key == 'name' or b == '':
                    assert a == b, (fn, key)
                elif fn.startswith('eval_per_seq'):
                    assert rg[0] == rw[0]
                    check_value(key, float(a), float(b), column_bound(key, bounds[rg[0]], float(b)) if not np.isnan(float(b)) else None, fn)
                else:
                    bd = None
                    if key in metrics:
                        bd = max(bounds[n][key] for n in names if key in bounds[n]) + metrics[key].count * EPS32 * abs(float(b))
                    check_value('pooled ' + key, float(a), float(b), bd, fn)
    assert list(metrics.keys()) == [str(k) for k in g['metric_keys']]
    assert [metrics[k].count for k in metrics] == g['metric_count'].tolist() and all(isinstance(v, PooledMetric) for v in metrics.values())
    assert list(cnt.keys()) == list(tot.keys()) == [str(k) for k in g['freq_keys']]
    assert [(cnt[k], tot[k]) for k in cnt] == list(zip(g['freq_cnt'].tolist(), g['freq_total'].tolist()))
    for k, want in zip(metrics, g['metric_mean'].tolist()):
        bd = max(bounds[n][k] for n in names if k in bounds[n]) + metrics[k].count * EPS32 * abs(want)
        check_value('pooled ' + k, metrics[k].mean(), want, bd, 'dictionaries')
    assert EA.compute_success_rates(scen) == tuple(g['success_rates'][:2].tolist())
    for c in mga.CATEGORIES[:2]:
        for s in scen[c]:
            assert int(s['label_idx']) == int(g['labels/' + s['name']]) and s['label'] == str(g['cluster_label_names'][int(s['label_idx'])])
    for c in mga.CATEGORIES:
        for s in scen[c]:
            assert list(s['eval_metrics'].keys()) == [str(k) for k in g[s['name'] + '/seq_keys']] and len(s['eval_metrics']) == 16


@pytest.mark.parametrize('batch_scenes', [256, 1])
def test_quant_eval_matches_reference(emu_ops, tmp_path, batch_scenes):
    g = golden(FIX)
    cluster, labels = cluster_files(tmp_path)
    scen = fresh_scenarios()
    out = str(tmp_path / 'out')
    res = EA.quant_eval(scen, cluster, labels, map_env(), out, batch_scenes=batch_scenes, device='cpu')
    check_quant_eval_outputs(g, out, res, scen)


def test_compute_metrics_and_feature_functions_are_the_kernel_with_one_scene(emu_ops):
    g = golden(FIX)
    metrics, cnt, tot = {}, {}, {}
    for cat, scene in all_scenes():
        metrics, cnt, tot, seq = EA.compute_metrics(scene, map_env(), 0, metrics, cnt, tot)
        want, bounds = scene_bounds(scene, g)
        assert list(seq.keys()) == list(EA.SEQ_KEYS)
        for k, v in seq.items():
            check_value(k, v, want[k], bounds.get(k), scene['name'])
        if cat != 'adv_failed':
            n = scene['name']
            f = EA.compute_coll_feat(scene['veh_att'], scene['fut_adv'], scene['dt'])
            f2 = CS.compute_coll_feat(scene['veh_att'], scene['fut_adv'], scene['dt'])
            assert sorted(f) == ['angvec', 'hvec', 'rel_s'] and sorted(f2) == ['ang', 'angvec', 'h', 'hvec'] and f['hvec'] == f2['hvec']
            fb = feat_bounds(scene, g)
            for k in ('hvec', 'angvec'):
                for a, b in zip(f[k], g[n + '/feat_' + k].tolist()):
                    check_value(k, a, b, fb[k], n)
            check_value('rel_s', f['rel_s'], float(g[n + '/feat_rel_s']), fb['rel_s'], n)
            check_value('h', f2['h'], float(g[n + '/feat_h']), fb['h'], n)
            check_value('ang', f2['ang'], float(g[n + '/feat_ang']), fb['ang'], n)
    assert [metrics[k].count for k in metrics] == [int(c) for c in g['metric_count']] and list(metrics) == [str(k) for k in g['metric_keys']]
    acc = EA.compute_accels(scene['fut_adv'][0, :, :2], scene['fut_adv'][0, :, 2:4], DT)
    ref = RS.accels(scene['fut_adv'][0].numpy(), scene['fut_adv'].shape[1], DT)
    for a, b in zip(acc, ref):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-4, atol=1e-4)


def test_crash_scene_without_a_fine_contact_raises(emu_ops, tmp_path):
    cluster, labels = cluster_files(tmp_path)
    scen = fresh_scenarios()
    moved = dict(scen['adv_failed'][0])                 # no collision at all, filed under sol_failed
    moved['name'] = 'sc_0009_nocontact'
    scen['sol_failed'] = scen['sol_failed'] + [moved]
    with pytest.raises(ValueError, match='sc_0009_nocontact'):
        EA.quant_eval(scen, cluster, labels, map_env(), str(tmp_path / 'out'), device='cpu')
    with pytest.raises(ValueError, match='only the ego'):
        EA.compute_coll_feat(moved['veh_att'][:1], moved['fut_adv'][:1], DT)
    with pytest.raises(NotImplementedError):
        EA.qual_eval()
    with pytest.raises(NotImplementedError):
        EA.viz_scenario()
    with pytest.raises(NotImplementedError):
        CS.cluster_scenarios([], str(tmp_path), 2, viz=True)


def test_cli(emu_ops, tmp_path, capsys):
    with pytest.raises(SystemExit, match='map environment with the drivable raster must be supplied from Python'):
        EA.main(['--scenarios', mga.SCEN_DIR, '--eval_quant'])
    cluster, labels = cluster_files(tmp_path)
    out = str(tmp_path / 'cli')
    scen, res = EA.main(['--scenarios', mga.SCEN_DIR, '--eval_quant', '--cluster_path', cluster, '--cluster_labels', labels, '--map_world',
                         'synthetic', '--out', out, '--device', 'cpu'])
    check_quant_eval_outputs(golden(FIX), os.path.join(out, 'eval_quant'), res, scen)
    # clustering CLI: the crash scenes of g18 into two types, then that file labels them
    dirs = [os.path.join(mga.SCEN_DIR, c) for c in mga.CATEGORIES[:2]]
    centers, lab, inertia, n_iter = CS.main(['--scenario_dirs'] + dirs + ['--k', '2', '--out', str(tmp_path / 'cl'), '--device', 'cpu'])
    with np.load(str(tmp_path / 'cl' / 'cluster.npz')) as f:
        assert f['centers'].shape == (2, 4) and f['labels'].tolist() == lab.tolist() and [str(n)[5:] for n in f['names']] == [s['name'] for _, s in all_scenes()[:5]]
        feats = f['feats']
    g = golden(FIX)
    for row, (_, s) in zip(feats, all_scenes()[:5]):
        fb = feat_bounds(s, g)
        assert np.abs(row[:2] - g[s['name'] + '/feat_angvec']).max() <= fb['angvec'] and np.abs(row[2:] - g[s['name'] + '/feat_hvec']).max() <= fb['hvec']
    clustering = EA.load_clustering(str(tmp_path / 'cl' / 'cluster.npz'))
    assert EA.predict_clusters(clustering, feats, 'cpu').tolist() == lab.tolist()


# ------------------------------------------------------------------------------------------------
# k-means
# ------------------------------------------------------------------------------------------------

def test_fit_kmeans_matches_scikit_learn(emu_ops):
    g = golden(FIX)
    feats, init = g['km/feats'], g['km/init']
    N = feats.shape[0]
    centers, labels, inertia, n_iter = CS.fit_kmeans(feats, init.shape[0], init=init, device='cpu')
    assert labels.tolist() == g['km/labels'].tolist() and n_iter == int(g['km/n_iter'])
    r = note('kmeans centres', np.abs(centers - g['km/centers']).max(), 4 * N * EPS64)
    r2 = note('kmeans inertia', abs(inertia - float(g['km/inertia'])), 4 * N * EPS64 * float(g['km/inertia']) + 4 * N * EPS64)
    print('k-means centres err/bound %.3g inertia err/bound %.3g' % (r, r2))
    assert r <= 1.0 and r2 <= 1.0
    again = CS.fit_kmeans(feats, init.shape[0], init=init, device='cpu')
    assert again[0].tobytes() == centers.tobytes() and again[1].tobytes() == labels.tobytes() and again[2] == inertia and again[3] == n_iter
    a = CS.fit_kmeans(feats, 4, seed=3, device='cpu')
    b = CS.fit_kmeans(feats, 4, seed=3, device='cpu')
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[2] == b[2] and a[3] == b[3]
    assert sorted(np.bincount(a[1], minlength=4).tolist()) == [10, 10, 10, 10]           # the four synthetic types are found from k-means++ too
    far = np.concatenate([init[:3], [[50.0, 50.0, 50.0, 50.0]]])
    with pytest.raises(ValueError, match='cluster 3 emptied'):
        CS.fit_kmeans(feats, 4, init=far, device='cpu')


def test_assign_cluster_labels_match_reference(emu_ops, tmp_path):
    g = golden(FIX)
    clustering = EA.FixedClustering(g['km/centers'])
    names = [str(n) for n in g['cluster_label_names']]
    for cat in mga.CATEGORIES[:2]:
        scenes = [dict(s) for s in scenarios()[cat]]
        path = str(tmp_path / (cat + '.csv'))
        feats = EA.assign_cluster(scenes, clustering, names, path, device='cpu')
        assert [int(s['label_idx']) for s in scenes] == [int(g['labels/' + s['name']]) for s in scenes] and len(feats) == len(scenes)
        assert open(path).read().splitlines() == str(g['csv/%s_labels.csv' % cat]).splitlines()
    import pickle
    pkl = str(tmp_path / 'c.pkl')
    with open(pkl, 'wb') as f:
        pickle.dump(clustering, f)
    assert np.array_equal(EA.load_clustering(pkl).cluster_centers_, g['km/centers'])


KM_SHAPES = [(11, 4, 3), (300, 4, 10), (257, 8, 64), (5, 1, 1)]


def km_case(N, F, k):
    x = synth.counter_uniform((N, F), 'km/x/%d/%d/%d' % (N, F, k), -1.0, 1.0)
    c = synth.counter_uniform((k, F), 'km/c/%d/%d/%d' % (N, F, k), -1.0, 1.0)
    return x, c


def check_kmeans_step(lib, N, F, k, device='cpu'):
    x, c = km_case(N, F, k)
    wl, wm, ws, wc, wi, gap = RS.kmeans_step(x, c)
    assert gap > 1e-9
    xt, ct = torch.from_numpy(x).to(device), torch.from_numpy(c).to(device)
    outs = [[v.cpu().numpy() for v in EA.kmeans_step(xt, ct, lib=lib)] for _ in range(2)]
    lab, mind, sums, counts, inertia = outs[0]
    assert lab.tolist() == wl.tolist() and counts.tolist() == wc.tolist()
    assert np.abs(mind - wm).max() <= 16 * EPS64 * max(wm.max(), 1e-300) * F
    assert np.abs(sums - ws).max() <= 4 * N * EPS64 and abs(inertia[0] - wi) <= 4 * N * EPS64 * wi
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes()
    return outs[0]


@pytest.mark.parametrize('N,F,k', KM_SHAPES)
def test_kmeans_step_matches_restatement(emu, N, F, k):
    check_kmeans_step(emu, N, F, k)


def test_kmeans_step_ties_and_refusals(emu):
    x = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.5, 0.0]], dtype=torch.float64)
    c = torch.tensor([[1.0, 0.0], [0.0, 0.0], [1.0, 0.0]], dtype=torch.float64)
    lab, mind, sums, counts, inertia = EA.kmeans_step(x, c, lib=emu)
    assert lab.tolist() == [1, 0, 0] and counts.tolist() == [2, 1, 0] and sums[2].tolist() == [0.0, 0.0] and float(inertia) == 0.25
    with pytest.raises(L.StriveHipError, match='F must be'):
        EA.kmeans_step(torch.zeros((3, 9), dtype=torch.float64), torch.zeros((2, 9), dtype=torch.float64), lib=emu)
    with pytest.raises(L.StriveHipError, match='k must be'):
        EA.kmeans_step(torch.zeros((3, 2), dtype=torch.float64), torch.zeros((65, 2), dtype=torch.float64), lib=emu)
    with pytest.raises(ValueError):
        EA.kmeans_step(torch.zeros((0, 2), dtype=torch.float64), torch.zeros((2, 2), dtype=torch.float64), lib=emu)
    args = [L.ptr(x), L.ptr(c), 3, 2, 3, L.ptr(lab), L.ptr(mind), L.ptr(sums), L.ptr(counts), L.ptr(inertia), None]
    for i in (0, 1, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        with pytest.raises(L.StriveHipError, match='null argument'):
            emu.call('strive_kmeans_step', *bad)


def test_grouping_is_pure_host_logic():
    mk = lambda T, D: dict(fut_adv=torch.zeros((2, T, 4)), z_adv=torch.zeros((2, D)))
    scenes = [mk(12, 32), mk(12, 32), mk(8, 32), mk(8, 32), mk(8, 16), mk(12, 32)]
    assert EA.group_by_steps(scenes, 256) == [[0, 1], [2, 3], [4], [5]]
    assert EA.group_by_steps(scenes, 1) == [[i] for i in range(6)] and EA.group_by_steps([], 4) == []
    with pytest.raises(ValueError):
        EA.group_by_steps(scenes, 0)
    assert len(EA.OUT_I) == 20 and len(EA.OUT_D) == 26 and len(set(EA.OUT_I + EA.OUT_D)) == 46


# ------------------------------------------------------------------------------------------------
# MI355X
# ------------------------------------------------------------------------------------------------

def gpu_against_emulator(emu, scenes, want_feat, what, **kw):
    hip = L.get_lib()
    want = run_scenes(emu, scenes, want_feat, **kw)
    got = run_scenes(hip, scenes, want_feat, device=DEV, **kw)
    for s, (wi, wd), (gi, gd) in zip(scenes, want, got):
        assert np.array_equal(gi, wi), (what, s['name'], gi, wi)
        ab = restated_scene(s, bool(want_feat[0]), with_map=kw.get('with_map', True), with_latents=kw.get('with_latents', True))['abs']
        close_to_restatement(gi, gd, dict(i=dict(zip(EA.OUT_I, wi.tolist())), d=dict(zip(EA.OUT_D, wd.tolist())), abs=ab), '%s %s' % (what, s['name']))
    return got


@pytest.mark.gpu
def test_gpu_kernel_matches_emulator(emu):
    scenes = [s for _, s in all_scenes()]
    got = gpu_against_emulator(emu, scenes, [1] * len(scenes), 'gpu')
    gpu_against_emulator(emu, scenes, [1] * len(scenes), 'gpu bare', with_map=False, with_latents=False)
    big = restated_case(63, 4, 32)[0]
    gpu_against_emulator(emu, [big], [1], 'gpu 63 others')
    # alone against batched, two positions
    hip = L.get_lib()
    rev = run_scenes(hip, scenes[::-1], [1] * len(scenes), device=DEV)
    for b, s in enumerate(scenes):
        oi1, od1 = run_scenes(hip, [s], [1], device=DEV)[0]
        assert oi1.tobytes() == got[b][0].tobytes() == rev[len(scenes) - 1 - b][0].tobytes()
        assert od1.tobytes() == got[b][1].tobytes() == rev[len(scenes) - 1 - b][1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('N,F,k', [(11, 4, 3), (300, 4, 10)])
def test_gpu_kmeans_step_matches_emulator(emu, N, F, k):
    want = check_kmeans_step(emu, N, F, k)
    got = check_kmeans_step(L.get_lib(), N, F, k, device=DEV)
    assert got[0].tolist() == want[0].tolist() and got[3].tolist() == want[3].tolist()
    assert np.abs(got[2] - want[2]).max() <= 16 * EPS64 * max(np.abs(want[2]).max(), 1.0) * N


@pytest.mark.gpu
def test_gpu_quant_eval_matches_reference(tmp_path):
    g = golden(FIX)
    cluster, labels = cluster_files(tmp_path)
    scen = fresh_scenarios()
    out = str(tmp_path / 'out')
    res = EA.quant_eval(scen, cluster, labels, EA.SyntheticMapWorld(), out, device=DEV)
    check_quant_eval_outputs(g, out, res, scen)
    feats, init = g['km/feats'], g['km/init']
    centers, lab, inertia, n_iter = CS.fit_kmeans(feats, 4, init=init, device=DEV)
    assert lab.tolist() == g['km/labels'].tolist() and n_iter == int(g['km/n_iter'])
    assert np.abs(centers - g['km/centers']).max() <= 4 * 40 * EPS64
