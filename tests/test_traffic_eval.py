"""Batched model evaluation (strive_amd/test_traffic.py -> strive_traffic_eval_metrics, strive_amd/csrc/eval_metrics.hip; checkpoints through
strive_amd/utils/torch.py) against the reference's src/test_traffic.py and the metric functions of src/losses/traffic_model.py.

Fixture g19_traffic_eval.npz (tests/golden/make_golden_traffic_eval.py, README_g19.md): ``inj/*`` the reference's compute_err,
compute_disp_err, compute_coll_rate_env (ego_only true and false) and compute_coll_rate_veh on injected predictions, ``run/*`` its
run_one_epoch with its own model.  The inputs are rebuilt by the generator's builders, which import without the reference.

Bounds against ``inj/*``.  Both sides start from the SAME fp32 unnormalised values (v * std + mean, one fp32 multiply and add); the
reference continues in fp32, the kernel in float64, so each bound is a bound on the reference's rounding.  eps32 = 2^-23 (one fp32
operation errs by at most eps32 / 2 relative).
  integers, flags, NaN-ness, L, W, statuses: equal (the tie conditions keep every threshold decision away from its threshold).
  pos_err: subtract (1/2), square (1/2 on top of twice the difference's), add (1/2), sqrt (halves, + 1/2): < 2 eps32 relative; granted
      4 eps32 |pos_err|.
  heading dot product: each unit component carries the norm's error (< 1.5 eps32) and the division (1/2): 2 eps32; two products and
      an addition: |dot' - dot| < delta = 6 eps32 (|dot| <= 1).  acos is rounded to 2 ulp and rad2deg to 1/2: 2 eps32 |angle|.
        1 - |dot| >= 1e-3: |angle' - angle| <= delta / sqrt(1 - dot^2) (delta is 1000 times smaller than the distance to +-1).
        1 - |dot| <  1e-3: |acos(x) - acos(x')| <= acos(1 - delta) <= sqrt(2 delta) = sqrt(12 eps32) rad.
  a mean over T fp32 values adds (T - 1) / 2 eps32 of the sum of the absolute values (recursive summation is the worst case;
      torch's pairwise sum is below it) and 1/2 for the division: minADE is granted max over the samples of
      [mean_t bound(s, t) + T eps32 ADE_s]; a minimum over perturbed values moves by at most the largest perturbation.  minFDE:
      the largest per-frame bound at the last step.
  APD: NS^2 Tc terms of relative error 2 eps32 summed in fp32, then one division: (3 + NS^2 Tc / 2) eps32 APD.
  grid ratios: a mean over R rows of sizes in fp32 (R / 2 eps32 worst case) and one division: (2 + R / 2) eps32 relative -- far
      below the 1e-3 the tie condition keeps them from a half-integer, so L and W are equal.
Against the float64 restatement (tests/traffic_eval_restated.py, the kernel's formulas in the kernel's order) and, on the MI355X,
against the host emulation: 16 eps64 relative (sums: relative to the sum of the absolute values -- every summed term here is
non-negative, so that is the value itself).

Bounds against ``run/*`` (the reference's own model; product rollouts differ from it within what tests/test_gpu_parity.py grants
decode_embedding against the reference on a textured raster: 1e-2 absolute in NORMALISED units per component, and 1e-4 relative +
2e-5 absolute for the embed's outputs).  Carried through each metric at the REFERENCE's recorded values:
  positions: 1e-2 * 15 m = 0.15 m per coordinate -> sqrt(2) 0.15 m per position error; means and minima over samples inherit it.
  headings (std 1): each component moves by <= 1e-2, the unit vector turns by <= asin(sqrt(2) 1e-2 / (|h| - sqrt(2) 1e-2)) with
      |h| the recorded heading norm (>= 0.9 asserted): < 0.91 degrees.
  APD: two positions move: 2 sqrt(2) 0.15 m.
  recon_loss = sum_c (x - m)^2 / 2 + const per frame: |d| <= sum_c |x - m|_c 1e-2 + 4 (1e-2)^2 / 2, averaged over the frames.
  kl_loss, z_logprob, z_mdist: first-order carried tolerance sum_i |df/dx_i| (1e-4 |x_i| + 2e-5) over the four latent tensors
      (autograd in float64 at the recorded values), doubled for the remainder; loss = recon + kl: the two bounds added.
  counters and frequencies: equal.

Largest error / bound per quantity: printed by the tests; profiles/r18_traffic_eval_ratios.md (written when STRIVE_WRITE_RATIOS is
set).  The host emulation runs the model at about a second per map-CNN evaluation: the host versions of the driver tests that run
the real model need STRIVE_SLOW=1; their GPU versions always run.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import traffic_eval_restated as RS
import make_golden_traffic_eval as G
from util import golden, product_model
from strive_amd import _lib as L
from strive_amd import ops
from strive_amd import synth
from strive_amd import test_traffic as TT
from strive_amd.losses import traffic_model as TM
from strive_amd.losses.common import kl_normal, log_normal
from strive_amd.utils import torch as UT
from strive_amd.constants import state_norm_tensors, att_norm_tensors

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
DEV = 'cuda:0'
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
SLOW = bool(os.environ.get('STRIVE_SLOW'))
RATIOS = {}
ROLL_TOL, EMB_RT, EMB_AT = 1e-2, 1e-4, 2e-5
LOSS_W = {'recon': 1.0, 'kl': 1.0, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0}
FLAGS = dict(test_recon_coll_rate=True, test_sample_disp_err=True, test_sample_coll_rate=True, test_sample_num=G.RUN_NS)


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
    """NaN-ness equal; |got - want| <= bound elementwise; the worst error / bound is printed and recorded."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(want))
    assert got.shape == want.shape, '%s %s: shape %s vs %s' % (what, key, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s %s: NaN pattern differs' % (what, key)
    ok = ~np.isnan(want)
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
            f.write('# Model evaluation (`strive_traffic_eval_metrics`, `strive_amd/test_traffic.py`): largest observed error / bound\n\n')
            f.write('| quantity | largest error / bound |\n|---|---|\n')
            for k in sorted(RATIOS):
                f.write('| %s | %.3g |\n' % (k, RATIOS[k]))


# ------------------------------------------------------------------------------------------------
# inputs, shared and never modified
# ------------------------------------------------------------------------------------------------

_CACHE = {}


def normalizers():
    from strive_amd.datasets.utils import MeanStdNormalizer
    if 'norm' not in _CACHE:
        _CACHE['norm'] = (MeanStdNormalizer(*state_norm_tensors()), MeanStdNormalizer(*att_norm_tensors()))
    return _CACHE['norm']


def fixture():
    if 'g' not in _CACHE:
        g = golden(G.FIX)
        _CACHE['g'] = {k: g[k] for k in g.files}
    return _CACHE['g']


def inj(case):
    if ('inj', case) not in _CACHE:
        _CACHE[('inj', case)] = G.inj_case(case)
    return _CACHE[('inj', case)]


def inj_env(device='cpu'):
    if ('env', device) not in _CACHE:
        raster, dx = G.inj_raster()
        _CACHE[('env', device)] = synth.SyntheticMapEnv(raster, dx).to(device)
    return _CACHE[('env', device)]


def run_kernel(lib, case, device='cpu', ego_only=True, groups=('err', 'disp', 'veh', 'env'), **kw):
    batch, mi, pred = inj(case)
    sn, an = normalizers()
    NS = pred.shape[1]
    want = {g_: True for g_ in groups if not (g_ == 'err' and (NS != 1 or pred.shape[2] != G.TG))}
    out = TT.traffic_eval_metrics(pred.to(device), batch.ptr.to(device), batch.lw.to(device), sn, an, gt=batch.future_gt.to(device),
                                  vis=batch.future_vis.to(device), map_env=inj_env(device), mapix=mi.to(device), env_ego_only=ego_only,
                                  lib=lib, **want, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def ego_tables(case):
    """float64 tables of the ego errors of a case, vectorised: dist, ang (deg), dot (B, NS, Tc), from the fp32 unnormalised values."""
    batch, _, pred = inj(case)
    sm, ss = [t.numpy() for t in state_norm_tensors()]
    ego = batch.ptr[:-1].numpy()
    Tc = min(pred.shape[2], G.TG)
    p = RS.unnorm(pred.numpy()[ego][:, :, :Tc], sm, ss).astype(np.float64)
    g_ = RS.unnorm(batch.future_gt.numpy()[ego][:, None, :Tc, :4], sm, ss).astype(np.float64)
    return pose_tables(g_, p)


def pose_tables(g_, p):
    with np.errstate(invalid='ignore'):
        dist = np.sqrt(((g_[..., :2] - p[..., :2]) ** 2).sum(-1))
        dot = ((g_[..., 2:4] / np.linalg.norm(g_[..., 2:4], axis=-1, keepdims=True)) * (p[..., 2:4] / np.linalg.norm(p[..., 2:4], axis=-1, keepdims=True))).sum(-1)
        ang = np.degrees(np.arccos(np.clip(dot, -1.0, 1.0)))
    return dist, ang, dot


def ang_bound(ang, dot):
    """Per-frame bound on the reference's fp32 heading error (degrees), see the module docstring."""
    with np.errstate(invalid='ignore', divide='ignore'):
        near = 1.0 - np.abs(dot) < 1e-3
        lin = np.degrees(6.0 * EPS32 / np.sqrt(np.maximum(1.0 - dot * dot, 1e-300)))
        return np.where(near, np.degrees(np.sqrt(12.0 * EPS32)), lin) + 2.0 * EPS32 * np.abs(ang)


def check_against_fixture(case, out_ego, out_all, what):
    g, p = fixture(), 'inj/%s/' % case
    batch, _, pred = inj(case)
    NS, T = pred.shape[1], pred.shape[2]
    Tc = min(T, G.TG)
    assert not out_ego['status'].any() and not out_all['status'].any()
    assert np.array_equal(out_ego['did_collide_veh'].astype(bool), g[p + 'veh/did_collide'].astype(bool)), what + ' did_collide_veh'
    assert out_ego['did_collide_veh'].sum() == g[p + 'veh/num'][0] and out_ego['did_collide_veh'].size == g[p + 'veh/num'][1]
    for tag, out in (('env_ego/', out_ego), ('env_all/', out_all)):
        assert np.array_equal(out['did_collide_map'].astype(bool), g[p + tag + 'did_collide'].astype(bool)), what + ' did_collide_map ' + tag
        assert out['did_collide_map'].sum() == g[p + tag + 'num'][0] and out['did_collide_map'].size == g[p + tag + 'num'][1]
        assert (int(out['grid_i'][0]), int(out['grid_i'][1])) == (int(g[p + tag + 'L']), int(g[p + tag + 'W'])), what + ' grid ' + tag
        rows = float(out['grid_i'][2])
        assert rows == g[p + tag + 'frac'].size
        check('grid_ratio', out['grid_d'], g[p + tag + 'ratio'], (2.0 + rows / 2.0) * EPS32 * np.abs(g[p + tag + 'ratio']), what + ' ' + tag)
    dist, ang, dot = ego_tables(case)
    ab = ang_bound(ang, dot)
    d = out_ego['disp']
    import warnings
    with np.errstate(invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)          # an ego with NaN frames: an all-NaN row, bound 0, value NaN on both sides
        bounds = {'pos_minADE': np.nanmax(4 * EPS32 * dist.mean(-1) + Tc * EPS32 * dist.mean(-1), axis=1),
                  'pos_minFDE': np.nanmax(4 * EPS32 * dist[:, :, -1], axis=1),
                  'ang_minADE': np.nanmax(ab.mean(-1) + Tc * EPS32 * ang.mean(-1), axis=1),
                  'ang_minFDE': np.nanmax(ab[:, :, -1], axis=1)}
    for c, k in enumerate(TT.DISP_KEYS[:4]):
        check(k, d[:, c], g[p + 'disp/' + k], np.nan_to_num(bounds[k], nan=0.0), what)
    check('APD', d[:, 4], g[p + 'disp/APD'], (3.0 + NS * NS * Tc / 2.0) * EPS32 * np.abs(np.nan_to_num(g[p + 'disp/APD'], nan=0.0)), what)
    if 'pos_err' in out_ego:
        vis = batch.future_vis.numpy() == 1.0
        assert np.isnan(out_ego['pos_err'][~vis]).all() and np.isnan(out_ego['ang_err'][~vis]).all(), 'NaN where vis != 1'
        sm, ss = [t.numpy() for t in state_norm_tensors()]
        _, a_all, dot_all = pose_tables(RS.unnorm(batch.future_gt.numpy()[..., :4], sm, ss).astype(np.float64),
                                        RS.unnorm(pred.numpy()[:, 0], sm, ss).astype(np.float64))
        check('pos_err', out_ego['pos_err'][vis], g[p + 'pos_err'], 4 * EPS32 * np.abs(np.nan_to_num(g[p + 'pos_err'], nan=0.0)), what)
        check('ang_err', out_ego['ang_err'][vis], g[p + 'ang_err'], np.nan_to_num(ang_bound(a_all, dot_all)[vis], nan=0.0), what)


def check_close64(got, want, what):
    """Two evaluations of the same float64 formulas: discrete outputs equal, continuous ones within 16 eps64 relative."""
    for k in sorted(set(got) & set(want)):
        if got[k].dtype.kind in 'iu':
            assert np.array_equal(got[k], want[k]), '%s %s' % (what, k)
        else:
            check('f64/' + k, got[k], want[k], 16 * EPS64 * np.abs(np.nan_to_num(want[k], nan=0.0)), what)


# ------------------------------------------------------------------------------------------------
# the fixture itself
# ------------------------------------------------------------------------------------------------

def test_fixture_tie_conditions():
    g = fixture()
    layers = [k[:-len('frac')] for k in g if k.endswith('/frac')]
    assert len(layers) >= 2 * len(G.CASES) + 2
    for p in layers:
        L_, W_ = int(g[p + 'L']), int(g[p + 'W'])
        assert np.abs(g[p + 'frac'].astype(np.float64) - 0.95).min() > 2.0 / (L_ * W_), p
        assert np.abs(g[p + 'ratio'] - np.floor(g[p + 'ratio']) - 0.5).min() > 1e-3, p
    for k in [k for k in g if k.endswith('iou')]:
        assert g[k].size and np.abs(g[k] - G.IOU_THRESH).min() > G.TIE_MARGIN, k
    assert sorted(G.CASES) == sorted({k.split('/')[1] for k in g if k.startswith('inj/')})
    assert [len(s) for s in G.RUN_SIZES] == [2, 1, 2] and len(g['run/keys']) == 3


# ------------------------------------------------------------------------------------------------
# host emulation: the kernel
# ------------------------------------------------------------------------------------------------

HOST_CASES = [c for c in G.CASES if c != 'ns20' or SLOW]


@pytest.mark.parametrize('case', HOST_CASES)
def test_kernel_matches_reference_fixture(emu, case):
    check_against_fixture(case, run_kernel(emu, case, ego_only=True), run_kernel(emu, case, ego_only=False), 'emu ' + case)


def restated(case, ego_only, grid_lw=None):
    key = ('rs', case, ego_only, grid_lw)
    if key not in _CACHE:
        batch, mi, pred = inj(case)
        sm, ss = [t.numpy() for t in state_norm_tensors()]
        am, as_ = [t.numpy() for t in att_norm_tensors()]
        raster, dx = G.inj_raster()
        _CACHE[key] = RS.metrics(pred.numpy(), batch.future_gt.numpy(), batch.future_vis.numpy(), batch.ptr.numpy(), batch.lw.numpy(), sm, ss,
                                 am, as_, raster=raster.numpy(), dx=dx.numpy(), mapix=mi.numpy(), ego_only=ego_only, grid_lw=grid_lw,
                                 err=pred.shape[1] == 1, disp=True, veh=ego_only, env=True)
    return _CACHE[key]


@pytest.mark.parametrize('case', ['ns1', 'ns3_t16', 'ns3_t8', 'one'] + (['ns3', 'ns20'] if SLOW else []))
def test_kernel_matches_restatement(emu, case):
    for ego_only in (True, False):
        check_close64(run_kernel(emu, case, ego_only=ego_only), restated(case, ego_only), 'restated %s ego_only=%s' % (case, ego_only))


def poisoned(case, device, ego_only):
    batch, mi, pred = inj(case)
    NA, NS = pred.shape[0], pred.shape[1]
    B = mi.numel()
    return {'pos_err': torch.full((NA, G.TG), -7.0, dtype=torch.float64, device=device), 'ang_err': torch.full((NA, G.TG), -7.0, dtype=torch.float64, device=device),
            'disp': torch.full((B, 5), -7.0, dtype=torch.float64, device=device), 'did_collide_veh': torch.full((NA, NS), -7, dtype=torch.int32, device=device),
            'did_collide_map': torch.full((B if ego_only else NA, NS), -7, dtype=torch.int32, device=device),
            'grid_i': torch.full((3,), -7, dtype=torch.int32, device=device), 'grid_d': torch.full((2,), -7.0, dtype=torch.float64, device=device),
            'status': torch.full((B,), -7, dtype=torch.int32, device=device)}


def check_batch_independence(lib, device):
    """The 5-agent scene alone (case ``one``) and as scene 2 of the four-scene batch (case ``ns3``), the grid held equal: the
    same bytes.  Groups that are not asked for leave poisoned buffers untouched."""
    full = run_kernel(lib, 'ns3', device, ego_only=False, grid=(18, 8))
    one = run_kernel(lib, 'one', device, ego_only=False, grid=(18, 8))
    o = inj('ns3')[0].ptr.numpy()
    assert one['disp'].tobytes() == full['disp'][2:3].tobytes()
    assert one['did_collide_veh'].tobytes() == full['did_collide_veh'][o[2]:o[3]].tobytes()
    assert one['did_collide_map'].tobytes() == full['did_collide_map'][o[2]:o[3]].tobytes()
    ego_full, ego_one = run_kernel(lib, 'ns3', device, grid=(18, 8)), run_kernel(lib, 'one', device, grid=(18, 8))
    assert ego_one['did_collide_map'].tobytes() == ego_full['did_collide_map'][2:3].tobytes()
    full1, one1 = run_kernel(lib, 'ns1', device, grid=(18, 8)), run_kernel(lib, 'one1', device, grid=(18, 8))
    for k in ('pos_err', 'ang_err', 'did_collide_veh'):
        assert one1[k].tobytes() == full1[k][o[2]:o[3]].tobytes(), k
    assert one1['disp'].tobytes() == full1['disp'][2:3].tobytes() and one1['did_collide_map'].tobytes() == full1['did_collide_map'][2:3].tobytes()
    a, b = run_kernel(lib, 'ns1', device), run_kernel(lib, 'ns1', device)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a), 'two runs give the same bytes'
    for groups in (('disp',), ('veh',), ('env',), ('err',)):
        out = run_kernel(lib, 'ns1', device, groups=groups, out=poisoned('ns1', device, True))
        owned = {'err': ('pos_err', 'ang_err'), 'disp': ('disp',), 'veh': ('did_collide_veh',), 'env': ('did_collide_map', 'grid_i', 'grid_d')}
        for g_, keys in owned.items():
            for k in keys:
                assert (out[k] == -7).all() == (g_ not in groups), 'group %s, buffer %s' % (groups, k)
        assert not out['status'].any()


def test_scene_outputs_do_not_depend_on_the_batch(emu):
    check_batch_independence(emu, 'cpu')


def test_statuses_leave_outputs_untouched(emu):
    batch, mi, pred = inj('ns3')
    sn, an = normalizers()
    args = dict(gt=batch.future_gt, vis=batch.future_vis, map_env=inj_env(), disp=True, veh=True, env=True, env_ego_only=False, lib=emu)
    o = batch.ptr.numpy()
    good = {k: v.numpy() for k, v in TT.traffic_eval_metrics(pred, batch.ptr, batch.lw, sn, an, mapix=mi, **args).items()}
    # scene 3: map index out of range
    bad_mi = mi.clone()
    bad_mi[3] = 2
    out = TT.traffic_eval_metrics(pred, batch.ptr, batch.lw, sn, an, mapix=bad_mi, out=poisoned('ns3', 'cpu', False), **args)
    assert out['status'].tolist() == [0, 0, 0, 3]
    assert (out['did_collide_veh'][o[3]:] == -7).all() and (out['did_collide_map'][o[3]:] == -7).all() and (out['disp'][3] == -7).all()
    assert np.array_equal(out['did_collide_veh'][:o[3]].numpy(), good['did_collide_veh'][:o[3]]) and out['disp'][:3].numpy().tobytes() == good['disp'][:3].tobytes()
    # scenes 1 and 2: offsets leave the arrays (scene 1 ends past the last agent, scene 2 ends before it starts)
    ptr2 = torch.tensor([0, 1, 40, 8, 27], dtype=torch.int32)
    out = TT.traffic_eval_metrics(pred, ptr2, batch.lw, sn, an, mapix=mi, out=poisoned('ns3', 'cpu', False), **args)
    assert out['status'].tolist() == [0, 2, 2, 0]
    assert (out['did_collide_veh'][o[1]:o[3]] == -7).all() and (out['disp'][1:3] == -7).all() and (out['disp'][3] != -7).any()
    # a grid above lin_max: every scene refuses, nothing is sampled
    big = batch.lw + 200.0
    out = TT.traffic_eval_metrics(pred, batch.ptr, big, sn, an, mapix=mi, out=poisoned('ns3', 'cpu', False), **args)
    assert out['status'].tolist() == [4, 4, 4, 4] and int(out['grid_i'][0]) > TT.LIN_MAX
    assert all((out[k] == -7).all() for k in ('disp', 'did_collide_veh', 'did_collide_map'))
    # refusals of the entry point itself
    with pytest.raises(ValueError, match='T 8 != Tg 12'):
        TT.traffic_eval_metrics(pred[:, :, :8], batch.ptr, batch.lw, sn, an, gt=batch.future_gt, vis=batch.future_vis, err=True, lib=emu)
    with pytest.raises(L.StriveHipError):
        emu.call('strive_traffic_eval_metrics', L.ptr(pred), None, None, L.ptr(batch.ptr.to(torch.int32)), L.ptr(batch.lw), L.f4([0] * 4), L.f4([1] * 4),
                 L.f4([0] * 4), L.f4([1] * 4), None, None, None, 0, 32, 0, 4, 27, 3, 12, 12, None, None, None, None, None, None, None,
                 L.ptr(torch.zeros(4, dtype=torch.int32)), None)


def test_edge_cases(emu):
    sn, an = normalizers()
    out = run_kernel(emu, 'ns1')
    assert np.isnan(out['disp'][:, 4]).all(), 'NS = 1: APD is 0 / 0'
    assert not out['did_collide_veh'][0].any(), 'a one-agent scene has no vehicle collision'
    batch, mi, pred = inj('ns3')
    nanpred = torch.full_like(pred, float('nan'))
    o = TT.traffic_eval_metrics(nanpred, batch.ptr, batch.lw, sn, an, map_env=inj_env(), mapix=mi, env=True, veh=True, env_ego_only=False, lib=emu)
    assert o['status'].tolist() == [0] * 4 and not o['did_collide_map'].any() and not o['did_collide_veh'].any()
    assert o['grid_i'].tolist() == [0, 0, 0] and torch.isnan(o['grid_d']).all(), 'no valid frame: no grid, no collision'


# ------------------------------------------------------------------------------------------------
# checkpoints (strive_amd/utils/torch.py)
# ------------------------------------------------------------------------------------------------

def test_state_round_trip_and_warnings(tmp_path, capsys):
    m, sd = product_model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    path = str(tmp_path / 'ckpt.pth')
    UT.save_state(path, m, opt, cur_epoch=7, min_val_loss=0.25)
    ck = torch.load(path)
    assert sorted(ck.keys()) == ['epoch', 'min_val_loss', 'model', 'optim'] and list(ck['model'].keys()) == list(sd.keys())
    from strive_amd.models.traffic_model import TrafficModel
    fresh = TrafficModel(4, 12, 256, 2)
    assert UT.load_state(path, fresh, optimizer=torch.optim.Adam(fresh.parameters(), lr=1e-3), map_location='cpu') == (7, 0.25)
    assert all(torch.equal(v, sd[k]) for k, v in fresh.state_dict().items())
    assert capsys.readouterr().out == ''
    # ignore_keys: neither saved, loaded nor reported
    UT.save_state(path, m, opt, ignore_keys=['map_encoder'] if any(k.startswith('map_encoder.') for k in sd) else [list(sd)[0].split('.')[0]])
    top = 'map_encoder' if any(k.startswith('map_encoder.') for k in sd) else list(sd)[0].split('.')[0]
    assert not any(k.split('.')[0] == top for k in torch.load(path)['model'])
    fresh = TrafficModel(4, 12, 256, 2)
    before = {k: v.clone() for k, v in fresh.state_dict().items()}
    UT.load_state(path, fresh)
    text = capsys.readouterr().out
    assert UT.WARN_MISSING in text and UT.WARN_UNEXPECTED not in text
    UT.load_state(path, fresh, ignore_keys=[top])
    assert capsys.readouterr().out == ''
    assert all(torch.equal(v, before[k]) == (k.split('.')[0] == top) or torch.equal(v, sd[k]) for k, v in fresh.state_dict().items())
    ck = torch.load(path)
    ck['model']['not_a_module.weight'] = torch.zeros(1)
    torch.save(ck, path)
    UT.load_state(path, fresh, ignore_keys=[top])
    text = capsys.readouterr().out
    assert UT.WARN_UNEXPECTED in text and 'not_a_module.weight' in text and UT.WARN_MISSING not in text
    assert UT.calc_conv_out(256, 7, 2) == 125 and UT.compute_kl_weight(5, 10, 0.5) == 0.25 and UT.compute_kl_weight(20, 10, 0.5) == 0.5
    assert UT.tensor_clamp(torch.tensor([-2.0, 0.5, 3.0]), torch.tensor([-1.0, 0.0, 0.0]), torch.tensor([1.0, 1.0, 1.0])).tolist() == [-1.0, 0.5, 1.0]
    assert UT.count_params(m) == sum(p.numel() for p in m.parameters()) and UT.c2c(torch.ones(2, requires_grad=True)).tolist() == [1.0, 1.0]


# ------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------

class StubModel(object):
    """A model with TrafficModel's evaluation surface whose "rollout" is the ground truth plus a latent-dependent shift: the
    driver's bookkeeping (accumulators, counters, statuses, key order) without the cost of the emulated network."""
    z_size = 4

    def get_normalizer(self):
        return normalizers()[0]

    def get_att_normalizer(self):
        return normalizers()[1]

    def embed(self, sg, map_idx, map_env):
        NA = sg.past.size(0)
        base = sg.past[:, -1, :4]
        return {'prior_out': (base * 0.1, torch.ones((NA, 4)) * 0.5), 'posterior_out': (base * 0.1 + 0.01, torch.ones((NA, 4)) * 0.25),
                'map_feat': None, 'past_feat': None}

    def rsample(self, mean, var):
        return mean + 0.3 * torch.sqrt(var) * torch.arange(mean.size(0)).view(-1, 1, 1)

    def decoder(self, sg, map_feat, past_feat, z, map_idx, map_env, nfuture=None):
        T = sg.future_gt.size(1) if nfuture is None else nfuture
        gt = sg.future_gt[:, :T, :4]
        if z.dim() == 2:
            return gt + 0.01 * z.unsqueeze(1)
        return gt.unsqueeze(1) + 0.01 * z.unsqueeze(2)


def stub_loss(sg, pred):
    return {'loss': pred['future_pred'].sum().view(1), 'recon_loss': pred['future_pred'][:, 0, 0], 'kl_loss': None}


def test_driver_bookkeeping_with_a_stub_model(emu_ops, tmp_path, capsys):
    batches = G.run_batches(['stub/%d' % b for b in range(3)])
    raster, dx = G.run_raster()
    env = synth.SyntheticMapEnv(raster, dx)
    pb = []
    em = TT.run_one_epoch(batches, StubModel(), env, stub_loss, 'cpu', str(tmp_path), per_batch=pb, **FLAGS)
    keys = list(em.keys())
    assert keys == ['Test Mean ' + k for k in ('loss', 'recon_loss', 'pos_err', 'ang_err', 'z_logprob', 'z_mdist') + TT.DISP_KEYS] + \
        ['Test (%s, %s) Collision Freq' % (a, b) for a in ('recon_', 'sample_') for b in ('_map', '_veh')]
    text = capsys.readouterr().out
    assert 'Final ===================================== ' in text and all('%s = %f' % (k, v) in text for k, v in em.items())
    # the means are those of the concatenated per-batch vectors, the frequencies those of the summed counters
    vis = [(b[0].future_vis == 1.0) for b in batches]
    cat = np.concatenate([r['recon/pos_err'][v].numpy() for r, v in zip(pb, vis)])
    assert abs(em['Test Mean pos_err'] - cat.mean()) <= 16 * EPS64 * len(cat) * cat.mean()
    cat = np.concatenate([r['sample/disp'][:, 4].numpy() for r in pb])
    assert abs(em['Test Mean APD'] - cat.mean()) <= 16 * EPS64 * len(cat) * cat.mean()
    assert em['Test (sample_, _map) Collision Freq'] == sum(int(r['sample/did_collide_map'].sum()) for r in pb) / float(G.RUN_NS * 5)
    assert em['Test (recon_, _veh) Collision Freq'] == sum(int(r['recon/did_collide_veh'].sum()) for r in pb) / float(sum(map(sum, G.RUN_SIZES)))
    # a refused scene surfaces after the loop, with its batch and scene
    bad = [(b, mi.clone()) for b, mi in batches]
    bad[2][1][1] = 5
    with pytest.raises(ValueError, match='batch 2, scene 1: map index out of range'):
        TT.run_one_epoch(bad, StubModel(), env, stub_loss, 'cpu', str(tmp_path), **FLAGS)
    for flag in ('test_recon_viz_multi', 'test_sample_viz_multi', 'test_sample_viz_rollout'):
        with pytest.raises(NotImplementedError):
            TT.run_one_epoch(batches, StubModel(), env, stub_loss, 'cpu', str(tmp_path), **{flag: True})


def reference_structure(m, batches, env, loss_fn, device):
    """The product's own public functions called the way the reference's loop calls them: three model calls per batch, the four
    metric functions, torch.cat and mean."""
    metrics, freq, preds = {}, {}, []
    sn, an = m.get_normalizer(), m.get_att_normalizer()
    with torch.no_grad():
        for sg, mi in batches:
            sg, mi = sg.clone().to(device), mi.to(device)
            pred = m(sg, mi, env, use_post_mean=True)
            bm = {**loss_fn(sg, pred), **loss_fn.compute_err(sg, pred, sn)}
            bm = {k: bm[k] for k in ['loss'] + [k for k in bm if k != 'loss']}
            recon = m.reconstruct(sg, mi, env)
            coll = {'future_pred': recon['future_pred'].unsqueeze(1)}
            bf = {'recon_' + k: v for k, v in TM.compute_coll_rate_env(sg, mi, coll, env, sn, an, ego_only=True).items()}
            bf.update({'recon_' + k: v for k, v in TM.compute_coll_rate_veh(sg, coll, sn, an).items()})
            samp = m.sample_batched(sg, mi, env, G.RUN_NS, include_mean=False)
            bm.update(TM.compute_disp_err(sg, samp, sn))
            bf.update({'sample_' + k: v for k, v in TM.compute_coll_rate_env(sg, mi, samp, env, sn, an, ego_only=True).items()})
            bf.update({'sample_' + k: v for k, v in TM.compute_coll_rate_veh(sg, samp, sn, an).items()})
            for k, v in bm.items():
                if v is not None:
                    metrics.setdefault(k, []).append(v)
            for k, v in bf.items():
                if k.startswith(('recon_num', 'sample_num')):
                    freq[k] = freq.get(k, 0.0) + float(v)
            preds.append((pred['future_pred'], recon['future_pred'], samp['future_pred']))
    em = {'Test Mean ' + k: (torch.mean(torch.cat(v)).item(), torch.cat(v)) for k, v in metrics.items()}
    for a in ('recon_', 'sample_'):
        for b in ('_map', '_veh'):
            em['Test (%s, %s) Collision Freq' % (a, b)] = (freq[a + 'num_coll' + b] / freq[a + 'num_traj' + b], None)
    return em, freq, preds


def check_driver_against_public_functions(device):
    m, _ = product_model(device=device)
    raster, dx = G.run_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(device)
    loss_fn = TM.TrafficModelLoss(LOSS_W)
    batches = G.run_batches()
    torch.manual_seed(3)
    want, freq, preds = reference_structure(m, batches, env, loss_fn, device)
    torch.manual_seed(3)
    pb = []
    got = TT.run_one_epoch([(b.clone(), mi) for b, mi in batches], m, env, loss_fn, device, '.', per_batch=pb, **FLAGS)
    assert list(got.keys()) == list(want.keys())
    for r, (p_fwd, p_rec, p_smp) in zip(pb, preds):
        assert torch.equal(r['future_pred'], p_fwd) and torch.equal(r['future_pred'], p_rec), 'one decode serves pred and recon_pred'
        assert torch.equal(r['sample/future_pred'], p_smp), 'the shared-embed sampled rollout equals sample_batched byte for byte'
    for k, (v, vec) in want.items():
        if vec is None:
            assert got[k] == v, k
        else:
            # the same values averaged in float64 here and in fp32 there: N eps32 / 2 of the mean of the absolute values (worst case of
            # a recursive sum) + the per-value rounding of the fp32 metric functions (the bounds of the module docstring, <= 8 eps32
            # relative for these well-conditioned batches, 1e-3 degrees for the angles near 0)
            n, mabs = vec.numel(), float(vec.abs().double().mean())
            bound = (n / 2.0 + 8.0) * EPS32 * mabs + (np.degrees(np.sqrt(12 * EPS32)) if 'ang' in k else 0.0)
            if k == 'Test Mean loss':
                # each batch's loss holds a mean over its visible frames, formed by the driver as a masked sum over ALL frames and by
                # forward over the compacted ones: two fp32 sums of at most F terms in different orders, F / 2 eps32 each at worst
                bound += max(int(b.future_vis.numel()) for b, _ in batches) * EPS32 * mabs
            check('driver/' + k[len('Test Mean '):], got[k], v, bound, 'driver vs public functions')


def carried_bounds(g):
    """Bounds of the module docstring for run/*, from the reference's recorded values."""
    nb = len(G.RUN_SIZES)
    sm, ss = [t.numpy() for t in state_norm_tensors()]
    pos = np.sqrt(2.0) * ROLL_TOL * 15.0
    hn = min(float(np.linalg.norm(g['run/b%d/%sfuture_pred' % (b, t)][..., 2:4], axis=-1).min()) for b in range(nb) for t in ('recon_', 'sample_'))
    assert hn >= 0.9
    ang = float(np.degrees(np.arcsin(np.sqrt(2.0) * ROLL_TOL / (hn - np.sqrt(2.0) * ROLL_TOL))))
    out = {'pos_err': pos, 'pos_minADE': pos, 'pos_minFDE': pos, 'APD': 2 * pos, 'ang_err': ang, 'ang_minADE': ang, 'ang_minFDE': ang}
    batches = G.run_batches()
    num, den = 0.0, 0
    for b, (sg, _) in enumerate(batches):
        x = g['run/b%d/recon_future_pred' % b][:, 0].astype(np.float64)
        d = np.abs(x - sg.future_gt[..., :4].numpy().astype(np.float64))[sg.future_vis.numpy() == 1.0]
        num += float((d.sum(-1) * ROLL_TOL + 2.0 * ROLL_TOL ** 2).sum())
        den += d.shape[0]
    out['recon_loss'] = num / den
    lat = {'kl_loss': [0.0, 0], 'z_logprob': [0.0, 0], 'z_mdist': [0.0, 0]}
    for b in range(nb):
        t = [torch.tensor(g['run/b%d/%s' % (b, k)], dtype=torch.float64, requires_grad=True) for k in ('prior_mu', 'prior_var', 'posterior_mu', 'posterior_var')]
        pm, pv, qm, qv = t
        fns = {'kl_loss': kl_normal(qm, qv, pm, pv), 'z_logprob': log_normal(qm, pm, pv), 'z_mdist': torch.norm((qm - pm) / torch.sqrt(pv), dim=-1)}
        for k, f in fns.items():
            for i in range(f.numel()):
                grads = torch.autograd.grad(f[i], t, retain_graph=True, allow_unused=True)
                lat[k][0] += 2.0 * sum(float((gr.abs() * (EMB_RT * x.detach().abs() + EMB_AT)).sum()) for gr, x in zip(grads, t) if gr is not None)
            lat[k][1] += f.numel()
    for k, (s, n) in lat.items():
        out[k] = s / n
    out['loss'] = out['recon_loss'] + out['kl_loss']
    return out


def check_driver_against_run_fixture(device):
    g = fixture()
    m, _ = product_model(device=device)
    raster, dx = G.run_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(device)
    noise = [torch.from_numpy(g['run/b%d/noise' % b]).to(device) for b in range(len(G.RUN_SIZES))]
    it = iter(noise)
    m.rsample = lambda mean, var: mean + next(it) * torch.sqrt(var)
    pb = []
    got = TT.run_one_epoch(G.run_batches(), m, env, TM.TrafficModelLoss(LOSS_W), device, '.', per_batch=pb, **FLAGS)
    assert list(got.keys()) == [str(k) for k in g['run/epoch_keys']]
    bounds = carried_bounds(g)
    for b, r in enumerate(pb):
        for tag, key in (('recon_map', 'recon/did_collide_map'), ('recon_veh', 'recon/did_collide_veh'), ('sample_map', 'sample/did_collide_map'),
                         ('sample_veh', 'sample/did_collide_veh')):
            assert np.array_equal(r[key].cpu().numpy().astype(bool), g['run/b%d/%s' % (b, tag)].astype(bool)), 'batch %d %s' % (b, tag)
    for k, v in zip(g['run/epoch_keys'], g['run/epoch_vals']):
        k = str(k)
        if k.startswith('Test Mean '):
            check('run/' + k[len('Test Mean '):], got[k], v, bounds[k[len('Test Mean '):]], 'driver vs reference run')
        else:
            assert got[k] == v, k
    return got


def test_cli_on_the_emulation(emu_ops, tmp_path, capsys):
    """One scene of one agent, two future steps (three map-CNN evaluations on the emulation): the report has the reference's lines."""
    m, sd = product_model(FT=2)
    ckpt = str(tmp_path / 'ckpt.pth')
    UT.save_state(ckpt, m, torch.optim.Adam(m.parameters(), lr=1e-3), cur_epoch=3)
    out = str(tmp_path / 'out')
    argv = ['--ckpt', ckpt, '--out', out, '--device', 'cpu', '--scenes', 'synthetic', '--num_scenes', '1', '--scene_sizes', '1', '1',
            '--batch_size', '1', '--future_len', '2', '--test_recon_coll_rate']
    em = TT.main(argv)
    lines = open(os.path.join(out, 'test_log.txt')).read().splitlines()
    capsys.readouterr()
    assert lines[0].startswith('Args: ') and 'Loaded checkpoint from epoch 3...' in lines and 'Final ===================================== ' in lines
    assert 'Num model params: %d' % UT.count_params(m) in lines
    body = lines[lines.index('Final ===================================== ') + 1:-1]
    assert body == ['%s = %f' % (k, v) for k, v in em.items()] and lines[-1].startswith('Test time: ')
    assert [ln.rsplit(' = ', 1)[0] for ln in body] == ['Test Mean ' + k for k in ('loss', 'recon_loss', 'kl_loss', 'pos_err', 'ang_err', 'z_logprob', 'z_mdist')] + \
        ['Test (recon_, _map) Collision Freq', 'Test (recon_, _veh) Collision Freq']
    assert em['Test (recon_, _veh) Collision Freq'] == 0.0 and np.isfinite(em['Test Mean pos_err'])
    with pytest.raises(NotImplementedError):
        TT.main(argv + ['--test_sample_viz_multi'])
    with pytest.raises(SystemExit):
        TT.main(['--ckpt', ckpt, '--out', out])
    capsys.readouterr()


@pytest.mark.skipif(not SLOW, reason='the emulated network takes minutes (STRIVE_SLOW=1)')
def test_driver_matches_public_functions_on_the_emulation(emu_ops):
    check_driver_against_public_functions('cpu')


@pytest.mark.skipif(not SLOW, reason='the emulated network takes minutes (STRIVE_SLOW=1)')
def test_driver_matches_reference_run_on_the_emulation(emu_ops):
    check_driver_against_run_fixture('cpu')


# ------------------------------------------------------------------------------------------------
# MI355X
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('case', list(G.CASES))
def test_gpu_kernel_matches_fixture_and_emulator(emu, case):
    lib = L.get_lib()
    for ego_only in (True, False):
        got = run_kernel(lib, case, DEV, ego_only=ego_only)
        check_close64(got, run_kernel(emu, case, ego_only=ego_only), 'gpu vs emu %s ego_only=%s' % (case, ego_only))
        if ego_only:
            ego = got
    check_against_fixture(case, ego, got, 'gpu ' + case)


@pytest.mark.gpu
def test_gpu_scene_outputs_do_not_depend_on_the_batch():
    check_batch_independence(L.get_lib(), DEV)


@pytest.mark.gpu
def test_gpu_driver_matches_reference_run_and_public_functions():
    check_driver_against_run_fixture(DEV)
    check_driver_against_public_functions(DEV)


@pytest.mark.gpu
def test_gpu_no_synchronisation_in_the_batch_loop():
    """run_one_epoch over FRESH host batches (new objects, as a loader yields them: nothing cached on them) with every
    synchronising call an error while the loader is being consumed.  The warm-up epoch runs on other objects and leaves only what
    belongs to the process (weight packs, the map pack, the linspace table, workspaces)."""
    m, _ = product_model(device=DEV)
    raster, dx = G.run_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    loss_fn = TM.TrafficModelLoss(LOSS_W)
    want = TT.run_one_epoch(G.run_batches(), m, env, loss_fn, DEV, '.', **dict(FLAGS, test_sample_num=0 + G.RUN_NS))
    fresh = G.run_batches()
    assert all(not b.past.is_cuda and '_strive_scene_info' not in b.__dict__ and '_strive_train_consts' not in b.__dict__ for b, _ in fresh)

    class Guarded(object):
        """The loader ends the guarded region: the driver's one read-back follows the last batch."""

        def __iter__(self):
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode('error')
            try:
                for item in fresh:
                    yield item
            finally:
                torch.cuda.set_sync_debug_mode(prev)
    torch.manual_seed(11)
    em = TT.run_one_epoch(Guarded(), m, env, loss_fn, DEV, '.', **FLAGS)
    assert torch.cuda.get_sync_debug_mode() == 0 and np.isfinite(em['Test Mean pos_err'])
    assert all(b.past.is_cuda for b, _ in fresh), 'the batches were moved inside the guarded loop'
    for k in ('Test Mean pos_err', 'Test Mean recon_loss', 'Test Mean kl_loss', 'Test (recon_, _map) Collision Freq'):
        assert em[k] == want[k], k                     # (the posterior-mean quantities do not depend on the noise)
