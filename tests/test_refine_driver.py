"""The refine driver (strive_amd/refine_traffic_tracks.py -> strive_refine_verdicts, strive_amd/csrc/eval_metrics.hip) against the
reference's src/refine_traffic_optim.py: ``compute_metrics`` (:84-121) and ``run_one_epoch`` (:228-392).

Fixture g22_refine_driver.npz (tests/golden/make_golden_refine_driver.py, README_g22.md): ``inj/s<k>/*`` the reference's
compute_metrics on each of five injected scenes alone, ``inj/batch/*`` its compute_coll_rate_env on the five as one batch, ``run/*``
its run_one_epoch with the optimisation replaced by an injector.  The inputs are rebuilt by the generator's builders, which import
without the reference.

Bounds.  Against ``inj/*`` both sides start from the SAME fp32 unnormalised values; the reference continues in fp32, the kernel in
float64.  eps32 = 2^-23, eps64 = 2^-52.
  flags, counts, success, L, W, valid rows, statuses: equal (the tie conditions keep every threshold decision away from its
      threshold: IoUs 1e-3 from 0.02, drivable fractions two samples from 0.95, ratios 1e-3 from a half-integer).
  grid ratios: the bound tests/test_traffic_eval.py derives: a mean over R rows of sizes in fp32 (R / 2 eps32 worst case) and one
      division: (2 + R / 2) eps32 relative.
Against the float64 restatement (tests/refine_restated.py, the kernel's formulas in the kernel's order) and, on the MI355X, against
the host emulation: integers equal, doubles within 16 eps64 relative.

Largest error / bound per quantity: printed by the tests; profiles/r24_refine_ratios.md (written when STRIVE_WRITE_RATIOS is set).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import refine_restated as RS
import make_golden_refine_driver as G
from util import golden, product_model
from strive_amd import _lib as L
from strive_amd import ops
from strive_amd import synth
from strive_amd import refine_traffic_tracks as RT
from strive_amd.constants import state_norm_tensors, att_norm_tensors
from strive_amd.datasets import tracks as tracks_io
from strive_amd.datasets.nuscenes_dataset import NuScenesDataset
from strive_amd.utils.scenario_gen import prepare_output_dict

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
DEV = 'cuda:0'
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CFG = os.path.join(REPO, 'tests', 'golden', 'g22_refine_traffic_optim.cfg')
RATIOS = {}
SHAPES = [(1, 1), (2, 12), (17, 12), (65, 12), (257, 1)]        # past one wave's lanes, past the 256 threads of the grid sum
INT_KEYS = ('did_veh', 'did_env', 'out_i', 'status')


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
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(want))
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
            f.write('# Refine verdicts (`strive_refine_verdicts`, `strive_amd/refine_traffic_tracks.py`): largest observed error / bound\n\n')
            f.write('| quantity | largest error / bound |\n|---|---|\n')
            for k in sorted(RATIOS):
                f.write('| %s | %.3g |\n' % (k, RATIOS[k]))


# ------------------------------------------------------------------------------------------------
# inputs, shared and never modified
# ------------------------------------------------------------------------------------------------

_CACHE = {}


class StubModel(object):
    """What the verdicts and the scenario writer read of a model: its two normalisers."""

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


def fixture():
    if 'g' not in _CACHE:
        g = golden(G.FIX)
        _CACHE['g'] = {k: g[k] for k in g.files}
    return _CACHE['g']


def env(device='cpu'):
    if ('env', device) not in _CACHE:
        raster, dx = G.inj_raster()
        _CACHE[('env', device)] = synth.SyntheticMapEnv(raster, dx).to(device)
    return _CACHE[('env', device)]


def inj(kinds=None):
    key = ('inj', None if kinds is None else tuple(kinds))
    if key not in _CACHE:
        _CACHE[key] = G.inj_case(kinds)
    return _CACHE[key]


def shape_case(n, T):
    """One scene of n agents over T steps on map 0: boxes scattered densely enough to overlap here and there, across roads and
    blocks, any heading, a few NaN frames."""
    key = ('shape', n, T)
    if key not in _CACHE:
        k = 'g22/shape/%d/%d' % (n, T)
        side = 6.0 * np.sqrt(n) + 8.0
        tr = np.zeros((n, T, 4))
        tr[:, :, 0] = 30.0 + synth.counter_uniform((n, 1), k + '/x') * side + 0.5 * np.arange(T)[None, :]
        tr[:, :, 1] = 30.0 + synth.counter_uniform((n, 1), k + '/y') * side
        ang = synth.counter_uniform((n, 1), k + '/h') * 2.0 * np.pi
        tr[:, :, 2], tr[:, :, 3] = np.cos(ang), np.sin(ang)
        if n > 2 and T > 1:
            tr[1, T // 2:] = np.nan
            tr[n - 1, 0, 1] = np.nan
        lw = np.asarray([[4.5, 2.0], [4.0, 1.75], [8.0, 2.5], [5.0, 2.25]])[(synth.counter_uniform((n,), k + '/lw') * 4).astype(int)]
        smean, sstd = state_norm_tensors()
        amean, astd = att_norm_tensors()
        traj = ((synth.f32(tr) - smean[:4]) / sstd[:4]).unsqueeze(1).contiguous()
        _CACHE[key] = (traj, (synth.f32(lw) - amean) / astd)
    return _CACHE[key]


class _Graph(object):
    def __init__(self, lw, ptr):
        self.lw, self.ptr = lw, torch.as_tensor(ptr, dtype=torch.long)


def run_kernel(lib, traj, lw, ptr, map_idx, device='cpu', **kw):
    out = RT.batch_verdicts(traj.to(device), model(), _Graph(lw.to(device), ptr), env(device), torch.as_tensor(map_idx).to(device), lib=lib, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_inj(lib, kinds=None, device='cpu', **kw):
    batch, mi, traj = inj(kinds)
    return run_kernel(lib, traj, batch.lw, batch.ptr, mi, device, **kw)


def restated(traj, lw, ptr, map_idx, **kw):
    sm, ss = [t.numpy() for t in state_norm_tensors()]
    am, as_ = [t.numpy() for t in att_norm_tensors()]
    raster, dx = G.inj_raster()
    return RS.verdicts(traj[:, 0].numpy(), ptr, lw.numpy(), sm, ss, am, as_, raster.numpy(), dx.numpy(), map_idx, **kw)


def restated_shape(n, T):
    key = ('rs', n, T)
    if key not in _CACHE:
        traj, lw = shape_case(n, T)
        _CACHE[key] = restated(traj, lw, [0, n], [0])
    return _CACHE[key]


def check_close64(got, want, what):
    """Two evaluations of the same float64 formulas: discrete outputs equal, continuous ones within 16 eps64 relative."""
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), '%s %s' % (what, k)
    check('f64/grid_d', got['grid_d'], want['grid_d'], 16 * EPS64 * np.abs(np.nan_to_num(want['grid_d'], nan=0.0)), what)


def sentinels(NA, B, device='cpu'):
    return {'did_veh': torch.full((NA,), -7, dtype=torch.int32, device=device), 'did_env': torch.full((NA,), -7, dtype=torch.int32, device=device),
            'out_i': torch.full((B, 8), -7, dtype=torch.int32, device=device), 'grid_d': torch.full((B, 2), -7.0, dtype=torch.float64, device=device),
            'status': torch.full((B,), -7, dtype=torch.int32, device=device)}


# ------------------------------------------------------------------------------------------------
# the fixture itself
# ------------------------------------------------------------------------------------------------

def test_fixture_tie_conditions():
    g = fixture()
    layers = [k[:-len('frac')] for k in g if k.endswith('/frac')]
    assert sorted(layers) == ['inj/batch/'] + ['inj/s%d/' % k for k in range(len(G.SIZES))]
    for p in layers:
        L_, W_ = int(g[p + 'L']), int(g[p + 'W'])
        assert np.abs(g[p + 'frac'].astype(np.float64) - 0.95).min() > 2.0 / (L_ * W_), p
        assert np.abs(g[p + 'ratio'] - np.floor(g[p + 'ratio']) - 0.5).min() > 1e-3, p
    for k in [k for k in g if k.endswith('iou')]:
        v = g[k][~np.isnan(g[k])]
        assert not v.size or np.abs(v - G.IOU_THRESH).min() > G.TIE_MARGIN, k
    assert sum(g['inj/s%d/iou' % k].size for k in range(len(G.SIZES))) > 20000
    # what the injected scenes exist for, in the reference's outputs
    own = np.concatenate([g['inj/s%d/did_env' % k] for k in range(len(G.SIZES))])
    flip = int(np.cumsum([0] + G.SIZES)[G.FLIP[0]]) + G.FLIP[1]
    assert np.nonzero(own != g['inj/batch/did_env'])[0].tolist() == [flip] and g['inj/batch/did_env'][flip] == 1
    assert {k: (int(g['inj/s%d/L' % k]), int(g['inj/s%d/W' % k])) for k in range(len(G.SIZES))} == G.OWN_GRID
    assert (int(g['inj/batch/L']), int(g['inj/batch/W'])) == G.BATCH_GRID and G.BATCH_GRID not in G.OWN_GRID.values()
    assert g['inj/s3/did_veh'].nonzero()[0].tolist() == [5, 9] and g['inj/s2/did_veh'].tolist() == [0, 1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------
# host emulation: the kernel
# ------------------------------------------------------------------------------------------------

def check_against_fixture(out, what):
    """The five scenes in ONE call against the reference's five per-scene calls."""
    g = fixture()
    ptr = np.cumsum([0] + G.SIZES)
    assert not out['status'].any(), what
    for k, n in enumerate(G.SIZES):
        p = 'inj/s%d/' % k
        lo, hi = ptr[k], ptr[k + 1]
        assert np.array_equal(out['did_veh'][lo:hi], g[p + 'did_veh']), '%s did_veh of scene %d' % (what, k)
        assert np.array_equal(out['did_env'][lo:hi], g[p + 'did_env']), '%s did_env of scene %d' % (what, k)
        veh, env_ = [int(v) for v in g[p + 'seq_metrics']]
        rows = g[p + 'frac'].size
        assert out['out_i'][k].tolist() == [veh, n, env_, n, int(veh == 0 and env_ == 0), int(g[p + 'L']), int(g[p + 'W']), rows], '%s out_i of scene %d' % (what, k)
        assert g[p + 'freq_cnt'].tolist() == [veh, env_] and g[p + 'freq_total'].tolist() == [n, n]
        check('grid_ratio', out['grid_d'][k], g[p + 'ratio'], (2.0 + rows / 2.0) * EPS32 * np.abs(g[p + 'ratio']), '%s scene %d' % (what, k))
    # the case a kernel with one grid per call fails: the truck of scene 2 is on the road under ITS scene's grid only
    flip = int(ptr[G.FLIP[0]]) + G.FLIP[1]
    assert out['did_env'][flip] == 0 and g['inj/batch/did_env'][flip] == 1


def test_kernel_matches_reference_fixture(emu):
    check_against_fixture(run_inj(emu), 'emu')


def test_compute_metrics_on_a_single_scene_graph(emu_ops):
    g = fixture()
    cnt, tot = {}, {}
    for k in range(len(G.SIZES)):
        batch, mi, traj = inj([k])
        z = torch.zeros((G.SIZES[k], 4))
        metrics, cnt, tot, seq = RT.compute_metrics({}, cnt, tot, z, traj, model(), batch, env(), mi, (z, z + 1.0))
        assert metrics == {} and [seq['veh_coll'], seq['env_coll']] == g['inj/s%d/seq_metrics' % k].tolist()
    want = np.sum([g['inj/s%d/freq_cnt' % k] for k in range(len(G.SIZES))], axis=0)
    assert [cnt['veh_coll'], cnt['env_coll']] == want.tolist() and tot == {'veh_coll': sum(G.SIZES), 'env_coll': sum(G.SIZES)}


@pytest.mark.parametrize('n,T', SHAPES)
def test_kernel_matches_restatement(emu, n, T):
    traj, lw = shape_case(n, T)
    want = restated_shape(n, T)
    check_close64(run_kernel(emu, traj, lw, [0, n], [0]), want, 'restated n=%d T=%d' % (n, T))
    if n >= 17:
        assert want['did_veh'].any() and not want['did_veh'].all() and want['did_env'].any() and not want['did_env'].all()


def test_restatement_matches_reference_fixture():
    """(the restatement itself is pinned: the two small scenes that carry the built-in cases)"""
    g = fixture()
    for k in (1, 2):
        batch, mi, traj = inj([k])
        r = restated(traj, batch.lw, batch.ptr.tolist(), mi.tolist())
        assert np.array_equal(r['did_veh'], g['inj/s%d/did_veh' % k]) and np.array_equal(r['did_env'], g['inj/s%d/did_env' % k])
        assert np.array_equal(r['frac'].astype(np.float32), g['inj/s%d/frac' % k])
        if not r['did_veh'].any():                       # (after a hit the reference leaves its loops: it forms fewer IoUs)
            ok = ~np.isnan(g['inj/s%d/iou' % k])
            assert np.array_equal(np.isnan(r['iou']), ~ok) and not ok.all()
            check('restated/iou', r['iou'][ok], g['inj/s%d/iou' % k][ok], 1e-9, 'restatement vs exact IoU, scene %d' % k)


def check_batch_independence(lib, device):
    """A scene alone and inside a batch (other neighbours, another number of workgroups per scene): the same bytes."""
    full = run_inj(lib, None, device)
    ptr = np.cumsum([0] + G.SIZES)
    for k in (0, 2, 3):
        one = run_inj(lib, [k], device)
        lo, hi = ptr[k], ptr[k + 1]
        assert one['did_veh'].tobytes() == full['did_veh'][lo:hi].tobytes() and one['did_env'].tobytes() == full['did_env'][lo:hi].tobytes()
        assert one['out_i'].tobytes() == full['out_i'][k:k + 1].tobytes() and one['grid_d'].tobytes() == full['grid_d'][k:k + 1].tobytes()
    a, b = run_inj(lib, None, device), run_inj(lib, [4, 1, 2], device)
    assert all(a[k].tobytes() == full[k].tobytes() for k in a), 'two runs give the same bytes'
    assert b['out_i'][2].tobytes() == full['out_i'][2].tobytes() and b['did_env'][67:].tobytes() == full['did_env'][ptr[2]:ptr[3]].tobytes()


def test_scene_outputs_do_not_depend_on_the_batch(emu):
    check_batch_independence(emu, 'cpu')


def test_out_of_range_statuses_leave_outputs_untouched(emu):
    """(emulation only: offsets that leave the arrays are refused before anything is read)"""
    batch, mi, traj = inj([0, 1, 2, 3])
    NA = int(traj.shape[0])
    good = run_kernel(emu, traj, batch.lw, batch.ptr, mi)
    bad_mi = mi.clone()
    bad_mi[3] = 2
    out = run_kernel(emu, traj, batch.lw, batch.ptr, bad_mi, out=sentinels(NA, 4))
    assert out['status'].tolist() == [0, 0, 0, 3]
    assert (out['did_veh'][8:] == -7).all() and (out['did_env'][8:] == -7).all() and (out['out_i'][3] == -7).all() and (out['grid_d'][3] == -7).all()
    assert all(out[k][:8].tobytes() == good[k][:8].tobytes() for k in ('did_veh', 'did_env')) and out['out_i'][:3].tobytes() == good['out_i'][:3].tobytes()
    bad_mi[3] = -1
    assert run_kernel(emu, traj, batch.lw, batch.ptr, bad_mi, out=sentinels(NA, 4))['status'].tolist() == [0, 0, 0, 3]
    # scene 1 ends past the last agent, scene 2 ends before it starts; scenes 0 and 3 are served
    out = run_kernel(emu, traj, batch.lw, [0, 1, 40, 8, NA], mi, out=sentinels(NA, 4))
    assert out['status'].tolist() == [0, 2, 2, 0]
    assert (out['did_veh'][1:8] == -7).all() and (out['out_i'][1:3] == -7).all() and (out['grid_d'][1:3] == -7).all()
    assert out['did_veh'][:1].tolist() == [0] and out['out_i'][3].tobytes() == good['out_i'][3].tobytes()
    out = run_kernel(emu, traj, batch.lw, [0, 0, 3, 8, NA], mi, out=sentinels(NA, 4))
    assert out['status'].tolist() == [2, 0, 0, 0], 'a scene without agents'
    with pytest.raises(L.StriveHipError):
        emu.call('strive_refine_verdicts', L.ptr(traj), L.ptr(batch.ptr.to(torch.int32)), L.ptr(batch.lw), L.f4([0] * 4), L.f4([1] * 4), L.f4([0] * 4),
                 L.f4([1] * 4), None, None, None, 0, 4, NA, 12, None, None, None, None, None, None)


def check_status_4(lib, device):
    """lin_max 20 serves the cars' 13 x 7 grid and refuses the trucks' 32 x 10: THAT scene alone, its outputs untouched."""
    batch, mi, traj = inj([1, 2, 3])
    NA = int(traj.shape[0])
    good = run_kernel(lib, traj, batch.lw, batch.ptr, mi, device)
    out = run_kernel(lib, traj, batch.lw, batch.ptr, mi, device, out=sentinels(NA, 3, device), lin_max=20)
    assert out['status'].tolist() == [0, 4, 0]
    assert (out['did_veh'][2:7] == -7).all() and (out['did_env'][2:7] == -7).all() and (out['out_i'][1] == -7).all() and (out['grid_d'][1] == -7).all()
    for k in ('did_veh', 'did_env'):
        assert out[k][:2].tobytes() == good[k][:2].tobytes() and out[k][7:].tobytes() == good[k][7:].tobytes(), k
    for k in ('out_i', 'grid_d'):
        assert out[k][0].tobytes() == good[k][0].tobytes() and out[k][2].tobytes() == good[k][2].tobytes(), k
    return out


def test_status_4_is_the_scenes_own(emu):
    check_status_4(emu, 'cpu')


def test_a_scene_without_a_valid_row(emu):
    traj, lw = shape_case(17, 12)
    out = run_kernel(emu, torch.full_like(traj, float('nan')), lw, [0, 17], [0])
    assert out['status'].tolist() == [0] and not out['did_veh'].any() and not out['did_env'].any()
    assert out['out_i'][0].tolist() == [0, 17, 0, 17, 1, 0, 0, 0] and np.isnan(out['grid_d']).all(), 'no valid frame: no grid, no collision'


# ------------------------------------------------------------------------------------------------
# the batcher
# ------------------------------------------------------------------------------------------------

def batches_of(events):
    return [what for kind, what in events if kind == 'batch']


def test_plan_batches():
    g = fixture()
    counts = [G.SIZES[k] for k in G.RUN_KINDS]
    ev = RT.plan_batches(counts, G.RUN_BATCH_SIZE, G.RUN_FEASIBILITY)
    assert batches_of(ev) == json.loads(str(g['run/batches'])) == G.RUN_BATCHES
    keep = ('Only ', 'Feasible', 'Batch NA', 'Formed batch')
    assert [w for k, w in ev if k == 'log'] == [str(ln) for ln in g['run/lines'] if str(ln).startswith(keep)]
    assert RT.plan_batches([], 10, 1) == [], 'an empty loader'
    ev = RT.plan_batches([1, 2, 1], 10, 3)
    assert batches_of(ev) == [] and [w for _, w in ev] == ['Only %d agents in scene, skipping...' % c for c in (1, 2, 1)], 'all infeasible'
    assert batches_of(RT.plan_batches([4, 5, 1], 100, 2)) == [[0, 1]], 'the last scene infeasible: what is queued still forms a batch'
    assert batches_of(RT.plan_batches([4, 50, 3, 3], 10, 1)) == [[0, 1], [2, 3]], 'one scene larger than batch_size'
    assert batches_of(RT.plan_batches([50], 10, 1)) == [[0]] and batches_of(RT.plan_batches([5, 5, 5], 10, 1)) == [[0, 1], [2]]
    b = RT.AgentCountBatcher(10, 1)
    assert b.push(3, False) == [('log', 'Feasible. Adding to batch...'), ('log', 'Batch NA: 3')]
    assert b.push(7, False)[-1] == ('batch', [0, 1]) and b.queue == [] and b.total == 0


# ------------------------------------------------------------------------------------------------
# the driver on injected results
# ------------------------------------------------------------------------------------------------

def listing(out):
    root = os.path.join(out, 'scenario_results')
    return sorted((d, fn) for d in os.listdir(root) for fn in os.listdir(os.path.join(root, d)))


def canon(obj):
    """JSON text with sorted keys: equal for equal content, NaN entries included."""
    return json.dumps(obj, sort_keys=True)


def strip(lines, out):
    """The log lines without the timing value and the path prefix."""
    return ['Optimized sequence' if ln.startswith('Optimized sequence in ') else ln.replace(out, 'OUT') for ln in lines]


def test_run_one_epoch_matches_reference_run(emu_ops, tmp_path, capsys):
    g = fixture()
    out = str(tmp_path / 'out')
    seen = []

    def refine(scene_graph, *a, **k):
        seen.append(np.diff(scene_graph.ptr.numpy()).tolist())
        return G.injected_refine(scene_graph, *a, **k)
    with open(str(tmp_path / 'log.txt'), 'w') as log:
        cnt, tot, kept = RT.run_one_epoch(G.RunLoader(), G.RUN_BATCH_SIZE, model(), env(), 'cpu', out, {}, feasibility_NA=G.RUN_FEASIBILITY,
                                          samp_future_len=G.T, save_future_len=G.T, optim_use_adam=True, num_iters=1, lr=0.05, save=True,
                                          log=log, refine_fn=refine, keep_results=True)
    lines = open(str(tmp_path / 'log.txt')).read().splitlines()
    assert capsys.readouterr().out.splitlines() == lines
    assert seen == [[G.SIZES[G.RUN_KINDS[i]] for i in b] for b in G.RUN_BATCHES] and [r['positions'] for r in kept] == G.RUN_BATCHES
    assert strip(lines, out) == strip([str(ln) for ln in g['run/lines']], 'OUT')
    assert lines[-2:] == [str(ln) for ln in g['run/rates_text']] == ['veh_coll = %f' % (cnt['veh_coll'] / tot['veh_coll']), 'env_coll = %f' % (cnt['env_coll'] / tot['env_coll'])]
    assert listing(out) == sorted(zip([str(d) for d in g['run/dirs']], [str(f) for f in g['run/files']]))
    for d, fn, text in zip(g['run/dirs'], g['run/files'], g['run/json']):
        with open(os.path.join(out, 'scenario_results', str(d), str(fn))) as f:
            assert canon(json.load(f)) == canon(json.loads(str(text))), fn
    # every file is what prepare_output_dict gives for its scene with the reference's arguments (:354-357)
    for r in kept:
        scenes = r['scene_graph'].to_data_list()
        ptr = r['scene_graph'].ptr.tolist()
        for b, pos in enumerate(r['positions']):
            d = 'success' if int(r['verdicts']['out_i'][b, 4]) else 'failed'
            want = prepare_output_dict(scenes[b], int(r['map_idx'][b]), env(), G.DT, model(), r['init_future_pred'][ptr[b]:ptr[b + 1]],
                                       r['final_result_traj'][ptr[b]:ptr[b + 1]][:, 0])
            with open(os.path.join(out, 'scenario_results', d, 'scene_%04d.json' % pos)) as f:
                assert canon(json.load(f)) == canon(want), pos
    # nothing is written without save
    RT.run_one_epoch(G.RunLoader(), G.RUN_BATCH_SIZE, model(), env(), 'cpu', str(tmp_path / 'dry'), {}, feasibility_NA=G.RUN_FEASIBILITY,
                     save=False, refine_fn=G.injected_refine)
    assert os.listdir(str(tmp_path / 'dry')) == []
    capsys.readouterr()


def test_copies_to_the_host_per_batch_do_not_depend_on_the_number_of_scenes(emu_ops, tmp_path, monkeypatch, capsys):
    """The batches of run/* hold 2, 3 and 1 scenes: each costs the driver two ``.cpu()`` calls (the integers; the tensors of the files)."""
    calls, marks = [0], []
    orig = torch.Tensor.cpu

    def counted(self, *a, **k):
        calls[0] += 1
        return orig(self, *a, **k)

    def refine(scene_graph, *a, **k):
        res = G.injected_refine(scene_graph, *a, **k)
        marks.append(calls[0])                      # (after the injector, which looks at ptr itself)
        return res
    monkeypatch.setattr(torch.Tensor, 'cpu', counted)
    RT.run_one_epoch(G.RunLoader(), G.RUN_BATCH_SIZE, model(), env(), 'cpu', str(tmp_path), {}, feasibility_NA=G.RUN_FEASIBILITY, save=True,
                     refine_fn=refine)
    marks.append(calls[0] + 1)                      # (the injector's own call, which the last batch has no successor to count)
    capsys.readouterr()
    assert len(marks) == 4 and [b - a for a, b in zip(marks, marks[1:])] == [3, 3, 3]


def test_rendering_and_wandb_raise(tmp_path):
    for flag in ('viz', 'use_wandb'):
        with pytest.raises(NotImplementedError):
            RT.run_one_epoch(G.RunLoader(), 20, model(), env(), 'cpu', str(tmp_path), {}, refine_fn=G.injected_refine, **{flag: True})
    assert not os.path.exists(str(tmp_path / 'scenario_results'))


def shifted_refine(scene_graph, map_idx, map_env, model_, loss_weights, num_iters, samp_future_len, save_future_len, optim_use_adam, lr):
    """A deterministic function of the batch: the ground truth moved sideways by an amount that grows with the agent's row."""
    fut = scene_graph.future_gt[:, :save_future_len, :4].clone()
    fut[:, :, 1] += 0.6 * torch.arange(fut.shape[0], dtype=fut.dtype, device=fut.device).view(-1, 1)
    z = torch.zeros((fut.shape[0], 4), device=fut.device)
    return scene_graph.future_gt[:, :, :4].clone(), z, fut.unsqueeze(1), {'prior_out': (z, z + 1.0)}


def check_planned_equals_collected(device, tmp_path):
    """A scene_source (counts -> plan -> one gather per batch) and the same scenes as a plain iterable (collected one by one): the
    same batches, verdicts, log lines and files, bit for bit."""
    raster, dx = synth.make_raster(M=2)
    menv = synth.SyntheticMapEnv(raster, dx).to(device)
    ds = NuScenesDataset(synth.make_tracks(n_scenes=3, n_agents=6, T=21, M=2), menv, npast=4, nfuture=12, seq_interval=2, device=device)
    src = RT.scene_source(ds, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert len(src) == len(ds) == 9 and sorted(src.order) == list(range(9)) and src.order != list(range(9))
    assert src.counts == [int(b.past.shape[0]) for b, _ in src]
    results = {}
    for name, loader in (('planned', src), ('collected', list(src))):
        out, seen = str(tmp_path / name), []

        def refine(scene_graph, *a, **k):
            seen.append({k_: scene_graph[k_].clone() for k_ in scene_graph.keys() if torch.is_tensor(scene_graph[k_]) and k_ not in ('x', 'pos')})
            return shifted_refine(scene_graph, *a, **k)
        with open(out + '.txt', 'w') as log:
            cnt, tot, kept = RT.run_one_epoch(loader, 8, model(), menv, device, out, {}, feasibility_NA=5, save=True, log=log, refine_fn=refine,
                                              dt=ds.dt, keep_results=True)
        results[name] = (seen, kept, cnt, tot, strip(open(out + '.txt').read().splitlines(), out), out)
    a, b = results['planned'], results['collected']
    assert len(a[0]) == len(b[0]) >= 2 and [r['positions'] for r in a[1]] == [r['positions'] for r in b[1]]
    assert any(len(r['positions']) > 1 for r in a[1]) and sum(len(r['positions']) for r in a[1]) < len(src), 'batches of several scenes; skipped scenes'
    for ga, gb in zip(a[0], b[0]):
        assert sorted(ga) == sorted(gb)
        for k in ga:
            assert ga[k].dtype == gb[k].dtype and torch.equal(torch.nan_to_num(ga[k].double(), nan=-7.0), torch.nan_to_num(gb[k].double(), nan=-7.0)), k
    for ra, rb in zip(a[1], b[1]):
        assert all(torch.equal(torch.nan_to_num(ra['verdicts'][k].double(), nan=-7.0), torch.nan_to_num(rb['verdicts'][k].double(), nan=-7.0)) for k in ra['verdicts'])
        assert torch.equal(ra['map_idx'], rb['map_idx'])
    assert a[2:5] == b[2:5] and listing(a[5]) == listing(b[5])
    for d, fn in listing(a[5]):
        assert open(os.path.join(a[5], 'scenario_results', d, fn)).read() == open(os.path.join(b[5], 'scenario_results', d, fn)).read(), fn


def test_planned_path_equals_collected_path(emu_ops, tmp_path, capsys):
    check_planned_equals_collected('cpu', tmp_path)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------

def test_config_file(tmp_path):
    cfg, ignored = RT.parse_cfg(['--config', CFG])
    assert ignored == ['data_dir', 'data_version', 'split', 'num_workers', 'viz']
    want = dict(out='./out/refine_traffic_optim_out', seq_interval=10, shuffle=True, batch_size=10, ckpt='./model_ckpt/traffic_model.pth',
                viz=False, save=True, feasibility_num=10, samp_future_len=16, save_future_len=12, num_iters=200, lr=0.05, loss_coll_veh=100.0,
                loss_coll_env=100.0, loss_init_z=0.01, loss_motion_prior=1.0, optim_use_adam=True, past_len=4, future_len=12, latent_size=32,
                seed=0, device='cuda:0', tracks=None)
    assert {k: cfg[k] for k in want} == want
    cfg, _ = RT.parse_cfg(['--config', CFG, '--num_iters', '3', '--out', 'o', '--optim_use_lbfgs', '--seed', '4'])
    assert (cfg['num_iters'], cfg['out'], cfg['optim_use_adam'], cfg['seed'], cfg['lr']) == (3, 'o', False, 4, 0.05), 'the command line wins'
    # the reference's defaults (:34-82) without a file
    cfg, ignored = RT.parse_cfg([])
    assert ignored == [] and (cfg['batch_size'], cfg['feasibility_num'], cfg['samp_future_len'], cfg['save_future_len'], cfg['num_iters'], cfg['lr'],
                              cfg['save'], cfg['shuffle'], cfg['seq_interval'], cfg['out']) == (4, 1, 16, 12, 10, 1.0, False, False, 10, './out/traffic_out')
    bad = str(tmp_path / 'bad.cfg')
    with open(bad, 'w') as f:
        f.write('num_iters: 5\nnum_itres: 6\n')
    with pytest.raises(ValueError, match='unknown key `num_itres`'):
        RT.parse_cfg(['--config', bad])
    with open(bad, 'w') as f:
        f.write('save: yes\n')
    with pytest.raises(ValueError, match='`save` takes True or False'):
        RT.parse_cfg(['--config', bad])
    with open(bad, 'w') as f:
        f.write('optim_use_lbfgs: True\nshuffle: False\nagent_types: [car, truck]\n')
    cfg, _ = RT.parse_cfg(['--config', bad])
    assert cfg['optim_use_adam'] is False and cfg['shuffle'] is False and cfg['agent_types'] == ['car', 'truck'] and cfg['num_classes'] == 2
    with pytest.raises(SystemExit, match='Must pass in model weights'):
        RT.main(['--out', str(tmp_path / 'o')])


# ------------------------------------------------------------------------------------------------
# MI355X
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_kernel_matches_emulator_and_fixture(emu):
    lib = L.get_lib()
    got = run_inj(lib, None, DEV)
    check_close64(got, run_inj(emu), 'gpu vs emu, the fixture batch')
    check_against_fixture(got, 'gpu')
    for n, T in SHAPES:
        traj, lw = shape_case(n, T)
        check_close64(run_kernel(lib, traj, lw, [0, n], [0], DEV), run_kernel(emu, traj, lw, [0, n], [0]), 'gpu vs emu n=%d T=%d' % (n, T))
    check_close64(check_status_4(lib, DEV), check_status_4(emu, 'cpu'), 'gpu vs emu, status 4')


@pytest.mark.gpu
def test_gpu_scene_outputs_do_not_depend_on_the_batch():
    check_batch_independence(L.get_lib(), DEV)


@pytest.mark.gpu
def test_gpu_planned_path_equals_collected_path(tmp_path, capsys):
    check_planned_equals_collected(DEV, tmp_path)
    capsys.readouterr()


@pytest.mark.gpu
def test_gpu_driver_end_to_end(tmp_path, capsys):
    """``python -m strive_amd.refine_traffic_tracks`` on the shipped config and a synthetic tracks file with the real
    ``refine_traffic_optim`` (Adam, 3 iterations): files, directories and rates are what ``batch_verdicts`` and
    ``prepare_output_dict`` give on the trajectories the driver returned; a second run with the same seed writes the same listing."""
    from strive_amd.datasets.utils import read_adv_scenes
    from strive_amd.utils import torch as UT
    path = str(tmp_path / 'tracks.npz')
    tracks_io.save_tracks(path, synth.make_tracks(n_scenes=2, n_agents=5, T=20))
    m, _ = product_model()
    ckpt = str(tmp_path / 'ckpt.pth')
    UT.save_state(ckpt, m, torch.optim.Adam(m.parameters(), lr=1e-3), cur_epoch=2)
    listings = []
    for run in ('a', 'b'):
        out = str(tmp_path / run)
        argv = ['--config', CFG, '--tracks', path, '--ckpt', ckpt, '--out', out, '--num_iters', '3', '--seq_interval', '3', '--feasibility_num', '2',
                '--batch_size', '8', '--seed', '7']
        cnt, tot, kept = RT.main(argv, keep_results=True)
        listings.append(listing(out))
        lines = open(os.path.join(out, 'refine_traffic_log.txt')).read().splitlines()
        assert lines[0].startswith('Args: ') and lines[-2:] == ['veh_coll = %f' % (cnt['veh_coll'] / tot['veh_coll']), 'env_coll = %f' % (cnt['env_coll'] / tot['env_coll'])]
        assert any(ln.startswith('Ignoring config keys') and 'viz' in ln for ln in lines)
    capsys.readouterr()
    assert listings[0] == listings[1] and 3 <= len(listings[0]) <= 4
    assert sorted(p for r in kept for p in r['positions']) == sorted(int(fn[6:10]) for _, fn in listings[1])
    raster, dx = synth.make_raster()
    menv = synth.SyntheticMapEnv(raster, dx).to(DEV)
    m = m.to(DEV)
    veh = envc = agents = 0
    for r in kept:
        sg = r['scene_graph']
        v = RT.batch_verdicts(r['final_result_traj'], m, sg, menv, r['map_idx'])
        assert all(torch.equal(torch.nan_to_num(v[k].double(), nan=-7.0), torch.nan_to_num(r['verdicts'][k].double(), nan=-7.0)) for k in v)
        oi = v['out_i'].cpu().numpy()
        assert not v['status'].any() and r['final_result_traj'].shape[1:] == (1, 12, 4)
        veh, envc, agents = veh + int(oi[:, 0].sum()), envc + int(oi[:, 2].sum()), agents + int(oi[:, 1].sum())
        scenes, ptr = sg.to_data_list(), sg.ptr.tolist()
        for b, pos in enumerate(r['positions']):
            d = 'success' if oi[b, 4] else 'failed'
            assert oi[b, 4] == int(oi[b, 0] == 0 and oi[b, 2] == 0) and (d, 'scene_%04d.json' % pos) in listings[1]
            want = prepare_output_dict(scenes[b], int(r['map_idx'][b]), menv, 0.5, m, r['init_future_pred'][ptr[b]:ptr[b + 1]],
                                       r['final_result_traj'][ptr[b]:ptr[b + 1]][:, 0])
            with open(os.path.join(out, 'scenario_results', d, 'scene_%04d.json' % pos)) as f:
                assert canon(json.load(f)) == canon(want), pos
    assert (cnt, tot) == ({'veh_coll': veh, 'env_coll': envc}, {'veh_coll': agents, 'env_coll': agents})
    for d in {d for d, _ in listings[1]}:                  # the scenario readers of the dataset and of eval_adv_gen take the files
        got = read_adv_scenes(os.path.join(out, 'scenario_results', d))
        assert len(got) == sum(1 for d2, _ in listings[1] if d2 == d) and all(sc['scene_fut'].shape[1:] == (12, 4) for sc in got)
