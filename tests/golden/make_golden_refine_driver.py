#!/usr/bin/env python3
"""Generate tests/golden/g22_refine_driver.npz: the reference's refine driver (src/refine_traffic_optim.py ``compute_metrics`` and
``run_one_epoch``), run by the reference itself in the build container.  Only outputs are stored; the inputs are rebuilt by the
builders below, which import without the reference (the tests, GPU tests included, call them).  It uses make_golden's import
stand-ins and the EXACT shapely stand-in and stubs configargparse (absent).  The file is described in tests/golden/README_g22.md.

inj/*: injected final trajectories.  World of ``synth.make_raster(M=2)`` (256 m, 0.25 m pixels; map 0: roads are the 18 m bands y or x
in [40 k, 40 k + 18)).  Five scenes ("kinds") of 1, 2, 5, 19 and 65 agents on maps (0, 1, 0, 0, 0); kinds 0 and 2 hold trucks (8 m x
2.5 m: L, W = 32, 10), the others cars (about 3.25 m x 1.75 m: 13, 7), so the scenes' own sampling grids differ and the grid of
one call on the whole batch (14, 7) is none of them.  Agent a of a scene drives along x in lane a % 4 of road band a // 12, slot
(a // 4) % 3; T = 12 steps of 0.5 s.  On top of that:
  kind 1 (map 1)  agent 1 stands at (145, 100): on the road of map 1, off the road of map 0; agent 0 has NaN frames 3, 4
  kind 2          agent 3 keeps agent 1's x at a lateral 5 m and closes to 1.5 m at the LAST step only (charged to agent 1)
                  agent 4, a truck, stands across the edge of a road band with its first sample row (of 32) off the road: on
                  the road under its scene's grid (310 of 320 samples), off it under the batch's 14 x 7 grid (91 of 98)
  kind 3          agent 5 overlaps the later agents 9 and 12 at every step (counted once); agent 9 overlaps 12 (charged to 9);
                  agent 12 overlaps earlier agents only (not charged); agent 14 is NaN throughout, agent 7 from step 5; agent 16
                  stands off the road
  kind 4          agents 30 and 50 overlap from step 6; agent 40 stands off the road
``inj/s<k>/*`` holds the reference's ``compute_metrics`` on scene k alone, ``inj/batch/*`` its ``compute_coll_rate_env`` on the batch.

run/*: the reference's ``run_one_epoch`` (save on, viz off) on a loader of nine single scenes (RUN_KINDS) with feasibility_NA 2 and
batch_size 20, its module-level ``refine_traffic_optim`` replaced by an injector that returns the ``inj`` trajectories of the
batch's scenes: batch compositions, log lines, the result directory, file name and JSON text of every scene, the final rates.

Tie conditions (asserted here on the reference's values and again in tests/test_refine_driver.py): every IoU more than 1e-3 from
0.02; every drivable fraction more than 2 / (L W) from 0.95; both grid ratios more than 1e-3 from a half-integer.

Usage:  python tests/golden/make_golden_refine_driver.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from strive_amd import synth                                                                  # noqa: E402
from strive_amd.graph import Data, Batch, clique_edge_index                                  # noqa: E402
from strive_amd.constants import state_norm_tensors, att_norm_tensors                        # noqa: E402

FIX = 'g22_refine_driver.npz'
DT, PT, T = 0.5, 4, 12
IOU_THRESH, TIE_MARGIN = 0.02, 1e-3
SIZES, MAPIX = [1, 2, 5, 19, 65], [0, 1, 0, 0, 0]
TRUCK_KINDS = (0, 2)
TRUCK_LW = (8.0, 2.5)
CAR_LW = [(3.25, 1.75), (3.5, 1.75), (3.0, 1.75), (3.25, 1.875), (3.25, 1.625)]
OWN_GRID = {0: (32, 10), 1: (13, 7), 2: (32, 10), 3: (13, 7), 4: (13, 7)}
BATCH_GRID = (14, 7)
FLIP = (2, 4)                                                 # (kind, agent) whose environment flag depends on whose grid is used
RUN_KINDS = [2, 0, 3, 1, 1, 4, 0, 2, 0]
RUN_FEASIBILITY, RUN_BATCH_SIZE = 2, 20
RUN_BATCHES = [[0, 2], [3, 4, 5], [7]]


# ------------------------------------------------------------------------------------------------
# inputs (no reference needed)
# ------------------------------------------------------------------------------------------------

def _lanes(kind):
    """World-frame states (n, PT + T, 6) and sizes (n, 2) of a scene: every agent straight along x in its own lane."""
    n = SIZES[kind]
    steps = np.arange(PT + T) - (PT - 1)                       # 0 at the last past step
    st = np.zeros((n, PT + T, 6))
    for a in range(n):
        d = 1.0 if a % 2 == 0 else -1.0
        v = 2.0 + 0.5 * (a % 5)
        st[a, :, 0] = 30.0 + 70.0 * ((a // 4) % 3) + (24.0 if d < 0 else 0.0) + d * v * DT * steps
        st[a, :, 1] = 40.0 * ((a // 12) % 6) + 3.0 + 4.0 * (a % 4)
        st[a, :, 2], st[a, :, 4] = d, v
    lw = np.asarray([TRUCK_LW if kind in TRUCK_KINDS else CAR_LW[(a + kind) % len(CAR_LW)] for a in range(n)])
    return st, lw


def world_traj(kind):
    """(n, T, 4) world-frame final trajectories of a scene, float64."""
    st, _ = _lanes(kind)
    tr = st[:, PT:, :4].copy()
    t = np.arange(T)

    def along_x(a, x0, y0, v=2.0):
        tr[a, :, 0], tr[a, :, 1], tr[a, :, 2], tr[a, :, 3] = x0 + v * DT * t, y0, 1.0, 0.0

    def stand(a, x, y, hx=1.0, hy=0.0):
        tr[a, :, 0], tr[a, :, 1], tr[a, :, 2], tr[a, :, 3] = x, y, hx, hy
    if kind == 1:
        stand(1, 145.0, 100.0)
        tr[0, 3:5] = np.nan
    if kind == 2:
        along_x(1, 40.0, 84.0, v=6.0)
        along_x(3, 40.0, 89.0, v=6.0)
        tr[3, T - 1, 1] = 85.5
        # the road band y in [80, 98) ends, in pixels rounded to nearest, at y = 97.875: the truck's front lies 0.2 m beyond
        stand(4, 100.0, 97.875 + 0.2 - 0.5 * TRUCK_LW[0], 0.0, 1.0)
    if kind == 3:
        along_x(5, 60.0, 129.0)
        along_x(9, 61.0, 129.5)
        along_x(12, 59.0, 128.5)
        tr[14] = np.nan
        tr[7, 5:] = np.nan
        stand(16, 145.0, 110.0)
    if kind == 4:
        along_x(30, 220.0, 169.0)
        along_x(50, 220.5, 175.0)
        tr[50, 6:, 1] = 169.5
        stand(40, 225.0, 110.0)
    return tr


def scene_data(kind):
    st, lw = _lanes(kind)
    n = st.shape[0]
    smean, sstd = state_norm_tensors()
    amean, astd = att_norm_tensors()
    state_t = (synth.f32(st) - smean) / sstd
    sem = np.zeros((n, 2))
    sem[:, 1 if kind in TRUCK_KINDS else 0] = 1.0
    fut = state_t[:, PT:PT + T].contiguous()
    return Data(x=torch.empty((n,)), pos=torch.empty((n,)), edge_index=clique_edge_index(n), past=state_t[:, :PT].contiguous(),
                past_gt=state_t[:, :PT].clone(), sem=synth.f32(sem), lw=(synth.f32(lw) - amean) / astd, past_vis=torch.ones((n, PT)),
                future=fut, future_gt=fut.clone(), future_vis=torch.ones((n, T)))


def inj_traj(kind):
    """(n, 1, T, 4) NORMALISED fp32: what the injected ``refine_traffic_optim`` returns as the scene's final trajectories."""
    smean, sstd = state_norm_tensors()
    return ((synth.f32(world_traj(kind)) - smean[:4]) / sstd[:4]).unsqueeze(1).contiguous()


def inj_case(kinds=None):
    """(batch, map_idx (B) long, final_result_traj (NA,1,T,4)) of the scenes ``kinds`` (default: all five)."""
    kinds = list(range(len(SIZES))) if kinds is None else list(kinds)
    batch = Batch.from_data_list([scene_data(k) for k in kinds])
    return batch, torch.tensor([MAPIX[k] for k in kinds], dtype=torch.long), torch.cat([inj_traj(k) for k in kinds], dim=0)


def inj_raster():
    return synth.make_raster(1024, 1024, M=2)


class _Dataset(object):
    dt = DT


class RunLoader(list):
    """The nine single scenes of run/*, as a batch-size-1 loader yields them."""
    dataset = _Dataset()

    def __init__(self):
        super().__init__((Batch.from_data_list([scene_data(k)]), torch.tensor([MAPIX[k]], dtype=torch.long)) for k in RUN_KINDS)


def injected_refine(scene_graph, map_idx, map_env, model, loss_weights, num_iters, samp_future_len, save_future_len, optim_use_adam, lr):
    """Stands in for ``refine_traffic_optim``: the scenes of the batch are recognised by their agent counts."""
    sizes = np.diff(np.asarray(scene_graph.ptr.cpu())).tolist()
    dev = scene_graph.past.device
    final = torch.cat([inj_traj(SIZES.index(n)) for n in sizes], dim=0).to(dev)
    NA = final.shape[0]
    prior = (torch.zeros((NA, 4), device=dev), torch.ones((NA, 4), device=dev))
    return scene_graph.future_gt[:, :, :4].clone(), torch.zeros((NA, 4), device=dev), final, {'prior_out': prior}


# ------------------------------------------------------------------------------------------------
# the reference's run
# ------------------------------------------------------------------------------------------------

class _StubModel(object):
    def __init__(self, nrm, att):
        self.nrm, self.att = nrm, att

    def get_normalizer(self):
        return self.nrm

    def get_att_normalizer(self):
        return self.att

    def parameters(self):
        return []


def import_refine():
    import importlib
    import make_golden_traffic_eval as G19
    R = G19.import_test_traffic()
    R.G19 = G19
    R.refine = importlib.import_module('refine_traffic_optim')

    class Recorder(G19._Recorder):
        """G19's recorder with a Polygon that takes NaN corners: ``check_pairwise_veh_coll`` builds polygons of NaN frames too (the
        exact stand-in works on rationals).  Their intersection and union areas are NaN, the IoU is NaN and the reference's
        ``cur_iou > VEH_COLL_THRESH`` is False: no hit.  Such IoUs are recorded as NaN."""

        def __init__(self, R_):
            super().__init__(R_)
            rec, base = self, self.Polygon

            class _Area(object):
                area = float('nan')

            class Polygon(base):
                def __init__(self, corners):
                    self.nan = bool(np.isnan(np.asarray(corners, dtype=np.float64)).any())
                    if not self.nan:
                        base.__init__(self, corners)

                def intersection(self, other):
                    return _Area() if self.nan or other.nan else base.intersection(self, other)

                def union(self, other):
                    if self.nan or other.nan:
                        rec.ious.append(float('nan'))
                        return _Area()
                    return base.union(self, other)
            self.Polygon = Polygon
    R.Recorder = Recorder
    return R


def tie_ok(R, ious, layers):
    return R.G19.tie_ok(ious[~np.isnan(ious)], layers)


def g22_inj(R, out):
    G19, M = R.G19, R.refine
    model = _StubModel(R.dutils.MeanStdNormalizer(*state_norm_tensors()), R.dutils.MeanStdNormalizer(*att_norm_tensors()))
    raster, dx = inj_raster()
    env = R.mg.ref_map_env(R, raster, dx)
    flags = {}
    orig = (M.check_pairwise_veh_coll, M.compute_coll_rate_env)
    seen = {}

    def veh(*a, **k):
        seen['veh'] = orig[0](*a, **k)
        return seen['veh']

    def envf(*a, **k):
        seen['env'] = orig[1](*a, **k)
        return seen['env']
    M.check_pairwise_veh_coll, M.compute_coll_rate_env = veh, envf
    try:
        for kind in range(len(SIZES)):
            batch, map_idx, traj = inj_case([kind])
            p = 'inj/s%d/' % kind
            n = SIZES[kind]
            with R.Recorder(R) as rec:
                z = torch.zeros((n, 4))
                res = M.compute_metrics({}, {}, {}, z, traj.clone(), model, batch, env, map_idx, (z, z + 1.0))
                ious, layers = rec.take()
            metrics, cnt, tot, seq = res
            assert metrics == {} and len(layers) <= 1
            out[p + 'seq_metrics'] = np.asarray([seq['veh_coll'], seq['env_coll']], dtype=np.int64)
            out[p + 'freq_cnt'] = np.asarray([cnt['veh_coll'], cnt['env_coll']], dtype=np.int64)
            out[p + 'freq_total'] = np.asarray([tot['veh_coll'], tot['env_coll']], dtype=np.int64)
            out[p + 'did_veh'] = np.asarray(seen['veh']['did_collide']).astype(np.uint8)
            out[p + 'did_env'] = seen['env']['did_collide'].numpy()[:, 0].astype(np.uint8)
            out[p + 'iou'] = ious.astype(np.float64)
            ok, why = tie_ok(R, ious, layers)
            assert ok, 'tie condition: %s in inj/s%d' % (why, kind)
            assert len(layers) == 1
            G19._store_layer(out, p, layers[0])
            assert (int(out[p + 'L']), int(out[p + 'W'])) == OWN_GRID[kind], (kind, out[p + 'L'], out[p + 'W'])
            flags[kind] = (out[p + 'did_veh'].astype(bool), out[p + 'did_env'].astype(bool))
            print('inj/s%d n %2d  veh %d  env %d  L %d W %d  IoUs formed %d' % (kind, n, seq['veh_coll'], seq['env_coll'], out[p + 'L'],
                                                                               out[p + 'W'], ious.size))
        # one reference call on the whole batch: the grid it forms is not the scenes' own
        batch, map_idx, traj = inj_case()
        with R.Recorder(R) as rec:
            ce = orig[1](batch, map_idx, traj.clone(), env, model.get_normalizer(), model.get_att_normalizer(), ego_only=False)
            _, layers = rec.take()
        ok, why = tie_ok(R, np.zeros((0,)), layers)
        assert ok, 'tie condition: %s in inj/batch' % why
        G19._store_layer(out, 'inj/batch/', layers[0])
        out['inj/batch/did_env'] = ce['did_collide'].numpy()[:, 0].astype(np.uint8)
        assert (int(out['inj/batch/L']), int(out['inj/batch/W'])) == BATCH_GRID
    finally:
        M.check_pairwise_veh_coll, M.compute_coll_rate_env = orig
    check_cases(flags, out['inj/batch/did_env'].astype(bool), batch.ptr.numpy())


def check_cases(flags, batch_env, ptr):
    """The properties the injected scenes exist for, from the reference's outputs."""
    veh, env = flags[0]
    assert not veh.any() and not env.any(), 'one truck on its lane'
    veh, env = flags[1]
    assert not veh.any() and not env.any(), 'agent 1 of kind 1 is on the road of map 1; NaN frames are no collision'
    veh, env = flags[2]
    assert veh.tolist() == [False, True, False, False, False], 'the pair (1, 3) overlaps at the last step only, charged to agent 1'
    assert not env.any(), 'the truck across the band edge is on the road under its scene\'s grid'
    veh, env = flags[3]
    assert [i for i in range(19) if veh[i]] == [5, 9], 'agent 5 overlaps two later agents (once), agent 12 only earlier ones'
    assert [i for i in range(19) if env[i]] == [16], 'agent 16 stands off the road; the all-NaN agent 14 does not collide'
    veh, env = flags[4]
    assert [i for i in range(65) if veh[i]] == [30] and [i for i in range(65) if env[i]] == [40]
    own = np.concatenate([flags[k][1] for k in range(len(SIZES))])
    diff = np.nonzero(own != batch_env)[0].tolist()
    assert diff == [int(ptr[FLIP[0]]) + FLIP[1]] and batch_env[diff[0]], 'the whole-batch grid flips exactly the truck of kind 2: %s' % diff


def g22_run(R, out):
    M = R.refine
    model = _StubModel(R.dutils.MeanStdNormalizer(*state_norm_tensors()), R.dutils.MeanStdNormalizer(*att_norm_tensors()))
    raster, dx = inj_raster()
    env = R.mg.ref_map_env(R, raster, dx)
    lines, comps = [], []
    orig = (M.refine_traffic_optim, R.logger.Logger.log, M.tqdm.tqdm)

    def refine(scene_graph, *a, **k):
        comps.append(np.diff(scene_graph.ptr.numpy()).tolist())
        return injected_refine(scene_graph, *a, **k)
    with tempfile.TemporaryDirectory() as tmp:
        M.refine_traffic_optim = refine
        R.logger.Logger.log = staticmethod(lambda s: lines.append(s.replace(tmp, 'OUT')) if isinstance(s, str) else None)
        M.tqdm.tqdm = lambda it: it
        try:
            with R.Recorder(R) as rec, contextlib.redirect_stdout(io.StringIO()):
                M.run_one_epoch(RunLoader(), RUN_BATCH_SIZE, model, env, torch.device('cpu'), tmp, {}, feasibility_NA=RUN_FEASIBILITY,
                                samp_future_len=T, save_future_len=T, optim_use_adam=True, num_iters=1, lr=0.05, viz=False, save=True)
                ious, layers = rec.take()
        finally:
            M.refine_traffic_optim, M.tqdm.tqdm = orig[0], orig[2]
            R.logger.Logger.log = staticmethod(orig[1])
        ok, why = tie_ok(R, ious, layers)
        assert ok, 'tie condition: %s in run/*' % why
        files = []
        for d in ('success', 'failed'):
            folder = os.path.join(tmp, 'scenario_results', d)
            for fn in sorted(os.listdir(folder)) if os.path.isdir(folder) else []:
                with open(os.path.join(folder, fn)) as f:
                    files.append((d, fn, f.read()))
    assert [[SIZES[RUN_KINDS[i]] for i in b] for b in RUN_BATCHES] == comps, comps
    saved = sorted(i for b in RUN_BATCHES for i in b)
    assert sorted(int(fn[6:10]) for _, fn, _ in files) == saved
    assert {d for d, _, _ in files} == {'success', 'failed'}
    for _, _, text in files:
        json.loads(text)
    out['run/batches'] = np.asarray(json.dumps(RUN_BATCHES))
    out['run/lines'] = np.asarray(lines)
    out['run/dirs'] = np.asarray([d for d, _, _ in files])
    out['run/files'] = np.asarray([fn for _, fn, _ in files])
    out['run/json'] = np.asarray([text for _, _, text in files])
    rates = [ln for ln in lines if ln.startswith(('veh_coll = ', 'env_coll = '))]
    assert len(rates) == 2 and lines[-2:] == rates
    out['run/rates_text'] = np.asarray(rates)
    print('\n'.join(ln for ln in lines if not ln.startswith('Optimized')))


def main():
    torch.set_num_threads(8)
    R = import_refine()
    out = {}
    g22_inj(R, out)
    g22_run(R, out)
    R.G19.save_deterministic(FIX, out)


if __name__ == '__main__':
    main()
