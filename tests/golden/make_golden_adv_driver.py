#!/usr/bin/env python3
"""Generate tests/golden/g23_adv_driver.npz: the reference's per-scene screening and ego verdicts (src/utils/scenario_gen.py
``determine_feasibility_nusc``, src/datasets/nuscenes_utils.py ``check_line_layer``, src/utils/adv_gen_optim.py
``compute_adv_gen_success``, src/utils/sol_optim.py ``compute_sol_success``), run by the reference itself in the build container.
Only outputs are stored; the inputs are rebuilt by the builders of tests/test_adv_driver.py (``screen_scene``, ``ego_scene``,
``two_line_lengths``, ``near_pair``, ``FEAS_CASES``, ``EGO_CASES``), which import without the reference.  It uses make_golden's import
stand-ins and the exact shapely stand-in, and adds ``tqdm`` and ``np.bool``, which src/adv_scenario_gen.py still uses.  The file is
described in tests/golden/README_g23.md.

feas/s<k>/<params>/*: ``determine_feasibility_nusc`` on scene k of ``FEAS_CASES`` ALONE over ``synth.make_raster(M=2)``, for every
entry of the tests' ``PARAMS``: ``feasible``, ``step``, ``dist`` (fp32, as returned), what its one ``check_line_layer`` call was
handed and gave (``sep_n``, the per-line count of samples on a 0 pixel, ``ratio`` = |agent - ego| / mean(dx) per line), ``max_vel``
and every cosine it formed, and the two ego speeds of src/adv_scenario_gen.py:176-195.
feas/joint/*: ONE ``check_line_layer`` call on the lines of the two scenes of ``two_line_lengths`` together.
ego/s<k>/*: ``check_single_veh_coll`` (through both success functions) on scene k of ``EGO_CASES`` alone: the flags, the collision
steps, both verdicts, every IoU formed, the ego's drivable fraction and its grid.
run/<planner>/*: src/adv_scenario_gen.py ``run_one_epoch`` (save on, viz off) on the tests' ``RunLoader(planner)`` with the five stages
replaced by the tests' injectors: batch compositions, logged lines, and the directory, file name and JSON text of every scene.

Tie conditions (asserted here on the reference's values and again in tests/test_adv_driver.py): see README_g23.md.

Usage:  python tests/golden/make_golden_adv_driver.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_adv_driver as T                                                                  # noqa: E402  (the builders)

FIX = 'g23_adv_driver.npz'
MARGIN = 1e-3


def import_adv():
    import make_golden_refine_driver as G22
    if not hasattr(np, 'bool'):
        np.bool = bool                                        # src/adv_scenario_gen.py:323
    if 'tqdm' not in sys.modules:
        tq = types.ModuleType('tqdm')
        tq.tqdm = lambda it, *a, **k: it
        sys.modules['tqdm'] = tq
    R = G22.import_refine()
    R.scen = importlib.import_module('utils.scenario_gen')
    R.adv = importlib.import_module('utils.adv_gen_optim')
    R.sol = importlib.import_module('utils.sol_optim')
    R.advloss = importlib.import_module('losses.adv_gen_nusc')
    return R


def ref_env(R):
    raster, dx = T.maps()
    return R.mg.ref_map_env(R, raster, dx)


def half_margin(x):
    return float(np.abs(x - np.floor(x) - 0.5).min()) if np.size(x) else 1.0


def rel_margin(x, thr):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)]
    return float((np.abs(x - thr) / max(abs(thr), 1e-30)).min()) if x.size and thr != 0 else 1.0


def g23_feas(R, out):
    nrm = R.dutils.MeanStdNormalizer(*T.state_norm_tensors())
    env = ref_env(R)
    seen = {}
    orig_line, orig_sum = R.nutils.check_line_layer, torch.sum

    def line(drivables, dx, start, end, mapixes):
        """The reference's call, and what it was handed; the per-line counts are taken from its own ``torch.sum``."""
        ln = torch.norm(start - end, dim=-1).double() / torch.mean(dx).double()
        seen['ratio'] = ln.numpy().copy()
        sums = []

        def rec_sum(x, *a, **k):
            r = orig_sum(x, *a, **k)
            if x.dtype == torch.bool:
                sums.append(r)
            return r
        torch.sum = rec_sum
        try:
            res = orig_line(drivables, dx, start, end, mapixes)
        finally:
            torch.sum = orig_sum
        seen['sep_zero'] = sums[-1].numpy().astype(np.int64)
        seen['sep_n'] = int(torch.max(torch.round(torch.norm(start - end, dim=-1) / torch.mean(dx)).int()).item())
        seen['blocked'] = res.numpy().copy()
        return res
    R.nutils.check_line_layer = line
    R.scen.nutils.check_line_layer = line
    try:
        for k, (smp, gt, m) in enumerate(T.FEAS_CASES()):
            n, NS, FT = int(smp.shape[0]), int(smp.shape[1]), int(smp.shape[2])
            for name in sorted(T.PARAMS):
                p = T.params(name, FT)
                seen.clear()
                pre = 'feas/s%d/%s/' % (k, name)
                feas, step, dist = R.scen.determine_feasibility_nusc(smp.clone(), nrm, p['thresh'], p['t0'], p['agent_vel'], p['infront_min'],
                                                                     p['check_sep'], env, torch.tensor([m]))
                # the two ego-speed rules, as src/adv_scenario_gen.py:176-195 forms them
                ego_gt = nrm.unnormalize(gt[0])
                gv = torch.max(torch.norm(ego_gt[1:, :2] - ego_gt[:-1, :2], dim=-1)).item() if gt.shape[1] > 1 else float('nan')
                ego_s = nrm.unnormalize(smp[0])
                ev = torch.max(torch.norm(ego_s[:, 1:, :2] - ego_s[:, :-1, :2], dim=-1)).item() if FT > 1 else float('nan')
                out[pre + 'ego_vel'] = np.asarray([ev, gv], dtype=np.float64)
                out[pre + 'none'] = np.asarray(feas is None)
                for v, thr in ((ev, p['ego_vel']), (gv, p['ego_vel'])):
                    assert not np.isfinite(v) or thr == 0 or abs(v - thr) / thr > MARGIN, (k, name, 'ego speed at its threshold')
                if feas is None:
                    assert n == 1
                    continue
                out[pre + 'feasible'] = feas.numpy().astype(np.uint8)
                out[pre + 'step'] = step.numpy().astype(np.int64)
                out[pre + 'dist'] = dist.numpy().astype(np.float32)
                u = nrm.unnormalize(smp)
                raw = torch.norm(u[0:1, :, p['t0']:, :2] - u[1:, :, p['t0']:, :2], dim=-1)
                d = raw
                if p['infront_min'] is not None:
                    e2a = u[1:, :, p['t0']:, :2] - u[0:1, :, p['t0']:, :2]
                    cos = torch.sum(e2a / torch.norm(e2a, dim=-1, keepdim=True) * u[0:1, :, p['t0']:, 2:4], dim=-1)
                    # the cosines that decide an agent's closest approach: of the (sample, step) no further away, before the mask,
                    # than the closest approach plus 1e-3 of it (all of them for an agent that is masked throughout)
                    decides = ~torch.isnan(cos) & (raw <= (dist * (1.0 + MARGIN)).view(-1, 1, 1))
                    assert not decides.any() or float((cos[decides] - p['infront_min']).abs().min()) > MARGIN, (k, name, 'cosine')
                    d = torch.where(cos >= p['infront_min'], raw, torch.full_like(raw, float('inf')))
                # every agent's closest approach decides ``some dist < thresh``
                assert rel_margin(dist.numpy(), p['thresh']) > MARGIN, (k, name, 'a closest approach at the threshold')
                # unique minima but for exact duplicates: the runner-up among the values that differ from the minimum
                # where a minimum was taken (over the steps; over the samples of the chosen step)
                dn = d.double().numpy()
                for a in range(n - 1):
                    for v in (dn[a].min(axis=0), dn[a][:, int(step[a]) - p['t0']]):
                        v = np.unique(v[np.isfinite(v)])
                        assert v.size < 2 or (v[1] - v[0]) / v[1] > 1e-5, (k, name, a, 'a near tie of minima')
                if FT > 1:
                    vel = torch.norm(u[1:, :, 1:, :2] - u[1:, :, :-1, :2], dim=-1).amax(dim=(1, 2))
                    out[pre + 'max_vel'] = vel.numpy().astype(np.float32)
                    assert p['agent_vel'] == 0 or rel_margin(vel.numpy(), p['agent_vel']) > MARGIN, (k, name, 'a speed at the threshold')
                if p['check_sep']:
                    out[pre + 'sep_zero'] = seen['sep_zero']
                    out[pre + 'sep_n'] = np.asarray(seen['sep_n'], dtype=np.int64)
                    out[pre + 'ratio'] = seen['ratio']
                    q = seen['ratio']                          # sep_n is the maximum: the lines within one sample of the longest decide it
                    assert half_margin(q[q >= q.max() - 1.0]) > MARGIN, (k, name, 'a line length at a half-integer')
                    assert np.array_equal(seen['blocked'], seen['sep_zero'] > 0)
                print('%-22s n %3d NS %2d  feasible %3d  sep_n %s' % (pre, n, NS, int(feas.sum()), seen.get('sep_n')))
        # the two scenes whose own sep_n differ: ONE check_line_layer call on both, which the reference never makes
        short, long_ = T.two_line_lengths()
        u = nrm.unnormalize(torch.cat([short[0], long_[0]]))
        seen.clear()
        line(env.nusc_raster[:, 0], env.nusc_dx, u[[1, 3], 0, 0, :2], u[[0, 2], 0, 0, :2], torch.tensor([0, 0]))
        out['feas/joint/blocked'] = seen['blocked'].astype(np.uint8)
        out['feas/joint/sep_n'] = np.asarray(seen['sep_n'], dtype=np.int64)
        assert seen['blocked'].tolist() == [True, False], 'the thin strip is hit at the long scene\'s sep_n'
    finally:
        R.nutils.check_line_layer = orig_line
        R.scen.nutils.check_line_layer = orig_line
        torch.sum = orig_sum


def g23_ego(R, out):
    model = types.SimpleNamespace(get_normalizer=lambda: nrm, get_att_normalizer=lambda: att)
    nrm, att = R.dutils.MeanStdNormalizer(*T.state_norm_tensors()), R.dutils.MeanStdNormalizer(*T.att_norm_tensors())
    env = ref_env(R)
    seen = {}
    orig = R.advloss.check_single_veh_coll

    def single(*a, **k):
        seen['coll'] = orig(*a, **k)
        return seen['coll']
    R.advloss.check_single_veh_coll = single
    try:
        for k, (traj, lw, atk, m) in enumerate(T.EGO_CASES()):
            n, Tn = int(traj.shape[0]), int(traj.shape[2])
            pre = 'ego/s%d/' % k
            g = T._Graph([0, n], lw=lw)
            with R.Recorder(R) as rec:
                adv = None if atk is None else bool(R.adv.compute_adv_gen_success(traj.clone(), model, g, atk))
                ious_adv, _ = rec.take()
                sol = bool(R.sol.compute_sol_success(traj.clone(), model, g, env, torch.tensor([m])))
                ious, layers = rec.take()
            hit, coll_t = seen['coll']
            out[pre + 'hit'] = np.asarray(hit).astype(np.uint8).reshape(-1)
            out[pre + 'coll_t'] = np.asarray(coll_t).astype(np.int64).reshape(-1)
            out[pre + 'adv'] = np.asarray(-1 if adv is None else int(adv), dtype=np.int64)
            out[pre + 'sol'] = np.asarray(int(sol), dtype=np.int64)
            out[pre + 'iou'] = ious.astype(np.float64)
            assert atk is None or np.array_equal(ious_adv, ious, equal_nan=True)
            ok, why = R.G19.tie_ok(ious[~np.isnan(ious)], layers)
            assert ok, 'tie condition: %s in %s' % (why, pre)
            assert len(layers) == 1
            R.G19._store_layer(out, pre, layers[0])
            print('%-10s n %3d T %2d  hits %3d  adv %s  sol %s  L %d W %d  IoUs %d' % (pre, n, Tn, int(np.sum(hit)), adv, sol, out[pre + 'L'],
                                                                                      out[pre + 'W'], ious.size))
    finally:
        R.advloss.check_single_veh_coll = orig


RUN_BATCHES = {'ego': [[0, 2], [6, 7], [8, 9], [11]], 'hardcode': [[0, 2], [6, 7], [8, 9], [11]]}
RUN_DIRS = {'ego': {0: 'adv_sol_success', 2: 'adv_failed', 6: 'adv_sol_success', 7: 'sol_failed', 8: 'adv_sol_success', 9: 'sol_failed',
                    11: 'adv_sol_success'},
            'hardcode': {0: 'adv_sol_success', 2: 'adv_failed', 6: 'adv_sol_success', 8: 'adv_sol_success', 9: 'sol_failed',
                         11: 'adv_sol_success'}}


def g23_run(R, out, planner_name):
    """The reference's ``run_one_epoch`` (save on, viz off) on ``RunLoader(planner_name)`` with the five stages replaced by the tests'
    injectors.  What ``Logger.log`` was handed is kept as text (a list or a dict through ``str``); the scene graphs it is handed are
    dropped, and so is the timing line."""
    import contextlib
    import io
    import json
    import tempfile
    M = importlib.import_module('adv_scenario_gen')
    planners = importlib.import_module('planners.hardcode_goalcond_nusc')
    Bt = T.AG.FeasibilityBatcher

    class Model(T.InjModel):
        def __init__(self):
            self.nrm = R.dutils.MeanStdNormalizer(*T.state_norm_tensors())
            self.att = R.dutils.MeanStdNormalizer(*T.att_norm_tensors())
            self.normalizer = self.nrm

        sample_batched = staticmethod(T.inj_sample)
    raster, dx = T.maps()
    env = R.mg.ref_map_env(R, raster, dx)
    lines, comps = [], []

    def log(s):
        if isinstance(s, (str, list, dict)):
            lines.append(str(s))

    def adv(cur_z, lr, weights, model_, scene_graph, *a, **k):
        comps.append(np.diff(scene_graph.ptr.numpy()).tolist())
        return T.inj_adv(cur_z, lr, weights, model_, scene_graph, *a, **k)
    orig = (M.run_init_optim, M.run_adv_gen_optim, M.run_find_solution_optim, planners.HardcodeNuscPlanner, R.logger.Logger.log,
            M.compute_coll_rate_env, M.tqdm.tqdm)
    loader = T.RunLoader(planner_name)
    with tempfile.TemporaryDirectory() as tmp:
        M.run_init_optim, M.run_adv_gen_optim, M.run_find_solution_optim = T.inj_init, adv, T.inj_sol
        planners.HardcodeNuscPlanner = T.InjPlanner
        R.logger.Logger.log = staticmethod(log)
        M.tqdm.tqdm = lambda it: it
        try:
            with R.Recorder(R) as rec, contextlib.redirect_stdout(io.StringIO()):
                def init_coll_env(*a, **k):
                    """:360, ``init_coll_env``: computed for the rendering alone, so its fractions decide nothing and are not kept."""
                    res = orig[5](*a, **k)
                    rec.layers.pop()
                    return res
                M.compute_coll_rate_env = init_coll_env
                M.run_one_epoch(loader, T.RUN_BATCH_SIZE, Model(), env, torch.device('cpu'), tmp, {}, planner_name=planner_name, viz=False,
                                save=True, **T.RUN_ARGS)
                ious, layers = rec.take()
        finally:
            M.run_init_optim, M.run_adv_gen_optim, M.run_find_solution_optim, planners.HardcodeNuscPlanner = orig[:4]
            R.logger.Logger.log = staticmethod(orig[4])
            M.compute_coll_rate_env, M.tqdm.tqdm = orig[5], orig[6]
        ok, why = R.G19.tie_ok(ious[~np.isnan(ious)], layers)
        assert ok, 'tie condition: %s in run/%s' % (why, planner_name)
        files = []
        for d in T.AG.RESULT_DIRS:
            folder = os.path.join(tmp, 'scenario_results', d)
            for fn in sorted(os.listdir(folder)) if os.path.isdir(folder) else []:
                with open(os.path.join(folder, fn)) as f:
                    files.append((d, fn, f.read()))
        lines = T.run_lines(lines, tmp)
    print('\n'.join(ln if len(ln) < 150 else ln[:150] + ' ...' for ln in lines))
    kinds = T.RUN_KINDS[planner_name]
    sizes = [1 + len(T.RUN_SCENES[k][1]) for k in kinds]
    want = [[sizes[i] for i in b] for b in RUN_BATCHES[planner_name]]
    if planner_name == 'hardcode':
        want[1] = [sizes[6]]                                  # the parked car stands where the planner drives: scene 7 is removed
    assert comps == want, comps
    assert {int(fn[6:10]): d for d, fn, _ in files} == RUN_DIRS[planner_name], [(d, fn) for d, fn, _ in files]
    for _, _, text in files:
        json.loads(text)
    # the events the loaders exist for
    for line in (Bt.SLOW[planner_name], Bt.ONLY_EGO, Bt.NONE_NEAR, Bt.NO_CATEGORY, Bt.FEASIBLE, Bt.FORMED):
        assert line in lines, line
    assert lines.count(Bt.NO_CATEGORY) == 1 and lines.count(Bt.FORMED) == 4
    removed = 'Planner already caused collision after init, removing from batch...'
    assert lines.count(removed) == (1 if planner_name == 'hardcode' else 0)
    tail = [ln for ln in lines if ln in (Bt.SLOW[planner_name], Bt.NONE_NEAR, Bt.FEASIBLE, Bt.FORMED)]
    if planner_name == 'ego':
        assert tail[-2:] == [Bt.NONE_NEAR, Bt.FORMED], 'the last scene is skipped and flushes the queue'
    else:
        assert tail[-3:] == [Bt.SLOW[planner_name], Bt.FEASIBLE, Bt.FORMED], '(sic) the slow last scene is queued'
    p = 'run/%s/' % planner_name
    out[p + 'batches'] = np.asarray(json.dumps(comps))
    out[p + 'lines'] = np.asarray(lines)
    out[p + 'dirs'] = np.asarray([d for d, _, _ in files])
    out[p + 'files'] = np.asarray([fn for _, fn, _ in files])
    out[p + 'json'] = np.asarray([text for _, _, text in files])


def main():
    torch.set_num_threads(8)
    R = import_adv()
    out = {}
    g23_feas(R, out)
    g23_ego(R, out)
    for planner_name in ('ego', 'hardcode'):
        g23_run(R, out, planner_name)
    R.G19.save_deterministic(FIX, out)


if __name__ == '__main__':
    main()
