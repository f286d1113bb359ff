"""The adv_scenario_gen driver (reference src/adv_scenario_gen.py:33-122, :108-548): the walk over the scene dataset of a tracks file,
every scene screened for a feasible attacker, batches of about ``batch_size`` agents, the three optimisation stages, the verdicts
and the scenario files.  What the reference does once per scene on the host is done once per batch on the device:

* ``screen_batch``: ``determine_feasibility_nusc`` (reference src/utils/scenario_gen.py:30-107) and the two ego-speed rules of
  reference src/adv_scenario_gen.py:176-195 for every scene of a batch of samples, each scene as if screened alone: ONE
  ``strive_feasibility_screen`` call, nothing read back.
* ``ego_verdicts``: ``check_single_veh_coll`` of the ego against the other agents of its scene, with what
  ``compute_adv_gen_success`` and ``compute_sol_success`` read from it (the attacker's flag, any hit, the ego's drivable test), for
  every scene of a batch: ONE ``strive_ego_verdicts`` call, nothing read back.
* ``FeasibilityBatcher``: the reference's queue of feasible scenes (:176-256) as a host state machine over the screening's integers:
  its log lines, its batches of about ``batch_size`` agents, and its treatment of the loader's last scene.
* ``run_one_epoch`` and the command line: the reference's program around them,

    python -m strive_amd.adv_scenario_gen_tracks --ckpt CKPT --tracks FILE [--scenario_path DIR] --out OUT [--config FILE]
        [--planner ego|hardcode] [--save]

  writes ``OUT/adv_gen_log.txt`` and, with ``--save``, ``OUT/scenario_results/{adv_failed,sol_failed,adv_sol_success}/scene_%04d.json``,
  the files ``eval_adv_gen``, ``cluster_scenarios``, ``eval_planner`` and the dataset's ``scenario_path`` read.  The arguments are the
  reference's, with its defaults, plus ``--tracks`` / ``--scenario_path``, ``--seed``, ``--device``, ``--screen_agents`` and
  ``--on_planner_error``.  ``OUT`` is used as given: the reference appends ``_<unix time>`` to it.  With ``--planner hardcode`` the map
  environment carries ``synth.make_lane_graph()`` (the reference's ``load_lanegraph``), or, with ``--maps FILE``, the lane graphs of
  that maps file, built on the device (datasets/maps.py).  Not offered: rendering (``--viz``), wandb,
  several ranks, and ``init_coll_env``, which the reference computes for its rendering alone.
"""
import json
import os
import time

import numpy as np
import torch

from . import _lib as L
from . import ops
from .eval_common import LIN_MAX, check_status, i32, lin_table, model_stats, outputs, pack_env, traj_arg
from .graph import Batch
from .refine_traffic_tracks import NO_RENDERING, SceneSource, _log, scene_source
from .train_traffic import DEVKIT_KEYS

SCREEN_I = ('n_others', 'n_within', 'n_feasible_any_category', 'n_feasible', 'heur_agt', 'heur_t', 'sep_n', 'verdict')
SCREEN_D = ('ego_vel_samples', 'ego_vel_gt', 'heur_dist')
EGO_I = ('n_others', 'n_hit', 'atk_hit', 'first_t', 'ego_env', 'L', 'W', 'rows')
VERDICT_FEASIBLE, VERDICT_EGO_SLOW, VERDICT_EGO_ONLY, VERDICT_NONE_NEAR, VERDICT_NO_CATEGORY = 0, 1, 2, 3, 4
PLANNER_RULE = {None: 0, 'ego': 1, 'hardcode': 2}
SCREEN_STATUS_TEXT = {2: 'agent offsets leave the arrays', 3: 'map index out of range', 5: 'a sample is not finite',
                      6: 'a separation line leaves the raster (or has more than 65536 samples)'}
EGO_STATUS_TEXT = {2: 'agent offsets leave the arrays, or the attacker index is outside 1..n-1', 3: 'map index out of range',
                   4: 'the drivable-area sampling grid of the ego is outside 1..%d samples per axis' % LIN_MAX}


def screen_batch(samples, model, scene_graph, map_env, map_idx, feasibility_thresh, feasibility_time=0, feasibility_vel=0.0,
                 feasibility_infront_min=None, check_non_drivable_separation=True, planner_name=None, ego_vel=0.0, allowed=None,
                 out=None, lib=None):
    """Every scene of a batch screened as the reference's loop screens it alone (:166-195): ONE ``strive_feasibility_screen`` call,
    nothing read back.  ``samples`` (NA,NS,FT,4) NORMALISED futures (``sample_pred['future_pred']``), ``scene_graph.ptr`` (B+1),
    ``map_idx`` (B).  The first four parameters after them are ``determine_feasibility_nusc``'s; ``planner_name`` chooses the ego-speed
    rule behind verdict 1 ('ego': ``scene_graph.future_gt``'s ego rows, 'hardcode': the ego's samples, None: no rule) and ``ego_vel`` is
    its threshold (the reference passes its ``feasibility_vel`` there and 0.0 to ``determine_feasibility_nusc``).  ``allowed`` (NA) marks
    the agents of the ``adv_attack_with`` category.  Returns tensors on the samples' device: per agent ``feasible``, ``within``,
    ``step``, ``best_samp``, ``sep_zero`` (NA) int32 and ``dist``, ``max_vel`` (NA) float64 (ego rows keep their fill values); per scene
    ``out_i`` (B,8) int32 in the order of SCREEN_I, ``out_d`` (B,3) float64 in the order of SCREEN_D, ``status`` (B) int32
    (SCREEN_STATUS_TEXT; the outputs of such a scene are untouched)."""
    smp = samples.detach()
    if smp.dim() != 4 or smp.shape[3] != 4:
        raise ValueError('screen_batch expects samples (NA,NS,FT,4)')
    smp = smp.to(torch.float32).contiguous()
    dev = smp.device
    lib = ops._lib_for(smp) if lib is None else lib
    NA, NS, FT = int(smp.shape[0]), int(smp.shape[1]), int(smp.shape[2])
    ptr = i32(scene_graph.ptr, dev)
    B = int(ptr.numel()) - 1
    mapix = i32(map_idx, dev, -1)
    if B < 0 or int(mapix.numel()) != B:
        raise ValueError('screen_batch expects ptr (B+1) and map_idx (B)')
    if planner_name not in PLANNER_RULE:
        raise ValueError("planner_name is 'ego', 'hardcode' or None")
    gt, Tg = None, 0
    if planner_name == 'ego':
        gt = scene_graph.future_gt.detach().to(device=dev, dtype=torch.float32)[..., :4].contiguous()
        if gt.dim() != 3 or int(gt.shape[0]) != NA:
            raise ValueError('screen_batch expects scene_graph.future_gt (NA,Tg,>=4)')
        Tg = int(gt.shape[1])
    alw = None
    if allowed is not None:
        alw = i32(allowed, dev, -1)
        if int(alw.numel()) != NA:
            raise ValueError('screen_batch expects allowed (NA)')
    inf = float('inf')
    out = outputs(out, dev, [('feasible', (NA,), torch.int32, 0), ('within', (NA,), torch.int32, 0), ('step', (NA,), torch.int32, -1),
                              ('best_samp', (NA,), torch.int32, -1), ('sep_zero', (NA,), torch.int32, 0),
                              ('dist', (NA,), torch.float64, inf), ('max_vel', (NA,), torch.float64, float('nan')),
                              ('out_i', (B, len(SCREEN_I)), torch.int32, 0), ('out_d', (B, len(SCREEN_D)), torch.float64, float('nan')),
                              ('status', (B,), torch.int32, 0)])
    if B == 0:
        return out
    if NA == 0:                                        # never hand a NULL pointer to the library
        smp = torch.zeros((1, NS, FT, 4), dtype=torch.float32, device=dev)
    sm, ss, _, _ = model_stats(model)
    use_infront = feasibility_infront_min is not None
    lib.call('strive_feasibility_screen', L.ptr(smp), L.ptr(ptr), L.ptr(mapix), None if alw is None else L.ptr(alw),
             None if gt is None else L.ptr(gt), sm, ss, ops._map_pack(pack_env(map_env), dev).ref(), float(feasibility_thresh),
             int(feasibility_time), float(feasibility_vel), float(ego_vel), int(use_infront),
             float(feasibility_infront_min) if use_infront else 0.0, int(bool(check_non_drivable_separation)),
             PLANNER_RULE[planner_name], B, NA, NS, FT, Tg, L.ptr(out['feasible']), L.ptr(out['within']), L.ptr(out['step']),
             L.ptr(out['best_samp']), L.ptr(out['dist']), L.ptr(out['sep_zero']), L.ptr(out['max_vel']), L.ptr(out['out_i']),
             L.ptr(out['out_d']), L.ptr(out['status']), L.stream_ptr(smp))
    return out


def ego_verdicts(final_result_traj, model, scene_graph, attack_agt=None, map_env=None, map_idx=None, out=None, lib=None,
                 lin_max=LIN_MAX):
    """The ego of every scene of a batch against the other agents of its scene, as ``check_single_veh_coll`` gives it on that scene
    alone: ONE ``strive_ego_verdicts`` call, nothing read back.  ``final_result_traj`` (NA,1,T,4) or (NA,T,4) and ``scene_graph.lw``
    NORMALISED, ``scene_graph.ptr`` (B+1); ``attack_agt`` (B) LOCAL attacker indices (1..n-1, or -1) or None; with ``map_env`` and
    ``map_idx`` (B) the ego's drivable test of ``compute_sol_success`` is made as well.  Returns tensors on the trajectories' device:
    ``hit``, ``coll_t`` (NA) int32 (the ego's row: any hit / the first step of the scene), ``out_i`` (B,8) int32 in the order of EGO_I,
    ``grid_d`` (B,2) float64, ``status`` (B) int32 (EGO_STATUS_TEXT; the outputs of such a scene are untouched).
    ``compute_adv_gen_success`` of scene b is ``out_i[b, 2] == 1``; ``compute_sol_success`` is ``out_i[b, 1] == 0 and out_i[b, 4] == 0``."""
    traj = traj_arg(final_result_traj, 'ego_verdicts')
    dev = traj.device
    lib = ops._lib_for(traj) if lib is None else lib
    NA, T = int(traj.shape[0]), int(traj.shape[1])
    ptr = i32(scene_graph.ptr, dev)
    B = int(ptr.numel()) - 1
    want_env = map_env is not None
    mapix = i32(map_idx, dev, -1) if want_env else None
    atk = i32(attack_agt, dev, -1) if attack_agt is not None else None
    if B < 0 or T < 1 or (want_env and int(mapix.numel()) != B) or (atk is not None and int(atk.numel()) != B):
        raise ValueError('ego_verdicts expects ptr (B+1), map_idx (B), attack_agt (B) and T >= 1')
    lw = scene_graph.lw.detach().to(device=dev, dtype=torch.float32).reshape(NA, 2).contiguous()
    out = outputs(out, dev, [('hit', (NA,), torch.int32, 0), ('coll_t', (NA,), torch.int32, T),
                              ('out_i', (B, len(EGO_I)), torch.int32, 0), ('grid_d', (B, 2), torch.float64, float('nan')),
                              ('status', (B,), torch.int32, 0)])
    if B == 0:
        return out
    if NA == 0:                                        # never hand a NULL pointer to the library
        traj = torch.zeros((1, T, 4), dtype=torch.float32, device=dev)
        lw = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    sm, ss, am, as_ = model_stats(model)
    lib.call('strive_ego_verdicts', L.ptr(traj), L.ptr(ptr), L.ptr(lw), None if atk is None else L.ptr(atk), sm, ss, am, as_,
             int(want_env), ops._map_pack(pack_env(map_env), dev).ref() if want_env else None, L.ptr(mapix) if want_env else None,
             L.ptr(lin_table(dev)) if want_env else None, int(lin_max), B, NA, T, L.ptr(out['hit']), L.ptr(out['coll_t']),
             L.ptr(out['out_i']), L.ptr(out['grid_d']), L.ptr(out['status']), L.stream_ptr(traj))
    return out


class FeasibilityBatcher(object):
    """The reference's queue of feasible scenes (src/adv_scenario_gen.py:176-256) as a host state machine.  ``push`` takes one
    scene's row of ``screen_batch``'s ``out_i`` (on the host), its agent count and whether it is the loader's last scene; it returns
    events in the reference's order: ``('log', line)`` with the reference's lines verbatim and at most one ``('batch', positions)``,
    the scenes (by the order they were pushed in) of a batch to optimise.

    (sic) On the loader's last scene a skip does not ``continue``: a last scene whose ego is too slow is still judged, and queued if
    it has a feasible attacker; a last scene that is skipped still flushes a non-empty queue."""
    SLOW = {'ego': 'Ego vehicle not moving more than velocity threshold, skipping...',
            'hardcode': 'Ego samples not moving more than velocity threshold, skipping...'}
    ONLY_EGO = 'Only ego vehicle in scene, skipping...'
    NONE_NEAR = 'Infeasible, no vehicles near ego, skipping...'
    NO_CATEGORY = 'No feasible attackers of requested category, skipping...'
    FEASIBLE = 'Feasible. Adding to batch...'
    CURRENT = 'Current batch NA: %d'
    FORMED = 'Formed batch! Starting optimization...'

    def __init__(self, batch_size, planner_name='ego'):
        if planner_name not in self.SLOW:
            raise ValueError("planner_name is 'ego' or 'hardcode'")
        self.batch_size, self.planner_name = batch_size, planner_name
        self.queue, self.total, self.pushed = [], 0, 0

    def push(self, row, count, is_last):
        n_others, n_any, n_feasible, verdict = int(row[0]), int(row[2]), int(row[3]), int(row[7])
        pos, ev = self.pushed, []
        self.pushed += 1
        skipped = []
        if verdict == VERDICT_EGO_SLOW:
            skipped.append(self.SLOW[self.planner_name])
        if not skipped or is_last:
            if n_others == 0:
                skipped.append(self.ONLY_EGO)
            elif n_any == 0:
                skipped.append(self.NONE_NEAR)
        ev += [('log', line) for line in skipped]
        if skipped and not is_last:
            return ev
        if n_others > 0 and n_any > 0:
            if n_feasible == 0:
                ev.append(('log', self.NO_CATEGORY))
            else:
                self.queue.append(pos)
                self.total += int(count)
                ev += [('log', self.FEASIBLE), ('log', self.CURRENT % self.total)]
        if (self.total < self.batch_size and not is_last) or not self.queue:
            return ev
        ev += [('log', self.FORMED), ('batch', self.queue)]
        self.queue, self.total = [], 0
        return ev


# ------------------------------------------------------------------------------------------------
# scenario files
# ------------------------------------------------------------------------------------------------

def batched_output_dicts(scene_graph, ptr_host, map_names, dt, model, init_fut_traj, adv_fut_traj, internal_ego, attack_agt, attack_t, adv_z,
                         prior_distrib, sol=None):
    """``prepare_output_dict(scene b, ...)`` (utils/scenario_gen.py) with its full key set for every scene b of a batch, equal value
    for value and in its key order, from ONE device->host copy (the sibling of ``refine_traffic_tracks.batched_output_dicts``, which
    writes the five tensors every scenario file has).  ``internal_ego`` (B,T,4) NORMALISED; ``attack_agt`` LOCAL and ``attack_t``: (B)
    host integers; ``adv_z`` (NA,Z); ``prior_distrib`` (mean, var) (NA,Z); ``sol``: None or ``(rows, sol_ptr_host, sol_traj (sNA,T,4)
    NORMALISED, sol_z (sNA,Z))`` with ``rows[b]`` the scene's place in the solution batch or None."""
    nrm, att = model.get_normalizer(), model.get_att_normalizer()
    parts = [('lw', att.unnormalize(scene_graph.lw)), ('sem', scene_graph.sem), ('past', nrm.unnormalize(scene_graph.past_gt)),
             ('fut_init', nrm.unnormalize(init_fut_traj)), ('fut_adv', nrm.unnormalize(adv_fut_traj)),
             ('fut_internal_ego', nrm.unnormalize(internal_ego)), ('z_adv', adv_z), ('mean', prior_distrib[0]), ('var', prior_distrib[1])]
    if sol is not None:
        parts += [('fut_sol', nrm.unnormalize(sol[2])), ('z_sol', sol[3])]
    parts = [(k, t.detach().to(torch.float32)) for k, t in parts]
    flat = torch.cat([t.reshape(-1) for _, t in parts]).cpu().numpy()
    host, o = {}, 0
    for k, t in parts:
        host[k] = flat[o:o + t.numel()].reshape(tuple(t.shape))
        o += t.numel()
    out = []
    for b in range(len(ptr_host) - 1):
        lo, hi = int(ptr_host[b]), int(ptr_host[b + 1])
        d = {'N': hi - lo, 'dt': dt, 'map': map_names[b]}
        for k in ('lw', 'sem', 'past', 'fut_init', 'fut_adv'):
            d[k] = host[k][lo:hi].tolist()
        d['fut_internal_ego'] = host['fut_internal_ego'][b].tolist()
        row = None if sol is None else sol[0][b]
        if row is not None:
            slo, shi = int(sol[1][row]), int(sol[1][row + 1])
            d['fut_sol'] = host['fut_sol'][slo:shi].tolist()
        d['attack_agt'], d['attack_t'] = int(attack_agt[b]), int(attack_t[b])
        d['z_adv'] = host['z_adv'][lo:hi].tolist()
        if row is not None:
            d['z_sol'] = host['z_sol'][slo:shi].tolist()
        d['z_prior'] = {'mean': host['mean'][lo:hi].tolist(), 'var': host['var'][lo:hi].tolist()}
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------
# the epoch
# ------------------------------------------------------------------------------------------------

# chunks of 64, 256 and 1024 agents were measured against the scene-by-scene path (profiles/r25_adv_verdict_bench.json): all are faster
# than it by far more than the repeats' spread; 256 is within 3 % of one chunk for everything and bounds the sampling's memory
DEFAULT_SCREEN_AGENTS = 256
RESULT_DIRS = ('adv_failed', 'sol_failed', 'adv_sol_success')


def _default_stage_fns():
    from .planners.hardcode_goalcond_nusc import HardcodeNuscPlanner
    from .utils.adv_gen_optim import run_adv_gen_optim
    from .utils.init_optim import run_init_optim
    from .utils.sol_optim import run_find_solution_optim
    return {'sample_batched': None, 'run_init_optim': run_init_optim, 'planner': HardcodeNuscPlanner, 'run_adv_gen_optim': run_adv_gen_optim,
            'run_find_solution_optim': run_find_solution_optim}


def _single_scenes(data_loader, device):
    """(scene_graph, map_idx, agent count, is it the last) of any iterable of single scenes: one scene of look-ahead."""
    it = iter(data_loader)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)
        scene_graph, map_idx = cur
        scene_graph, map_idx = scene_graph.to(device), torch.as_tensor(map_idx).reshape(-1).to(device)
        yield scene_graph, map_idx, int(scene_graph.future_gt.size(0)), nxt is None
        cur = nxt


def _join(scenes, device):
    """One batch of held single scenes [(data list, map_idx)], as the reference's GraphBatch.from_data_list / torch.cat."""
    batch = Batch.from_data_list([d for dl, _ in scenes for d in dl])
    batch.ptr, batch.batch = batch.ptr.to(device), batch.batch.to(device)
    return batch, torch.cat([mi for _, mi in scenes], dim=0)


def _screen_chunks(data_loader, screen_agents, device):
    """Chunks of consecutive scenes holding about ``screen_agents`` agents: (positions, counts, scene_graph, map_idx, holds the last,
    held).  A SceneSource is gathered with one launch per chunk; any other iterable is collected scene by scene."""
    if isinstance(data_loader, SceneSource):
        counts, n, lo = data_loader.counts, len(data_loader), 0
        while lo < n:
            hi, tot = lo, 0
            while hi < n and (hi == lo or tot < screen_agents):
                tot += counts[hi]
                hi += 1
            positions = list(range(lo, hi))
            scene_graph, map_idx = data_loader.gather(positions)
            yield positions, [counts[p] for p in positions], scene_graph, map_idx, hi == n, None
            lo = hi
        return
    positions, counts, held, tot = [], [], {}, 0
    for pos, (scene_graph, map_idx, count, is_last) in enumerate(_single_scenes(data_loader, device)):
        positions.append(pos)
        counts.append(count)
        held[pos] = (scene_graph.to_data_list(), map_idx)
        tot += count
        if tot >= screen_agents or is_last:
            scene_graph, map_idx = (scene_graph, map_idx) if len(positions) == 1 else _join([held[p] for p in positions], device)
            yield positions, counts, scene_graph, map_idx, is_last, held
            positions, counts, held, tot = [], [], {}, 0


def run_one_epoch(data_loader, batch_size, model, map_env, device, out_path, loss_weights, planner_name=None, planner_cfg='default',
                  feasibility_thresh=10.0, feasibility_time=4, feasibility_vel=0.5, feasibility_infront_min=0.0, feasibility_check_sep=True,
                  sol_future_len=16, num_iters=300, lr=0.05, viz=False, save=True, adv_attack_with=None, log=None, dt=None,
                  keep_results=False, screen_agents=DEFAULT_SCREEN_AGENTS, init_iters=(75, 100), on_planner_error='raise', stage_fns=None):
    """Run through ``data_loader`` -- a ``scene_source`` or any iterable of single-scene ``(scene_graph, map_idx)`` -- and find possible
    scenarios (reference src/adv_scenario_gen.py:108-548, its signature; ``viz`` defaults to False here).  Scenes are sampled and
    screened in chunks of about ``screen_agents`` agents: one ``sample_batched`` and one ``screen_batch`` call and ONE read-back per chunk
    (``screen_agents=1``: one scene per call, the reference's order of random draws).  The screening's rows drive a
    ``FeasibilityBatcher``; every batch it forms goes through the init fit, with 'hardcode' the planner rollout, the second fit and the
    removal of the scenes where the planner already collides, then the adversarial stage, the solution stage of the succeeded scenes
    and the scenario files.  The driver's own read-backs per batch: one per ``ego_verdicts`` call and one for the files, whatever the
    number of scenes.  ``init_iters``: the iterations of the two init fits; ``on_planner_error='drop'``: a scene the closed loop lost
    gets a log line and no file; ``stage_fns``: replacements for ``sample_batched``, ``run_init_optim``, ``planner`` (the class),
    ``run_adv_gen_optim``, ``run_find_solution_optim``, same arguments and returns.  ``log``: an open text file that receives the lines
    too; ``dt``: the scenes' time step (default ``data_loader.dataset.dt``).  Returns the number of files per result directory and,
    with ``keep_results``, a second item: per batch a dict of what was judged (``positions``, ``scene_graph``, ``map_idx``,
    ``final_result_traj``, ``attack_agt`` (local), ``adv_succeeded``, ``sol_succeeded``, ``sol_scene_graph``, ``sol_map_idx``,
    ``sol_result_traj``, ``dropped``)."""
    if viz:
        raise NotImplementedError('viz ' + NO_RENDERING)
    if planner_name not in ('ego', 'hardcode'):
        raise ValueError("planner_name is 'ego' or 'hardcode'")
    device = torch.device(device)
    fns = _default_stage_fns()
    fns.update(stage_fns or {})
    sample_fn = model.sample_batched if fns['sample_batched'] is None else fns['sample_batched']
    dataset = getattr(data_loader, 'dataset', None)
    if dt is None:
        if dataset is None:
            raise ValueError('run_one_epoch needs dt=... for a loader without a .dataset')
        dt = dataset.dt
    cat_column = None
    if adv_attack_with is not None:
        if dataset is None or adv_attack_with not in dataset.categories:
            raise ValueError('adv_attack_with=%r needs a loader whose .dataset has that category' % (adv_attack_with,))
        cat_column = dataset.categories.index(adv_attack_with)
    os.makedirs(out_path, exist_ok=True)
    scenes_path = os.path.join(out_path, 'scenario_results')
    if save:
        os.makedirs(scenes_path, exist_ok=True)
    batcher = FeasibilityBatcher(batch_size, planner_name)
    written, kept, held, count_of = {k: 0 for k in RESULT_DIRS}, [], {}, {}
    start_t = time.time()
    for positions, counts, scene_graph, map_idx, has_last, chunk_held in _screen_chunks(data_loader, screen_agents, device):
        with torch.no_grad():
            sample_pred = sample_fn(scene_graph, map_idx, map_env, 20, include_mean=True)
        allowed = None if cat_column is None else (scene_graph.sem[:, cat_column] == 1).to(torch.int32)
        scr = screen_batch(sample_pred['future_pred'], model, scene_graph, map_env, map_idx, feasibility_thresh, feasibility_time, 0.0,
                           feasibility_infront_min, feasibility_check_sep, planner_name, feasibility_vel, allowed)
        # ---- the chunk's read-back: every integer of its screening ----
        B = len(positions)
        ints = torch.cat([scr['out_i'].reshape(-1), scr['status']]).cpu().numpy()
        rows, status = ints[:B * len(SCREEN_I)].reshape(B, len(SCREEN_I)), ints[B * len(SCREEN_I):]
        check_status(status.tolist(), SCREEN_STATUS_TEXT, 'strive_feasibility_screen', positions)
        if chunk_held is not None:
            held.update(chunk_held)
        count_of.update(zip(positions, counts))
        for k, pos in enumerate(positions):
            for kind, what in batcher.push(rows[k], counts[k], has_last and k == B - 1):
                if kind == 'log':
                    _log(log, what)
                    continue
                if isinstance(data_loader, SceneSource):
                    batch, batch_map_idx = data_loader.gather(what)
                else:
                    batch, batch_map_idx = _join([held[p] for p in what], device)
                res = _optimise_batch(list(what), [count_of[p] for p in what], batch, batch_map_idx, model, map_env, device, loss_weights, planner_name, planner_cfg,
                                      feasibility_time, feasibility_infront_min, sol_future_len, num_iters, lr, init_iters, on_planner_error,
                                      fns, log, start_t, dt, scenes_path if save else None, written)
                if keep_results and res is not None:
                    kept.append(res)
                start_t = time.time()
            held = {p: v for p, v in held.items() if p in batcher.queue or p > pos}
            count_of = {p: v for p, v in count_of.items() if p in batcher.queue or p > pos}
    return (written, kept) if keep_results else written


def _readback(tensors):
    """ONE device->host copy of integer tensors, split again on the host."""
    flat = torch.cat([t.reshape(-1).to(torch.int32) for t in tensors]).cpu().numpy()
    out, o = [], 0
    for t in tensors:
        out.append(flat[o:o + t.numel()].reshape(tuple(t.shape)))
        o += t.numel()
    return out


def _ego_mask(scene_graph, device):
    NA = int(scene_graph.past.size(0))
    mask = torch.zeros((NA,), dtype=torch.bool, device=device)
    mask[scene_graph.ptr[:-1].to(device)] = True
    return mask


def _optimise_batch(positions, counts, scene_graph, map_idx, model, map_env, device, loss_weights, planner_name, planner_cfg, feasibility_time,
                    feasibility_infront_min, sol_future_len, num_iters, lr, init_iters, on_planner_error, fns, log, start_t, dt,
                    scenes_path, written):
    """One optimisation batch (reference :258-538); ``counts``: the scenes' agent counts, from which the batch's offsets are formed on
    the host.  Returns what ``keep_results`` keeps, or None for a batch that was given up."""
    from .utils.scenario_gen import detach_embed_info
    nrm, att = model.get_normalizer(), model.get_att_normalizer()
    B = len(positions)
    ptr_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ego_mask = _ego_mask(scene_graph, device)
    with torch.no_grad():
        embed_info_attached = model.embed(scene_graph, map_idx, map_env)
    embed_info = detach_embed_info(embed_info_attached)
    planner = None
    if planner_name == 'hardcode':
        from .planners.hardcode_goalcond_nusc import CONFIG_DICT
        from .planners.planner import PlannerConfig
        if planner_cfg not in CONFIG_DICT:
            raise ValueError('planner_cfg %r is not one of %s' % (planner_cfg, sorted(CONFIG_DICT)))
        _log(log, 'Using planner config:')
        _log(log, str(CONFIG_DICT[planner_cfg]))
        planner = fns['planner'](map_env, PlannerConfig(**CONFIG_DICT[planner_cfg]))
    z_init = embed_info_attached['posterior_out'][0].detach()
    init_traj = scene_graph.future_gt[:, :, :4].clone().detach()
    _log(log, 'Running initialization optimization...')
    z_init, init_fit_traj, _ = fns['run_init_optim'](z_init, init_traj, scene_graph.future_vis, 0.1, loss_weights, model, scene_graph, map_env,
                                                     map_idx, init_iters[0], embed_info, embed_info['prior_out'])
    if planner_name == 'hardcode':
        planner.reset(nrm.unnormalize(scene_graph.past_gt[:, -1, :]), att.unnormalize(scene_graph.lw), scene_graph.batch, B, map_idx)
        plan_t = np.linspace(model.dt, model.dt * model.FT, model.FT)
        init_agt_ptr = ptr_host - np.arange(B + 1)
        planner_init = planner.rollout(nrm.unnormalize(init_fit_traj[~ego_mask]).contiguous(), plan_t, init_agt_ptr, plan_t,
                                       control_all=False).to(scene_graph.future_gt)
        init_traj[ego_mask] = nrm.normalize(planner_init)
        _log(log, 'Fine-tune init with planner rollout...')
        z_init, init_fit_traj, _ = fns['run_init_optim'](z_init, init_traj, scene_graph.future_vis, lr, loss_weights, model, scene_graph,
                                                         map_env, map_idx, init_iters[1], embed_info, embed_info['prior_out'])
        # the scenes where the planner collides with the fitted scene already: ONE call, one read-back
        v = ego_verdicts(init_fit_traj, model, scene_graph)
        out_i, status = _readback([v['out_i'], v['status']])
        check_status(status.tolist(), EGO_STATUS_TEXT, 'strive_ego_verdicts', positions)
        bvalid = out_i[:, 1] == 0
        if int(bvalid.sum()) < B:
            _log(log, 'Planner already caused collision after init, removing from batch...')
            if int(bvalid.sum()) == 0:
                _log(log, 'No valid sequences left in batch! Skipping...')
                return None
            avalid = torch.zeros((int(ego_mask.numel()),), dtype=torch.bool)
            for b in range(B):
                if bvalid[b]:
                    avalid[int(ptr_host[b]):int(ptr_host[b + 1])] = True
            avalid = avalid.to(device)
            map_idx = map_idx[torch.as_tensor(bvalid, device=device)]
            positions = [p for b, p in enumerate(positions) if bvalid[b]]
            counts = [c for b, c in enumerate(counts) if bvalid[b]]
            ptr_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            z_init, init_traj = z_init[avalid], init_traj[avalid]
            scene_graph = Batch.from_data_list([g for b, g in enumerate(scene_graph.to_data_list()) if bvalid[b]]).to(device)
            B = len(positions)
            ego_mask = _ego_mask(scene_graph, device)
            with torch.no_grad():
                embed_info_attached = model.embed(scene_graph, map_idx, map_env)
            embed_info = detach_embed_info(embed_info_attached)
    with torch.no_grad():
        init_future_pred = model.decode_embedding(z_init, embed_info_attached, scene_graph, map_idx, map_env)['future_pred'].detach()
        init_future_pred[ego_mask] = init_traj[ego_mask]        # the ego is the data or the planner's rollout, not our fit of it

    # ---- adversarial optimisation ----
    cur_z = z_init.clone().detach()
    pm, pv = embed_info['prior_out']
    tgt_prior_distrib, other_prior_distrib = (pm[ego_mask], pv[ego_mask]), (pm[~ego_mask], pv[~ego_mask])
    extra = {'on_planner_error': on_planner_error} if on_planner_error != 'raise' else {}
    cur_z, final_result_traj, final_decoder_out, attack_agt, attack_t = fns['run_adv_gen_optim'](
        cur_z, lr, loss_weights, model, scene_graph, map_env, map_idx, num_iters, embed_info, planner_name, tgt_prior_distrib,
        other_prior_distrib, feasibility_time, feasibility_infront_min, planner=planner, planner_viz_out=None, **extra)
    dropped = sorted(int(b) for b in final_decoder_out.get('scenes_dropped', []))
    atk_local = np.asarray(attack_agt).astype(np.int64) - ptr_host[:-1]
    atk_dev = torch.as_tensor(atk_local, dtype=torch.int32)
    atk_dev[dropped] = -1
    v = ego_verdicts(final_result_traj, model, scene_graph, atk_dev.to(device))
    out_i, status, maps = _readback([v['out_i'], v['status'], map_idx])
    check_status(status.tolist(), EGO_STATUS_TEXT, 'strive_ego_verdicts', positions)
    adv_succeeded = [bool(out_i[b, 2] == 1) for b in range(B)]

    # ---- the solution batch of the succeeded scenes ----
    sol_succeeded, sol, kept_sol = [False] * B, None, (None, None, None)
    if any(adv_succeeded):
        _log(log, 'Batch adv optim successes:')
        _log(log, str(adv_succeeded))
        _log(log, 'Solution scene graph:')
        graphs = scene_graph.to_data_list()
        sol_scene_graph = Batch.from_data_list([graphs[b] for b in range(B) if adv_succeeded[b]]).to(device)
        _log(log, 'Adv gen succeeded! Finding solution...')
        sol_bmask = torch.tensor(adv_succeeded)
        sol_amask = torch.zeros((int(ego_mask.numel()),), dtype=torch.bool)
        for b in range(B):
            if adv_succeeded[b]:
                sol_amask[int(ptr_host[b]):int(ptr_host[b + 1])] = True
        sol_amask, sol_bmask = sol_amask.to(device), sol_bmask.to(device)
        sol_ego_mask = _ego_mask(sol_scene_graph, device)
        sol_map_idx = map_idx[sol_bmask]
        sol_embed_info = {k: (val[sol_amask] if torch.is_tensor(val) else (val[0][sol_amask], val[1][sol_amask])) for k, val in embed_info.items()}
        sol_tgt_prior = (tgt_prior_distrib[0][sol_bmask], tgt_prior_distrib[1][sol_bmask])
        sol_other_prior = (sol_embed_info['prior_out'][0][~sol_ego_mask], sol_embed_info['prior_out'][1][~sol_ego_mask])
        sol_z, sol_result_traj, _ = fns['run_find_solution_optim'](
            cur_z.clone().detach()[sol_amask], final_result_traj[sol_amask], sol_future_len, lr, loss_weights, model, sol_scene_graph, map_env,
            sol_map_idx, num_iters, sol_embed_info, sol_tgt_prior, sol_other_prior)
        sv = ego_verdicts(sol_result_traj[:, 0:1], model, sol_scene_graph, None, map_env, sol_map_idx)
        sol_i, sol_status = _readback([sv['out_i'], sv['status']])
        sol_ptr = np.concatenate([[0], np.cumsum([c for b, c in enumerate(counts) if adv_succeeded[b]])]).astype(np.int64)
        rows = np.cumsum(adv_succeeded) - 1
        check_status(sol_status.tolist(), EGO_STATUS_TEXT, 'strive_ego_verdicts', [positions[b] for b in range(B) if adv_succeeded[b]])
        for b in range(B):
            if adv_succeeded[b]:
                sol_succeeded[b] = bool(sol_i[rows[b], 1] == 0 and sol_i[rows[b], 4] == 0)
        sol = ([int(rows[b]) if adv_succeeded[b] else None for b in range(B)], sol_ptr, sol_result_traj[:, 0], sol_z)
        kept_sol = (sol_scene_graph, sol_map_idx, sol_result_traj)
    _log(log, 'Optimized sequence in %f sec!' % (time.time() - start_t))

    # ---- the scenario files: everything they hold in one copy ----
    if scenes_path is not None:
        dicts = batched_output_dicts(scene_graph, ptr_host, [map_env.map_list[int(m)] for m in maps], dt, model, init_future_pred,
                                     final_result_traj[:, 0], final_decoder_out['future_pred'][scene_graph.ptr[:-1].to(device)].detach(),
                                     atk_local, attack_t, cur_z, embed_info['prior_out'], sol)
    for b in range(B):
        if b in dropped:
            _log(log, 'The planner rollout failed in scene %d during the adversarial stage, dropping it...' % positions[b])
            continue
        result_dir = 'adv_failed' if not adv_succeeded[b] else ('adv_sol_success' if sol_succeeded[b] else 'sol_failed')
        written[result_dir] += 1
        if scenes_path is not None:
            cur_scene_out_path = os.path.join(scenes_path, result_dir)
            os.makedirs(cur_scene_out_path, exist_ok=True)
            fout_path = os.path.join(cur_scene_out_path, 'scene_%04d.json' % positions[b])
            _log(log, 'Saving scene to %s' % fout_path)
            with open(fout_path, 'w') as writer:
                json.dump(dicts[b], writer)
    return {'positions': positions, 'scene_graph': scene_graph, 'map_idx': map_idx, 'final_result_traj': final_result_traj,
            'attack_agt': atk_local.tolist(), 'adv_succeeded': adv_succeeded, 'sol_succeeded': sol_succeeded, 'sol_scene_graph': kept_sol[0],
            'sol_map_idx': kept_sol[1], 'sol_result_traj': kept_sol[2], 'dropped': dropped}


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------

# keys of a config file that are accepted and ignored: they describe the devkit's data, or (viz) ask for rendering
IGNORED_KEYS = DEVKIT_KEYS + ('split', 'val_size', 'use_challenge_splits', 'viz')
LOSS_WEIGHTS = (('coll_veh', 'loss_coll_veh', 20.0), ('coll_veh_plan', 'loss_coll_veh_plan', 20.0), ('coll_env', 'loss_coll_env', 20.0),
                ('motion_prior', 'loss_motion_prior', 1.0), ('motion_prior_atk', 'loss_motion_prior_atk', 0.005), ('init_z', 'loss_init_z', 0.5),
                ('init_z_atk', 'loss_init_z_atk', 0.05), ('motion_prior_ext', 'loss_motion_prior_ext', 0.0001),
                ('match_ext', 'loss_match_ext', 10.0), ('adv_crash', 'loss_adv_crash', 2.0), ('sol_coll_veh', 'sol_loss_coll_veh', 10.0),
                ('sol_coll_env', 'sol_loss_coll_env', 10.0), ('sol_motion_prior', 'sol_loss_motion_prior', 0.005),
                ('sol_init_z', 'sol_loss_init_z', 0.0), ('sol_motion_prior_ext', 'sol_loss_motion_prior_ext', 0.001),
                ('sol_match_ext', 'sol_loss_match_ext', 10.0), ('init_match_ext', 'init_loss_match_ext', 10.0),
                ('init_motion_prior_ext', 'init_loss_motion_prior_ext', 0.1))
# name, type, default, what it is -- the reference's argument names and defaults (its src/adv_scenario_gen.py:33-106 and the base arguments
# it uses); lists are nargs='+', bool is a store_true flag
ARGUMENTS = (
    ('out', str, './out/traffic_out', 'where adv_gen_log.txt and scenario_results/ go (used as given)'),
    ('ckpt', str, None, 'a save_state file with the traffic model\'s weights'),
    ('batch_size', int, 4, 'a batch is optimised as soon as its feasible scenes hold this many agents'),
    ('past_len', int, 4, 'observed frames per window'),
    ('future_len', int, 12, 'predicted frames per window'),
    ('map_obs_size_pix', int, 256, 'side of the square map crop around an agent, in pixels'),
    ('latent_size', int, 32, 'width of the latent z'),
    ('agent_types', [str], None, 'the agent categories; must be the category set that has normalisation statistics for their number'),
    ('num_classes', int, 2, 'number of agent categories when --agent_types is not given'),
    ('tracks', str, None, 'tracks file (datasets/tracks.py) to take the scenes from'),
    ('scenario_path', str, None, 'a directory of scenario files appended to the scenes'),
    ('maps', str, None, 'a maps file (datasets/maps.py) with the maps the scenes name; default: the synthetic maps'),
    ('seq_interval', int, 10, 'steps from the start of one window of a scene to the start of the next'),
    ('shuffle', bool, False, 'walk the scenes in a random order (drawn from --seed)'),
    ('adv_attack_with', str, None, 'attack with agents of this category only'),
    ('planner', str, 'ego', "'ego': the recorded ego future (replay); 'hardcode': the rule-based planner in closed loop"),
    ('planner_cfg', str, 'default', 'the rule-based planner\'s configuration'),
    ('feasibility_thresh', float, 10.0, 'an attacker must come this close (m) to the ego in some sample'),
    ('feasibility_time', int, 4, 'only steps from this one on count'),
    ('feasibility_vel', float, 0.5, 'the ego must move at least this far in some step'),
    ('feasibility_infront_min', float, 0.0, 'smallest cosine between the ego\'s heading and the direction to the attacker'),
    ('feasibility_check_sep', bool, False, 'attacker and ego must not be separated by non-drivable area'),
) + tuple((arg, float, default, 'loss weight %s' % key) for key, arg, default in LOSS_WEIGHTS) + (
    ('sol_future_len', int, 16, 'steps rolled out by the solution stage'),
    ('num_iters', int, 300, 'optimisation iterations of the adversarial and of the solution stage'),
    ('lr', float, 0.05, 'step size of Adam'),
    ('viz', bool, False, 'rendering; not available'),
    ('save', bool, False, 'write the scenario files'),
    ('device', str, 'cuda:0', 'torch device of model, data and maps'),
    ('seed', int, 0, 'seeds the shuffle and the latent draws'),
    ('screen_agents', int, DEFAULT_SCREEN_AGENTS, 'scenes are sampled and screened in chunks of about this many agents (1: scene by scene)'),
    ('on_planner_error', str, 'raise', "'drop': a scene whose planner rollout fails in the closed loop is dropped, not the run"),
)


def parse_cfg(argv=None):
    """Defaults < ``--config`` file < command line (``refine_traffic_tracks.parse_cfg``'s rules, which are ``train_traffic.read_config``'s):
    the reference's flat ``key: value`` files; devkit keys and ``viz`` in a file are ignored and reported.  ``--viz`` on the command
    line raises."""
    from .refine_traffic_tracks import get_parser, parse_cfg as parse
    argv = list(__import__('sys').argv[1:] if argv is None else argv)
    if '--viz' in argv:
        raise NotImplementedError('--viz ' + NO_RENDERING)
    parser = get_parser(ARGUMENTS, 'Adversarial scenario generation on a tracks file', optimiser_switch=False)
    cfg, ignored = parse(argv, ARGUMENTS, parser, IGNORED_KEYS)
    if cfg['planner'] not in ('ego', 'hardcode') or cfg['on_planner_error'] not in ('raise', 'drop'):
        raise ValueError("--planner is 'ego' or 'hardcode'; --on_planner_error is 'raise' or 'drop'")
    return cfg, ignored


def main(argv=None, keep_results=False):
    """The command line.  Returns what ``run_one_epoch`` returns (``keep_results`` is handed on to it)."""
    from . import synth
    from .constants import NUSC_BIKE_PARAMS
    from .eval_traffic_tracks import tracks_loader
    from .models.traffic_model import TrafficModel
    from .train_traffic import categories_for
    from .utils.torch import count_params, load_state
    cfg, ignored = parse_cfg(argv)
    if cfg['ckpt'] is None:
        raise SystemExit('Must pass in model weights to do scenario generation! (--ckpt)')
    categories_for(cfg)
    os.makedirs(cfg['out'], exist_ok=True)
    with open(os.path.join(cfg['out'], 'adv_gen_log.txt'), 'w') as log:
        _log(log, 'Args: ' + str(cfg))
        if ignored:
            _log(log, 'Ignoring config keys that describe the devkit\'s data or ask for rendering: ' + ', '.join(ignored))
        device = torch.device(cfg['device'])
        _log(log, 'Using device %s...' % str(device))
        torch.manual_seed(cfg['seed'])
        data_cfg = {k: cfg[k] for k in ('tracks', 'scenario_path', 'maps', 'num_classes', 'past_len', 'future_len', 'seq_interval')}
        # (the reference's load_lanegraph=(cfg.planner == 'hardcode'): a maps file brings its own lane graphs, built on the device)
        loader, map_env = tracks_loader(dict(data_cfg, load_lanegraph=cfg['planner'] == 'hardcode'), device)
        if cfg['planner'] == 'hardcode' and cfg['maps'] is None:
            lane_graph = synth.make_lane_graph()
            map_env.lane_graphs = {name: lane_graph for name in map_env.map_list}
        dataset = loader.dataset
        source = scene_source(dataset, cfg['shuffle'], torch.Generator().manual_seed(cfg['seed']))
        model = TrafficModel(cfg['past_len'], cfg['future_len'], cfg['map_obs_size_pix'], len(dataset.categories),
                             latent_size=cfg['latent_size']).to(device)
        ckpt_epoch, _ = load_state(cfg['ckpt'], model, map_location=device)
        _log(log, 'Loaded checkpoint from epoch %d...' % ckpt_epoch)
        _log(log, 'Num model params: %d' % count_params(model))
        model.set_normalizer(dataset.get_state_normalizer())
        model.set_att_normalizer(dataset.get_att_normalizer())
        model.set_bicycle_params(NUSC_BIKE_PARAMS)
        loss_weights = {key: cfg[arg] for key, arg, _ in LOSS_WEIGHTS}
        model.train()
        return run_one_epoch(source, cfg['batch_size'], model, map_env, device, cfg['out'], loss_weights, planner_name=cfg['planner'],
                             planner_cfg=cfg['planner_cfg'], feasibility_thresh=cfg['feasibility_thresh'],
                             feasibility_time=cfg['feasibility_time'], feasibility_vel=cfg['feasibility_vel'],
                             feasibility_infront_min=cfg['feasibility_infront_min'], feasibility_check_sep=cfg['feasibility_check_sep'],
                             sol_future_len=cfg['sol_future_len'], num_iters=cfg['num_iters'], lr=cfg['lr'], viz=cfg['viz'],
                             save=cfg['save'], adv_attack_with=cfg['adv_attack_with'], log=log, keep_results=keep_results,
                             screen_agents=cfg['screen_agents'], on_planner_error=cfg['on_planner_error'])


if __name__ == '__main__':
    main()
