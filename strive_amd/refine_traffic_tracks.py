"""The refine driver (reference src/refine_traffic_optim.py:34-121, :228-505) around ``refine_traffic_optim``: the walk over the
scene dataset of a tracks file, single scenes accumulated into batches of about ``batch_size`` agents, the per-scene collision
verdicts, the ``success/`` and ``failed/`` scenario files and the pooled ``veh_coll`` / ``env_coll`` rates:

    python -m strive_amd.refine_traffic_tracks --ckpt CKPT --tracks FILE [--scenario_path DIR] --out OUT [--config FILE]

writes ``OUT/refine_traffic_log.txt`` and, with ``--save``, ``OUT/scenario_results/{success,failed}/scene_%04d.json``.  The arguments
are the reference's, with its defaults, plus ``--tracks`` / ``--scenario_path`` (``eval_traffic_tracks.tracks_loader``), ``--seed`` and
``--device``.  ``OUT`` is used as given: the reference appends ``_<unix time>`` to it.  Rendering (``--viz``), wandb and the
reference's skipping of a batch that raised a ``RuntimeError`` are not offered; single process only.

Differences in HOW, not in what is written:

* The reference calls ``compute_metrics`` once per scene on a single-scene graph (shapely polygons, one ``check_on_layer`` pass and
  its read-backs per scene).  Here a batch has ONE ``strive_refine_verdicts`` call (``batch_verdicts``): every scene gets the verdicts
  of its own call, including the sampling grid ``check_on_layer`` forms from that scene's rows alone.
* A batch is read back in two copies whatever its number of scenes: the integers (verdicts, statuses, map indices) and, with
  ``save``, the unnormalised tensors of all its scenario files.
* A ``scene_source`` knows every scene's agent count on the host, so the batches are planned up front (``plan_batches``) and each
  is one ``dataset.get_batch`` launch; no scene is loaded singly.  Any other iterable of single scenes is collected with
  ``to_data_list()`` / ``Batch.from_data_list`` as the reference does.  Both give the same batches.
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
from .refine_traffic_optim import refine_traffic_optim
from .train_traffic import DEVKIT_KEYS, read_config
from .utils.scenario_gen import log_freq_stat, print_metrics

OUT_I = ('num_coll_veh', 'num_traj_veh', 'env_coll', 'env_total', 'success', 'L', 'W', 'rows')
STATUS_TEXT = {2: 'agent offsets leave the arrays', 3: 'map index out of range',
               4: 'the drivable-area sampling grid of the scene is outside 1..%d samples per axis' % LIN_MAX}
NO_RENDERING = 'renders scenes with matplotlib and the nuScenes map API; rendering is not part of strive_amd'
# keys of a config file that are accepted and ignored: they describe the devkit's data, or (viz) ask for rendering
IGNORED_KEYS = DEVKIT_KEYS + ('split', 'use_challenge_splits', 'viz')


def _log(log, line):
    print(line)
    if log is not None:
        log.write(line + '\n')
        log.flush()


# ------------------------------------------------------------------------------------------------
# verdicts
# ------------------------------------------------------------------------------------------------

def batch_verdicts(final_result_traj, model, scene_graph, map_env, map_idx, out=None, lib=None, lin_max=LIN_MAX):
    """The collision verdicts of every scene of a batch, each as the reference's ``compute_metrics`` (:84-121) gives them on that
    scene alone: ONE ``strive_refine_verdicts`` call, nothing read back.  ``final_result_traj`` (NA,1,T,4) or (NA,T,4) and
    ``scene_graph.lw`` NORMALISED, ``scene_graph.ptr`` (B+1), ``map_idx`` (B).  Returns tensors on the trajectories' device:
    ``did_veh``, ``did_env`` (NA) int32, ``out_i`` (B,8) int32 in the order of OUT_I, ``grid_d`` (B,2) float64 (the ratios L and W were
    rounded from), ``status`` (B) int32 (STATUS_TEXT; the outputs of such a scene are untouched).  ``out`` supplies output buffers."""
    traj = traj_arg(final_result_traj, 'batch_verdicts')
    dev = traj.device
    lib = ops._lib_for(traj) if lib is None else lib
    NA, T = int(traj.shape[0]), int(traj.shape[1])
    ptr = i32(scene_graph.ptr, dev)
    B = int(ptr.numel()) - 1
    mapix = i32(map_idx, dev, -1)
    if B < 0 or int(mapix.numel()) != B or T < 1:
        raise ValueError('batch_verdicts expects ptr (B+1), map_idx (B) and T >= 1')
    lw = scene_graph.lw.detach().to(device=dev, dtype=torch.float32).reshape(NA, 2).contiguous()
    out = outputs(out, dev, [('did_veh', (NA,), torch.int32, 0), ('did_env', (NA,), torch.int32, 0),
                             ('out_i', (B, len(OUT_I)), torch.int32, 0), ('grid_d', (B, 2), torch.float64, float('nan')),
                             ('status', (B,), torch.int32, 0)])
    if B == 0:
        return out
    if NA == 0:                                        # never hand a NULL pointer to the library
        traj = torch.zeros((1, T, 4), dtype=torch.float32, device=dev)
        lw = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    sm, ss, am, as_ = model_stats(model)
    lib.call('strive_refine_verdicts', L.ptr(traj), L.ptr(ptr), L.ptr(lw), sm, ss, am, as_, ops._map_pack(pack_env(map_env), dev).ref(),
             L.ptr(mapix), L.ptr(lin_table(dev)), int(lin_max), B, NA, T, L.ptr(out['did_veh']), L.ptr(out['did_env']),
             L.ptr(out['out_i']), L.ptr(out['grid_d']), L.ptr(out['status']), L.stream_ptr(traj))
    return out


def compute_metrics(metrics, freq_metrics_cnt, freq_metrics_total, cur_z, final_result_traj, model, scene_graph, map_env, map_idx,
                    prior_distrib):
    """The reference's ``compute_metrics`` (:84-121), signature and return value, on top of ``batch_verdicts``: all inputs
    NORMALISED, ``final_result_traj`` (NA,1,FT,4).  On a single-scene graph it gives the reference's numbers; on a batch, the sums
    of its scenes' numbers.  (``cur_z`` and ``prior_distrib`` are not used, as in the reference.)"""
    v = batch_verdicts(final_result_traj, model, scene_graph, map_env, map_idx)
    host = torch.cat([v['out_i'].reshape(-1), v['status']]).cpu().numpy()
    B = int(v['status'].numel())
    check_status(host[B * len(OUT_I):].tolist(), STATUS_TEXT, 'strive_refine_verdicts')
    oi = host[:B * len(OUT_I)].reshape(B, len(OUT_I))
    seq_metrics = dict()
    freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'veh_coll', int(oi[:, 0].sum()), int(oi[:, 1].sum()))
    seq_metrics['veh_coll'] = int(oi[:, 0].sum())
    freq_metrics_cnt, freq_metrics_total = log_freq_stat(freq_metrics_cnt, freq_metrics_total, 'env_coll', int(oi[:, 2].sum()), int(oi[:, 3].sum()))
    seq_metrics['env_coll'] = int(oi[:, 2].sum())
    return metrics, freq_metrics_cnt, freq_metrics_total, seq_metrics


# ------------------------------------------------------------------------------------------------
# batches of about batch_size agents
# ------------------------------------------------------------------------------------------------

class AgentCountBatcher(object):
    """The reference's accumulation of single scenes into optimisation batches (:262-310) as a state machine: ``push`` takes the
    next scene's agent count and whether it is the loader's last scene, and returns the events it causes, in order: ``('log',
    line)`` and at most one ``('batch', [positions])``.  A scene with fewer than ``feasibility_NA`` agents is skipped; a feasible
    one is queued; the queue becomes a batch as soon as its agents reach ``batch_size``, or at the last scene (also when that
    scene itself was skipped) unless it is empty."""

    def __init__(self, batch_size, feasibility_NA=1):
        self.batch_size, self.feasibility_NA = int(batch_size), int(feasibility_NA)
        self.queue, self.total, self.position = [], 0, 0

    def push(self, count, is_last):
        events = []
        i, count = self.position, int(count)
        self.position += 1
        if count < self.feasibility_NA:
            events.append(('log', 'Only %d agents in scene, skipping...' % count))
            if not is_last:
                return events
        else:
            events.append(('log', 'Feasible. Adding to batch...'))
            self.queue.append(i)
            self.total += count
            events.append(('log', 'Batch NA: %d' % self.total))
        if (self.total < self.batch_size and not is_last) or not self.queue:
            return events
        events.append(('log', 'Formed batch! Starting optimization...'))
        events.append(('batch', self.queue))
        self.queue, self.total = [], 0
        return events


def plan_batches(counts, batch_size, feasibility_NA=1):
    """Pure host function: the events (AgentCountBatcher) of a whole loader whose scenes have ``counts`` agents, in loader order."""
    counts = [int(c) for c in counts]
    batcher = AgentCountBatcher(batch_size, feasibility_NA)
    events = []
    for i, c in enumerate(counts):
        events += batcher.push(c, i == len(counts) - 1)
    return events


class SceneSource(object):
    """What the reference's ``GraphDataLoader(dataset, batch_size=1, shuffle=...)`` yields -- single-scene ``(Batch, map_idx)`` -- over a
    ``NuScenesDataset``, with what lets a driver skip loading scenes singly: ``counts``, the host agent count of every scene in
    iteration order, and ``gather(positions)``, ONE ``dataset.get_batch`` launch for the scenes at these positions of the iteration
    order.  The order is drawn once, at construction (``generator``: a host torch.Generator), so that ``counts`` describes every
    iteration."""

    def __init__(self, dataset, shuffle=False, generator=None):
        self.dataset = dataset
        n = len(dataset)
        self.order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
        self.counts = np.diff(dataset.batch_ptr(self.order)).astype(np.int64).tolist() if n else []

    def __len__(self):
        return len(self.order)

    def __iter__(self):
        for i in self.order:
            yield self.dataset.get_batch([i])

    def gather(self, positions):
        return self.dataset.get_batch([self.order[p] for p in positions])


def scene_source(dataset, shuffle=False, generator=None):
    return SceneSource(dataset, shuffle, generator)


def _planned_batches(source, batch_size, feasibility_NA, log):
    for kind, what in plan_batches(source.counts, batch_size, feasibility_NA):
        if kind == 'log':
            _log(log, what)
        else:
            scene_graph, map_idx = source.gather(what)
            yield what, scene_graph, map_idx


def _collected_batches(data_loader, batch_size, feasibility_NA, device, log):
    """Any iterable of single scenes, as the reference walks it: one scene of look-ahead tells which is the last."""
    batcher = AgentCountBatcher(batch_size, feasibility_NA)
    held = {}
    it = iter(data_loader)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)
        scene_graph, map_idx = cur
        scene_graph, map_idx = scene_graph.to(device), torch.as_tensor(map_idx).reshape(-1).to(device)
        held[batcher.position] = (scene_graph.to_data_list(), map_idx)
        for kind, what in batcher.push(int(scene_graph.future_gt.size(0)), nxt is None):
            if kind == 'log':
                _log(log, what)
            else:
                batch = Batch.from_data_list([d for p in what for d in held[p][0]])
                batch.ptr, batch.batch = batch.ptr.to(device), batch.batch.to(device)
                yield what, batch, torch.cat([held[p][1] for p in what], dim=0)
        held = {p: v for p, v in held.items() if p in batcher.queue}
        cur = nxt


# ------------------------------------------------------------------------------------------------
# scenario files
# ------------------------------------------------------------------------------------------------

def batched_output_dicts(scene_graph, ptr_host, map_names, dt, model, init_fut_traj, adv_fut_traj):
    """``prepare_output_dict(scene b, ...)`` (utils/scenario_gen.py) for every scene b of a batch, equal value for value, from ONE
    device->host copy: the tensors are unnormalised on the device for the whole batch (element-wise, so a scene's values do not
    depend on its neighbours), packed, copied and sliced on the host.  ``ptr_host``: the batch's agent offsets (B+1) on the host;
    ``map_names`` (B); ``init_fut_traj`` / ``adv_fut_traj`` (NA,T,4) NORMALISED."""
    nrm, att = model.get_normalizer(), model.get_att_normalizer()
    parts = [('lw', att.unnormalize(scene_graph.lw)), ('sem', scene_graph.sem), ('past', nrm.unnormalize(scene_graph.past_gt)),
             ('fut_init', nrm.unnormalize(init_fut_traj)), ('fut_adv', nrm.unnormalize(adv_fut_traj))]
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
        for k, _ in parts:
            d[k] = host[k][lo:hi].tolist()
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------
# the epoch
# ------------------------------------------------------------------------------------------------

def run_one_epoch(data_loader, batch_size, model, map_env, device, out_path, loss_weights, feasibility_NA=1, samp_future_len=12,
                  save_future_len=12, optim_use_adam=False, num_iters=10, lr=1.0, viz=False, save=True, use_wandb=False, log=None,
                  refine_fn=None, dt=None, keep_results=False):
    """Run through ``data_loader`` -- a ``scene_source`` or any iterable of single-scene ``(scene_graph, map_idx)`` --, sample futures
    and refine them to avoid collisions (reference :228-392).  Per batch: ``refine_fn`` (default ``refine_traffic_optim``; same
    arguments and return value), one ``batch_verdicts`` call, two device->host copies, then the scenario files
    ``scenario_results/{success,failed}/scene_%04d.json``, numbered by the scene's position in the loader's order.  ``log``: an open
    text file that receives the lines too; ``dt``: the scenes' time step (default: ``data_loader.dataset.dt``).  Returns the
    counter dicts ``(freq_metrics_cnt, freq_metrics_total)`` and, with ``keep_results``, a third item: per batch a dict of the loader
    ``positions``, the batch (``scene_graph``, ``map_idx``), the ``verdicts`` (device tensors), ``init_future_pred`` and
    ``final_result_traj``."""
    if viz:
        raise NotImplementedError('viz ' + NO_RENDERING)
    if use_wandb:
        raise NotImplementedError('use_wandb: wandb logging is not part of strive_amd')
    device = torch.device(device)
    refine_fn = refine_traffic_optim if refine_fn is None else refine_fn
    if dt is None:
        if not hasattr(data_loader, 'dataset'):
            raise ValueError('run_one_epoch needs dt=... for a loader without a .dataset')
        dt = data_loader.dataset.dt
    os.makedirs(out_path, exist_ok=True)
    scenes_path = os.path.join(out_path, 'scenario_results')
    if save:
        os.makedirs(scenes_path, exist_ok=True)
    metrics, freq_cnt, freq_total, kept = {}, {}, {}, []
    if isinstance(data_loader, SceneSource):
        batches = _planned_batches(data_loader, batch_size, feasibility_NA, log)
    else:
        batches = _collected_batches(data_loader, batch_size, feasibility_NA, device, log)
    while True:
        start_t = time.time()
        item = next(batches, None)
        if item is None:
            break
        positions, scene_graph, map_idx = item
        B = len(positions)
        init_future_pred, cur_z, optim_result_traj, embed_info = refine_fn(scene_graph, map_idx, map_env, model, loss_weights, num_iters,
                                                                           samp_future_len, save_future_len, optim_use_adam, lr)
        verdicts = batch_verdicts(optim_result_traj, model, scene_graph, map_env, map_idx)
        # ---- read-back 1: every integer of the batch ----
        ints = torch.cat([verdicts['out_i'].reshape(-1), verdicts['status'], map_idx.reshape(-1).to(torch.int32),
                          scene_graph.ptr.reshape(-1).to(torch.int32)]).cpu().numpy()
        n_oi = B * len(OUT_I)
        out_i, status = ints[:n_oi].reshape(B, len(OUT_I)), ints[n_oi:n_oi + B]
        maps, ptr_host = ints[n_oi + B:n_oi + 2 * B], ints[n_oi + 2 * B:]
        check_status(status.tolist(), STATUS_TEXT, 'strive_refine_verdicts', positions)
        for b in range(B):               # (pooled as the reference's per-scene log_freq_stat calls pool them)
            log_freq_stat(freq_cnt, freq_total, 'veh_coll', int(out_i[b, 0]), int(out_i[b, 1]))
            log_freq_stat(freq_cnt, freq_total, 'env_coll', int(out_i[b, 2]), int(out_i[b, 3]))
        _log(log, 'Optimized sequence in %f sec!' % (time.time() - start_t))
        if save:
            # ---- read-back 2: everything the batch's files hold ----
            dicts = batched_output_dicts(scene_graph, ptr_host, [map_env.map_list[int(m)] for m in maps], dt, model, init_future_pred,
                                         optim_result_traj[:, 0])
            for b in range(B):
                cur_scene_out_path = os.path.join(scenes_path, 'success' if out_i[b, 4] else 'failed')
                os.makedirs(cur_scene_out_path, exist_ok=True)
                fout_path = os.path.join(cur_scene_out_path, 'scene_%04d.json' % positions[b])
                _log(log, 'Saving scene to %s' % fout_path)
                with open(fout_path, 'w') as writer:
                    json.dump(dicts[b], writer)
        if keep_results:
            kept.append({'positions': list(positions), 'scene_graph': scene_graph, 'map_idx': map_idx, 'verdicts': verdicts,
                         'init_future_pred': init_future_pred, 'final_result_traj': optim_result_traj})
    print_metrics(metrics, freq_cnt, freq_total, log=lambda line: _log(log, line))
    return (freq_cnt, freq_total, kept) if keep_results else (freq_cnt, freq_total)


# ------------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------------

# name, type, default, what it is -- the reference's argument names and defaults (its src/refine_traffic_optim.py:34-82 and the base
# arguments it uses); lists are nargs='+', bool is a store_true flag
ARGUMENTS = (
    ('out', str, './out/traffic_out', 'where refine_traffic_log.txt and scenario_results/ go (used as given)'),
    ('ckpt', str, None, 'a save_state file with the traffic model\'s weights'),
    ('batch_size', int, 4, 'a batch is optimised as soon as its scenes hold this many agents'),
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
    ('feasibility_num', int, 1, 'a scene with fewer agents is skipped'),
    ('samp_future_len', int, 16, 'steps rolled out during the optimisation'),
    ('save_future_len', int, 12, 'steps of the result that are judged and saved'),
    ('loss_coll_veh', float, 100.0, 'weight of the vehicle-vehicle collision penalty'),
    ('loss_coll_env', float, 100.0, 'weight of the off-road penalty'),
    ('loss_init_z', float, 0.01, 'weight of the distance to the initial latent'),
    ('loss_motion_prior', float, 1.0, 'weight of the latent\'s likelihood under the prior'),
    ('num_iters', int, 10, 'optimisation iterations'),
    ('lr', float, 1.0, 'step size of the optimiser'),
    ('viz', bool, False, 'rendering; not available'),
    ('save', bool, False, 'write the scenario files'),
    ('device', str, 'cuda:0', 'torch device of model, data and maps'),
    ('seed', int, 0, 'seeds the shuffle and the latent draws'),
)


def get_parser(arguments=ARGUMENTS, description='Sample+optim motion model on a tracks file', optimiser_switch=True):
    """The command line of a driver from its ARGUMENTS table (``optimiser_switch``: this driver's ``--optim_use_lbfgs``)."""
    import argparse
    p = argparse.ArgumentParser(description=description)
    p.add_argument('-c', '--config', type=str, default=None, help='file of `key: value` lines; the command line wins over it')
    for name, kind, default, text in arguments:
        if kind is bool:
            p.add_argument('--' + name, action='store_true', default=default, help=text)
        elif isinstance(kind, list):
            p.add_argument('--' + name, type=kind[0], nargs='+', default=default, help=text)
        else:
            p.add_argument('--' + name, type=kind, default=default, help=text)
    if optimiser_switch:
        p.add_argument('--optim_use_lbfgs', dest='optim_use_adam', action='store_false', default=True,
                       help='LBFGS (20 inner iterations, strong-Wolfe line search) instead of Adam')
    return p


def parse_cfg(argv=None, arguments=ARGUMENTS, parser=None, ignored_keys=IGNORED_KEYS):
    """Defaults < ``--config`` file < command line, by the rules of ``train_traffic.parse_cfg``: an unknown key in the file is an
    error; the keys that describe the devkit's data or ask for rendering (IGNORED_KEYS) are accepted and ignored, and reported.  A
    flag is ``key: True`` / ``key: False`` in the file.  Returns the config dict and the ignored keys.  (``arguments``, ``parser``,
    ``ignored_keys``: another driver's table, the parser made from it and its ignored keys.)"""
    p = get_parser() if parser is None else parser
    argv = list(__import__('sys').argv[1:] if argv is None else argv)
    pre, _ = p.parse_known_args(argv)
    ignored, file_args = [], []
    if pre.config is not None:
        known = {a.dest: a for a in p._actions}
        # the parser's own switches, by the name they are written with (``--optim_use_lbfgs`` stores into ``optim_use_adam``)
        flags = {a.option_strings[-1].lstrip('-') for a in p._actions if a.nargs == 0 and isinstance(a.const, bool)}
        for k, v in read_config(pre.config):
            if k in ignored_keys:
                ignored.append(k)
                continue
            if k in flags:
                if v.lower() not in ('true', 'false'):
                    raise ValueError('%s: `%s` takes True or False' % (pre.config, k))
                if v.lower() == 'true':
                    file_args.append('--' + k)
                continue
            if k not in known or k in ('config', 'help', 'optim_use_adam'):
                raise ValueError('%s: unknown key `%s`' % (pre.config, k))
            if v[:1] == '[' and v[-1:] == ']':                 # a YAML list: [a, b]
                v = ' '.join(s.strip().strip('\'"') for s in v[1:-1].split(','))
            file_args += ['--' + k] + (v.split() if known[k].nargs in ('+', '*') else [v.strip('\'"')])
    cfg = vars(p.parse_args(file_args + argv))
    if cfg.get('agent_types') is not None:
        cfg['num_classes'] = len(cfg['agent_types'])
    return cfg, ignored


def main(argv=None, keep_results=False):
    """The command line.  Returns what ``run_one_epoch`` returns (``keep_results`` is handed on to it)."""
    from .constants import NUSC_BIKE_PARAMS
    from .eval_traffic_tracks import tracks_loader
    from .models.traffic_model import TrafficModel
    from .train_traffic import categories_for
    from .utils.torch import count_params, load_state
    cfg, ignored = parse_cfg(argv)
    if cfg['ckpt'] is None:
        raise SystemExit('Must pass in model weights to sample traffic! (--ckpt)')
    categories_for(cfg)
    os.makedirs(cfg['out'], exist_ok=True)
    with open(os.path.join(cfg['out'], 'refine_traffic_log.txt'), 'w') as log:
        _log(log, 'Args: ' + str(cfg))
        if ignored:
            _log(log, 'Ignoring config keys that describe the devkit\'s data or ask for rendering: ' + ', '.join(ignored))
        device = torch.device(cfg['device'])
        _log(log, 'Using device %s...' % str(device))
        torch.manual_seed(cfg['seed'])
        loader, map_env = tracks_loader({k: cfg[k] for k in ('tracks', 'scenario_path', 'maps', 'num_classes', 'past_len', 'future_len',
                                                             'seq_interval')}, device)
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
        loss_weights = {'coll_veh': cfg['loss_coll_veh'], 'coll_env': cfg['loss_coll_env'], 'motion_prior': cfg['loss_motion_prior'],
                        'init_z': cfg['loss_init_z']}
        model.train()
        return run_one_epoch(source, cfg['batch_size'], model, map_env, device, cfg['out'], loss_weights,
                             feasibility_NA=cfg['feasibility_num'], samp_future_len=cfg['samp_future_len'],
                             save_future_len=cfg['save_future_len'], optim_use_adam=cfg['optim_use_adam'], num_iters=cfg['num_iters'],
                             lr=cfg['lr'], viz=cfg['viz'], save=cfg['save'], log=log, keep_results=keep_results)


if __name__ == '__main__':
    main()
