"""Quantitative evaluation of a trained traffic model (reference src/test_traffic.py:84-277): reconstruction loss and errors at the
posterior mean, best-of-N displacement errors and sample diversity, and the map / vehicle collision rates of reconstructions and
of prior samples.

Differences in HOW, not in what is reported:

* Every batch is encoded ONCE (``_encode_once``): one ``embed``, one decode at the posterior mean that serves both the
  reference's ``model(..., use_post_mean=True)`` and ``model.reconstruct(...)`` (the same kernels on the same inputs), and the
  sampled rollout starts from that embed's map / past features and prior.
* The metric functions of the reference map onto at most two launches of ``strive_traffic_eval_metrics`` per batch
  (``traffic_eval_metrics``): the mean rollout as one sample (err, plus env and veh with ``test_recon_coll_rate``) and the
  samples (disp, env, veh).
* Host batches are moved through pinned, non-blocking copies, their scene structure is taken from the host copies
  (``ops.prime_scene_info``), and a loss that offers ``dense_terms`` (``TrafficModelLoss``) is asked for its terms dense with
  a mask instead of compacted; a batch that arrives already on the device has its scene offsets read back once by the model.
* Nothing is read back inside the batch loop: every metric key has a float64 (sum, count) accumulator on the device, masked
  sums over the dense outputs replace the reference's compaction, the collision counters stay on the device, and the kernel's
  statuses are checked after the last batch (a non-zero status raises ``ValueError`` naming the batch and the scene).

``python -m strive_amd.test_traffic --ckpt CKPT --scenes synthetic --test_recon_coll_rate --test_sample_disp_err
--test_sample_coll_rate --out OUT`` writes the reference's report to ``OUT/test_log.txt``.
"""
import os
import time

import torch

from . import _lib as L
from . import ops
from .eval_common import LIN_MAX, host_stats, i32, lin_table, outputs, pack_env
from .losses.common import log_normal

G_ERR, G_DISP, G_VEH, G_ENV, G_GRID_GIVEN = 1, 2, 4, 8, 16
DISP_KEYS = ('pos_minADE', 'pos_minFDE', 'ang_minADE', 'ang_minFDE', 'APD')
STATUS_TEXT = {2: 'agent offsets leave the arrays', 3: 'map index out of range',
               4: 'the drivable-area sampling grid is outside 1..%d samples per axis' % LIN_MAX}


def traffic_eval_metrics(pred, ptr, lw, state_normalizer, att_normalizer, gt=None, vis=None, map_env=None, mapix=None,
                         err=False, disp=False, veh=False, env=False, env_ego_only=True, grid=None, out=None, lib=None, stats=None):
    """The raw kernel on one prediction set: ``pred`` (NA,NS,T,4), ``gt`` (NA,Tg,6) and ``lw`` (NA,2) NORMALISED, ``vis`` (NA,Tg),
    ``ptr`` (B+1), ``map_env`` + ``mapix`` (B) for ``env``.  Returns a dict of tensors on ``pred``'s device and reads nothing back:
    ``pos_err``, ``ang_err`` (NA,Tg) float64 [err]; ``disp`` (B,5) float64 in the order of DISP_KEYS [disp]; ``did_collide_veh``
    (NA,NS) int32 [veh]; ``did_collide_map`` (B,NS) or (NA,NS) int32, ``grid_i`` (3) = L, W, valid rows and ``grid_d`` (2) = the
    ratios L and W were rounded from [env]; ``status`` (B) int32 (STATUS_TEXT).  ``grid=(L, W)`` uses that sampling grid instead of
    forming it from the batch; ``out`` supplies output buffers (a group that is not asked for leaves its buffers untouched);
    ``stats = host_stats(...)`` replaces the two normalisers (loops convert them once)."""
    lib = ops._lib_for(pred) if lib is None else lib
    dev = pred.device
    if pred.dim() != 4 or pred.shape[3] != 4:
        raise ValueError('traffic_eval_metrics expects pred (NA,NS,T,4)')
    pred = pred.detach().to(torch.float32).contiguous()
    NA, NS, T = int(pred.shape[0]), int(pred.shape[1]), int(pred.shape[2])
    ptr = i32(ptr, dev)
    B = int(ptr.numel()) - 1
    if B < 0 or NS < 1 or T < 1:
        raise ValueError('traffic_eval_metrics expects ptr (B+1), NS >= 1 and T >= 1')
    lw = lw.detach().to(device=dev, dtype=torch.float32).reshape(NA, 2).contiguous()
    Tg = T
    if gt is not None:
        gt = gt.detach().to(device=dev, dtype=torch.float32).contiguous()
        Tg = int(gt.shape[1])
        if gt.dim() != 3 or gt.shape[0] != NA or gt.shape[2] != 6:
            raise ValueError('gt must be (NA,Tg,6)')
    if vis is not None:
        vis = vis.detach().to(device=dev, dtype=torch.float32).reshape(NA, Tg).contiguous()
    if (err or disp) and gt is None or err and vis is None:
        raise ValueError('err needs gt and vis, disp needs gt')
    if err and T != Tg:
        raise ValueError('err compares pred and gt step by step: T %d != Tg %d' % (T, Tg))
    if env and (map_env is None or mapix is None):
        raise ValueError('env needs map_env and mapix')
    nan = float('nan')
    spec = [('pos_err', (NA, Tg), torch.float64, nan), ('ang_err', (NA, Tg), torch.float64, nan)] if err else []
    spec += [('disp', (B, 5), torch.float64, nan)] if disp else []
    spec += [('did_collide_veh', (NA, NS), torch.int32, 0)] if veh else []
    spec += [('did_collide_map', (B if env_ego_only else NA, NS), torch.int32, 0), ('grid_i', (3,), torch.int32, 0),
             ('grid_d', (2,), torch.float64, nan)] if env else []
    out = outputs(out, dev, spec + [('status', (B,), torch.int32, 0)])
    map_ref = lin = mapix_t = None
    groups = (G_ERR if err else 0) | (G_DISP if disp else 0) | (G_VEH if veh else 0) | (G_ENV if env else 0)
    if env:
        if grid is not None:
            groups |= G_GRID_GIVEN
            for i, v in enumerate((int(grid[0]), int(grid[1]), 1)):          # (fills are launches: no staging copy, no synchronisation)
                out['grid_i'][i:i + 1].fill_(v)
        map_ref = ops._map_pack(pack_env(map_env), dev).ref()
        lin = lin_table(dev)
        mapix_t = i32(mapix, dev, B)
    if B == 0 or groups == 0:
        return out
    if NA == 0:                                        # never hand a NULL pointer to the library
        pred = torch.zeros((1, NS, T, 4), dtype=torch.float32, device=dev)
        lw = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    p = lambda key: L.ptr(out[key]) if key in out else None
    sm, ss, am, as_ = host_stats(state_normalizer, att_normalizer) if stats is None else stats
    lib.call('strive_traffic_eval_metrics', L.ptr(pred), L.ptr(gt), L.ptr(vis), L.ptr(ptr), L.ptr(lw), sm, ss, am, as_,
             map_ref, L.ptr(mapix_t), L.ptr(lin), LIN_MAX, groups, 1 if env_ego_only else 0, B, NA, NS, T, Tg,
             p('pos_err') if err else None, p('ang_err') if err else None, p('disp') if disp else None,
             p('did_collide_veh') if veh else None, p('did_collide_map') if env else None, p('grid_i') if env else None,
             p('grid_d') if env else None, p('status'), L.stream_ptr(pred))
    return out


def _encode_once(model, scene_graph, map_idx, map_env, num_samples=0, nfuture=None):
    """What the reference computes with ``model(..., use_post_mean=True)``, ``model.reconstruct(...)`` and
    ``model.sample_batched(..., include_mean=False)`` (reference src/models/traffic_model.py:178-257, :319-370) from ONE embed:
    returns ``(pred, sample_pred)``; ``pred`` serves as the reference's ``recon_pred`` too, ``sample_pred`` is None for
    ``num_samples == 0``.  The noise is drawn by ``model.rsample`` exactly as ``sample_batched`` draws it."""
    emb = model.embed(scene_graph, map_idx, map_env)
    pmu, pvar = emb['prior_out']
    qmu, qvar = emb['posterior_out']
    pred = {'prior_out': (pmu, pvar), 'posterior_out': (qmu, qvar),
            'future_pred': model.decoder(scene_graph, emb['map_feat'], emb['past_feat'], qmu, map_idx, map_env)}
    if num_samples <= 0:
        return pred, None
    NA, NS, D = pmu.size(0), num_samples, model.z_size
    smu = pmu.view(1, NA, D).expand(NS, NA, D)
    svar = pvar.view(1, NA, D).expand(NS, NA, D)
    z = model.rsample(smu, svar)
    fut = model.decoder(scene_graph, emb['map_feat'], emb['past_feat'], z.transpose(0, 1), map_idx, map_env, nfuture=nfuture)
    dist = torch.distributions.Normal(smu, torch.sqrt(svar), validate_args=False)
    sample_pred = {'prior_out': (pmu, pvar), 'z_samp': z.transpose(0, 1), 'future_pred': fut,
                   'z_logprob': dist.log_prob(z).sum(dim=-1).transpose(0, 1),
                   'z_mdist': torch.norm((z - smu) / torch.sqrt(svar), dim=-1).transpose(0, 1)}
    return pred, sample_pred


def _to_device(obj, device, keep=()):
    """``obj.to(device)`` in place for a graph (or a tensor), host tensors going through pinned staging copies and non-blocking
    transfers (``params.upload``): a pageable copy would block the host once per tensor.  Returns the moved object and the HOST
    copies of the attributes named in ``keep`` (None where the attribute was on a device already)."""
    from . import params
    if torch.is_tensor(obj):
        return params.upload(obj, device), {}
    host = {}
    for k in obj.keys():
        v = obj[k]
        if torch.is_tensor(v):
            if k in keep:
                host[k] = None if v.is_cuda else v
            obj[k] = params.upload(v, device)
    return obj, host


class _Accumulators(object):
    """float64 (sum, count) per metric key and integer counters, all on the device, in the order the keys first appear."""

    def __init__(self, device):
        self.device = device
        self.sums, self.counts, self.freq = {}, {}, {}

    def add(self, key, values, mask=None):
        v = values.detach().to(torch.float64)
        if mask is None:
            s, c = v.sum(), torch.full((), v.numel(), dtype=torch.int64, device=v.device)
        else:
            s, c = torch.where(mask, v, torch.zeros_like(v)).sum(), mask.sum()
        if key not in self.sums:
            self.sums[key] = torch.zeros((), dtype=torch.float64, device=self.device)
            self.counts[key] = torch.zeros((), dtype=torch.int64, device=self.device)
        self.sums[key] += s
        self.counts[key] += c

    def count(self, key, value):
        if key not in self.freq:
            self.freq[key] = torch.zeros((), dtype=torch.int64, device=self.device)
        self.freq[key] += value


def _log(log, line):
    print(line)
    if log is not None:
        log.write(line + '\n')
        log.flush()


def run_one_epoch(data_loader, model, map_env, loss_fn, device, out_path,
                  test_recon_viz_multi=False,
                  test_recon_coll_rate=False,
                  test_sample_viz_multi=False,
                  test_sample_viz_rollout=False,
                  test_sample_disp_err=False,
                  test_sample_coll_rate=False,
                  test_sample_num=3,
                  test_sample_future_len=None,
                  use_challenge_splits=False,
                  log=None, per_batch=None):
    """Run through ``data_loader`` -- any iterable of ``(scene_graph, map_idx)`` -- and report what the reference reports
    (reference src/test_traffic.py:84-277), in its key order and line formats.  Returns the ``epoch_metrics`` dict (the reference
    returns nothing).  ``log``: an open text file that receives the lines too; ``per_batch``: a list that receives, per batch,
    the dict of device tensors the batch produced (tests).  The three ``*_viz_*`` flags render and are not available."""
    if test_recon_viz_multi or test_sample_viz_multi or test_sample_viz_rollout:
        raise NotImplementedError('the viz flags render scenes with matplotlib and the nuScenes map API; rendering is not part of '
                                  'strive_amd')
    device = torch.device(device)
    acc = _Accumulators(device)
    statuses = []
    want_samples = test_sample_disp_err or test_sample_coll_rate
    sn, an = model.get_normalizer(), model.get_att_normalizer()
    stats = host_stats(sn, an)
    for bi, (scene_graph, map_idx) in enumerate(data_loader):
        with torch.no_grad():
            scene_graph, host = _to_device(scene_graph, device, keep=('ptr', 'edge_index'))
            map_idx, _ = _to_device(map_idx, device)
            if host.get('ptr') is not None and '_strive_scene_info' not in scene_graph.__dict__:
                ops.prime_scene_info(scene_graph, host['ptr'], host.get('edge_index'))       # structure from the host copies
            B, NA = int(map_idx.size(0)), int(scene_graph.past.size(0))
            pred, sample_pred = _encode_once(model, scene_graph, map_idx, map_env, test_sample_num if want_samples else 0,
                                             test_sample_future_len)
            rec = {}
            # a loss with dense_terms (TrafficModelLoss) gives the same terms without the compaction its forward synchronises
            # for; any other callable is called as the reference calls it
            if hasattr(loss_fn, 'dense_terms'):
                loss_dict, loss_masks = loss_fn.dense_terms(scene_graph, pred)
            else:
                loss_dict, loss_masks = loss_fn(scene_graph, pred), {}
            for k in [k for k in loss_dict if k == 'loss'] + [k for k in loss_dict if k != 'loss']:     # the reference's order
                if loss_dict[k] is not None:
                    acc.add(k, loss_dict[k], loss_masks.get(k))
                    rec[k] = loss_dict[k]
            # the mean rollout as one "sample": compute_err, and the reconstruction's collision rates
            m = traffic_eval_metrics(pred['future_pred'].unsqueeze(1), scene_graph.ptr, scene_graph.lw, sn, an, gt=scene_graph.future_gt,
                                     vis=scene_graph.future_vis, map_env=map_env, mapix=map_idx, err=True, veh=test_recon_coll_rate,
                                     env=test_recon_coll_rate, env_ego_only=True, stats=stats)
            statuses.append(m['status'])
            vis = scene_graph.future_vis == 1.0
            acc.add('pos_err', m['pos_err'], vis)
            acc.add('ang_err', m['ang_err'], vis)
            pmu, pvar = pred['prior_out']
            qmu = pred['posterior_out'][0]
            rec['z_logprob'] = log_normal(qmu, pmu, pvar)
            rec['z_mdist'] = torch.norm((qmu - pmu) / torch.sqrt(pvar), dim=-1)
            acc.add('z_logprob', rec['z_logprob'])
            acc.add('z_mdist', rec['z_mdist'])
            rec.update({'recon/' + k: v for k, v in m.items()})
            if test_recon_coll_rate:
                acc.count('recon_num_coll_map', m['did_collide_map'].sum())
                acc.count('recon_num_traj_map', B)
                acc.count('recon_num_coll_veh', m['did_collide_veh'].sum())
                acc.count('recon_num_traj_veh', NA)
            if want_samples:
                NS = int(sample_pred['future_pred'].size(1))
                s = traffic_eval_metrics(sample_pred['future_pred'], scene_graph.ptr, scene_graph.lw, sn, an, gt=scene_graph.future_gt,
                                         map_env=map_env, mapix=map_idx, disp=test_sample_disp_err, veh=test_sample_coll_rate,
                                         env=test_sample_coll_rate, env_ego_only=True, stats=stats)
                statuses.append(s['status'])
                rec.update({'sample/' + k: v for k, v in s.items()})
                rec['sample/future_pred'] = sample_pred['future_pred']
                if test_sample_disp_err:
                    for c, k in enumerate(DISP_KEYS):
                        acc.add(k, s['disp'][:, c])
                if test_sample_coll_rate:
                    acc.count('sample_num_coll_map', s['did_collide_map'].sum())
                    acc.count('sample_num_traj_map', NS * B)
                    acc.count('sample_num_coll_veh', s['did_collide_veh'].sum())
                    acc.count('sample_num_traj_veh', NS * NA)
            if per_batch is not None:
                rec['future_pred'] = pred['future_pred']
                per_batch.append(rec)

    # ---- the one read-back ----
    keys = list(acc.sums.keys())
    fkeys = list(acc.freq.keys())
    host, freq = {}, {}
    if statuses:
        scalars = [acc.sums[k] for k in keys] + [acc.counts[k] for k in keys] + [acc.freq[k] for k in fkeys]
        vals = torch.cat([t.reshape(-1).to(torch.float64) for t in scalars + statuses]).cpu().tolist()
        nk, nf = len(keys), len(fkeys)
        host = {k: (vals[i], vals[nk + i]) for i, k in enumerate(keys)}
        freq = {k: vals[2 * nk + i] for i, k in enumerate(fkeys)}
        o = 2 * nk + nf
        calls_per_batch = 2 if want_samples else 1
        for ci, t in enumerate(statuses):
            for sc in range(int(t.numel())):
                code = int(vals[o + sc])
                if code != 0:
                    raise ValueError('batch %d, scene %d: %s (status %d of strive_traffic_eval_metrics, %s rollout)' % (
                        ci // calls_per_batch, sc, STATUS_TEXT.get(code, 'refused'), code,
                        'sampled' if ci % calls_per_batch == 1 else 'mean'))
            o += int(t.numel())

    epoch_metrics = {}
    for k in keys:
        s, c = host[k]
        epoch_metrics['Test Mean ' + k] = s / c if c > 0 else float('nan')
    used_prefixes = [p for p, on in (('recon_', test_recon_coll_rate), ('sample_', test_sample_coll_rate)) if on]
    for pref in used_prefixes:
        for post in ('_map', '_veh'):
            if pref + 'num_coll' + post in freq:
                epoch_metrics['Test (%s, %s) Collision Freq' % (pref, post)] = freq[pref + 'num_coll' + post] / freq[pref + 'num_traj' + post]
    _log(log, 'Final ===================================== ')
    for k, v in epoch_metrics.items():
        _log(log, '%s = %f' % (k, v))
    return epoch_metrics


class _SyntheticLoader(object):
    """``--scenes synthetic``: ``num_scenes`` scenes of ``synth.make_batch`` with LO..HI agents, ``batch_size`` scenes per batch."""

    def __init__(self, num_scenes, scene_sizes, batch_size, seed, nmaps=1, past_len=4, future_len=12, num_classes=2):
        from . import synth
        lo, hi = int(scene_sizes[0]), int(scene_sizes[1])
        sizes = (lo + (synth.counter_uniform((num_scenes,), 'test_traffic/sizes/%d' % seed) * (hi - lo + 1)).astype(int)).tolist()
        self.batches = [(sizes[i:i + batch_size], 'test_traffic/%d/%d' % (seed, i)) for i in range(0, num_scenes, batch_size)]
        self.nmaps, self.kw = nmaps, dict(PT=past_len, FT=future_len, NC=num_classes)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        from . import synth
        for sizes, key in self.batches:
            yield synth.make_batch(sizes, key=key, M=self.nmaps, **self.kw)


def get_parser():
    import argparse
    p = argparse.ArgumentParser(description='Test motion model')
    p.add_argument('--out', type=str, default='./out/test_traffic_out', help='output directory (test_log.txt)')
    p.add_argument('--ckpt', type=str, required=True, help='checkpoint written by save_state (utils/torch.py)')
    p.add_argument('--batch_size', type=int, default=8, help='scenes per batch')
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--scenes', type=str, default=None, choices=['synthetic'], help='where the scenes come from')
    p.add_argument('--num_scenes', type=int, default=16)
    p.add_argument('--scene_sizes', type=int, nargs=2, default=[2, 8], metavar=('LO', 'HI'), help='agents per scene')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--past_len', type=int, default=4)
    p.add_argument('--future_len', type=int, default=12)
    p.add_argument('--map_obs_size_pix', type=int, default=256)
    p.add_argument('--latent_size', type=int, default=32)
    p.add_argument('--num_classes', type=int, default=2, help='semantic classes of the agents (the reference: len(categories))')
    for flag, text in (('test_recon_viz_multi', 'rendering; not available'), ('test_recon_coll_rate', 'collision rates of reconstructions'),
                       ('test_sample_viz_multi', 'rendering; not available'), ('test_sample_viz_rollout', 'rendering; not available'),
                       ('test_sample_disp_err', 'min displacement errors (ADE, FDE, angle versions) and APD over the samples'),
                       ('test_sample_coll_rate', 'collision rates of the prior samples')):
        p.add_argument('--' + flag, action='store_true', help=text)
    p.add_argument('--test_sample_num', type=int, default=3, help='futures to sample from the prior')
    p.add_argument('--test_sample_future_len', type=int, default=None, help='steps to sample instead of future_len')
    return p


def main(argv=None):
    from . import synth
    from .constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors
    from .datasets.utils import MeanStdNormalizer
    from .losses.traffic_model import TrafficModelLoss
    from .models.traffic_model import TrafficModel
    from .utils.torch import count_params, load_state
    cfg = vars(get_parser().parse_args(argv))
    if cfg['scenes'] is None:
        raise SystemExit('test_traffic: the nuScenes loader is not part of strive_amd; call run_one_epoch(loader, model, map_env, ...) '
                         'from Python with your own iterable of (scene_graph, map_idx), or use --scenes synthetic')
    os.makedirs(cfg['out'], exist_ok=True)
    with open(os.path.join(cfg['out'], 'test_log.txt'), 'w') as log:
        _log(log, 'Args: ' + str(cfg))
        device = torch.device(cfg['device'])
        _log(log, 'Using device %s...' % str(device))
        raster, dx = synth.make_raster()
        map_env = synth.SyntheticMapEnv(raster, dx).to(device)
        loader = _SyntheticLoader(cfg['num_scenes'], cfg['scene_sizes'], cfg['batch_size'], cfg['seed'], past_len=cfg['past_len'],
                                  future_len=cfg['future_len'], num_classes=cfg['num_classes'])
        model = TrafficModel(cfg['past_len'], cfg['future_len'], cfg['map_obs_size_pix'], cfg['num_classes'],
                             latent_size=cfg['latent_size']).to(device)
        loss_fn = TrafficModelLoss({'recon': 1.0, 'kl': 1.0, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0}).to(device)
        ckpt_epoch, _ = load_state(cfg['ckpt'], model, map_location=device)
        _log(log, 'Loaded checkpoint from epoch %d...' % ckpt_epoch)
        _log(log, 'Num model params: %d' % count_params(model))
        model.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
        model.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
        model.set_bicycle_params(NUSC_BIKE_PARAMS)
        model.eval()
        start_t = time.time()
        epoch_metrics = run_one_epoch(loader, model, map_env, loss_fn, device, cfg['out'],
                                      test_recon_viz_multi=cfg['test_recon_viz_multi'], test_recon_coll_rate=cfg['test_recon_coll_rate'],
                                      test_sample_viz_multi=cfg['test_sample_viz_multi'],
                                      test_sample_viz_rollout=cfg['test_sample_viz_rollout'],
                                      test_sample_disp_err=cfg['test_sample_disp_err'], test_sample_coll_rate=cfg['test_sample_coll_rate'],
                                      test_sample_num=cfg['test_sample_num'], test_sample_future_len=cfg['test_sample_future_len'], log=log)
        _log(log, 'Test time: %f s' % (time.time() - start_t))
    return epoch_metrics


if __name__ == '__main__':
    main()
