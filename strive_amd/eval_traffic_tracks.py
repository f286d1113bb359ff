"""Model evaluation (``test_traffic.run_one_epoch``) on the scene dataset of a tracks file and / or a scenario directory:

    python -m strive_amd.eval_traffic_tracks --ckpt CKPT --tracks FILE [--scenario_path DIR] --test_recon_coll_rate ... --out OUT

takes test_traffic's arguments and writes the same report to ``OUT/test_log.txt``; the options that describe synthetic scenes
(``--scenes``, ``--num_scenes``, ``--scene_sizes``, ``--seed``) are refused.  It is a module of its own because
``strive_amd/test_traffic.py`` is one of the files every change here is measured with and therefore stays as it is; all it adds to
that file's ``main`` is where the loader comes from.  The scenes live on the maps of ``--maps FILE`` (a maps file, datasets/maps.py)
or, without it, on the maps of ``synth.make_raster`` that the tracks file names ('synthetic-<m>'); batches come from ``NuScenesDataset.loader`` (datasets/nuscenes_dataset.py), assembled on the device; the model
takes the dataset's normalisers.
"""
import os
import time

import torch

from . import test_traffic as TT


SYNTHETIC_ONLY = ('scenes', 'num_scenes', 'scene_sizes', 'seed')


def maps_file_env(path, needed, device, load_lanegraph=False):
    """Map environment of ``--maps FILE`` (datasets/maps.py ``map_env_from_file``: rasters and, with ``load_lanegraph``, lane graphs
    built on the device).  ``needed``: the map names the scenes carry; one that the file lacks ends the run with a message naming it."""
    from .datasets.maps import load_maps, map_env_from_file
    try:
        mf = load_maps(path)
    except ValueError as e:
        raise SystemExit('--maps: %s' % e)
    for name in needed:
        if name not in mf.names:
            raise SystemExit('--maps %s has no map named %r (it holds: %s)' % (path, name, ', '.join(mf.names)))
    return map_env_from_file(mf, load_lanegraph=load_lanegraph, device=device)


def scenario_map_names(*dirs):
    """The map names of the scenario files (``*.json``) in the directories, in order of appearance; a missing directory has none."""
    import glob
    import json
    names = []
    for d in dirs:
        for path in sorted(glob.glob(os.path.join(d, '*.json'))):
            with open(path, 'r') as f:
                jd = json.load(f)
            if jd is not None and jd['map'] not in names:
                names.append(jd['map'])
    return names


def one_map_source(cfg, other):
    """``--maps`` and the driver's synthetic world (``--map_world`` / ``--lane_world``) both name the map environment."""
    if cfg.get('maps') is not None and cfg.get(other) is not None:
        raise SystemExit('--maps and --%s both name the map environment: pass one of them' % other)


def tracks_loader(cfg, device):
    """(loader, map_env) of ``cfg['tracks']`` and / or ``cfg['scenario_path']``; ``loader.dataset`` is the NuScenesDataset.  The maps
    are those of ``cfg['maps']`` (a maps file, datasets/maps.py; lane graphs with ``cfg['load_lanegraph']``) or, without it, the
    synthetic ones."""
    from . import synth
    from .datasets.nuscenes_dataset import NuScenesDataset
    from .datasets.tracks import load_tracks
    from .datasets.utils import NUSC_NORM_STATS, read_adv_scenes
    if cfg.get('tracks') is None and cfg.get('scenario_path') is None:
        raise SystemExit('eval_traffic_tracks needs --tracks FILE and / or --scenario_path DIR')
    by_count = {len(k): list(k) for k in NUSC_NORM_STATS}          # the category sets that have normalisation statistics
    if cfg.get('num_classes', 2) not in by_count:
        raise SystemExit('--num_classes %d: normalisation statistics exist for %s categories' % (cfg['num_classes'], sorted(by_count)))
    cats = by_count[cfg.get('num_classes', 2)]
    tr = load_tracks(cfg['tracks']) if cfg.get('tracks') is not None else None
    maps = list(tr['scene_map']) if tr is not None else []
    if cfg.get('scenario_path') is not None:
        maps += [sc['map'] for sc in read_adv_scenes(cfg['scenario_path'])]
    if cfg.get('maps') is not None:
        map_env = maps_file_env(cfg['maps'], maps, device, load_lanegraph=bool(cfg.get('load_lanegraph', False)))
    else:
        nmaps = 1 + max([int(m.rsplit('-', 1)[1]) for m in maps if m.startswith('synthetic-')] + [0])
        raster, dx = synth.make_raster(M=nmaps)
        map_env = synth.SyntheticMapEnv(raster, dx).to(device)
    ds = NuScenesDataset(tr, map_env, categories=cats, npast=cfg.get('past_len', 4), nfuture=cfg.get('future_len', 12),
                         seq_interval=cfg.get('seq_interval', 1), scenario_path=cfg.get('scenario_path'), device=device)
    return ds.loader(cfg.get('batch_size', 8)), map_env


def get_parser():
    p = TT.get_parser()
    p.description = 'Test motion model on a tracks file'
    for a in [a for a in p._actions if a.dest in SYNTHETIC_ONLY]:      # refused: they describe test_traffic's synthetic scenes
        a.help, a.default = 'not used here', None
    p.add_argument('--tracks', type=str, default=None, help='the tracks file (datasets/tracks.py)')
    p.add_argument('--scenario_path', type=str, default=None, help='a directory of scenario files appended to the scenes')
    p.add_argument('--maps', type=str, default=None, help='a maps file (datasets/maps.py) with the maps the scenes name; default: the synthetic maps')
    return p


def main(argv=None):
    from .constants import NUSC_BIKE_PARAMS
    from .losses.traffic_model import TrafficModelLoss
    from .models.traffic_model import TrafficModel
    from .utils.torch import count_params, load_state
    cfg = vars(get_parser().parse_args(argv))
    given = [k for k in SYNTHETIC_ONLY if cfg[k] is not None]
    if given:
        raise SystemExit('eval_traffic_tracks takes its scenes from --tracks / --scenario_path: --%s does not apply' % given[0])
    os.makedirs(cfg['out'], exist_ok=True)
    with open(os.path.join(cfg['out'], 'test_log.txt'), 'w') as log:
        TT._log(log, 'Args: ' + str(cfg))
        device = torch.device(cfg['device'])
        TT._log(log, 'Using device %s...' % str(device))
        loader, map_env = tracks_loader(cfg, device)
        model = TrafficModel(cfg['past_len'], cfg['future_len'], cfg['map_obs_size_pix'], cfg['num_classes'],
                             latent_size=cfg['latent_size']).to(device)
        loss_fn = TrafficModelLoss({'recon': 1.0, 'kl': 1.0, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0}).to(device)
        ckpt_epoch, _ = load_state(cfg['ckpt'], model, map_location=device)
        TT._log(log, 'Loaded checkpoint from epoch %d...' % ckpt_epoch)
        TT._log(log, 'Num model params: %d' % count_params(model))
        model.set_normalizer(loader.dataset.get_state_normalizer())
        model.set_att_normalizer(loader.dataset.get_att_normalizer())
        model.set_bicycle_params(NUSC_BIKE_PARAMS)
        model.eval()
        start_t = time.time()
        flags = ('test_recon_viz_multi', 'test_recon_coll_rate', 'test_sample_viz_multi', 'test_sample_viz_rollout', 'test_sample_disp_err',
                 'test_sample_coll_rate', 'test_sample_num', 'test_sample_future_len')
        epoch_metrics = TT.run_one_epoch(loader, model, map_env, loss_fn, device, cfg['out'], log=log, **{k: cfg[k] for k in flags})
        TT._log(log, 'Test time: %f s' % (time.time() - start_t))
    return epoch_metrics


if __name__ == '__main__':
    main()
