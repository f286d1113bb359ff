"""Pictures of a trained model on the scene dataset of a tracks file and / or a scenario directory:

    python -m strive_amd.viz_traffic_tracks --ckpt CKPT --tracks FILE [--scenario_path DIR] [--maps FILE] --out OUT
        [--test_recon_viz_multi] [--test_sample_viz_multi] [--test_sample_viz_rollout] [--test_sample_num N]
        [--test_sample_future_len T] [--max_scenes K] [--mp4]

the three picture sets of the reference's test_traffic (reference src/test_traffic.py:139-208), under its names:
``OUT/viz_recon_multi/test_recon_multi_%08d_pred.png`` (reconstruction over the ground truth),
``OUT/viz_sample_multi/test_sample_multi_%08d_pred.png`` (all samples) and
``OUT/viz_sample_rollout/test_sample_rollout_%08d_pred.png`` with its frame directories ``..._pred_%03d/frame%04d.png`` (bounds
[-45, -45, 45, 45] around the scene's centroid).  It is a module of its own, like eval_traffic_tracks: ``strive_amd/test_traffic.py``
stays as it is and keeps refusing these flags.  Loader, maps and model set-up are eval_traffic_tracks'.  Per batch: one
``reconstruct`` and / or one ``sample_batched``, then ONE table launch, ONE render launch and ONE read-back for every picture of every
scene (datasets/nuscenes_utils.py ``viz_scene_graphs``); the scene offsets come from the batch's host copy.
"""
import argparse
import os

import torch

from . import eval_traffic_tracks as ETT

VIZ_FLAGS = ('test_recon_viz_multi', 'test_sample_viz_multi', 'test_sample_viz_rollout')
ROLLOUT_BOUNDS = [-45.0, -45.0, 45.0, 45.0]


def get_parser():
    p = argparse.ArgumentParser(description='Draw a motion model\'s reconstructions, samples and roll-outs on a tracks file')
    p.add_argument('--out', type=str, default='./out/viz_traffic_out', help='output directory')
    p.add_argument('--ckpt', type=str, required=True, help='checkpoint written by save_state (utils/torch.py)')
    p.add_argument('--tracks', type=str, default=None, help='the tracks file (datasets/tracks.py)')
    p.add_argument('--scenario_path', type=str, default=None, help='a directory of scenario files appended to the scenes')
    p.add_argument('--maps', type=str, default=None, help='a maps file (datasets/maps.py); default: the synthetic maps')
    p.add_argument('--batch_size', type=int, default=8, help='scenes per batch')
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--past_len', type=int, default=4)
    p.add_argument('--future_len', type=int, default=12)
    p.add_argument('--map_obs_size_pix', type=int, default=256)
    p.add_argument('--latent_size', type=int, default=32)
    p.add_argument('--num_classes', type=int, default=2)
    p.add_argument('--test_recon_viz_multi', action='store_true', help='the reconstruction of every scene over its ground truth')
    p.add_argument('--test_sample_viz_multi', action='store_true', help='the samples of every scene')
    p.add_argument('--test_sample_viz_rollout', action='store_true', help='the samples of every scene, frame by frame')
    p.add_argument('--test_sample_num', type=int, default=3, help='futures to sample from the prior')
    p.add_argument('--test_sample_future_len', type=int, default=None, help='steps to sample instead of future_len')
    p.add_argument('--max_scenes', type=int, default=None, help='stop after this many scenes')
    p.add_argument('--L', type=int, default=None, help='picture size in pixels (default: the map environment\'s crop size)')
    p.add_argument('--mp4', action='store_true', help='encode every frame directory with ffmpeg and remove the frames')
    return p


def batch_calls(cfg, out, data_idx, B, recon_pred, sample_pred):
    """The reference's viz_scene_graph calls of one batch of B scenes (src/test_traffic.py:139-208), scene by scene per picture set."""
    calls = []
    for bidx in range(B):
        idx = data_idx + bidx
        if cfg['test_recon_viz_multi']:
            calls.append(dict(bidx=bidx, out_path=os.path.join(out, 'viz_recon_multi', 'test_recon_multi_%08d_pred' % idx),
                              future_pred=recon_pred, viz_traj=True, make_video=False, show_gt=True))
        if cfg['test_sample_viz_multi']:
            calls.append(dict(bidx=bidx, out_path=os.path.join(out, 'viz_sample_multi', 'test_sample_multi_%08d_pred' % idx),
                              future_pred=sample_pred, viz_traj=True, make_video=False, show_gt=False))
        if cfg['test_sample_viz_rollout']:
            calls.append(dict(bidx=bidx, out_path=os.path.join(out, 'viz_sample_rollout', 'test_sample_rollout_%08d_pred' % idx),
                              future_pred=sample_pred, viz_traj=False, make_video=True, viz_bounds=ROLLOUT_BOUNDS, center_viz=True))
    return calls


def viz_batches(cfg, loader, model, map_env, log=print):
    """-> the number of pictures written for ``loader``'s batches (at most ``cfg['max_scenes']`` scenes)."""
    from . import scene_draw
    from .datasets import nuscenes_utils as nutils
    draw_env = map_env if cfg.get('L') is None else _SizedEnv(map_env, cfg['L'])      # the model keeps reading map_env's own crops
    sn, an = model.get_normalizer(), model.get_att_normalizer()
    data_idx, written = 0, 0
    for scene_graph, map_idx in loader:
        with torch.no_grad():
            ptr = scene_draw.host_ptr(scene_graph)
            B = int(ptr.shape[0]) - 1
            if cfg.get('max_scenes') is not None:
                B = min(B, cfg['max_scenes'] - data_idx)
            if B <= 0:
                break
            recon_pred = sample_pred = None
            if cfg['test_recon_viz_multi']:
                recon_pred = model.reconstruct(scene_graph, map_idx, map_env)['future_pred']
            if cfg['test_sample_viz_multi'] or cfg['test_sample_viz_rollout']:
                sample_pred = model.sample_batched(scene_graph, map_idx, map_env, cfg['test_sample_num'], include_mean=False,
                                                   nfuture=cfg['test_sample_future_len'])['future_pred']
            calls = batch_calls(cfg, cfg['out'], data_idx, B, recon_pred, sample_pred)
            written += nutils.viz_scene_graphs(scene_graph, map_idx, draw_env, calls, sn, an, mp4=cfg.get('mp4', False), log=log, ptr=ptr)
            data_idx += B
    return written


class _SizedEnv(object):
    """``map_env`` with another picture size: the rasters are shared."""

    def __init__(self, env, L_):
        self.__dict__.update(env.__dict__)
        self.L = self.W = int(L_)


def main(argv=None):
    from . import render
    from .constants import NUSC_BIKE_PARAMS
    from .models.traffic_model import TrafficModel
    from .utils.torch import load_state
    cfg = vars(get_parser().parse_args(argv))
    if not any(cfg[k] for k in VIZ_FLAGS):
        raise SystemExit('viz_traffic_tracks draws nothing without one of --%s' % ', --'.join(VIZ_FLAGS))
    if cfg['max_scenes'] is not None and cfg['max_scenes'] < 1:
        raise SystemExit('--max_scenes is at least 1')
    if cfg['test_sample_num'] < 1:
        raise SystemExit('--test_sample_num is at least 1')
    render.check_ffmpeg(cfg['mp4'])
    device = torch.device(cfg['device'])
    loader, map_env = ETT.tracks_loader(cfg, device)
    model = TrafficModel(cfg['past_len'], cfg['future_len'], cfg['map_obs_size_pix'], cfg['num_classes'],
                         latent_size=cfg['latent_size']).to(device)
    load_state(cfg['ckpt'], model, map_location=device)
    model.set_normalizer(loader.dataset.get_state_normalizer())
    model.set_att_normalizer(loader.dataset.get_att_normalizer())
    model.set_bicycle_params(NUSC_BIKE_PARAMS)
    model.eval()
    os.makedirs(cfg['out'], exist_ok=True)
    n = viz_batches(cfg, loader, model, map_env)
    print('%d pictures written under %s' % (n, cfg['out']))
    return n


if __name__ == '__main__':
    main()
