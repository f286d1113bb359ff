"""Pictures (and video frames) of a directory of scenario files, rendered on the device (reference src/viz_scenario_dir.py).

    python -m strive_amd.viz_scenario_dir --scenarios DIR --out OUT [--viz_video] [--mp4] --map_world synthetic

Every scene gives ``OUT/<name>.png`` -- all trajectories over the map crop around the ego -- and with ``--viz_video`` the frames
``OUT/<name>_vid_000/frame%04d.png``.  The pictures of up to ``--batch_scenes`` scenes are rendered in one kernel launch and read
back once (strive_amd.render); ``OUT`` is used as given."""
import os

import torch

from . import render
from .datasets.utils import read_adv_scenes


def plan_scenario(scene, map_env, out_path, L=720, W=720, video=False):
    """What the reference's viz_scenario (src/viz_scenario_dir.py:53-107) draws, as a plan for render.render_plans: the crop around
    the ego at step T // 2 (T the number of past steps, as there), bounds = the largest centroid offset at that step."""
    if L != W:
        raise ValueError('only square pictures are rendered (L == W)')
    scene_past = scene['scene_past'][:, :, :4]
    scene_fut = scene['scene_fut']
    lw = scene['veh_att']
    T = scene_past.size(1)
    crop_pos = scene_fut[0:1, T // 2, :2]
    centroid_states = scene_fut[:, T // 2, :2] - crop_pos
    bound_max = torch.amax(torch.abs(centroid_states)).item()
    bounds = [-bound_max, -bound_max, bound_max, bound_max]
    scene_traj = torch.cat([scene_past, scene_fut], dim=1)
    NA, NT, _ = scene_traj.size()
    map_idx = map_env.map_list.index(scene['map'])
    crop_kin = torch.cat([crop_pos, torch.tensor([[1.0, 0.0]])], dim=1)
    crop_traj, crop_lw = render.objs2crop(crop_kin[0], scene_traj.reshape(NA * NT, 4), lw, bounds, L, W)
    crop_traj = crop_traj.reshape(NA, NT, 4)
    pictures = [(out_path + '.png', render.build_draw_list(crop_traj, crop_lw, viz_traj=True, traj_markers=[False] * NA), 0)]
    videos = []
    if video:
        pictures += [(p, dl, 0) for p, dl in zip(render.video_frame_paths(out_path + '_vid', NT), render.frame_draw_lists(crop_traj, crop_lw))]
        videos.append(out_path + '_vid_000')
    return {'crop_kin': crop_kin[0], 'mapix': map_idx, 'bounds': bounds, 'pictures': pictures, 'videos': videos}


def viz_scenario(scene, map_env, out_path, L=720, W=720, video=False, mp4=False):
    render.check_ffmpeg(mp4)
    return render.render_plans([plan_scenario(scene, map_env, out_path, L, W, video)], map_env, L, mp4=mp4)


def viz_scenario_dir(cfg, map_env=None):
    """Every ``*.json`` of ``cfg['scenarios']`` into ``cfg['out']`` (reference :109-138)."""
    render.check_ffmpeg(cfg.get('mp4', False))
    if not os.path.exists(cfg['scenarios']):
        raise SystemExit('Could not find scenario_dir %s!' % cfg['scenarios'])
    os.makedirs(cfg['out'], exist_ok=True)
    scenes = read_adv_scenes(cfg['scenarios'])
    print('Loaded:')
    print([s['name'] for s in scenes])
    if map_env is None:
        map_env = synthetic_map_world(cfg.get('device', 'cuda:0'))
    L = int(cfg.get('L', 720))
    step = max(1, int(cfg.get('batch_scenes', 36)))
    n = 0
    for i in range(0, len(scenes), step):
        plans = [plan_scenario(s, map_env, os.path.join(cfg['out'], s['name']), L, L, cfg.get('viz_video', False)) for s in scenes[i:i + step]]
        n += render.render_plans(plans, map_env, L, mp4=cfg.get('mp4', False))
    return n


def synthetic_map_world(device):
    from .eval_adv_gen import SyntheticMapWorld
    env = SyntheticMapWorld()
    env.nusc_raster, env.nusc_dx = env.nusc_raster.to(device), env.nusc_dx.to(device)
    return env


def get_parser():
    import argparse
    p = argparse.ArgumentParser(description='Viz scenarios')
    p.add_argument('--out', type=str, default='./out/viz_scenarios_out', help='directory to save the pictures to (used as given)')
    p.add_argument('--scenarios', type=str, required=True, help='directory with scenario json files')
    p.add_argument('--viz_video', action='store_true', help='also render one frame per step')
    p.add_argument('--mp4', action='store_true', help='turn the frames into <out>_vid_000.mp4 with ffmpeg and remove them')
    p.add_argument('--map_world', type=str, default=None, choices=['synthetic'], help='map environment with the rasters')
    p.add_argument('--maps', type=str, default=None, help='a maps file (datasets/maps.py) with the maps the scenes name, instead of --map_world')
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--L', type=int, default=720, help='picture edge in pixels')
    p.add_argument('--batch_scenes', type=int, default=36, help='scenes per kernel launch')
    return p


def parse_cfg(argv=None):
    return vars(get_parser().parse_args(argv))


def main(argv=None):
    cfg = parse_cfg(argv)
    render.check_ffmpeg(cfg['mp4'])
    from .eval_traffic_tracks import maps_file_env, one_map_source, scenario_map_names
    one_map_source(cfg, 'map_world')
    if cfg['map_world'] is None and cfg['maps'] is None:
        raise SystemExit('viz_scenario_dir: the nuScenes devkit and data are not available here; pass a map environment from Python '
                         '(viz_scenario_dir(cfg, map_env)) or use --map_world synthetic')
    print('Args: ' + str(cfg))
    if cfg['maps'] is not None:
        return viz_scenario_dir(cfg, maps_file_env(cfg['maps'], scenario_map_names(cfg['scenarios']), cfg['device']))
    return viz_scenario_dir(cfg)


if __name__ == '__main__':
    main()
