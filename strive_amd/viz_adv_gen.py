"""Qualitative evaluation of generated scenarios, rendered on the device (reference src/eval_adv_gen.py:523-640).

    python -m strive_amd.viz_adv_gen --scenarios DIR --out OUT --viz_res adv_sol_success --viz_stage init adv sol --map_world synthetic

``OUT/<category>/<scene>/viz_<stage>.png`` (and ``viz_init_map.png``, and with ``--viz_video`` the frames
``viz_<stage>_vid_000/frame%04d.png``), the pictures of up to ``--batch_scenes`` scenes per kernel launch (strive_amd.render)."""
import os

import numpy as np
import torch

from . import render
from .eval_adv_gen import read_adv_scenes

STAGES = ['init', 'adv', 'sol']


def plan_scenario(scene, stage, map_env, out_path, L=720, W=720, video=False):
    """What the reference's viz_scenario (src/eval_adv_gen.py:537-640) draws for one stage, as a plan for render.render_plans, or
    None where it draws nothing ('sol' of a scene without ``fut_sol``).  The crop is the same for every stage: centred on the mean
    of the collision position, the ego's first position and the attacker's first observed position."""
    assert stage in STAGES
    if L != W:
        raise ValueError('only square pictures are rendered (L == W)')
    viz_out_path = os.path.join(out_path, 'viz_' + stage)
    scene_past = scene['past'][:, :, :4]
    if stage == 'sol' and 'fut_sol' not in scene:
        return None
    scene_fut = scene['fut_' + stage]
    lw = scene['veh_att']
    atk_agt = scene['attack_agt'] if 'attack_agt' in scene else 0
    atk_t = scene['attack_t'] if 'attack_t' in scene else scene_fut.size(1) // 2
    atk_past_idx = torch.nonzero(~torch.isnan(scene_past[atk_agt, :, 0]), as_tuple=True)[0][0]
    pts = [scene['fut_adv'][0, atk_t, :2], scene_past[0, 0, :2], scene_past[atk_agt, atk_past_idx, :2]]
    crop_pos = (pts[0] + pts[1] + pts[2]) / 3
    bound_diffs = torch.cat([p - crop_pos for p in pts], dim=0)
    bound_max = max(30.0, torch.amax(torch.abs(bound_diffs)).item() + 5.0)
    bounds = [-bound_max, -bound_max, bound_max, bound_max]
    scene_traj = torch.cat([scene_past, scene_fut], dim=1)
    NA, NT, _ = scene_traj.size()
    map_idx = map_env.map_list.index(scene['map'])
    crop_kin = torch.cat([crop_pos.unsqueeze(0), torch.tensor([[1.0, 0.0]])], dim=1)
    crop_traj, crop_lw = render.objs2crop(crop_kin[0], scene_traj.reshape(NA * NT, 4), lw, bounds, L, W)
    crop_traj = crop_traj.reshape(NA, NT, 4)
    colors, alphas, widths, msizes = render.get_adv_coloring(NA, atk_agt if stage != 'init' else None, 0, alpha=True, linewidth=True,
                                                             markersize=True)
    # the others first, then the ego, the attacker last
    order = np.arange(NA)
    order = order[order != atk_agt][1:]
    order = np.concatenate([order, [0, atk_agt]]).astype(np.int64)
    pick = lambda v: [v[i] for i in order]
    crop_traj, crop_lw = crop_traj[order], crop_lw[order]
    colors, alphas, widths, msizes = pick(colors), pick(alphas), pick(widths), pick(msizes)
    pictures = []
    if stage == 'init':
        pictures.append((viz_out_path + '_map.png', [], 0))
    pictures.append((viz_out_path + '.png',
                     render.build_draw_list(crop_traj, crop_lw, viz_traj=True, color=colors, alpha=alphas, traj_linewidth=widths,
                                            traj_markers=[False] * len(order), traj_markersize=msizes), 0))
    videos = []
    if video:
        frames = render.frame_draw_lists(crop_traj, crop_lw, color=colors)
        pictures += [(p, dl, 0) for p, dl in zip(render.video_frame_paths(viz_out_path + '_vid', NT), frames)]
        videos.append(viz_out_path + '_vid_000')
    return {'crop_kin': crop_kin[0], 'mapix': map_idx, 'bounds': bounds, 'pictures': pictures, 'videos': videos}


def viz_scenario(scene, stage, map_env, out_path, L=720, W=720, video=False, mp4=False):
    render.check_ffmpeg(mp4)
    plan = plan_scenario(scene, stage, map_env, out_path, L, W, video)
    return 0 if plan is None else render.render_plans([plan], map_env, L, mp4=mp4)


def qual_eval(scenarios, viz_res, viz_stage, map_env, out_path, viz_video=False, L=720, batch_scenes=36, mp4=False):
    """(reference :523-535) ``scenarios``: {category: scenes}; 'sol' is skipped for ``adv_failed``."""
    render.check_ffmpeg(mp4)
    n = 0
    for resname in viz_res:
        scenes = scenarios[resname]
        for i in range(0, len(scenes), max(1, int(batch_scenes))):
            plans = []
            for scene in scenes[i:i + max(1, int(batch_scenes))]:
                scene_path = os.path.join(out_path, resname, scene['name'])
                os.makedirs(scene_path, exist_ok=True)
                for stage in viz_stage:
                    if resname == 'adv_failed' and stage == 'sol':
                        continue
                    plan = plan_scenario(scene, stage, map_env, scene_path, L, L, viz_video)
                    if plan is not None:
                        plans.append(plan)
            n += render.render_plans(plans, map_env, L, mp4=mp4)
    return n


def get_parser():
    import argparse
    p = argparse.ArgumentParser(description='Qualitative evaluation of generated scenarios')
    p.add_argument('--out', type=str, default='./out/eval_adv_gen_out', help='output directory (used as given)')
    p.add_argument('--scenarios', type=str, required=True, help='directory with adv_failed, adv_sol_success and sol_failed')
    p.add_argument('--viz_res', type=str, nargs='+', default=['adv_sol_success'], choices=['adv_sol_success', 'sol_failed', 'adv_failed'])
    p.add_argument('--viz_stage', type=str, nargs='+', default=['adv'], choices=STAGES)
    p.add_argument('--viz_video', action='store_true', help='also render one frame per step')
    p.add_argument('--mp4', action='store_true', help='turn the frames into .mp4 with ffmpeg and remove them')
    p.add_argument('--map_world', type=str, default=None, choices=['synthetic'], help='map environment with the rasters')
    p.add_argument('--maps', type=str, default=None, help='a maps file (datasets/maps.py) with the maps the scenes name, instead of --map_world')
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--L', type=int, default=720, help='picture edge in pixels')
    p.add_argument('--batch_scenes', type=int, default=36, help='scenes per kernel launch')
    return p


def main(argv=None):
    cfg = vars(get_parser().parse_args(argv))
    render.check_ffmpeg(cfg['mp4'])
    from .eval_traffic_tracks import maps_file_env, one_map_source, scenario_map_names
    one_map_source(cfg, 'map_world')
    if cfg['map_world'] is None and cfg['maps'] is None:
        raise SystemExit('viz_adv_gen: the nuScenes devkit and data are not available here; pass a map environment from Python '
                         '(qual_eval(scenarios, viz_res, viz_stage, map_env, out)) or use --map_world synthetic')
    if not os.path.exists(cfg['scenarios']):
        raise SystemExit('Could not find scenario_dir %s!' % cfg['scenarios'])
    from .viz_scenario_dir import synthetic_map_world
    scenarios = {}
    for resname in cfg['viz_res']:
        res_path = os.path.join(cfg['scenarios'], resname)
        scenarios[resname] = read_adv_scenes(res_path) if os.path.exists(res_path) else []
    if cfg['maps'] is not None:
        world = maps_file_env(cfg['maps'], scenario_map_names(*[os.path.join(cfg['scenarios'], r) for r in cfg['viz_res']]), cfg['device'])
    else:
        world = synthetic_map_world(cfg['device'])
    return qual_eval(scenarios, cfg['viz_res'], cfg['viz_stage'], world, cfg['out'],
                     viz_video=cfg['viz_video'], L=cfg['L'], batch_scenes=cfg['batch_scenes'], mp4=cfg['mp4'])


if __name__ == '__main__':
    main()
