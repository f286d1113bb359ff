"""Raster lookups with the reference's names (reference src/datasets/nuscenes_utils.py:205-390).
``get_map_obs`` and ``get_coll_point`` run the HIP gather kernels; the two small checks used only
outside the optimisation closure are torch glue."""
import numpy as np
import torch

from .. import ops


# The names strive_amd.dropin lays over the reference's datasets/nuscenes_utils.py.  The picture functions at the end of this file
# are not among them: next to a reference checkout its own matplotlib functions keep drawing.
__all__ = ['angle_diff', 'heading_change_rate', 'velocity', 'gen_car_coords', 'get_map_obs', 'get_coll_point', 'check_on_layer',
           'check_line_layer']


class _RawEnv(object):
    def __init__(self, maps, dx, bounds, L, W):
        self.nusc_raster, self.nusc_dx, self.bounds, self.L, self.W = maps, dx, list(bounds), L, W


def angle_diff(theta1, theta2):
    """Difference of two angle arrays folded into [-pi, pi) (reference :134-143), numpy in the arrays' own type: shifted by half
    a turn, reduced with the floored modulo, shifted back; what still exceeds pi loses a turn."""
    half_turn, turn = np.pi, 2 * np.pi
    folded = np.mod(theta1 - theta2 + half_turn, turn) - half_turn
    return np.where(folded > half_turn, folded - turn, folded)


def _lead_filled(diff, isnan):
    """Backward differences ``diff`` (one per frame pair) on the frames: frame 0 and every frame that follows a NaN frame take
    the forward difference instead -- except the last frame, which keeps its backward one (reference :155-171, :183-198)."""
    T = isnan.shape[0]
    k = np.maximum(np.arange(T) - 1, 0)
    lead = np.zeros((T,), dtype=bool)
    lead[1:] = isnan[:-1] & ~isnan[1:]
    lead[T - 1] = False
    k[lead] = np.arange(T)[lead]
    return diff[k]


def heading_change_rate(h, t):
    """(T) heading rates of angles that may be NaN (reference :145-171); host numpy, used for scenario files only -- the
    track records go through the HIP post-processing kernel, which restates the same rule."""
    return _lead_filled(angle_diff(h[1:], h[:-1]) / (t[1:] - t[:-1]), np.isnan(h))


def velocity(pos, t):
    """(T,D) velocities of positions that may be NaN (reference :173-199); host numpy, see heading_change_rate."""
    return _lead_filled((pos[1:, :] - pos[:-1, :]) / (t[1:] - t[:-1]).reshape((-1, 1)), np.isnan(np.sum(pos, axis=1)))


def gen_car_coords(xys, hs, C, L, W, bounds=None, ls=None, ws=None):
    """World coordinates (B,C,L,W,2) of a grid attached to each car (reference :205-232); torch glue."""
    B = hs.size(0)
    dev = hs.device
    if bounds is not None:
        lwise = torch.linspace(bounds[0], bounds[2], L, device=dev).view(1, 1, L, 1)
        wwise = torch.linspace(bounds[1], bounds[3], W, device=dev).view(1, 1, 1, W)
    elif ls is not None and ws is not None:
        lwise = torch.linspace(-1.0, 1.0, L, device=dev).view(1, 1, L, 1) * ls.view(B, 1, 1, 1) / 2
        wwise = torch.linspace(-1.0, 1.0, W, device=dev).view(1, 1, 1, W) * ws.view(B, 1, 1, 1) / 2
    else:
        raise ValueError('pass either bounds or ls and ws')
    hc, hsn = hs[:, 0].view(B, 1, 1, 1), hs[:, 1].view(B, 1, 1, 1)
    out = torch.stack((lwise * hc - wwise * hsn, lwise * hsn + wwise * hc), 4) + xys.view(B, 1, 1, 1, 2)
    return out.expand(B, C, L, W, 2)


def get_map_obs(maps, dx, frame, mapixes, bounds, L=256, W=256):
    """uint8 crop (B,C,L,W) in the frame of each car, bit-exact vs the reference (:234-264)."""
    return ops.map_crop(_RawEnv(maps, dx, bounds, L, W), frame, mapixes)


def _grid_size(dx, lw, half):
    mdx = torch.mean(dx) * (0.5 if half else 1.0)
    mlw = torch.mean(lw, dim=0)
    return torch.round(mlw[0] / mdx).int().item(), torch.round(mlw[1] / mdx).int().item()


def get_coll_point(drivables, dx, cars, lw, mapixes, return_iou=False):
    """Mean position of the non-drivable samples in each car box, NaN if none / all (reference :334-390).
    ``drivables`` is the (M,H,W) layer-0 view of the raster."""
    gl, gw = _grid_size(dx, lw, True)
    M, H, W = drivables.shape
    if drivables.is_contiguous():
        rast = drivables.view(M, 1, H, W)
    elif drivables.stride(2) == 1 and drivables.stride(1) == W and drivables.stride(0) % (H * W) == 0:
        # ``nusc_raster[:, 0]`` of a (M,C,H,W) raster: re-view the parent storage, no copy
        Cc = drivables.stride(0) // (H * W)
        rast = torch.as_strided(drivables, (M, Cc, H, W), (Cc * H * W, H * W, W, 1))
    else:
        rast = drivables.contiguous().view(M, 1, H, W)
    env = _RawEnv(rast, dx, [0, 0, 0, 0], 1, 1)
    pt, cnt = ops.coll_point(env, cars, lw, mapixes, gl, gw)
    if return_iou:
        frac = cnt.to(torch.float32) / float(gl * gw)
        frac = torch.where((cnt == 0) | (cnt == gl * gw), torch.full_like(frac, float('nan')), frac)
        return pt, frac
    return pt


def _pixels(xys, dx, mapixes, H, W):
    B = xys.shape[0]
    pix = torch.round(xys / dx[mapixes].view(B, *([1] * (xys.dim() - 2)), 2)).long()
    outside = (pix[..., 1] < 0) | (pix[..., 1] >= H) | (pix[..., 0] < 0) | (pix[..., 0] >= W)
    pix[outside] = 0
    return pix


def check_on_layer(drivables, dx, cars, lw, mapixes):
    """Fraction of the car box on pixels marked 1 (reference :266-298); torch glue."""
    L, W = _grid_size(dx, lw, False)
    B = cars.size(0)
    xys = gen_car_coords(cars[:, :2], cars[:, 2:], 1, L, W, ls=lw[:, 0], ws=lw[:, 1])[:, 0]
    pix = _pixels(xys, dx, mapixes, drivables.shape[1], drivables.shape[2])
    m = mapixes.view(B, 1, 1).expand(B, L, W)
    return torch.sum(drivables[m, pix[..., 1], pix[..., 0]].float(), dim=[1, 2]) / (L * W)


def check_line_layer(drivables, dx, start, end, mapixes):
    """True where the segment crosses a 0 pixel (reference :300-332); torch glue."""
    B = start.size(0)
    n = torch.max(torch.round(torch.norm(start - end, dim=-1) / torch.mean(dx)).int()).item()
    w = torch.linspace(0.0, 1.0, n).view(1, n, 1).to(start.device)
    pts = start.view(B, 1, 2) * (1.0 - w) + end.view(B, 1, 2) * w
    pix = torch.round(pts / dx[mapixes].view(B, 1, 2)).long()
    m = mapixes.view(B, 1).expand(B, n)
    return torch.sum(drivables[m, pix[..., 1], pix[..., 0]] == 0, dim=-1) > 0


# ------------------------------------------------------------------------------------------------------------------------
# pictures of a live batch (reference :477-653)
# ------------------------------------------------------------------------------------------------------------------------

def create_video(img_path_form, out_path, fps):
    """The reference's ffmpeg command (:623-630), in a fresh child process."""
    import subprocess
    subprocess.run(['ffmpeg', '-y', '-r', str(fps), '-i', img_path_form, '-vcodec', 'libx264', '-crf', '18', '-pix_fmt', 'yuv420p', out_path])


def viz_scene_graphs(scene_graph, map_idx, map_env, calls, state_normalizer, att_normalizer, mp4=False, fps=2, workers=None, log=print,
                     ptr=None):
    """Any number of ``viz_scene_graph`` calls on ONE batch -- ``calls``: dicts of that function's arguments from ``bidx`` on
    (``bidx`` and ``out_path`` required) -- served by ONE table launch (strive_scene_draw_tables), ONE render launch and ONE
    read-back; then the PNG files are written on a thread pool (render.write_pngs).  The batch is not written.  -> the number of
    pictures.  ``ptr``: the batch's scene offsets on the host, where the caller has them (otherwise the batch's own host copy, or
    one read-back).  ``mp4``: run the reference's ffmpeg command per frame directory and remove the frames, as the reference does;
    without it the frames stay as PNG files."""
    import shutil
    from .. import render, scene_draw
    render.check_ffmpeg(mp4)
    paths, pictures, videos = scene_draw.draw_calls(scene_graph, map_idx, map_env, calls, state_normalizer, att_normalizer, ptr=ptr)
    for path in paths:
        log('saving %s' % path)
    render.write_pngs(paths, pictures, workers)
    if mp4:
        import os
        for vdir in videos:
            create_video(os.path.join(vdir, 'frame%04d.png'), vdir + '.mp4', fps)
            shutil.rmtree(vdir)
    return len(paths)


def viz_scene_graph(scene_graph, map_idx, map_env, bidx, out_path, state_normalizer, att_normalizer, future_pred=None, aidx=None,
                    viz_traj=False, make_video=True, show_gt=False, traj_color_val=None, traj_color_bounds=None,
                    viz_bounds=[-17.0, -38.5, 60.0, 38.5], center_viz=False, car_colors=None, show_gt_idx=None, crop_t=None, ow_gt=None,
                    mp4=False):
    """Pictures of scene ``bidx`` of a NORMALISED batch (reference :477-621, same arguments and defaults): ``<out_path>.png`` and,
    with ``make_video``, the frames ``<out_path>_%03d/frame%04d.png`` of every sample (kept as PNG files unless ``mp4``).  Drawn on
    the device (``viz_scene_graphs`` with one call); the batch is left as it is, where the reference unnormalises it in place and
    normalises it back.  ``traj_color_val`` / ``traj_color_bounds`` are not offered."""
    call = dict(bidx=bidx, out_path=out_path, future_pred=future_pred, aidx=aidx, viz_traj=viz_traj, make_video=make_video, show_gt=show_gt,
                traj_color_val=traj_color_val, traj_color_bounds=traj_color_bounds, viz_bounds=viz_bounds, center_viz=center_viz,
                car_colors=car_colors, show_gt_idx=show_gt_idx, crop_t=crop_t, ow_gt=ow_gt)
    return viz_scene_graphs(scene_graph, map_idx, map_env, [call], state_normalizer, att_normalizer, mp4=mp4)
