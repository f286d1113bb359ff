"""Scenario pictures without matplotlib: the host layer of strive_render_pictures (include/strive_hip.h).

``build_draw_list`` lists what the reference's ``viz_map_crop`` puts on its axes for given trajectories (reference
src/datasets/nuscenes_utils.py:655-702, :733-853), in the order matplotlib draws it; ``render_pictures`` renders any number of such
lists over their map crops in ONE kernel launch; ``write_png`` encodes a picture with zlib alone.  Nothing here imports matplotlib
or PIL.  The coverage rule is the library's own (4 x 4 sub-samples, stated in the header), not Agg's."""
import ctypes as C
import struct
import zlib

import numpy as np
import torch

from . import _lib as L
from . import ops

# ---- colours (matplotlib's CSS4 names and its default property cycle, as the reference uses them) ----
COLORS = {
    'white': '#FFFFFF', 'black': '#000000', 'k': '#000000', 'darkgray': '#A9A9A9', 'coral': '#FF7F50', 'orange': '#FFA500',
    'gold': '#FFD700', 'lightblue': '#ADD8E6', 'cornflowerblue': '#6495ED', 'orangered': '#FF4500', 'lawngreen': '#7CFC00',
}
COLOR_CYCLE = ['#1f77b4', '#ff7f0e', '#2ca02c', '#d62728', '#9467bd', '#8c564b', '#e377c2', '#7f7f7f', '#bcbd22']
MAP_COLORS = ['darkgray', 'coral', 'orange', 'gold', 'lightblue', 'lightblue']        # render_map_observation (:719-720)
MAP_ALPHAS = [1.0, 0.6, 0.6, 0.6, 1.0, 0.5]
MAX_LAYERS = 6

# Strokes and markers arrive in points, as in the reference.  The reference's figure (dpi=200, tight_layout, bbox_inches='tight')
# shows a 720-unit crop on axes 900 pixels wide (measured with matplotlib 3.10.8): one point is 200/72
# figure pixels = (200/72) 720/900 crop units.
PX_PER_PT = (200.0 / 72.0) * 720.0 / 900.0


def px_per_pt(L_):
    """Picture pixels per point for an L-pixel picture: the reference's axes stay 900 figure pixels wide whatever the crop's L."""
    return PX_PER_PT * float(L_) / 720.0


_figure_px_per_pt = px_per_pt          # render_pictures has an argument of that name


EDGE_PT = 1.0            # plot_box: plt.fill(..., linewidth=1.0)
HEADING_PT = 1.5         # plot_box: plt.plot(arrow, 'k') at rcParams['lines.linewidth']
MARKER_EDGE_PT = 1.0     # scatter strokes its markers in the face colour, 1 pt wide (recorded in fixture g24)

KIND_CAR, KIND_POLYLINE, KIND_DISC = 0, 1, 2
PRIM_FLOATS = 16

# gist_rainbow's anchors (matplotlib's public colour map data): x, (r, g, b); 256-entry table, linear between the anchors
_GIST_RAINBOW = ((0.000, (1.00, 0.00, 0.16)), (0.030, (1.00, 0.00, 0.00)), (0.215, (1.00, 1.00, 0.00)), (0.400, (0.00, 1.00, 0.00)),
                 (0.586, (0.00, 1.00, 1.00)), (0.770, (0.00, 0.00, 1.00)), (0.954, (1.00, 0.00, 1.00)), (1.000, (1.00, 0.00, 0.75)))


def plt_color(i):
    """Entry i of the default colour cycle (reference :713-715)."""
    return COLOR_CYCLE[i]


def to_rgb(color):
    """(r, g, b) floats in [0, 1] of a colour name of the table, a '#rrggbb' string or a 3/4-tuple."""
    if isinstance(color, str):
        h = COLORS.get(color, color)
        if not (h.startswith('#') and len(h) == 7):
            raise ValueError('unknown colour %r' % (color,))
        return tuple(int(h[i:i + 2], 16) / 255.0 for i in (1, 3, 5))
    c = tuple(float(v) for v in color)
    if len(c) not in (3, 4):
        raise ValueError('a colour is a name, #rrggbb or an (r, g, b) tuple')
    return c[:3]


def gist_rainbow(x):
    """The colours scatter(c=x, cmap='gist_rainbow', norm=Normalize(0, 1)) gives: a 256-entry table indexed by int(256 x)."""
    xs = np.array([a[0] for a in _GIST_RAINBOW])
    grid = np.linspace(0.0, 1.0, 256)
    lut = np.stack([np.interp(grid, xs, np.array([a[1][k] for a in _GIST_RAINBOW])) for k in range(3)], axis=1)
    ix = np.clip((np.asarray(x, dtype=np.float64) * 256).astype(np.int64), 0, 255)
    return lut[ix]


def get_adv_coloring(NA, attack_agt, tgt_agt, alpha=False, linewidth=False, markersize=False, cycle_color=False):
    """Colours (and, on request, alphas, line widths and marker sizes) of NA agents with the attacker in orangered and the target in
    lawngreen (reference src/datasets/nuscenes_utils.py:434-476)."""
    base = [plt_color(n % 9) for n in range(NA)] if cycle_color else ['cornflowerblue'] * NA
    if attack_agt is not None:
        base[attack_agt] = 'orangered'
    if tgt_agt is not None:
        base[tgt_agt] = 'lawngreen'
    out = [base]

    def table(common, special):
        t = [common] * NA
        for a in (attack_agt, tgt_agt):
            if a is not None:
                t[a] = special
        return t
    if alpha:
        out.append(table(1.0, 1.0))
    if linewidth:
        out.append(table(2.5, 3.5))
    if markersize:
        out.append(table(10.0, 15.0))
    return out[0] if len(out) == 1 else tuple(out)


def objs2crop(center, obj_center, obj_lw, bounds, L_, W_):
    """Objects (N, 4) x, y, hx, hy and sizes (n, 2) in the pixel frame of the crop around ``center`` (x, y, hx, hy): the reference's
    values (src/datasets/map_env.py:231-254 with objects2frame, src/datasets/nuscenes_utils.py:398-414), in the input's precision."""
    ctr = center.detach().cpu().numpy()
    obj = obj_center.detach().cpu().numpy()
    theta = np.arctan2(ctr[3], ctr[2])
    cos, sin = np.cos(theta), np.sin(theta)
    rot = np.array([[cos, -sin], [sin, cos]])                      # get_rot(theta).T
    loc = np.dot(obj[:, :2] - ctr[:2].reshape(1, 2), rot)
    newh = np.arctan2(obj[:, 3], obj[:, 2]) - theta
    local = np.concatenate([loc, np.stack((np.cos(newh), np.sin(newh)), 1)], axis=1)
    sl = L_ / float(bounds[2] - bounds[0])
    sw = W_ / float(bounds[3] - bounds[1])
    local[:, 0] -= bounds[0]
    local[:, 1] -= bounds[1]
    local[:, 0] *= sl
    local[:, 1] *= sw
    pix_lw = torch.stack([obj_lw[:, 0] * sl, obj_lw[:, 1] * sw], dim=1)
    return torch.from_numpy(local), pix_lw


# ------------------------------------------------------------------------------------------------------------------------
# what the reference puts on the axes
# ------------------------------------------------------------------------------------------------------------------------

def _car(kin, lw, color, alpha):
    return {'kind': 'car', 'center': (float(kin[0]), float(kin[1])), 'heading': (float(kin[2]), float(kin[3])),
            'l': float(lw[0]), 'w': float(lw[1]), 'color': to_rgb(color), 'alpha': float(alpha)}


def _obj_observation(markers, lines, cars, car_kin, car_lw, viz_traj, viz_init_car, color, alpha, traj_linewidth, traj_markers,
                     traj_markersize):
    """render_obj_observation (:733-835) without color_traj: appends to the three z-order groups in insertion order."""
    kin = car_kin.detach().cpu()
    lw = car_lw.detach().cpu()
    if kin.dim() == 3:
        kin = kin.unsqueeze(1)
    elif kin.dim() != 4:
        raise ValueError('car_kin is (NA, T, 4) or (NA, NS, T, 4)')
    NA, NS, T, _ = kin.shape
    col = lambda n: color[n] if color is not None else plt_color(n % 9)
    if viz_traj:
        if traj_markers is None:
            traj_markers = [True] * NA
        for n in range(NA):
            for s in range(NS):
                valid = torch.sum(torch.isnan(kin[n, s]), dim=1) == 0
                pts = kin[n, s][valid][:, :2].numpy().astype(np.float64)
                carr = np.linspace(0, 1.0, T)[valid.numpy()]
                a = alpha[n] if alpha is not None else 0.7
                width = traj_linewidth[n] if traj_linewidth is not None else 1.0
                msize = traj_markersize[n] if traj_markersize is not None else 8.0
                if pts.shape[0] > 0:
                    lines.append({'kind': 'line', 'verts': pts, 'color': to_rgb(col(n)), 'alpha': float(a), 'linewidth': float(width)})
                mcol = gist_rainbow(carr) if traj_markers[n] else np.tile(np.array(to_rgb(col(n))), (pts.shape[0], 1))
                markers.append({'kind': 'markers', 'verts': pts, 'colors': mcol, 'alpha': float(a), 'size': float(msize)})
        if viz_init_car:
            for n in range(NA):
                for s in range(1):                      # the initial car of sample 0 only (:807)
                    nonnan = torch.nonzero(~torch.isnan(kin[n, s, :, 0]), as_tuple=True)[0]
                    if nonnan.numel() == 0:
                        raise IndexError('agent %d has no observed step (the reference fails here as well)' % n)
                    cars.append(_car(kin[n, s, int(nonnan[0])], lw[n], col(n), alpha[n] if alpha is not None else 0.7))
    else:
        for n in range(NA):
            for s in range(NS):
                for t in range(T):
                    if int(torch.sum(torch.isnan(kin[n, s, t]))) == 0:
                        a = alpha[n] if alpha is not None else 0.7
                        a = a if t == 0 else 0.1 + (1.0 - (float(t) / T)) * 0.2
                        cars.append(_car(kin[n, s, t], lw[n], col(n), a))


def build_draw_list(car_kin, car_lw, gt_kin=None, viz_traj=False, color=None, alpha=None, traj_linewidth=None, traj_markers=None,
                    traj_markersize=None):
    """The artists viz_map_crop (reference :655-702) draws over the map for these arguments, as a list of dicts in matplotlib's
    draw order (by z-order, then insertion): markers (1), lines (2), cars (3).
      {'kind': 'markers', 'verts' (n, 2), 'colors' (n, 3), 'alpha', 'size' (points^2)}
      {'kind': 'line', 'verts' (n, 2), 'color', 'alpha', 'linewidth' (points)}
      {'kind': 'car', 'center', 'heading', 'l', 'w', 'color', 'alpha'}         (fill, 1 pt black outline, 1.5 pt black heading)
    ``color_traj`` is not offered."""
    markers, lines, cars = [], [], []
    if gt_kin is not None and car_lw is not None:
        _obj_observation(markers, lines, cars, gt_kin, car_lw, viz_traj, False, ['white'] * gt_kin.size(0), None, None, None, None)
    if car_kin is not None and car_lw is not None:
        _obj_observation(markers, lines, cars, car_kin, car_lw, viz_traj, True, color, alpha, traj_linewidth, traj_markers,
                         traj_markersize)
    return markers + lines + cars


def pack_draw_lists(draw_lists, k=PX_PER_PT):
    """-> (prims (NP, 16) float32, verts (NV, 2) float32, ranges (F, 2) int32): the tables of strive_render_pictures; ``k``: picture
    pixels per point."""
    recs, verts, ranges, nv = [], [], [], 0

    def rec(kind, rgb, alpha):
        r = np.zeros((PRIM_FLOATS,), dtype=np.float32)
        r[0:1].view(np.int32)[0] = kind
        r[7:10] = rgb
        r[10] = alpha
        return r
    for dl in draw_lists:
        begin = len(recs)
        for a in dl:
            if a['kind'] == 'car':
                r = rec(KIND_CAR, a['color'], a['alpha'])
                r[1:3], r[3:5], r[5], r[6] = a['center'], a['heading'], a['l'], a['w']
                r[11], r[12] = a.get('edge_px', EDGE_PT * k), a.get('heading_px', HEADING_PT * k)
                recs.append(r)
            elif a['kind'] == 'line':
                v = np.asarray(a['verts'], dtype=np.float32).reshape(-1, 2)
                r = rec(KIND_POLYLINE, a['color'], a['alpha'])
                r[11] = a['width_px'] if 'width_px' in a else a['linewidth'] * k
                r[13:15].view(np.int32)[:] = (nv, nv + v.shape[0])
                verts.append(v)
                nv += v.shape[0]
                recs.append(r)
            elif a['kind'] == 'markers':
                v = np.asarray(a['verts'], dtype=np.float32).reshape(-1, 2)
                d = a['diameter_px'] if 'diameter_px' in a else (np.sqrt(a['size']) + MARKER_EDGE_PT) * k
                for i in range(v.shape[0]):
                    r = rec(KIND_DISC, a['colors'][i], a['alpha'])
                    r[1:3], r[5] = v[i], d
                    recs.append(r)
            else:
                raise ValueError('unknown artist kind %r' % (a['kind'],))
        ranges.append((begin, len(recs)))
    prims = np.stack(recs, axis=0) if recs else np.zeros((0, PRIM_FLOATS), dtype=np.float32)
    vt = np.concatenate(verts, axis=0) if verts else np.zeros((0, 2), dtype=np.float32)
    return prims, vt, np.array(ranges, dtype=np.int32).reshape(-1, 2)


def render_tables(map_env, crop_kin, mapix, bounds, L_, prims, verts, ranges, no_map=None, W_=None):
    """One launch of strive_render_pictures over ready tables -> (F, L, L, 3) uint8 on the map's device.  ``bounds``: one list of 4
    for all pictures or one per picture."""
    if W_ is not None and int(W_) != int(L_):
        raise ValueError('only square pictures are rendered (L == W): the reference mixes the two axes otherwise')
    raster = map_env.nusc_raster
    dev = raster.device
    lib = ops._lib_for(raster)
    M, Cc, H, W = raster.shape
    if Cc > MAX_LAYERS:
        raise ValueError('the map has %d layers; the colour list has %d' % (Cc, MAX_LAYERS))
    L_ = int(L_)
    F = int(crop_kin.shape[0])
    mapix = np.asarray(torch.as_tensor(mapix).cpu(), dtype=np.int64).reshape(F)
    if F and (mapix.min() < 0 or mapix.max() >= M):
        raise ValueError('map index out of range')
    if bounds and not isinstance(bounds[0], (list, tuple)):
        bounds = [bounds] * F
    ranges = np.asarray(ranges, dtype=np.int32).reshape(F, 2)
    prims = np.ascontiguousarray(prims, dtype=np.float32).reshape(-1, PRIM_FLOATS)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 2)
    if F and (ranges.min() < 0 or ranges.max() > prims.shape[0]):
        raise ValueError('primitive range out of the table')
    # the crop's fp32 tables, once per distinct set of bounds
    lin_of, lin, lin_ix = {}, [], []
    for b in bounds:
        key = tuple(float(v) for v in b)
        if key not in lin_of:
            lin_of[key] = len(lin)
            lin.append(torch.stack([torch.linspace(key[0], key[2], L_), torch.linspace(key[1], key[3], L_)]))
        lin_ix.append(lin_of[key])
    # every host table in one buffer, one upload
    i32 = np.concatenate([mapix.astype(np.int32), np.array(lin_ix, dtype=np.int32), ranges.reshape(-1),
                          (np.zeros((F,)) if no_map is None else np.asarray(no_map)).astype(np.int32).reshape(F)])
    f32 = [prims.reshape(-1), crop_kin.detach().cpu().to(torch.float32).numpy().reshape(-1), verts.reshape(-1)] + \
          [t.numpy().reshape(-1) for t in lin]
    host = torch.from_numpy(np.concatenate(f32 + [i32.view(np.float32)]))
    tab = host.to(dev, non_blocking=True) if dev.type != 'cpu' else host
    off = [0]
    for n in (prims.size, F * 4, verts.size, len(lin) * 2 * L_, F, F, 2 * F, F):
        off.append(off[-1] + n)
    base = tab.data_ptr()
    job = L.StriveRenderJob()
    job.prims, job.pose, job.verts, job.lin, job.mapix, job.lin_ix, job.prim_range, job.no_map = [base + 4 * o for o in off[:8]]
    job.F, job.L, job.W, job.NP, job.NV = F, L_, L_, prims.shape[0], verts.shape[0]
    out = torch.empty((F, L_, L_, 3), dtype=torch.uint8, device=dev)
    _launch(lib, map_env, job, out)
    return out


def _launch(lib, map_env, job, out):
    """strive_render_pictures over a job whose tables are set: adds the reference's layer colours and the map."""
    raster = map_env.nusc_raster.contiguous()
    M, Cc, H, W = raster.shape
    for i in range(MAX_LAYERS):
        rgb = to_rgb(MAP_COLORS[i])
        for c in range(3):
            job.layer_rgb[i * 3 + c] = rgb[c]
        job.layer_alpha[i] = MAP_ALPHAS[i]
    mp = L.StriveMap()
    dx = map_env.nusc_dx.to(raster.device).contiguous()
    mp.raster, mp.dx, mp.M, mp.C, mp.H, mp.W = raster.data_ptr(), dx.data_ptr(), M, Cc, H, W
    mp.L, mp.Wc = job.L, job.L
    lib.call('strive_render_pictures', C.byref(mp), C.byref(job), L.ptr(out), L.stream_ptr(out))


def render_device_tables(map_env, L_, F, pose, mapix, prim_range, prims, verts, lin, lin_ix, no_map, out=None, W_=None):
    """One launch of strive_render_pictures over tables that are on the map's device already (strive_scene_draw_tables wrote them):
    nothing is uploaded and nothing is read.  ``pose`` (F, 4) fp32, ``mapix`` (F) int32, ``prim_range`` (F, 2) int32, ``prims``
    (NP, 16) fp32 and ``verts`` (NV, 2) fp32 are device tensors; ``lin`` (NB, 2, L) fp32, ``lin_ix`` (F) and ``no_map`` (F) int32 are
    device tensors or device addresses.  -> ``out`` (F, L, L, 3) uint8, allocated unless given.  A picture whose map index is out
    of range keeps a white background (the table kernel reports it in the picture's status word)."""
    if W_ is not None and int(W_) != int(L_):
        raise ValueError('only square pictures are rendered (L == W): the reference mixes the two axes otherwise')
    raster = map_env.nusc_raster
    if raster.shape[1] > MAX_LAYERS:
        raise ValueError('the map has %d layers; the colour list has %d' % (raster.shape[1], MAX_LAYERS))
    for name, t in (('pose', pose), ('mapix', mapix), ('prim_range', prim_range), ('prims', prims), ('verts', verts)):
        if t.device != raster.device or not t.is_contiguous():
            raise ValueError('%s must be a contiguous tensor on the map\'s device' % name)
    F, L_ = int(F), int(L_)
    if tuple(pose.shape) != (F, 4) or mapix.numel() != F or tuple(prim_range.shape) != (F, 2) or prims.dim() != 2 or \
            prims.shape[1] != PRIM_FLOATS or verts.dim() != 2 or verts.shape[1] != 2:
        raise ValueError('the tables do not have the shapes of %d pictures' % F)
    if out is None:
        out = torch.empty((F, L_, L_, 3), dtype=torch.uint8, device=raster.device)
    elif out.device != raster.device or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != F * L_ * L_ * 3:
        raise ValueError('out is a contiguous (F, L, L, 3) uint8 tensor on the map\'s device')
    addr = lambda t: t.data_ptr() if torch.is_tensor(t) else int(t)           # noqa: E731
    job = L.StriveRenderJob()
    job.pose, job.mapix, job.prim_range, job.prims, job.verts = [t.data_ptr() for t in (pose, mapix, prim_range, prims, verts)]
    job.lin, job.lin_ix, job.no_map = addr(lin), addr(lin_ix), addr(no_map)
    job.F, job.L, job.W, job.NP, job.NV = F, L_, L_, prims.shape[0], verts.shape[0]
    _launch(ops._lib_for(raster), map_env, job, out)
    return out


def render_pictures(map_env, crop_kin, mapix, bounds, L_, draw_lists, no_map=None, px_per_pt=None, W_=None):
    """F pictures (F, L, L, 3) uint8 RGB (row 0 at the top) on the map's device in ONE kernel launch: picture f shows the crop of
    ``get_map_crop_pos(crop_kin[f:f+1], mapix[f:f+1], bounds[f], L, L)`` under ``draw_lists[f]`` (build_draw_list, coordinates in
    objs2crop's frame); ``no_map[f]``: white background; ``px_per_pt``: picture pixels per point of stroke width (default: the
    reference figure's, px_per_pt(L))."""
    prims, verts, ranges = pack_draw_lists(draw_lists, _figure_px_per_pt(L_) if px_per_pt is None else float(px_per_pt))
    return render_tables(map_env, crop_kin, mapix, bounds, L_, prims, verts, ranges, no_map, W_)


def read_back(pictures):
    """Device pictures -> numpy, through one pinned buffer and one synchronisation."""
    if pictures.device.type == 'cpu':
        return pictures.numpy()
    host = torch.empty(pictures.shape, dtype=pictures.dtype, pin_memory=True)
    host.copy_(pictures, non_blocking=True)
    torch.cuda.current_stream(pictures.device).synchronize()
    return host.numpy()


def write_png(path, array, level=3):
    """An (H, W, 3) uint8 RGB array as an 8-bit truecolour PNG (filter 0 on every row), with zlib and struct only."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('write_png takes an (H, W, 3) uint8 array')
    H, W, _ = a.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    rows[:, 1:] = a.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + chunk(b'IEND', b''))


WRITE_PNG_WORKERS = 8        # measured: tools/scene_draw_bench.py, profiles/r29_scene_draw_bench.json (README)


def write_pngs(paths, pictures, workers=None, level=3):
    """``write_png(paths[i], pictures[i])`` for every i on a pool of ``workers`` threads (zlib releases the interpreter lock while it
    compresses): the same files, byte for byte.  Missing directories are made.  The default is a fixed small number, never the
    machine's processor count."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    if len(paths) != len(pictures):
        raise ValueError('%d paths for %d pictures' % (len(paths), len(pictures)))
    workers = WRITE_PNG_WORKERS if workers is None else int(workers)
    if not 1 <= workers <= 16:
        raise ValueError('write_pngs takes 1 to 16 workers')
    for d in sorted({os.path.dirname(p) or '.' for p in paths}):
        os.makedirs(d, exist_ok=True)
    if workers == 1 or len(paths) <= 1:
        for p, a in zip(paths, pictures):
            write_png(p, a, level)
        return len(paths)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for _ in pool.map(lambda pa: write_png(pa[0], pa[1], level), zip(paths, pictures)):
            pass
    return len(paths)


# ------------------------------------------------------------------------------------------------------------------------
# what the two drivers share: plans -> one launch, one read-back, PNG files
# ------------------------------------------------------------------------------------------------------------------------

def frame_draw_lists(crop_traj, crop_lw, color=None, alpha=None):
    """The NT pictures of viz_map_crop_video (reference src/datasets/nuscenes_utils.py:632-653) for (NA, NT, 4) trajectories: frame
    t shows every agent observed at t (viz_traj off, one step: the first-frame alpha)."""
    NT = crop_traj.size(1)
    return [build_draw_list(crop_traj[:, None, t:t + 1, :], crop_lw, viz_traj=False, color=color, alpha=alpha) for t in range(NT)]


def video_frame_paths(outdir, NT):
    """<outdir>_000/frame%04d.png, the reference's names for its one sample (viz_map_crop_video is handed <out>_vid)."""
    import os
    return [os.path.join(outdir + '_000', 'frame%04d.png' % t) for t in range(NT)]


def check_ffmpeg(mp4):
    import shutil
    if mp4 and shutil.which('ffmpeg') is None:
        raise RuntimeError('--mp4 needs ffmpeg on the path; without it the frames are kept as PNG files')


def render_plans(plans, map_env, L_, mp4=False, fps=2, log=print):
    """``plans``: dicts {'crop_kin' (4,), 'mapix', 'bounds', 'pictures': [(path, draw_list, no_map)], 'videos': [frame directory]}.
    Every picture of every plan goes through ONE render_pictures call and ONE read-back; then the PNG files are written."""
    import os
    import shutil
    import subprocess
    kin, mapix, bounds, dls, nomap, paths = [], [], [], [], [], []
    for p in plans:
        for path, dl, nm in p['pictures']:
            kin.append(torch.as_tensor(p['crop_kin'], dtype=torch.float32).reshape(4))
            mapix.append(int(p['mapix']))
            bounds.append(list(p['bounds']))
            dls.append(dl)
            nomap.append(int(nm))
            paths.append(path)
    if not paths:
        return 0
    pics = read_back(render_pictures(map_env, torch.stack(kin), mapix, bounds, L_, dls, no_map=nomap))
    for path, pic in zip(paths, pics):
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        log('saving %s' % path)
        write_png(path, pic)
    for p in plans:
        for vdir in p.get('videos', []):
            if mp4:
                # the reference's command (create_video, :622-630), as a fresh child process; the frames go, as there
                subprocess.run(['ffmpeg', '-y', '-r', str(fps), '-i', os.path.join(vdir, 'frame%04d.png'), '-vcodec', 'libx264',
                                '-crf', '18', '-pix_fmt', 'yuv420p', vdir + '.mp4'])
                shutil.rmtree(vdir)
            else:
                log('frames kept in %s (no --mp4: ffmpeg is not run)' % vdir)
    return len(paths)
