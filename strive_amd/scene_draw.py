"""Pictures of a live batch: the host layer of strive_scene_draw_tables (include/strive_hip.h).

A *call* is the argument set of one ``viz_scene_graph`` (reference src/datasets/nuscenes_utils.py:477-621) as a dict.  ``draw_calls``
turns any number of calls on one batch into views and pictures, builds every draw table on the device in ONE launch, renders them
in ONE launch of strive_render_pictures and reads pictures and status words back in ONE copy.  Nothing is read back in between: the
capacities of the tables follow from shapes, which the host knows.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import ops, params, render

TRAJ, CENTER, CROP_T, OW_GT = 1, 2, 4, 8                          # view flags (STRIVE_SCENE_DRAW_*)
BAD_MAP, NO_STEP, BAD_CROP_T, BAD_VIEW = 1, 2, 4, 8                # status bits
VIEW_INTS, PIC_INTS, MAX_PREDS = 16, 8, 4
DEFAULT_BOUNDS = [-17.0, -38.5, 60.0, 38.5]
CALL_KEYS = ('bidx', 'out_path', 'future_pred', 'aidx', 'viz_traj', 'make_video', 'show_gt', 'traj_color_val', 'traj_color_bounds',
             'viz_bounds', 'center_viz', 'car_colors', 'show_gt_idx', 'crop_t', 'ow_gt', 'car_alpha', 'traj_linewidth', 'traj_markersize')


def host_ptr(scene_graph):
    """The scene offsets (B + 1) on the host: the copy the batch carries (ops.prime_scene_info / ops.scene_info) or ONE read-back."""
    ptr = scene_graph.ptr
    info = scene_graph.__dict__.get('_strive_scene_info')
    if info is not None and info.ptr_sig == (ptr.data_ptr(), ptr._version, tuple(ptr.shape)):
        return info.ptr_cpu.numpy().astype(np.int64)
    return ptr.cpu().numpy().astype(np.int64)


def norm_struct(state_normalizer, att_normalizer):
    nrm = L.StriveNorm()
    sm, ss = state_normalizer.mean_vals.cpu().numpy(), state_normalizer.std_vals.cpu().numpy()
    am, as_ = att_normalizer.mean_vals.cpu().numpy(), att_normalizer.std_vals.cpu().numpy()
    if sm.shape[0] < 4 or am.shape[0] < 2:
        raise ValueError('the state normaliser has at least 4 components and the attribute normaliser 2')
    for i in range(min(6, sm.shape[0])):
        nrm.state_mean[i], nrm.state_std[i] = float(sm[i]), float(ss[i])
    for i in range(2):
        nrm.att_mean[i], nrm.att_std[i] = float(am[i]), float(as_[i])
    return nrm


def _style_rows(n, colors, alpha, linewidth, markersize):
    rows = np.zeros((n, 8), dtype=np.float32)
    for name, t in (('car_colors', colors), ('car_alpha', alpha), ('traj_linewidth', linewidth), ('traj_markersize', markersize)):
        if t is not None and len(t) < n:
            raise ValueError('%s has %d entries for a scene of %d agents' % (name, len(t), n))
    rows[:, 0:3] = [render.to_rgb(colors[j]) for j in range(n)] if colors is not None else \
        np.array([render.to_rgb(render.plt_color(j)) for j in range(9)])[np.arange(n) % 9]
    rows[:, 3] = 0.7 if alpha is None else np.asarray(alpha[:n], dtype=np.float64)
    rows[:, 4] = 1.0 if linewidth is None else np.asarray(linewidth[:n], dtype=np.float64)
    rows[:, 5] = 8.0 if markersize is None else np.asarray(markersize[:n], dtype=np.float64)
    return rows


class Plan(object):
    """Views, pictures and file names of a list of calls on one batch; every table the device needs, as host arrays."""

    def __init__(self, calls, ptr, PT, FT, L_):
        self.preds, self.pred_shape, self.ow_gt = [], [], None
        self.views, self.view_f, self.pictures, self.lin_ix, self.paths, self.videos, self.view_of_call = [], [], [], [], [], [], []
        self.styles, self.rainbow, self._rb_of, self._lin_of, self.lin_keys = [], [], {}, {}, []
        self.NP = self.NV = 0
        style_rows = 0
        B = ptr.shape[0] - 1
        self.rb_gt = self._rainbow(PT + FT)
        self.rb_one = self._rainbow(1)
        for ci, call in enumerate(calls):
            unknown = [k for k in call if k not in CALL_KEYS]
            if unknown:
                raise TypeError('viz_scene_graph has no argument %r' % unknown[0])
            if call.get('traj_color_val') is not None or call.get('traj_color_bounds') is not None:
                raise NotImplementedError('traj_color_val / traj_color_bounds are not drawn (no driver of the reference passes them)')
            bidx = int(call['bidx'])
            if not 0 <= bidx < B:
                raise IndexError('bidx %d of a batch of %d scenes' % (bidx, B))
            n = int(ptr[bidx + 1] - ptr[bidx])
            pred = call.get('future_pred')
            set_ix, NS, FPT = -1, 1, FT
            if pred is not None:
                if pred.dim() not in (3, 4) or pred.size(-1) != 4 or pred.size(0) != int(ptr[-1]):
                    raise ValueError('future_pred is (NA, FT, 4) or (NA, NS, FT, 4)')
                for i, p in enumerate(self.preds):
                    if p is pred:
                        set_ix = i
                if set_ix < 0:
                    if len(self.preds) == MAX_PREDS:
                        raise ValueError('one launch draws at most %d different future_pred tensors' % MAX_PREDS)
                    set_ix = len(self.preds)
                    self.preds.append(pred)
                    self.pred_shape.append((pred.size(1), pred.size(2)) if pred.dim() == 4 else (1, pred.size(1)))
                NS, FPT = self.pred_shape[set_ix]
            NT = PT + FPT
            show_gt = bool(call.get('show_gt', False)) or call.get('show_gt_idx') is not None
            aidx = call.get('aidx')
            d = (0, n) if aidx is None else ((int(aidx), 1) if 0 <= int(aidx) < n else (0, 0))
            g = (0, 0)
            flags = 0
            if show_gt and pred is not None:
                g = d
                if call.get('show_gt_idx') is not None:
                    k = int(call['show_gt_idx'])
                    g = (g[0] + k, 1) if 0 <= k < g[1] else (0, 0)
                ow = call.get('ow_gt')
                if ow is not None:
                    if self.ow_gt is not None and self.ow_gt is not ow:
                        raise ValueError('one launch draws one ow_gt tensor')
                    if tuple(ow.shape) != (int(ptr[-1]), FT, 4):
                        raise ValueError('ow_gt is (NA, FT, 4)')
                    self.ow_gt = ow
                    flags |= OW_GT
            viz_traj = bool(call.get('viz_traj', False))
            flags |= TRAJ if viz_traj else 0
            crop_t = call.get('crop_t')
            if call.get('center_viz', False):
                flags |= CENTER
            elif crop_t is not None:
                flags |= CROP_T
            b = [float(v) for v in (call.get('viz_bounds') or DEFAULT_BOUNDS)]
            key = tuple(b)
            if key not in self._lin_of:
                self._lin_of[key] = len(self.lin_keys)
                self.lin_keys.append(key)
            style = -1
            if any(call.get(k) is not None for k in ('car_colors', 'car_alpha', 'traj_linewidth', 'traj_markersize')):
                style = style_rows
                self.styles.append(_style_rows(n, call.get('car_colors'), call.get('car_alpha'), call.get('traj_linewidth'),
                                               call.get('traj_markersize')))
                style_rows += n
            # the video's frames take the colours only (viz_map_crop_video passes nothing else on)
            vstyle = -1
            if call.get('make_video', True) and call.get('car_colors') is not None:
                vstyle = style_rows
                self.styles.append(_style_rows(n, call['car_colors'], None, None, None))
                style_rows += n
            out_path = call['out_path']
            first = len(self.views)

            def view(style_ix):
                self.views.append([bidx, flags, d[0], d[1], g[0], g[1], 0 if crop_t is None else int(crop_t), set_ix, self._rainbow(NT), style_ix]
                                  + [0] * (VIEW_INTS - 10))
                self.view_f.append([b[0], b[1], L_ / float(b[2] - b[0]), L_ / float(b[3] - b[1])])
                return len(self.views) - 1

            def picture(v, s, t, ng, ns, nt):
                steps = ng * (PT + FT) + d[1] * ns * nt
                pcap = steps + ng + d[1] * ns + d[1] if viz_traj else steps
                vcap = steps if viz_traj else 0
                self.pictures.append([v, s, t, self.NP, self.NV, pcap, vcap, 0])
                self.lin_ix.append(self._lin_of[key])
                self.NP += pcap
                self.NV += vcap
            v = view(style)
            picture(v, -1, 0, g[1], NS, NT)
            self.paths.append(out_path + '.png')
            if call.get('make_video', True):
                v = view(vstyle)
                for s in range(NS):
                    vdir = out_path + '_%03d' % s
                    self.videos.append(vdir)
                    for t in range(NT):
                        picture(v, s, t, 0, 1, 1)
                        self.paths.append(os.path.join(vdir, 'frame%04d.png' % t))
            self.view_of_call.append((first, len(self.views)))
        if self.NP >= 2 ** 31 // 16 or self.NV >= 2 ** 30:
            raise ValueError('the draw tables of this launch are too large')

    def _rainbow(self, T):
        if T not in self._rb_of:
            self._rb_of[T] = sum(r.shape[0] for r in self.rainbow)
            self.rainbow.append(render.gist_rainbow(np.linspace(0, 1.0, T)).astype(np.float32).reshape(T, 3))
        return self._rb_of[T]


class DeviceTables(object):
    """What strive_scene_draw_tables wrote, as device tensors (views into two buffers) -- and the host tables that go with them."""
    pass


def draw_tables(scene_graph, map_idx, state_normalizer, att_normalizer, calls, L_, num_maps, ptr=None):
    """-> DeviceTables of the calls' pictures: ONE upload of the host's small tables, ONE kernel launch, no read-back."""
    past_gt, future_gt, lw = scene_graph.past_gt, scene_graph.future_gt, scene_graph.lw
    dev = past_gt.device
    lib = ops._lib_for(past_gt)
    ptr = host_ptr(scene_graph) if ptr is None else np.asarray(ptr, dtype=np.int64)
    NA, PT = int(past_gt.shape[0]), int(past_gt.shape[1])
    FT = int(future_gt.shape[1])
    if int(ptr[-1]) != NA or past_gt.shape[2] < 4 or future_gt.shape[2] < 4 or tuple(lw.shape) != (NA, 2):
        raise ValueError('the batch holds past_gt (NA, PT, >= 4), future_gt (NA, FT, >= 4) and lw (NA, 2)')
    plan = Plan(calls, ptr, PT, FT, int(L_))
    F, NV_ = len(plan.pictures), len(plan.views)
    t = DeviceTables()
    t.plan, t.F, t.L = plan, F, int(L_)
    if F == 0:
        return t
    B = ptr.shape[0] - 1
    style = np.concatenate(plan.styles, axis=0) if plan.styles else np.zeros((0, 8), dtype=np.float32)
    rainbow = np.concatenate(plan.rainbow, axis=0)
    lin = [torch.stack([torch.linspace(k[0], k[2], t.L), torch.linspace(k[1], k[3], t.L)]).numpy().reshape(-1) for k in plan.lin_keys]
    i32 = [np.asarray(plan.views, dtype=np.int32).reshape(-1), np.asarray(plan.pictures, dtype=np.int32).reshape(-1),
           np.asarray(plan.lin_ix, dtype=np.int32), np.zeros((F,), dtype=np.int32), ptr.astype(np.int32)]
    f32 = [np.asarray(plan.view_f, dtype=np.float64).astype(np.float32).reshape(-1), style.reshape(-1), rainbow.reshape(-1)] + lin
    host = torch.from_numpy(np.concatenate([a.view(np.float32) for a in i32] + f32))
    tab = params.upload(host, dev)
    off = [0]
    for a in i32 + f32[:3]:
        off.append(off[-1] + a.size)
    base = tab.data_ptr()
    at = lambda i: base + 4 * off[i]           # noqa: E731
    # outputs: prims first (16-byte aligned), then verts, pose, and the int tables
    sizes = [plan.NP * 16, plan.NV * 2, F * 4, F, F * 2]
    oo = [0]
    for s in sizes:
        oo.append(oo[-1] + (s + 3) // 4 * 4)
    out = torch.empty((max(oo[-1], 4),), dtype=torch.float32, device=dev)
    ob = out.data_ptr()
    job = L.StriveSceneDraw()
    keep = [tab, out]

    def f32c(x):
        x = x.detach()
        x = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.to(torch.float32).contiguous()
        keep.append(x)
        return x.data_ptr()
    job.past_gt, job.future_gt, job.lw = f32c(past_gt), f32c(future_gt), f32c(lw)
    job.ow_gt = f32c(plan.ow_gt) if plan.ow_gt is not None else None
    for i, p in enumerate(plan.preds):
        job.pred[i] = f32c(p)
        job.pred_NS[i], job.pred_FPT[i] = plan.pred_shape[i]
    mi = map_idx if (map_idx.dtype == torch.int64 and map_idx.is_contiguous()) else map_idx.to(torch.int64).contiguous()
    keep.append(mi)
    if mi.device != dev or mi.numel() != B:
        raise ValueError('map_idx holds one map index per scene, on the batch\'s device')
    job.map_idx = mi.data_ptr()
    job.views, job.pictures, job.scene_ptr, job.view_f, job.style, job.rainbow = at(0), at(1), at(4), at(5), at(6), at(7)
    t.lin_ix_ptr, t.no_map_ptr, t.lin_ptr = at(2), at(3), base + 4 * off[8]
    job.prims, job.verts, job.pose, job.mapix, job.prim_range = [ob + 4 * o for o in oo[:5]]
    job.k = render.px_per_pt(t.L)
    job.NA, job.B, job.M, job.PT, job.FT = NA, B, int(num_maps), PT, FT
    job.past_stride, job.future_stride = int(past_gt.shape[2]), int(future_gt.shape[2])
    job.NVIEW, job.F, job.NP, job.NV = NV_, F, plan.NP, plan.NV
    job.rb_rows, job.rb_gt_off, job.rb_one_off, job.style_rows = rainbow.shape[0], plan.rb_gt, plan.rb_one, style.shape[0]
    job.edge_px, job.heading_px = render.EDGE_PT * job.k, render.HEADING_PT * job.k
    for j in range(9):
        for c, v in enumerate(render.to_rgb(render.plt_color(j))):
            job.cycle_rgb[j * 3 + c] = v
    job.norm = norm_struct(state_normalizer, att_normalizer)
    # pictures and status words share one buffer, so that they come back in one copy
    t.status_off = (F * t.L * t.L * 3 + 3) // 4 * 4
    t.buffer = torch.empty((t.status_off + 4 * F,), dtype=torch.uint8, device=dev)
    job.status = t.buffer.data_ptr() + t.status_off
    lib.call('strive_scene_draw_tables', C.byref(job), L.stream_ptr(past_gt))
    t.keep, t.out = keep, out
    t.prims = out[oo[0]:oo[0] + plan.NP * 16].view(plan.NP, 16)
    t.verts = out[oo[1]:oo[1] + plan.NV * 2].view(plan.NV, 2)
    t.pose = out[oo[2]:oo[2] + F * 4].view(F, 4)
    t.mapix = out[oo[3]:oo[3] + F].view(torch.int32)
    t.prim_range = out[oo[4]:oo[4] + 2 * F].view(torch.int32).view(F, 2)
    t.status = t.buffer[t.status_off:].view(torch.int32)
    return t


def render_drawn(map_env, t):
    """The pictures of ``t`` (draw_tables), rendered into ``t.buffer`` by one launch, no read-back -> (F, L, L, 3) uint8 device view."""
    n = t.F * t.L * t.L * 3
    pics = t.buffer[:n].view(t.F, t.L, t.L, 3)
    render.render_device_tables(map_env, t.L, t.F, t.pose, t.mapix, t.prim_range, t.prims, t.verts, t.lin_ptr, t.lin_ix_ptr, t.no_map_ptr, pics)
    return pics


def check_status(t, status):
    """Raises what the reference raises for the first picture whose status word is set."""
    bad = np.nonzero(status)[0]
    if bad.size == 0:
        return
    f = int(bad[0])
    word = int(status[f])
    view = t.plan.views[t.plan.pictures[f][0]]
    where = 'scene %d (%s)' % (view[0], t.plan.paths[f])
    if word & BAD_VIEW:
        raise RuntimeError('%s: the view does not fit the batch\'s shapes' % where)
    if word & BAD_MAP:
        raise ValueError('%s: map index out of range' % where)
    if word & BAD_CROP_T:
        raise IndexError('%s: crop_t %d is out of range' % (where, view[6]))
    if word & NO_STEP:
        raise IndexError('%s: agent %d has no observed step (the reference fails here as well)' % (where, (word >> 8) - 1))


def draw_calls(scene_graph, map_idx, map_env, calls, state_normalizer, att_normalizer, ptr=None):
    """-> (paths, pictures (F, L, L, 3) uint8 numpy, video directories) of the calls: one table launch, one render launch, one
    read-back.  Raises before anything is returned if a picture's status word is set."""
    L_ = int(map_env.L)
    if int(map_env.W) != L_:
        raise ValueError('only square pictures are rendered (L == W): the reference mixes the two axes otherwise')
    t = draw_tables(scene_graph, map_idx, state_normalizer, att_normalizer, calls, L_, int(map_env.nusc_raster.shape[0]), ptr=ptr)
    if t.F == 0:
        return [], np.zeros((0, L_, L_, 3), dtype=np.uint8), []
    render_drawn(map_env, t)
    host = render.read_back(t.buffer)
    status = host[t.status_off:t.status_off + 4 * t.F].view(np.int32)
    check_status(t, status)
    return t.plan.paths, host[:t.F * L_ * L_ * 3].reshape(t.F, L_, L_, 3), t.plan.videos
