#!/usr/bin/env python3
"""Generate tests/golden/g24_render.npz: WHAT THE REFERENCE DRAWS, as data -- no pictures.

Runs the reference's own ``viz_map_crop`` (src/datasets/nuscenes_utils.py), ``viz_scenario`` of src/viz_scenario_dir.py and of
src/eval_adv_gen.py, and ``NuScenesMapEnv.objs2crop`` with matplotlib's Agg backend in the build container, and records for every
figure the axes' artists in the order matplotlib draws them (sorted by z-order, stable), together with the crop pose, the bounds and
``objs2crop``'s outputs of every call.  The file is described in tests/golden/README_g24.md.

Nothing of the reference is changed except ``plt.grid``: the reference calls ``plt.grid(b=None)`` and matplotlib 3.10 no longer has
``b=``; the stand-in drops that keyword.  The artists are read in a figure hook (``rcParams['figure.hooks']``) on the draw that
``savefig`` makes; the map environment is a subclass that notes the arguments and results of ``get_map_crop_pos`` / ``objs2crop``;
``ffmpeg`` (absent) is a do-nothing script on the PATH of this process, so the reference's video loop runs to its end.

Usage:  python tests/golden/make_golden_render.py
"""
import os
import shutil
import stat
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import matplotlib as mpl                                          # noqa: E402
mpl.use('Agg')
import make_golden as mg                                         # noqa: E402
from make_golden_planner_eval import save_deterministic         # noqa: E402
import render_restated as rr                                     # noqa: E402
from strive_amd import synth                                     # noqa: E402

FIGS = []          # one entry per figure the reference saved: the artists of its axes at the last draw
CALLS = []         # get_map_crop_pos / objs2crop calls
KIND = {'line': 1, 'markers': 2, 'polygon': 3}


def _artists(ax):
    from matplotlib.collections import PathCollection
    from matplotlib.colors import to_rgb
    from matplotlib.lines import Line2D
    from matplotlib.patches import Polygon
    kids = [a for a in ax.get_children() if a is not ax.patch]
    kids = sorted(kids, key=lambda a: a.get_zorder())                 # as Axes.draw does: stable
    out = []
    for a in kids:
        if isinstance(a, Line2D):
            out.append({'kind': 'line', 'verts': np.asarray(a.get_xydata(), dtype=np.float64), 'face': to_rgb(a.get_color()),
                        'edge': (0, 0, 0), 'alpha': a.get_alpha(), 'width': a.get_linewidth(), 'zorder': a.get_zorder()})
        elif isinstance(a, PathCollection):
            fc = np.asarray(a.get_facecolors(), dtype=np.float64)
            off = np.asarray(a.get_offsets(), dtype=np.float64).reshape(-1, 2)
            if fc.shape[0] == 1 and off.shape[0] != 1:
                fc = np.tile(fc, (off.shape[0], 1))
            out.append({'kind': 'markers', 'verts': off, 'colors': fc, 'face': (0, 0, 0), 'edge': (0, 0, 0), 'alpha': a.get_alpha(),
                        'width': float(np.asarray(a.get_sizes()).reshape(-1)[0]), 'zorder': a.get_zorder(),
                        'edgewidth': float(np.asarray(a.get_linewidths()).reshape(-1)[0])})
        elif isinstance(a, Polygon):
            out.append({'kind': 'polygon', 'verts': np.asarray(a.get_xy(), dtype=np.float64), 'face': a.get_facecolor()[:3],
                        'edge': a.get_edgecolor()[:3], 'alpha': a.get_alpha(), 'width': a.get_linewidth(), 'zorder': a.get_zorder()})
    return out


def figure_hook(fig):
    rec = {'artists': [], 'nimages': 0, 'xlim': (0, 0), 'ylim': (0, 0)}
    FIGS.append(rec)

    def on_draw(event):
        ax = fig.axes[-1]
        rec['artists'] = _artists(ax)
        rec['nimages'] = len(ax.images)
        rec['xlim'], rec['ylim'] = ax.get_xlim(), ax.get_ylim()
    fig.canvas.mpl_connect('draw_event', on_draw)


def store(out, tag, figs):
    out[tag + '/nfig'] = np.array(len(figs))
    for fi, rec in enumerate(figs):
        arts = rec['artists']
        meta = np.zeros((len(arts), 12), dtype=np.float64)
        for i, a in enumerate(arts):
            meta[i] = [KIND[a['kind']], a['zorder'], a['alpha'], a['width'], *a['face'], *a['edge'], a['verts'].shape[0],
                       a.get('edgewidth', 0.0)]
            out['%s/f%d/a%d/verts' % (tag, fi, i)] = a['verts']
            if a['kind'] == 'markers':
                out['%s/f%d/a%d/colors' % (tag, fi, i)] = a['colors']
        out['%s/f%d/meta' % (tag, fi)] = meta
        out['%s/f%d/nimages' % (tag, fi)] = np.array(rec['nimages'])
        out['%s/f%d/lims' % (tag, fi)] = np.array(list(rec['xlim']) + list(rec['ylim']), dtype=np.float64)


def main():
    R = mg.import_reference()
    mg._install_exact_shapely()
    if 'configargparse' not in sys.modules:
        sys.modules['configargparse'] = types.ModuleType('configargparse')
    import importlib
    import matplotlib.pyplot as plt
    ref_viz_dir = importlib.import_module('viz_scenario_dir')
    ref_eval = importlib.import_module('eval_adv_gen')
    real_grid = plt.grid
    plt.grid = lambda *a, **k: real_grid(*a, **{key: v for key, v in k.items() if key != 'b'})      # the one patch
    mpl.rcParams['figure.hooks'] = ['make_golden_render:figure_hook']

    class NotingEnv(R.map_env.NuScenesMapEnv):
        def get_map_crop_pos(self, pos, mapixes, bounds=None, L=None, W=None):
            CALLS.append({'pose': pos.numpy().copy(), 'mapix': mapixes.numpy().copy(), 'bounds': np.array(bounds, dtype=np.float64), 'L': L})
            return super().get_map_crop_pos(pos, mapixes, bounds=bounds, L=L, W=W)

        def objs2crop(self, center, obj_center, obj_lw, map_idx, bounds=None, L=None, W=None):
            res = super().objs2crop(center, obj_center, obj_lw, map_idx, bounds=bounds, L=L, W=W)
            CALLS[-1]['o2c_in'] = obj_center.numpy().copy()
            CALLS[-1]['o2c_lw_in'] = obj_lw.numpy().copy()
            CALLS[-1]['o2c'] = res[0].numpy().copy()
            CALLS[-1]['o2c_lw'] = res[1].numpy().copy()
            return res

    raster, dx = synth.make_raster(mg.RASTER_HW, mg.RASTER_HW, M=1)
    env = mg.ref_map_env(R, raster, dx)
    env.__class__ = NotingEnv
    out = {}
    tmp = tempfile.mkdtemp()
    fake = os.path.join(tmp, 'bin')
    os.makedirs(fake)
    with open(os.path.join(fake, 'ffmpeg'), 'w') as f:
        f.write('#!/bin/sh\nexit 0\n')
    os.chmod(os.path.join(fake, 'ffmpeg'), stat.S_IRWXU)
    os.environ['PATH'] = fake + os.pathsep + os.environ['PATH']

    # ---- A: viz_map_crop on hand-made trajectories in the crop frame (render_restated.DIRECT_CASES) ----
    L = 64
    x = torch.zeros((4, L, L))
    for name, kw in rr.direct_cases().items():
        del FIGS[:]
        R.nutils.viz_map_crop(x, os.path.join(tmp, name + '.png'), indiv=False, **kw)
        assert len(FIGS) == 1 and FIGS[0]['nimages'] == 5, (name, len(FIGS))
        store(out, 'direct/' + name, FIGS)

    # ---- B: src/viz_scenario_dir.py viz_scenario ----
    for name, scene in rr.dir_scenes().items():
        del FIGS[:], CALLS[:]
        ref_viz_dir.viz_scenario(scene, env, os.path.join(tmp, 'dir_' + name), L=L, W=L, video=True)
        NT = scene['scene_past'].size(1) + scene['scene_fut'].size(1)
        assert len(FIGS) == 1 + NT and len(CALLS) == 1, (name, len(FIGS), len(CALLS))
        store(out, 'dir/' + name, FIGS)
        for k, v in CALLS[0].items():
            out['dir/%s/%s' % (name, k)] = np.asarray(v)

    # ---- C: src/eval_adv_gen.py viz_scenario ----
    for name, scene in rr.adv_scenes().items():
        for stage in ('init', 'adv', 'sol'):
            del FIGS[:], CALLS[:]
            d = os.path.join(tmp, 'adv_' + name + '_' + stage)
            os.makedirs(d)
            ref_eval.viz_scenario(scene, stage, env, d, L=L, W=L, video=(stage == 'adv'))
            store(out, 'adv/%s/%s' % (name, stage), FIGS)
            out['adv/%s/%s/ncalls' % (name, stage)] = np.array(len(CALLS))
            if CALLS:
                for k, v in CALLS[0].items():
                    out['adv/%s/%s/%s' % (name, stage, k)] = np.asarray(v)
    save_deterministic('g24_render.npz', out)
    shutil.rmtree(tmp)


if __name__ == '__main__':
    import make_golden_render as me          # one copy of the module: the figure hook is looked up by name
    me.main()
