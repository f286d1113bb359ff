#!/usr/bin/env python3
"""Generate tests/golden/g26_scene_graph.npz: WHAT THE REFERENCE'S viz_scene_graph DRAWS for a live batch, as data -- no pictures.

Runs the reference's own ``viz_scene_graph`` (src/datasets/nuscenes_utils.py:477-621) and both ``viz_optim_results``
(src/utils/scenario_gen.py:149-187, src/refine_traffic_optim.py:123-144) on the batch of tests/scene_draw_restated.py (``g26_inputs``,
``g26_calls``) with matplotlib's Agg backend, and records per call: the artists of every figure in matplotlib's draw order (the hook,
``_artists`` and ``store`` of make_golden_render.py), the crop pose, the bounds, the inputs and outputs of every ``objs2crop`` call and
the file names the reference reports saving.  The file is described in tests/golden/README_g26.md.

Nothing of the reference is changed except ``plt.grid`` (``plt.grid(b=None)``: matplotlib 3.10 no longer has ``b=``; the stand-in
drops that keyword), as for fixture g24.  Every call gets a copy of the batch: the reference unnormalises its argument in place and
normalises it back, which changes last bits.  ``ffmpeg`` (absent) is a do-nothing script on the PATH of this process.

Usage:  python tests/golden/make_golden_scene_graph.py
"""
import contextlib
import io
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
import make_golden_render as mgr                                 # noqa: E402
from make_golden_planner_eval import save_deterministic         # noqa: E402
import scene_draw_restated as sr                                 # noqa: E402
from strive_amd import synth                                     # noqa: E402

O2C = []           # objs2crop calls of the running viz_scene_graph


def record(out, tag, figs, o2c, saved, tmp, raised=''):
    mgr.store(out, tag, figs)
    out[tag + '/raised'] = np.array(raised, dtype='U')
    out[tag + '/ncalls'] = np.array(len(o2c))
    for i, c in enumerate(o2c):
        for k, v in c.items():
            out['%s/o2c%d/%s' % (tag, i, k)] = np.asarray(v)
    names = [os.path.relpath(p, tmp) for p in saved]
    out[tag + '/saved'] = np.array(names if names else [''], dtype='U')


def main():
    R = mg.import_reference()
    mg._install_exact_shapely()
    if 'configargparse' not in sys.modules:
        sys.modules['configargparse'] = types.ModuleType('configargparse')
    import importlib
    import matplotlib.pyplot as plt
    real_grid = plt.grid
    plt.grid = lambda *a, **k: real_grid(*a, **{key: v for key, v in k.items() if key != 'b'})      # the one patch
    mpl.rcParams['figure.hooks'] = ['make_golden_render:figure_hook']
    ref_refine = importlib.import_module('refine_traffic_optim')

    class NotingEnv(R.map_env.NuScenesMapEnv):
        def objs2crop(self, center, obj_center, obj_lw, map_idx, bounds=None, L=None, W=None):
            res = super().objs2crop(center, obj_center, obj_lw, map_idx, bounds=bounds, L=L, W=W)
            O2C.append({'pose': center.numpy().copy(), 'mapix': np.array(int(map_idx)), 'bounds': np.array(bounds, dtype=np.float64),
                        'in': obj_center.numpy().copy(), 'lw_in': obj_lw.numpy().copy(), 'out': res[0].numpy().copy(),
                        'lw_out': res[1].numpy().copy()})
            return res

    raster, dx = synth.make_raster(mg.RASTER_HW, mg.RASTER_HW, M=2)
    env = mg.ref_map_env(R, raster, dx)
    env.__class__ = NotingEnv
    env.L = env.W = sr.G26_L
    batch, map_idx, ptr, preds, ow = sr.g26_inputs()
    sn = R.dutils.MeanStdNormalizer(*mg.state_norm_tensors())
    an = R.dutils.MeanStdNormalizer(*mg.att_norm_tensors())
    model = types.SimpleNamespace(get_normalizer=lambda: sn, get_att_normalizer=lambda: an)
    out = {}
    tmp = tempfile.mkdtemp()
    fake = os.path.join(tmp, 'bin')
    os.makedirs(fake)
    with open(os.path.join(fake, 'ffmpeg'), 'w') as f:
        f.write('#!/bin/sh\nexit 0\n')
    os.chmod(os.path.join(fake, 'ffmpeg'), stat.S_IRWXU)
    os.environ['PATH'] = fake + os.pathsep + os.environ['PATH']

    def run(fn):
        """-> (figures, objs2crop calls, saved paths, what the reference raised) of fn(a fresh copy of the batch).  A figure the
        reference opened but did not get to save (it raised while filling it) is not counted."""
        del mgr.FIGS[:], O2C[:]
        buf = io.StringIO()
        raised = ''
        with contextlib.redirect_stdout(buf):
            try:
                fn(batch.clone())
            except IndexError as e:
                raised = 'IndexError: %s' % e
                plt.close('all')
        saved = [line[len('saving '):] for line in buf.getvalue().splitlines() if line.startswith('saving ')]
        return list(mgr.FIGS)[:len(saved)], list(O2C), saved, raised

    # ---- A: viz_scene_graph ----
    for name, kw in sr.g26_calls(preds, ow).items():
        kw = dict(kw)
        bidx = kw.pop('bidx')
        figs, o2c, saved, raised = run(lambda g: R.nutils.viz_scene_graph(g, map_idx, env, bidx, os.path.join(tmp, name), sn, an, **kw))
        print('%-20s %3d figures %s' % (name, len(figs), raised))
        record(out, 'call/' + name, figs, o2c, saved, tmp, raised)

    # ---- B: the two viz_optim_results; each makes two viz_scene_graph calls (1 figure, then 1 + NS NT figures) ----
    one = preds['one']
    NT = batch.past_gt.size(1) + one.size(2)
    for name, fn in (
            ('optim_adv', lambda g: R.scenario_gen.viz_optim_results(os.path.join(tmp, 'optim_adv'), g, map_idx, env, model, one, 'hardcode', 2, 6,
                                                                     bidx=0, show_gt_idx=0, ow_gt=ow)),
            ('optim_refine', lambda g: ref_refine.viz_optim_results(os.path.join(tmp, 'optim_refine'), g, map_idx, env, model, one, bidx=0))):
        figs, o2c, saved, raised = run(fn)
        assert len(figs) == 2 + NT and not raised, (name, len(figs), raised)
        per = len(o2c) // 2
        record(out, 'call/%s/c0' % name, figs[:1], o2c[:per], saved[:1], tmp)
        record(out, 'call/%s/c1' % name, figs[1:], o2c[per:], saved[1:], tmp)
    save_deterministic('g26_scene_graph.npz', out)
    shutil.rmtree(tmp)


if __name__ == '__main__':
    main()
