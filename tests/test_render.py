"""Scenario pictures (strive_render_pictures, strive_amd/render.py, viz_scenario_dir, viz_adv_gen).

1. what is drawn -- artists, order, colours, crop pose, bounds, objs2crop -- equals what the reference draws (fixture g24, recorded
   from the reference's own functions under matplotlib; tests/golden/README_g24.md);
2. the kernel equals the float64 restatement of its stated rule (tests/render_restated.py) within one level, away from sub-samples
   that sit on a primitive boundary;
3. exact cases: the map composite, orientation, an axis-aligned car, no_map;
4. a picture does not depend on its neighbours in the launch; GPU and host emulation agree;
5. a gross-error check against Agg; 6. host functions and error paths; 7. the two command lines end to end on the GPU.
Kernel cases run through the host emulation without a GPU and again, marked gpu, on the MI355X."""
import os
import shutil
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

from strive_amd import _lib as L, ops, render, synth, viz_adv_gen, viz_scenario_dir
import render_restated as rr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'hipemu'))
G18 = os.path.join(HERE, 'golden', 'g18_scenarios')
EPS32 = 2.0 ** -23
TILE = 16            # the kernel's tile edge
PASS = 256           # primitives per cull pass
WHITE = np.ones((3,), dtype=np.float32)
LAYER_RGB = [np.array(render.to_rgb(c), dtype=np.float32) for c in render.MAP_COLORS]


@pytest.fixture(scope='module')
def g24():
    return np.load(os.path.join(HERE, 'golden', 'g24_render.npz'))


@pytest.fixture()
def on(monkeypatch):
    """on('cpu'): the operators run on the host emulation; on('gpu'): on the product library.  Returns the device."""
    def select(where):
        if where == 'gpu':
            return torch.device('cuda', 0)
        import build as emu_build
        emu = L.StriveLib(emu_build.build(), require_all=True)
        monkeypatch.setattr(ops, '_lib_for', lambda *tensors: emu)
        return torch.device('cpu')
    return select


BOTH = [pytest.param('cpu', id='emulated'), pytest.param('gpu', marks=pytest.mark.gpu, id='gpu')]


class Env(object):
    def __init__(self, dev, C=4, M=1, hw=256):
        r, dx = synth.make_raster(hw, hw, C=C, M=M)
        self.nusc_raster, self.nusc_dx = r.to(dev), dx.to(dev)
        self.map_list = ['synthetic-%d' % i for i in range(M)]


def tables(dev, env, pose, mapix, bounds, Lp, prims, verts, ranges, no_map=None):
    out = render.render_tables(env, torch.as_tensor(pose, dtype=torch.float32).reshape(-1, 4), mapix, bounds, Lp, prims, verts, ranges,
                               no_map=no_map)
    assert out.device.type == dev.type and out.dtype == torch.uint8
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# 1. the reference pin
# ------------------------------------------------------------------------------------------------------------------------

def as_artists(draw_list):
    """A draw list as the artists matplotlib holds for it: (kind, zorder, alpha, width, face, edge, verts[, colours])."""
    out = []
    for a in draw_list:
        if a['kind'] == 'markers':
            out.append((2, 1, a['alpha'], a['size'], None, None, a['verts'], a['colors']))
        elif a['kind'] == 'line':
            out.append((1, 2, a['alpha'], a['linewidth'], a['color'], (0, 0, 0), a['verts']))
        else:
            cx, cy = a['center']
            h = np.arctan2(a['heading'][1], a['heading'][0])
            c, s = np.cos(h), np.sin(h)
            l, w = a['l'], a['w']
            box = np.array([[-l / 2, -w / 2], [l / 2, -w / 2], [l / 2, w / 2], [-l / 2, w / 2], [-l / 2, -w / 2]])
            corners = np.stack([box[:, 0] * c - box[:, 1] * s + cx, box[:, 0] * s + box[:, 1] * c + cy], axis=1)
            out.append((3, 3, a['alpha'], render.EDGE_PT, a['color'], (0, 0, 0), corners))
            out.append((1, 3, a['alpha'], render.HEADING_PT, (0, 0, 0), (0, 0, 0), np.array([[cx, cy], [cx + l / 2 * c, cy + l / 2 * s]])))
    return out


def compare_figure(g, tag, draw_list):
    """-> the worst |difference| / (eps32 max|coordinate|) over the figure's geometry; everything else must be equal."""
    meta = g[tag + '/meta']
    mine = as_artists(draw_list)
    assert len(mine) == meta.shape[0], '%s: %d artists, the reference drew %d' % (tag, len(mine), meta.shape[0])
    worst = 0.0
    scale = max([1.0] + [float(np.abs(g['%s/a%d/verts' % (tag, i)]).max()) for i in range(meta.shape[0]) if meta[i, 10] > 0])
    for i, a in enumerate(mine):
        m = meta[i]
        assert (a[0], a[1]) == (int(m[0]), int(m[1])), '%s artist %d: kind / z-order' % (tag, i)
        assert a[2] == pytest.approx(m[2], abs=1e-15) and a[3] == m[3], '%s artist %d: alpha / width' % (tag, i)
        want = g['%s/a%d/verts' % (tag, i)]
        assert a[6].shape == want.shape, '%s artist %d: %s vertices, the reference has %s' % (tag, i, a[6].shape, want.shape)
        if a[0] == 2:
            cols = g['%s/a%d/colors' % (tag, i)]
            assert np.allclose(a[7], cols[:, :3], atol=1e-12) and np.allclose(cols[:, 3], m[2]), '%s artist %d: marker colours' % (tag, i)
            assert m[11] == render.MARKER_EDGE_PT
        else:
            assert tuple(a[4]) == tuple(m[4:7]) and tuple(a[5]) == tuple(m[7:10]), '%s artist %d: colours' % (tag, i)
        if want.size:
            worst = max(worst, float(np.abs(a[6] - want).max()) / (EPS32 * scale))
    assert worst <= 4.0, '%s: geometry off by %.2f eps32 max|coordinate|' % (tag, worst)
    return worst


def test_build_draw_list_draws_what_viz_map_crop_draws(g24):
    worst = {}
    for name, kw in rr.direct_cases().items():
        kw = dict(kw)
        for ref_name, mine in (('car_colors', 'color'), ('car_alpha', 'alpha')):
            if ref_name in kw:
                kw[mine] = kw.pop(ref_name)
        dl = render.build_draw_list(kw.pop('car_kin'), kw.pop('car_lw'), **kw)
        assert int(g24['direct/%s/nfig' % name]) == 1 and len(dl) > 0
        worst[name] = compare_figure(g24, 'direct/%s/f0' % name, dl)
    print('worst geometry ratios (eps32 max|coordinate|), direct:', worst)


def check_plan(g, tag, plan, first_fig=0):
    assert np.array_equal(np.asarray(plan['crop_kin'], dtype=np.float32).reshape(1, 4), g[tag + '/pose'])
    assert np.array_equal(np.array(plan['bounds'], dtype=np.float64), g[tag + '/bounds']) and plan['mapix'] == int(g[tag + '/mapix'][0])
    assert len(plan['pictures']) == int(g[tag + '/nfig'])
    return max(compare_figure(g, '%s/f%d' % (tag, i), dl) for i, (_, dl, nm) in enumerate(plan['pictures']))


def test_viz_scenario_dir_draws_what_the_reference_draws(g24):
    env = Env('cpu', hw=8)
    worst = {}
    for name, scene in rr.dir_scenes().items():
        plan = viz_scenario_dir.plan_scenario(scene, env, '/x/' + name, L=64, W=64, video=True)
        worst[name] = check_plan(g24, 'dir/' + name, plan)
        NT = scene['scene_past'].size(1) + scene['scene_fut'].size(1)
        assert [p for p, _, _ in plan['pictures']] == ['/x/%s.png' % name] + ['/x/%s_vid_000/frame%04d.png' % (name, t) for t in range(NT)]
    print('worst geometry ratios, viz_scenario_dir:', worst)


def test_viz_adv_gen_draws_what_the_reference_draws(g24):
    env = Env('cpu', hw=8)
    worst = {}
    for name, scene in rr.adv_scenes().items():
        for stage in ('init', 'adv', 'sol'):
            tag = 'adv/%s/%s' % (name, stage)
            plan = viz_adv_gen.plan_scenario(scene, stage, env, '/x', L=64, W=64, video=(stage == 'adv'))
            if int(g24[tag + '/nfig']) == 0:
                assert plan is None and stage == 'sol' and 'fut_sol' not in scene
                continue
            worst[tag] = check_plan(g24, tag, plan)
            names = [os.path.basename(p) for p, _, _ in plan['pictures']]
            assert names[:2] == (['viz_init_map.png', 'viz_init.png'] if stage == 'init' else names[:2]) and 'viz_%s.png' % stage in names
            if stage == 'init':
                assert plan['pictures'][0][1] == []
    assert len(worst) == 9          # four scenes, three stages, three of the scenes without fut_sol
    print('worst geometry ratios, viz_adv_gen:', worst)


def test_objs2crop_gives_the_reference_values(g24):
    worst = 0.0
    tags = ['dir/' + n for n in rr.dir_scenes()] + ['adv/%s/adv' % n for n in rr.adv_scenes()]
    for tag in tags:
        pose, b = torch.from_numpy(g24[tag + '/pose'])[0], list(g24[tag + '/bounds'])
        obj, lw = torch.from_numpy(g24[tag + '/o2c_in']), torch.from_numpy(g24[tag + '/o2c_lw_in'])
        got, got_lw = render.objs2crop(pose, obj, lw, b, 64, 64)
        env = object.__new__(__import__('strive_amd.datasets.map_env', fromlist=['x']).NuScenesMapEnv)
        env.bounds, env.L, env.W = [0, 0, 1, 1], 7, 7
        got2, got2_lw = env.objs2crop(pose, obj, lw, None, bounds=b, L=64, W=64)
        assert torch.equal(got[~torch.isnan(got)], got2[~torch.isnan(got2)]) and torch.equal(got_lw, got2_lw)
        want = g24[tag + '/o2c']
        assert got.dtype == torch.float32 and np.array_equal(np.isnan(got.numpy()), np.isnan(want))
        ok = ~np.isnan(want)
        worst = max(worst, float(np.abs(got.numpy() - want)[ok].max()) / (EPS32 * float(np.abs(want[ok]).max())))
        assert np.array_equal(got_lw.numpy(), g24[tag + '/o2c_lw'])
    print('objs2crop worst ratio: %.3f eps32 max|coordinate|' % worst)
    assert worst <= 4.0


def test_colour_table_is_matplotlibs():
    mc = pytest.importorskip('matplotlib.colors')
    mpl = pytest.importorskip('matplotlib')
    for name in ('white', 'black', 'darkgray', 'coral', 'orange', 'gold', 'lightblue', 'cornflowerblue', 'orangered', 'lawngreen'):
        assert render.to_rgb(name) == mc.to_rgb(name), name
    cyc = mpl.rcParamsDefault['axes.prop_cycle'].by_key()['color']
    assert [render.plt_color(i) for i in range(9)] == cyc[:9]
    assert [render.to_rgb(render.plt_color(i)) for i in range(9)] == [mc.to_rgb(c) for c in cyc[:9]]
    x = np.linspace(0, 1, 37)
    assert np.allclose(render.gist_rainbow(x), mpl.colormaps['gist_rainbow'](x)[:, :3], atol=1e-12)
    colors, alpha, lw, ms = render.get_adv_coloring(4, 2, 0, alpha=True, linewidth=True, markersize=True)
    assert colors == ['lawngreen', 'cornflowerblue', 'orangered', 'cornflowerblue'] and alpha == [1.0] * 4
    assert lw == [3.5, 2.5, 3.5, 2.5] and ms == [15.0, 10.0, 15.0, 10.0]
    assert render.get_adv_coloring(2, None, None, cycle_color=True) == [render.plt_color(0), render.plt_color(1)]


# ------------------------------------------------------------------------------------------------------------------------
# 2. the kernel against the float64 restatement
# ------------------------------------------------------------------------------------------------------------------------

def special_prims(Lp):
    """The geometry cases of the rule, around an Lp-pixel picture; -> prims, verts."""
    c = Lp / 2.0 + 0.3
    V = np.array([[2.1, 3.2], [Lp - 2.2, Lp - 3.1], [2.3, Lp - 2.4], [Lp - 3.3, 2.6], [Lp * 0.4, Lp * 0.9],        # 0-5: crosses itself
                  [5.5, 5.5],                                                                                  # 5-6: one vertex
                  [c, 2.2], [c, 2.2], [c + 4.1, 3.3], [c + 4.1, 3.3],                                          # 6-10: coincident vertices
                  [1.0, 1.0], [np.nan, 2.0], [3.0, 3.0]], dtype=np.float32)                                     # 10-13: a NaN vertex
    P = [rr.car(c, c, 0.6, 0.8, 3 * Lp, 3 * Lp, (0.2, 0.5, 0.9), 0.35),                 # covers the whole picture
         rr.car(-40.0, -50.0, 1.0, 0.2, 6.0, 3.0, (1, 0, 0), 1.0),                      # wholly outside
         rr.car(Lp - 1.2, c, -0.3, 0.9, 7.0, 3.1, (0.9, 0.3, 0.1), 1.0),                # across the border, alpha 1
         rr.car(c - 3.3, c + 2.2, 0.8, -0.6, 0.0, 4.2, (0.1, 0.8, 0.2), 0.8),           # l = 0
         rr.car(c, np.nan, 1.0, 0.0, 5.0, 2.0, (0, 0, 1), 1.0),                         # a NaN
         rr.car(c, c, np.nan, 0.0, 5.0, 2.0, (0, 0, 1), 1.0),
         rr.car(c + 2.2, c - 3.1, 0.0, 0.0, 5.3, 2.1, (0.6, 0.1, 0.7), 0.0),            # alpha 0 (and a zero heading)
         rr.car(c - 1.1, c - 4.2, 0.0, 0.0, 4.3, 2.3, (0.6, 0.6, 0.1), 0.9),            # zero heading = (1, 0)
         rr.polyline(0, 5, 1.7, (0.1, 0.1, 0.6), 0.5), rr.polyline(5, 6, 3.0, (1, 0, 0), 1.0), rr.polyline(6, 10, 2.2, (0.0, 0.6, 0.6), 0.7),
         rr.polyline(10, 13, 2.0, (1, 0, 0), 1.0), rr.polyline(3, 3, 2.0, (1, 0, 0), 1.0),
         rr.disc(c + 1.0, c + 1.1, 5.2, (0.9, 0.8, 0.1), 0.6), rr.disc(c + 2.9, c + 1.4, 5.2, (0.9, 0.8, 0.1), 0.6),       # two overlapping discs
         rr.disc(np.nan, c, 3.0, (1, 0, 0), 1.0), rr.disc(-30.0, 5.0, 4.0, (1, 0, 0), 1.0), rr.disc(0.2, 0.3, 3.1, (0.3, 0.3, 0.3), 1.0)]
    return np.stack(P), V


RESTATED_CASES = [(1, 'special'), (1, 3), (15, 40), (16, 0), (16, 1), (17, 'special'), (17, PASS), (20, 40), (33, PASS + 1), (33, 'special'),
                  (65, 3 * PASS - 5), (65, 'special')]


@pytest.mark.parametrize('where', BOTH)
def test_kernel_equals_the_float64_restatement(on, where):
    dev = on(where)
    env = Env(dev)
    shares = {}
    for Lp, n in RESTATED_CASES:
        prims, verts = special_prims(Lp) if n == 'special' else rr.random_prims(n, Lp, seed=rr.case_seed(Lp, n))
        if Lp == 33 and n == PASS + 1:
            prims[PASS] = rr.disc(16.4, 16.6, 40.0, (0.0, 0.2, 0.4), 1.0)           # the first primitive of the second pass hides the first pass
        bounds = [-20.0, -20.0, 20.0, 20.0]
        pose = [[60.0, 70.0, 0.6, 0.8]]
        got = tables(dev, env, pose, [0], bounds, Lp, prims, verts, [[0, prims.shape[0]]])[0]
        crop = crop_of(dev, env, pose, [0], bounds, Lp)[0]
        want, margin = rr.render_ref(prims, verts, Lp, rr.composite_map(crop, LAYER_RGB, render.MAP_ALPHAS))
        coord = max([float(Lp)] + [float(np.nanmax(np.abs(a))) for a in (prims[:, 1:3], prims[:, 5:7], verts) if a.size and not np.isnan(a).all()])
        coord = min(coord, 3.0 * Lp + 100.0)
        left_out = margin < 16 * EPS32 * coord
        assert left_out.mean() <= 0.02, 'L %d, %s primitives: %.1f %% of the pixels sit on a boundary' % (Lp, n, 100 * left_out.mean())
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32)).max(axis=2)
        assert diff[~left_out].max(initial=0) <= 1, 'L %d, %s primitives: %d pixels off by more than one level' % (Lp, n, int((diff[~left_out] > 1).sum()))
        shares[(Lp, n)] = (float((diff[~left_out] == 1).mean()) if (~left_out).any() else 0.0, float(left_out.mean()))
        if n == 0:
            assert np.array_equal(got, rr.to_bytes(rr.composite_map(crop, LAYER_RGB, render.MAP_ALPHAS)))
        if Lp == 33 and n == PASS + 1:
            assert np.array_equal(got[16, 16], rr.to_bytes(np.array([0.0, 0.2, 0.4], dtype=np.float32)))
    print('%s: (L, primitives) -> (share of pixels one level off, share left out): %s' % (where, shares))


@pytest.mark.parametrize('where', BOTH)
def test_a_path_blends_once_and_every_marker_on_its_own(on, where):
    dev = on(where)
    env = Env(dev)
    Lp = 17
    V = np.array([[2.0, 2.0], [15.0, 15.0], [2.0, 15.0], [15.0, 2.0]], dtype=np.float32)          # crosses itself at (8.5, 8.5)
    line = rr.polyline(0, 4, 3.0, (0.0, 0.0, 1.0), 0.5)
    discs = [rr.disc(6.5, 8.5, 8.0, (1.0, 0.0, 0.0), 0.5), rr.disc(10.5, 8.5, 8.0, (1.0, 0.0, 0.0), 0.5)]
    one = lambda c, col, a: c + np.float32(a) * (np.asarray(col, dtype=np.float32) - c)
    got = tables(dev, env, [[0, 0, 1, 0]], [0], [-1.0, -1, 1, 1], Lp, np.stack([line]), V, [[0, 1]], no_map=[1])[0]
    assert np.array_equal(got[8, 8], rr.to_bytes(one(WHITE, (0, 0, 1), 0.5))), 'the crossing of a path is stroked once'
    got = tables(dev, env, [[0, 0, 1, 0]], [0], [-1.0, -1, 1, 1], Lp, np.stack(discs), V, [[0, 2]], no_map=[1])[0]
    assert np.array_equal(got[8, 8], rr.to_bytes(one(one(WHITE, (1, 0, 0), 0.5), (1, 0, 0), 0.5))), 'overlapping markers blend twice'
    assert np.array_equal(got[8, 4], rr.to_bytes(one(WHITE, (1, 0, 0), 0.5)))


# ------------------------------------------------------------------------------------------------------------------------
# 3. exact cases
# ------------------------------------------------------------------------------------------------------------------------

def crop_of(dev, env, pose, mapix, bounds, Lp):
    e = ops._OverrideEnv(env, bounds, Lp, Lp)
    return ops.map_crop(e, torch.as_tensor(pose, dtype=torch.float32).reshape(-1, 4).to(dev), torch.as_tensor(mapix).to(dev)).cpu().numpy()


NOPRIM = (np.zeros((0, 16), dtype=np.float32), np.zeros((0, 2), dtype=np.float32))


@pytest.mark.parametrize('where', BOTH)
@pytest.mark.parametrize('C', [1, 4, 6])
def test_map_only_picture_is_the_composited_crop(on, where, C):
    dev = on(where)
    env = Env(dev, C=C, M=2)
    pose = [[60.0, 70.0, 0.6, 0.8], [33.25, 20.5, -1.0, 0.0], [40.0, 41.0, 0.28, -0.96]]
    mapix = [0, 1, 1]
    bounds = [[-20.0, -20.0, 20.0, 20.0], [-9.5, -9.5, 9.5, 9.5], [-20.0, -20.0, 20.0, 20.0]]
    for Lp in (20, 33):
        got = tables(dev, env, pose, mapix, bounds, Lp, NOPRIM[0], NOPRIM[1], [[0, 0]] * 3)
        for f in range(3):
            crop = crop_of(dev, env, [pose[f]], [mapix[f]], bounds[f], Lp)[0]
            assert crop.shape == (C, Lp, Lp) and 0 < crop[0].mean() < 1
            assert np.array_equal(got[f], rr.to_bytes(rr.composite_map(crop, LAYER_RGB, render.MAP_ALPHAS))), (Lp, f)


@pytest.mark.parametrize('where', BOTH)
def test_orientation_no_map_and_a_closed_form_car(on, where):
    dev = on(where)
    env = Env(dev, C=1)
    # one raster pixel set: world (x, y) = (10, 6) m at 0.25 m per pixel -> raster[24, 40]; a crop of 16 pixels of 1 m around (8, 8),
    # heading +x, looks it up at l index 10, w index 6: picture column 10, row 16 - 1 - 6
    env.nusc_raster.zero_()
    env.nusc_raster[0, 0, 24, 40] = 1
    b = [-8.0, -8.0, 7.0, 7.0]
    got = tables(dev, env, [[8.0, 8.0, 1.0, 0.0]], [0], b, 16, NOPRIM[0], NOPRIM[1], [[0, 0]])[0]
    crop = crop_of(dev, env, [[8.0, 8.0, 1.0, 0.0]], [0], b, 16)[0]
    assert crop[0, 10, 6] == 1 and crop.sum() == 1
    dark = rr.to_bytes(LAYER_RGB[0])
    want = np.full((16, 16, 3), 255, dtype=np.uint8)
    want[9, 10] = dark
    assert np.array_equal(got, want)
    # no_map: white whatever the raster holds
    env.nusc_raster.fill_(1)
    got = tables(dev, env, [[8.0, 8.0, 1.0, 0.0]] * 2, [0, 0], b, 16, NOPRIM[0], NOPRIM[1], [[0, 0]] * 2, no_map=[1, 0])
    assert (got[0] == 255).all() and (got[1] == dark).all()
    # an axis-aligned car with its edges on whole pixels: fill x in [5, 11], y in [6, 10]; outline 2 wide: [4, 12] x [5, 11] without
    # (6, 10) x (7, 9); heading stroke 2 wide: x in [7, 12], y in [7, 9]
    a = np.float32(0.5)
    col = np.array([0.2, 0.4, 0.6], dtype=np.float32)
    prims = np.stack([rr.car(8.0, 8.0, 1.0, 0.0, 6.0, 4.0, col, a, se=2.0, sl=2.0)])
    got = tables(dev, env, [[8.0, 8.0, 1.0, 0.0]], [0], b, 16, prims, NOPRIM[1], [[0, 1]], no_map=[1])[0]
    c = np.ones((16, 16, 3), dtype=np.float32)
    x = np.arange(16)[None, :] + 0.5
    y = (15 - np.arange(16))[:, None] + 0.5
    box = lambda x0, x1, y0, y1: ((x > x0) & (x < x1) & (y > y0) & (y < y1))[:, :, None]
    c = np.where(box(5, 11, 6, 10), c + a * (col - c), c)
    c = np.where(box(4, 12, 5, 11) & ~box(6, 10, 7, 9), c + a * (0 - c), c)
    c = np.where(box(7, 12, 7, 9), c + a * (0 - c), c)
    assert np.array_equal(got, rr.to_bytes(c))
    assert (got[5, 8] == 128).all() and (got[3, 8] == 255).all() and (got[7, 8] == rr.to_bytes((1 - a) * (WHITE + a * (col - WHITE)))).all()


# ------------------------------------------------------------------------------------------------------------------------
# 4. independence; GPU against emulation
# ------------------------------------------------------------------------------------------------------------------------

def crowd(dev):
    """18 pictures of other scenes and maps in one launch; picture 7 is the one under test."""
    env = Env(dev, M=2)
    Lp = 33
    P, V, R, pose, mapix, bounds = [], [], [], [], [], []
    np_, nv = 0, 0
    for f in range(18):
        p, v = rr.random_prims(5 + 17 * f, Lp, seed=77 + f)
        for r in p:
            if int(r[0:1].view(np.int32)[0]) == rr.POLYLINE:
                r[13:15].view(np.int32)[:] += nv
        P.append(p); V.append(v)
        R.append([np_, np_ + p.shape[0]])
        np_ += p.shape[0]; nv += v.shape[0]
        pose.append([40.0 + 3 * f, 50.0 + 2 * f, np.cos(0.4 * f), np.sin(0.4 * f)])
        mapix.append(f % 2)
        bounds.append([-10.0 - f, -10.0 - f, 10.0 + f, 10.0 + f])
    return env, Lp, np.concatenate(P), np.concatenate(V), R, pose, mapix, bounds


@pytest.mark.parametrize('where', BOTH)
def test_a_picture_does_not_depend_on_its_neighbours(on, where):
    dev = on(where)
    env, Lp, P, V, R, pose, mapix, bounds = crowd(dev)
    allp = tables(dev, env, pose, mapix, bounds, Lp, P, V, R)
    alone = tables(dev, env, [pose[7]], [mapix[7]], [bounds[7]], Lp, P, V, [R[7]])
    assert np.array_equal(allp[7], alone[0])
    assert len({allp[f].tobytes() for f in range(18)}) == 18


@pytest.mark.gpu
def test_gpu_and_emulation_agree(on, monkeypatch):
    env, Lp, P, V, R, pose, mapix, bounds = crowd(torch.device('cuda', 0))
    gpu = tables(torch.device('cuda', 0), env, pose, mapix, bounds, Lp, P, V, R)
    dev = on('cpu')
    env = crowd(dev)[0]
    emu = tables(dev, env, pose, mapix, bounds, Lp, P, V, R)
    diff = np.abs(gpu.astype(np.int32) - emu.astype(np.int32))
    print('GPU against emulation: %d of %d bytes differ' % (int((diff > 0).sum()), diff.size))
    assert diff.max() <= 1


# ------------------------------------------------------------------------------------------------------------------------
# 5. Agg, a gross-error check
# ------------------------------------------------------------------------------------------------------------------------
AGG_MEAN_ABS_MEASURED = 1.0076      # levels, measured when this test was written (profiles/r26_render_ratios.md)


def agg_picture(crop, draw_list, Lp):
    import matplotlib
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    from matplotlib.patches import Polygon
    dpi = 100.0
    fig = Figure(figsize=(Lp / dpi, Lp / dpi), dpi=dpi)
    canvas = FigureCanvasAgg(fig)
    ax = fig.add_axes([0, 0, 1, 1])
    ax.axis('off')
    pt = render.px_per_pt(Lp) * 72.0 / dpi           # a reference point in points of this canvas
    ext = (0, Lp, 0, Lp)                         # pixel i covers [i, i + 1]: no half-pixel offset, as the kernel
    ax.imshow(np.ones((Lp, Lp, 3)), origin='lower', extent=ext, interpolation='nearest')
    for i in range(crop.shape[0]):
        rgba = np.zeros((Lp, Lp, 4))
        rgba[:, :, :3] = render.to_rgb(render.MAP_COLORS[i])
        rgba[:, :, 3] = crop[i].T * render.MAP_ALPHAS[i]
        ax.imshow(rgba, origin='lower', extent=ext, interpolation='nearest')
    for a in draw_list:
        if a['kind'] == 'markers':
            ax.scatter(a['verts'][:, 0], a['verts'][:, 1], c=a['colors'], s=a['size'] * pt * pt, alpha=a['alpha'], linewidths=render.MARKER_EDGE_PT * pt, zorder=1)
        elif a['kind'] == 'line':
            ax.plot(a['verts'][:, 0], a['verts'][:, 1], '-', c=a['color'], alpha=a['alpha'], linewidth=a['linewidth'] * pt, zorder=2)
        else:
            art = as_artists([a])
            ax.add_patch(Polygon(art[0][6][:4], closed=True, facecolor=a['color'], edgecolor='k', alpha=a['alpha'], linewidth=pt, zorder=3))
            ax.plot(art[1][6][:, 0], art[1][6][:, 1], 'k', alpha=a['alpha'], linewidth=1.5 * pt, zorder=3)
    ax.set_xlim(0, Lp)
    ax.set_ylim(0, Lp)
    canvas.draw()
    return np.asarray(canvas.buffer_rgba())[:, :, :3].copy()


def test_agg_draws_much_the_same_picture(on):
    pytest.importorskip('matplotlib')
    dev = on('cpu')
    env = Env(dev, hw=1024)
    Lp = 96
    scene = rr.adv_scenes()['sc_0002_early']
    plan = viz_adv_gen.plan_scenario(scene, 'adv', env, '/x', L=Lp, W=Lp)
    dl = plan['pictures'][0][1]
    got = render.render_pictures(env, plan['crop_kin'].reshape(1, 4), [plan['mapix']], plan['bounds'], Lp, [dl]).numpy()[0]
    crop = crop_of(dev, env, plan['crop_kin'].reshape(1, 4), [plan['mapix']], plan['bounds'], Lp)[0]
    agg = agg_picture(crop, dl, Lp)
    assert agg.shape == got.shape == (Lp, Lp, 3)
    mad = float(np.abs(agg.astype(np.float64) - got.astype(np.float64)).mean())
    flipped = float(np.abs(agg[::-1].astype(np.float64) - got.astype(np.float64)).mean())
    print('mean |Agg - kernel rule| = %.4f levels (upside down: %.4f)' % (mad, flipped))
    assert (got != 255).any() and len(dl) >= 8
    assert mad <= 2 * AGG_MEAN_ABS_MEASURED


# ------------------------------------------------------------------------------------------------------------------------
# 6. host
# ------------------------------------------------------------------------------------------------------------------------

def read_png(path):
    """8-bit RGB, filter 0 only (what write_png writes) -> (H, W, 3)."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, size = 8, b'', None
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b'IHDR':
            size = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    W, H = size[:2]
    assert size[2:] == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (65, 65)])
def test_write_png_round_trips(tmp_path, shape):
    Image = pytest.importorskip('PIL.Image')
    a = np.random.RandomState(shape[0]).randint(0, 256, size=shape + (3,)).astype(np.uint8)
    p = str(tmp_path / 'a.png')
    render.write_png(p, a)
    with Image.open(p) as im:
        assert im.mode == 'RGB' and np.array_equal(np.asarray(im), a)
    assert np.array_equal(read_png(p), a)
    with pytest.raises(ValueError):
        render.write_png(p, a.astype(np.float32))


def test_error_paths(on, monkeypatch, tmp_path):
    dev = on('cpu')
    env = Env(dev)
    one = (torch.tensor([[8.0, 8.0, 1.0, 0.0]]), [0], [-4.0, -4.0, 4.0, 4.0])
    with pytest.raises(ValueError, match='square'):
        render.render_pictures(env, *one, 16, [[]], W_=17)
    job, mp = L.StriveRenderJob(), L.StriveMap()
    job.F, job.L, job.W, mp.C = 0, 16, 17, 4
    import ctypes
    with pytest.raises(L.StriveHipError, match='square'):
        ops._lib_for().call('strive_render_pictures', ctypes.byref(mp), ctypes.byref(job), L.ptr(torch.zeros(4, dtype=torch.uint8)), None)
    job.W, mp.C = 16, 7
    with pytest.raises(L.StriveHipError, match='layers'):
        ops._lib_for().call('strive_render_pictures', ctypes.byref(mp), ctypes.byref(job), L.ptr(torch.zeros(4, dtype=torch.uint8)), None)
    with pytest.raises(ValueError, match='layers'):
        render.render_pictures(Env(dev, C=7), *one, 16, [[]])
    with pytest.raises(ValueError, match='map index'):
        render.render_pictures(env, one[0], [1], one[2], 16, [[]])
    scene = dict(rr.dir_scenes()['sc_0006_alone'])
    scene['map'] = 'boston-seaport'
    with pytest.raises(ValueError, match='not in list'):
        viz_scenario_dir.plan_scenario(scene, env, str(tmp_path / 'x'), L=16, W=16)
    with pytest.raises(ValueError, match='square'):
        viz_scenario_dir.plan_scenario(scene, env, str(tmp_path / 'x'), L=16, W=17)
    monkeypatch.setenv('PATH', str(tmp_path))
    for main, extra in ((viz_scenario_dir.main, []), (viz_adv_gen.main, [])):
        with pytest.raises(RuntimeError, match='ffmpeg'):
            main(['--scenarios', G18, '--out', str(tmp_path / 'o'), '--map_world', 'synthetic', '--mp4'] + extra)
    assert not (tmp_path / 'o').exists()


@pytest.mark.parametrize('nscenes', [1, 5])
def test_drivers_launch_once_and_read_back_once_per_batch(on, monkeypatch, tmp_path, nscenes):
    dev = on('cpu')
    env = Env(dev, hw=1024)
    calls = {'launch': 0, 'read': 0, 'pictures': 0}
    real_call = ops._lib_for().call
    real_read = render.read_back

    def counting_call(name, *a):
        calls['launch'] += name == 'strive_render_pictures'
        return real_call(name, *a)

    def counting_read(p):
        calls['read'] += 1
        calls['pictures'] += p.shape[0]
        return real_read(p)
    monkeypatch.setattr(ops._lib_for(), 'call', counting_call)
    monkeypatch.setattr(render, 'read_back', counting_read)
    src = tmp_path / 'scenes'
    src.mkdir()
    files = sorted(os.path.join(d, f) for d, _, fs in os.walk(G18) for f in fs)[:nscenes]
    for f in files:
        shutil.copy(f, str(src / os.path.basename(f)))
    n = viz_scenario_dir.viz_scenario_dir({'scenarios': str(src), 'out': str(tmp_path / 'a'), 'viz_video': True, 'L': 8, 'batch_scenes': 36}, env)
    assert (calls['launch'], calls['read']) == (1, 1) and calls['pictures'] == n > nscenes
    n = viz_scenario_dir.viz_scenario_dir({'scenarios': str(src), 'out': str(tmp_path / 'b'), 'L': 8, 'batch_scenes': 2}, env)
    assert (calls['launch'], calls['read']) == (1 + (nscenes + 1) // 2,) * 2 and n == nscenes
    calls.update(launch=0, read=0, pictures=0)
    scenes = viz_adv_gen.read_adv_scenes(str(src))
    n = viz_adv_gen.qual_eval({'adv_sol_success': scenes}, ['adv_sol_success'], ['init', 'adv', 'sol'], env, str(tmp_path / 'c'), viz_video=True, L=8)
    assert (calls['launch'], calls['read']) == (1, 1) and calls['pictures'] == n
    assert n == sum(1 + 2 * (1 + s['past'].size(1) + s['fut_adv'].size(1)) for s in scenes)       # no fut_sol: two stages, one map picture


# ------------------------------------------------------------------------------------------------------------------------
# 7. the command lines, on the GPU
# ------------------------------------------------------------------------------------------------------------------------

def boxes_mask(draw_list, Lp, grow):
    """Pixels of an Lp picture that a primitive's bounding box (grown by its stroke and ``grow``) touches, and one mask per primitive."""
    masks = []
    k = render.px_per_pt(Lp)
    for a in draw_list:
        if a['kind'] == 'car':
            v, g = as_artists([a])[0][6], 0.5 * (render.EDGE_PT + render.HEADING_PT) * k
        elif a['kind'] == 'line':
            v, g = a['verts'], 0.5 * a['linewidth'] * k
        else:
            v, g = a['verts'], 0.5 * (np.sqrt(a['size']) + render.MARKER_EDGE_PT) * k
        if v.shape[0] == 0:
            continue
        x0, x1 = int(np.floor(v[:, 0].min() - g - grow)), int(np.ceil(v[:, 0].max() + g + grow))
        y0, y1 = int(np.floor(v[:, 1].min() - g - grow)), int(np.ceil(v[:, 1].max() + g + grow))
        m = np.zeros((Lp, Lp), dtype=bool)
        m[max(0, Lp - y1):max(0, Lp - y0), max(0, x0):max(0, x1)] = True
        masks.append(m)
    return masks


def check_overview(overview, map_only, draw_list, Lp):
    changed = (overview != map_only).any(axis=2)
    masks = boxes_mask(draw_list, Lp, 0.0)
    assert not (changed & ~np.logical_or.reduce(masks)).any(), 'the overview differs from the map outside every bounding box'
    for m in masks:
        assert not m.any() or (changed & m).any(), 'a primitive left no trace in its bounding box'


@pytest.mark.gpu
def test_viz_scenario_dir_command_line(tmp_path):
    out = str(tmp_path / 'out')
    src = os.path.join(G18, 'adv_sol_success')
    n = viz_scenario_dir.main(['--scenarios', src, '--out', out, '--map_world', 'synthetic', '--L', '96', '--viz_video'])
    scenes = viz_scenario_dir.read_adv_scenes(src)
    want = set()
    for s in scenes:
        NT = s['scene_past'].size(1) + s['scene_fut'].size(1)
        want |= {s['name'] + '.png'} | {os.path.join(s['name'] + '_vid_000', 'frame%04d.png' % t) for t in range(NT)}
    have = {os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs}
    assert have == want and n == len(want)
    for f in have:
        assert read_png(os.path.join(out, f)).shape == (96, 96, 3)
    env = viz_scenario_dir.synthetic_map_world('cuda:0')
    for s in scenes:
        plan = viz_scenario_dir.plan_scenario(s, env, os.path.join(out, s['name']), L=96, W=96)
        bare = render.render_pictures(env, plan['crop_kin'].reshape(1, 4), [plan['mapix']], plan['bounds'], 96, [[]]).cpu().numpy()[0]
        assert (bare != 255).any()
        check_overview(read_png(os.path.join(out, s['name'] + '.png')), bare, plan['pictures'][0][1], 96)


@pytest.mark.gpu
def test_viz_adv_gen_command_line(tmp_path):
    out = str(tmp_path / 'out')
    n = viz_adv_gen.main(['--scenarios', G18, '--out', out, '--map_world', 'synthetic', '--L', '96', '--viz_video', '--viz_res', 'adv_sol_success',
                          'adv_failed', '--viz_stage', 'init', 'adv', 'sol'])
    want = set()
    env = viz_scenario_dir.synthetic_map_world('cuda:0')
    for cat in ('adv_sol_success', 'adv_failed'):
        for s in viz_adv_gen.read_adv_scenes(os.path.join(G18, cat)):
            NT = s['past'].size(1) + s['fut_adv'].size(1)
            base = os.path.join(cat, s['name'])
            want |= {os.path.join(base, 'viz_init_map.png')}
            for stage in ('init', 'adv'):
                want |= {os.path.join(base, 'viz_%s.png' % stage)} | {os.path.join(base, 'viz_%s_vid_000' % stage, 'frame%04d.png' % t) for t in range(NT)}
            plan = viz_adv_gen.plan_scenario(s, 'init', env, os.path.join(out, base), L=96, W=96)
            check_overview(read_png(os.path.join(out, base, 'viz_init.png')), read_png(os.path.join(out, base, 'viz_init_map.png')),
                           plan['pictures'][1][1], 96)
    have = {os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs}
    assert have == want and n == len(want)
    for f in have:
        assert read_png(os.path.join(out, f)).shape == (96, 96, 3)
