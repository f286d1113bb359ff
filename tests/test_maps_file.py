"""Maps files (strive_amd/datasets/maps.py) and the lane graphs built on the device (strive_amd/csrc/lane_graph.hip):

  * against fixture g25 -- the reference's own process_lanegraph and flip (tests/golden/make_golden_maps.py);
  * against the float64 restatement of the stated device rule (tests/lane_graph_restated.py), every output byte;
  * the edge grid against the host's ``edge_grid`` of the same edge table, identical;
  * sizes, trimming, degrees, refusals, alone against batched, the file format, the rasters, the planner, the command lines.

Without a GPU the kernels run through the host emulation of the unmodified .hip (tests/hipemu); the ``gpu`` tests run the same
checks on the MI355X.  The restatement is what links the two: emulation == restatement and GPU == restatement, byte for byte.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import lane_graph_restated as lr
from strive_amd import synth
from strive_amd.datasets import maps
from strive_amd.datasets.map_env import map_env_from_geometry
from strive_amd.planners.planner import PlannerConfig
from strive_amd.planners.hardcode_goalcond_nusc import HardcodeNuscPlanner, PackedLaneGraph, CONFIG_DICT, edge_grid

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 1e-6


@pytest.fixture()
def emu_ops():
    from planner_worlds import emulated_ops
    with emulated_ops() as emu:
        yield emu


def build(t, device, eps=EPS, flip=False, height=0.0):
    return maps.build_lane_graph(t, eps=eps, flip=flip, height=height, device=device)


def assert_bytes_equal(got, want, what=''):
    """got: DeviceLaneGraph.host_tables(); want: the restated dict"""
    want = lr.device_view(want)
    for k in lr.DEVICE_TABLES:
        a, b = got[k].view(np.uint8), want[k].astype(got[k].dtype, copy=False).view(np.uint8)
        assert a.shape == b.shape, '%s %s: %d bytes, the restatement has %d' % (what, k, a.size, b.size)
        assert int((a != b).sum()) == 0, '%s %s: %d bytes differ' % (what, k, int((a != b).sum()))


def against_restatement(t, device, what='', flip=False, height=0.0):
    want = lr.restate(t, EPS, flip, height)
    g = build(t, device, flip=flip, height=height)
    assert (g.N, g.M, g.MI) == (want['xy'].shape[0], want['edges'].shape[0], want['pred_idx'].shape[0])
    assert_bytes_equal(g.host_tables(), want, what)
    return g, want


# ------------------------------------------------------------------------------------------------
# 1. fixture g25: the reference
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def g25():
    z = np.load(os.path.join(GOLDEN, 'g25_lane_graph.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def g25_map(m):
    z = g25()
    t = {k: z['m%d_%s' % (m, k)] for k in ('pts', 'lane_ptr', 'out_ptr', 'out_idx', 'in_ptr', 'in_idx')}
    name = str(z['names'][m])
    return name, t, name.startswith('singapore'), float(z['heights'][m])


def lists_of(z, m, key):
    p, i = z['m%d_%s_ptr' % (m, key)], z['m%d_%s_idx' % (m, key)].tolist()
    return [i[p[v]:p[v + 1]] for v in range(len(p) - 1)]


def check_g25(device):
    z = g25()
    assert float(z['eps']) == EPS and [str(n).split('-')[0] for n in z['names']] == ['singapore', 'singapore', 'boston', 'singapore']
    differ = total = 0
    for m in range(4):
        name, t, flip, height = g25_map(m)
        g = build(t, device, flip=flip, height=height)
        assert np.array_equal(g['xy'], z['m%d_xy' % m]), name
        assert g['out_edges'] == lists_of(z, m, 'out_edges') and g['in_edges'] == lists_of(z, m, 'in_edges'), name
        assert np.array_equal(g['edgeixes'], z['m%d_edgeixes' % m]), name
        want = z['m%d_edges' % m]
        assert np.array_equal(g['edges'][:, :2], want[:, :2]), name
        # one differently rounded product under a square root and one division: every entry within 2 units in the last place
        u = lr.ulps(g['edges'][:, 2:5], want[:, 2:5])
        assert int(u.max()) <= 2, '%s: %d ulp' % (name, int(u.max()))
        differ += int((u != 0).sum())
        total += u.size
        assert g['ee2ix'] == {(int(a), int(b)): k for k, (a, b) in enumerate(z['m%d_edgeixes' % m].tolist())}
    print('g25: %d of %d entries of edges[:, 2:5] are not bit-equal to the reference' % (differ, total))
    return differ


def test_g25_reference_cpu(emu_ops):
    check_g25('cpu')


@pytest.mark.gpu
def test_g25_reference_gpu():
    check_g25('cuda')


def test_g25_length_rule_was_chosen_by_counting():
    """the rule stated in include/strive_hip.h agrees with the reference's edge lengths more often than the unfused one"""
    fused = unfused = total = 0
    for m in range(4):
        name, t, flip, height = g25_map(m)
        want = g25()['m%d_edges' % m][:, 4]
        fused += int((lr.restate(t, EPS, flip, height)['edges'][:, 4] == want).sum())
        unfused += int((lr.restate(t, EPS, flip, height, length=lr.length_unfused)['edges'][:, 4] == want).sum())
        total += want.size
    assert fused == total and unfused < fused


# ------------------------------------------------------------------------------------------------
# 2. the restatement of the device rule: every byte; PackedLaneGraph of the restated dict
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def synth_world():
    lanes, out, inc = synth.dirty_lanes(*synth.make_lanes(extent=96.0))
    return lr.tables(lanes, out, inc)


def check_restatement(device):
    for m in range(4):
        name, t, flip, height = g25_map(m)
        g, want = against_restatement(t, device, name, flip, height)
        host = PackedLaneGraph({k: want[k] for k in maps.DeviceLaneGraph.KEYS}, 2.0, device)
        dev = g.packed(2.0)
        assert (host.N, host.M, host.xydistmax) == (dev.N, dev.M, dev.xydistmax)
        assert {k: host.grid[k] for k in dev.grid} == dev.grid
        assert sorted(host.t) == sorted(dev.t)
        for k in host.t:
            a = host.t[k].cpu().numpy()
            b = dev.t[k].cpu().numpy().view(np.uint8).reshape(-1)[:a.size]
            if k in ('succ', 'pred'):
                a, b = a.view(lr.LANE_NODE), b.view(lr.LANE_NODE)
                assert np.array_equal(a['n'], b['n']) and np.array_equal(a['node'], b['node']) and int(lr.ulps(a['len'], b['len']).max()) <= 2
            elif k in ('succ_len', 'pred_len', 'edges', 'xy'):
                assert int(lr.ulps(a.view(np.float64), b.view(np.float64)).max()) <= (0 if k in ('xy', 'edges') else 2), k
            else:
                assert np.array_equal(a, b), k
    against_restatement(synth_world(), device, 'synthetic')


def test_restatement_cpu(emu_ops):
    check_restatement('cpu')


@pytest.mark.gpu
def test_restatement_gpu():
    check_restatement('cuda')


def test_lengths_are_symmetric_and_come_from_the_final_positions(emu_ops):
    name, t, flip, height = g25_map(0)
    assert flip
    g = build(t, 'cpu', flip=True, height=height)
    h = g.host_tables()
    xy = h['xy'].reshape(-1, 2)
    fwd = {(v, int(u)): float(l) for v in range(g.N) for u, l in zip(h['succ_idx'][h['succ_ptr'][v]:h['succ_ptr'][v + 1]],
                                                                      h['succ_len'][h['succ_ptr'][v]:h['succ_ptr'][v + 1]])}
    n = 0
    for v in range(g.N):
        for u, l in zip(h['pred_idx'][h['pred_ptr'][v]:h['pred_ptr'][v + 1]], h['pred_len'][h['pred_ptr'][v]:h['pred_ptr'][v + 1]]):
            assert float(l) == lr.length(xy[u, 0] - xy[v, 0], xy[u, 1] - xy[v, 1])
            if (int(u), v) in fwd:
                assert fwd[(int(u), v)] == float(l)
                n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------------
# 3. the edge grid against edge_grid()
# ------------------------------------------------------------------------------------------------

def edge_tables():
    g = lr.restate(g25_map(2)[1], EPS)['edges']
    border = np.array([[4.0, 8.0, 1.0, 0.0, 4.0], [8.0, 8.0, 0.0, 1.0, 4.0], [12.5, 3.25, -0.6, 0.8, 2.5]])     # the first lies on y = 8
    single = np.array([[103.7, -20.4, 0.28, -0.96, 3.1]])
    return {'g25': g, 'border': border, 'single': single, 'synthetic': lr.restate(synth_world(), EPS)['edges']}


def check_edge_grid(device):
    for name, edges in edge_tables().items():
        for margin in (2.0, 0.0):
            for cell in (4.0, 1.5):
                want = edge_grid(edges, margin, cell)
                e = torch.from_numpy(np.ascontiguousarray(edges)).to(device)
                before = maps.stats['readbacks']
                grid, cell_ptr, cell_edges = maps.device_edge_grid(e, edges.shape[0], margin, cell)
                assert maps.stats['readbacks'] - before == 1
                what = '%s margin %g cell %g' % (name, margin, cell)
                assert grid == {k: want[k] for k in grid}, what
                assert np.array_equal(cell_ptr.cpu().numpy(), want['cell_ptr']), what
                assert np.array_equal(cell_edges.cpu().numpy(), want['cell_edges']), what


def test_edge_grid_cpu(emu_ops):
    check_edge_grid('cpu')


@pytest.mark.gpu
def test_edge_grid_gpu():
    check_edge_grid('cuda')


# ------------------------------------------------------------------------------------------------
# 4. sizes
# ------------------------------------------------------------------------------------------------

def chain_world(npoints, seed=5):
    """a chain of lanes of the given point counts; every other lane ends ON its successor's first point"""
    rs = np.random.RandomState(seed)
    lanes, p = [], rs.uniform(100, 200, 2)
    for k, n in enumerate(npoints):
        ln = lr.walk(rs, p, n, turn=0.02)
        lanes.append(ln)
        p = ln[-1] if k % 2 == 0 else ln[-1] + rs.uniform(0.4, 0.6, 2)
    out = [[k + 1] for k in range(len(lanes) - 1)] + [[]]
    return lr.tables(lanes, out)


SIZE_WORLDS = {'1 lane': [2], '2 lanes': [3, 2], '65 lanes': [2, 3, 64, 65, 5] * 13, '257 lanes': ([2, 3, 7, 4] * 64 + [257])[:257],
               'long lanes': [1025, 257, 64, 65, 3, 2]}


@pytest.mark.parametrize('name', sorted(SIZE_WORLDS))
def test_sizes(emu_ops, name):
    npoints = SIZE_WORLDS[name]
    assert name != '257 lanes' or (len(npoints) == 257 and npoints[-1] == 257)
    g, want = against_restatement(chain_world(npoints), 'cpu', name)
    trimmed = sum(1 for k in range(len(npoints) - 1) if k % 2 == 0)
    assert g.N == sum(npoints) - trimmed


def test_runs_of_near_equal_points(emu_ops):
    rs = np.random.RandomState(9)
    base = lr.walk(rs, (50.0, 60.0), 130)
    mid = lr.with_run(base, 10, count=2)                  # points 10, 11, 12 near-equal: the last of the run survives
    end = lr.with_run(base, 129, count=2)                 # a run that ends at the lane's end
    across = lr.with_run(base, 62, count=4)               # points 62 .. 66: across the 64-point boundary
    for name, lane, gone in (('mid', mid, [10, 11]), ('end', end, [129, 130]), ('across', across, [62, 63, 64, 65])):
        g, want = against_restatement(lr.tables([lane], [[]]), 'cpu', name)
        keep = np.ones((lane.shape[0],), dtype=bool)
        keep[gone] = False
        assert np.array_equal(g['xy'], lane[keep]) and g.N == 130 and np.array_equal(g['xy'], base), name


# ------------------------------------------------------------------------------------------------
# 5. trimming   6. degrees
# ------------------------------------------------------------------------------------------------

def test_trimming(emu_ops):
    rs = np.random.RandomState(3)
    A = lr.walk(rs, (10.0, 20.0), 6)
    B, C, X = lr.walk(rs, A[-1], 4), lr.walk(rs, A[-2], 3), lr.walk(rs, A[-1] + 0.5, 3)
    # one trim
    g, _ = against_restatement(lr.tables([A, B], [[1], []]), 'cpu', 'one trim')
    assert g.N == 5 + 4 and g['out_edges'][4] == [5] and g['in_edges'][5] == [4] and np.array_equal(g['xy'][:5], A[:5])
    # two trims in a row from two successors (the second comparison uses the new last point); an absent successor between them
    g, _ = against_restatement(lr.tables([A, B, C], [[1, -1, 2], [], []]), 'cpu', 'two trims')
    assert g.N == 4 + 4 + 3 and g['out_edges'][3] == [4, 8] and np.array_equal(g['xy'][:4], A[:4])
    # a successor that is near but not within eps does not trim
    g, _ = against_restatement(lr.tables([A, X], [[1], []]), 'cpu', 'no trim')
    assert g.N == 6 + 3
    # a two-point lane trimmed to one node that carries both connection lists
    D = lr.walk(rs, (40.0, 40.0), 2)
    E, F = lr.walk(rs, D[-1], 3), lr.walk(rs, D[0] - 5.0, 4)
    g, _ = against_restatement(lr.tables([F, D, E], [[1], [2], []]), 'cpu', 'one node')
    assert g.N == 4 + 1 + 3 and g['out_edges'][4] == [5] and g['in_edges'][4] == [3] and np.array_equal(g['xy'][4], D[0])
    # a ring lane whose successor is itself
    ang = np.linspace(0.0, 2 * np.pi, 9)
    ring = np.array([70.0, 70.0]) + 6.3 * np.stack([np.cos(ang), np.sin(ang)], -1)
    ring[-1] = ring[0]
    g, _ = against_restatement(lr.tables([ring], [[0]], [[0]]), 'cpu', 'ring')
    assert g.N == 8 and g['out_edges'][7] == [0] and g['in_edges'][0] == [7] and g.M == 8


def test_degrees_past_the_inline_slots_in_list_order(emu_ops):
    rs = np.random.RandomState(4)
    lanes, out, inc = [], [], []
    for deg in range(1, 10):                               # out-degrees 1 .. 9
        hub = len(lanes)
        H = lr.walk(rs, (100.0 * deg, 50.0), 3)
        lanes.append(H)
        spokes = list(range(hub + 1, hub + 1 + deg))[::-1]                 # list order is not lane order
        out.append(spokes)
        inc.append([])
        for k in range(deg):
            lanes.append(lr.walk(rs, H[-1] + np.array([1.0, 0.4 * k]), 2))
            out.append([])
            inc.append([hub])
    for deg in range(1, 7):                                # in-degrees 1 .. 6
        sink = len(lanes)
        S = lr.walk(rs, (100.0 * deg, 500.0), 3)
        lanes.append(S)
        feeders = list(range(sink + 1, sink + 1 + deg))
        out.append([])
        inc.append(feeders[1:] + feeders[:1])
        for k in range(deg):
            lanes.append(lr.walk(rs, S[0] - np.array([3.0, 0.5 * k]), 2))
            out.append([sink])
            inc.append([])
    t = lr.tables(lanes, out, inc)
    g, want = against_restatement(t, 'cpu', 'degrees')
    h = g.host_tables()
    start = np.concatenate([[0], np.cumsum([len(l) for l in lanes])])
    assert sorted(set(int(n) for n in h['succ']['n'])) == [0] + list(range(1, 10))
    assert sorted(set(int(n) for n in h['pred']['n'])) == list(range(0, 7))
    for l in range(len(lanes)):
        last, first = int(start[l + 1]) - 1, int(start[l])
        if out[l]:
            assert g['out_edges'][last] == [int(start[o]) for o in out[l]]
            assert h['succ']['node'][last][:min(4, len(out[l]))].tolist() == [int(start[o]) for o in out[l]][:4]
        if inc[l]:
            assert g['in_edges'][first] == [int(start[o + 1]) - 1 for o in inc[l]]


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------

def test_refusals_name_the_rule_and_the_lowest_lane(emu_ops):
    rs = np.random.RandomState(6)
    ok = [lr.walk(rs, (20.0 * k, 5.0), 4) for k in range(6)]

    def refused(lanes, out, inc=None):
        t = lr.tables(lanes, out, inc)
        with pytest.raises(lr.Refusal) as want:
            lr.restate(t, EPS)
        with pytest.raises(ValueError) as got:
            maps.build_lane_graph(t, eps=EPS, device='cpu', name='boston-seaport')
        assert 'boston-seaport' in str(got.value)
        return want.value, str(got.value)
    none = [[] for _ in ok]
    # rule 1: the first point of lanes 4 and 2 is a duplicate of the second -> lane 2 is named
    bad = [l.copy() for l in ok]
    bad[4][1] = bad[4][0]
    bad[2][1] = bad[2][0] + 1e-9
    want, msg = refused(bad, none)
    assert (want.status, want.lane) == (1, 2) and 'rule 1' in msg and 'lane 2' in msg
    # rule 2: two-point lanes whose two successors start on their two points: lanes 3 and 1 are left empty -> lane 1
    bad = [l.copy() for l in ok]
    bad[1], bad[3] = ok[1][:2].copy(), ok[3][:2].copy()
    bad[2][0], bad[0][0] = bad[1][1], bad[1][0]
    bad[4][0], bad[5][0] = bad[3][1], bad[3][0]
    want, msg = refused(bad, [[], [2, 0], [], [4, 5], [], []])
    assert (want.status, want.lane) == (2, 1) and 'rule 2' in msg and 'lane 1' in msg
    # rule 3: an edge not longer than eps -- a connection that rule 2 does not see
    bad = [l.copy() for l in ok]
    bad[1][0] = bad[0][-1]                                  # lane 0 is trimmed by lane 1 ...
    bad[5][0] = bad[0][-2] + 1e-9                           # ... and its new last node then lies on lane 5's first: listed BEFORE lane 1
    want, msg = refused(bad, [[5, 1], [], [], [], [], []])
    assert (want.status, want.lane) == (3, 0) and 'rule 3' in msg and 'lane 0' in msg
    # rule 4: the same successor twice (lanes 4 and 3) -> the lower node belongs to lane 3
    want, msg = refused(ok, [[], [], [], [0, 0], [1, 2, 1], []])
    assert (want.status, want.lane) == (4, 3) and 'rule 4' in msg and 'lane 3' in msg


# ------------------------------------------------------------------------------------------------
# 8. alone against batched   9. file handling   10. rasters
# ------------------------------------------------------------------------------------------------

def world_maps(names):
    """small maps: the synthetic world's layers with the lanes of a g25 world"""
    out = {}
    for k, name in enumerate(names):
        lanes, o, i = lr.fixture_world(20 + k, (30.0 + 7.0 * k, 40.0))
        s = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)
        out[name] = {'size': (64.0 + 8 * k, 96.0), 'lanes': lanes, 'outgoing': o, 'incoming': i,
                     'layers': {'drivable_area': [[s(2, 3, 60, 50 + k), s(10, 10, 20, 22)], [s(70, 5, 90, 30)]],
                                'carpark_area': [[s(30, 30, 40, 44)]] if k % 2 == 0 else [],
                                'road_divider': [np.array([[0.0, 20.0], [50.0, 21.5 + k], [90.0, 60.0]])],
                                'lane_divider': [np.array([[5.0, 5.0], [5.0, 55.0]]), np.array([[80.0, 2.0], [60.0, 33.0]])]}}
    return out


def check_alone_against_batched(device, tmp_path):
    names = ['boston-seaport', 'singapore-queenstown', 'singapore-onenorth', 'singapore-hollandvillage']
    four = world_maps(names)
    maps.save_maps(str(tmp_path / 'four.npz'), four)
    maps.save_maps(str(tmp_path / 'one.npz'), {names[2]: four[names[2]]})
    before = maps.stats['readbacks']
    env4 = maps.map_env_from_file(str(tmp_path / 'four.npz'), load_lanegraph=True, device=device)
    assert maps.stats['readbacks'] - before == 4, 'one read-back per map between count and fill, none after the fill'
    env1 = maps.map_env_from_file(str(tmp_path / 'one.npz'), load_lanegraph=True, device=device)
    assert env4.map_list == names and env1.map_list == names[2:3]
    a, b = env1.lane_graphs[names[2]], env4.lane_graphs[names[2]]
    ha, hb = a.host_tables(), b.host_tables()
    for k in ha:
        assert ha[k].tobytes() == hb[k].tobytes(), k
    before = maps.stats['readbacks']
    pa, pb = a.packed(2.0), b.packed(2.0)
    assert maps.stats['readbacks'] - before == 2 and a.packed(2.0) is pa, 'one read-back per grid; cached per xydistmax'
    assert pa.grid == pb.grid and sorted(pa.t) == sorted(pb.t)
    for k in pa.t:
        assert torch.equal(pa.t[k], pb.t[k]), k
    assert a.packed(1.0) is not pa and a.packed(1.0).xydistmax == 1.0


def test_alone_against_batched_cpu(emu_ops, tmp_path):
    check_alone_against_batched('cpu', tmp_path)


@pytest.mark.gpu
def test_alone_against_batched_gpu(tmp_path):
    check_alone_against_batched('cuda', tmp_path)


def test_file_round_trip(tmp_path):
    src = world_maps(['boston-seaport', 'singapore-onenorth'])
    path = str(tmp_path / 'm.npz')
    maps.save_maps(path, src)
    z = np.load(path, allow_pickle=False)
    assert all(z[k].dtype != object for k in z.files) and int(z['format_version']) == maps.FORMAT_VERSION
    mf = maps.load_maps(path)
    assert mf.names == list(src) and mf.size('singapore-onenorth') == (72.0, 96.0)
    geo = mf.geometry()
    for name in src:
        lanes, o, i = mf.lanes(name)
        assert o == src[name]['outgoing'] and i == src[name]['incoming'] and len(lanes) == len(src[name]['lanes'])
        assert all(np.array_equal(a, b) for a, b in zip(lanes, src[name]['lanes']))
        for lname, shapes in src[name]['layers'].items():
            got = geo[name]['layers'].get(lname, [])
            assert len(got) == len(shapes)
            for a, b in zip(got, shapes):
                if lname in ('road_divider', 'lane_divider'):
                    assert np.array_equal(a, b)
                else:
                    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    maps.save_maps(str(tmp_path / 'again.npz'), {n: dict(geo[n], **dict(zip(('lanes', 'outgoing', 'incoming'), mf.lanes(n)))) for n in mf.names})
    z2 = np.load(str(tmp_path / 'again.npz'), allow_pickle=False)
    assert sorted(z.files) == sorted(z2.files) and all(np.array_equal(z[k], z2[k]) for k in z.files)


def test_file_validation_names_the_key(tmp_path):
    path = str(tmp_path / 'm.npz')
    maps.save_maps(path, world_maps(['boston-seaport', 'singapore-onenorth']))
    good = dict(np.load(path, allow_pickle=False))

    def refused(key, change, pickle=False):
        a = dict(good)
        if change is None:
            del a[key]
        else:
            a[key] = change(a[key].copy())
        p = str(tmp_path / 'bad.npz')
        with open(p, 'wb') as f:
            np.savez(f, **a)
        with pytest.raises(ValueError, match=key):
            maps.load_maps(p)

    def set_(i, v):
        def f(a):
            a[i] = v
            return a
        return f
    for key in good:
        refused(key, None)                                                    # a missing key
    refused('format_version', lambda a: np.int64(99))
    refused('map_size', lambda a: a.astype(np.float32))                       # dtype
    refused('lane_pts', lambda a: a.reshape(-1))                              # shape
    refused('lane_pts', set_((3, 0), np.nan))
    refused('map_size', set_((0, 1), -5.0))
    refused('map_names', set_(1, 'boston-seaport'))                           # a name twice
    refused('lane_ptr', set_(2, good['lane_ptr'][1] - 1))                     # not monotone
    refused('lane_ptr', set_(-1, good['lane_ptr'][-1] + 1))                   # past the point table
    refused('lane_ptr', set_(1, good['lane_ptr'][0] + 1))                     # a lane of one point
    refused('lane_map_ptr', set_(-1, good['lane_map_ptr'][-1] + 1))
    refused('ring_ptr', set_(1, good['ring_ptr'][2] + 1))
    refused('layer_ptr', lambda a: a[:-1])
    refused('out_idx', set_(0, int(good['lane_map_ptr'][1])))                 # a lane index of ANOTHER map
    refused('in_idx', set_(0, -2))
    refused('out_ptr', set_(-1, good['out_ptr'][-1] - 1))
    refused('map_names', lambda a: np.asarray(a.tolist(), dtype=object))      # an object array
    with pytest.raises(ValueError, match='cannot read'):
        maps.load_maps(str(tmp_path / 'absent.npz'))


def check_rasters(device, tmp_path):
    src = world_maps(['boston-seaport', 'singapore-onenorth', 'singapore-queenstown'])
    path = str(tmp_path / 'm.npz')
    maps.save_maps(path, src)
    geo = {n: {'size': src[n]['size'], 'layers': {k: v for k, v in src[n]['layers'].items() if v}} for n in src}
    for layers in (maps.DEFAULT_LAYERS, ('lane_divider', 'drivable_area')):
        want = map_env_from_geometry(geo, layers, pix_per_m=4, device=device)
        got = maps.map_env_from_file(path, layers=layers, pix_per_m=4, device=device)
        assert got.map_list == want.map_list and got.layer_map == want.layer_map and not hasattr(got, 'lane_graphs')
        assert torch.equal(got.nusc_raster, want.nusc_raster) and torch.equal(got.nusc_dx, want.nusc_dx)
        assert int(got.nusc_raster[1].sum()) > 0 and int(got.nusc_raster[0].sum()) > 0
    noflip = maps.map_env_from_file(path, flip_singapore=False, load_lanegraph=True, device=device)
    flip = maps.map_env_from_file(path, load_lanegraph=True, device=device)
    assert not torch.equal(noflip.nusc_raster[1], flip.nusc_raster[1]) and torch.equal(noflip.nusc_raster[0], flip.nusc_raster[0])
    a, b = noflip.lane_graphs['singapore-onenorth'], flip.lane_graphs['singapore-onenorth']
    assert np.array_equal(b['xy'][:, 1], 72.0 - a['xy'][:, 1]) and np.array_equal(b['edges'][:, 3], -a['edges'][:, 3])


def test_rasters_cpu(emu_ops, tmp_path):
    check_rasters('cpu', tmp_path)


@pytest.mark.gpu
def test_rasters_gpu(tmp_path):
    check_rasters('cuda', tmp_path)


def test_make_maps_file(emu_ops, tmp_path):
    """the synthetic file: a flipped and an unflipped map, a road polygon with holes, dividers, and lanes whose cleaning (both
    rules) gives back the lane graph of synth.make_lane_graph"""
    path = str(tmp_path / 'm.npz')
    src = synth.make_maps_file(path, extent=96.0)
    assert list(src) == ['boston-seaport', 'singapore-onenorth'] and len(src['boston-seaport']['layers']['drivable_area'][0]) > 1
    env = maps.map_env_from_file(path, load_lanegraph=True)
    want = synth.make_lane_graph(extent=96.0)
    g = env.lane_graphs['boston-seaport']
    assert sum(len(l) for l in src['boston-seaport']['lanes']) > g.N == want['xy'].shape[0]
    assert np.array_equal(g['xy'], want['xy']) and g['out_edges'] == want['out_edges'] and g['in_edges'] == want['in_edges']
    assert np.array_equal(g['edgeixes'], want['edgeixes']) and g['ee2ix'] == want['ee2ix']
    assert int(lr.ulps(g['edges'], want['edges']).max()) <= 2
    s = env.lane_graphs['singapore-onenorth']
    assert np.array_equal(s['xy'][:, 1], 96.0 - want['xy'][:, 1])
    assert set(dict(g)) == set(maps.DeviceLaneGraph.KEYS) and len(g) == 6
    with pytest.raises(KeyError):
        g['nodes']


# ------------------------------------------------------------------------------------------------
# 11. the planner on a DeviceLaneGraph and on the equivalent dict
# ------------------------------------------------------------------------------------------------

class LaneEnv(object):
    def __init__(self, lane_graphs):
        self.map_list = list(lane_graphs)
        self.lane_graphs = lane_graphs


def check_planner(device, tmp_path):
    from planner_worlds import agent, make_world
    lanes, outgoing = synth.make_lanes()
    path = str(tmp_path / 'm.npz')
    maps.save_maps(path, {'boston-seaport': {'size': (256.0, 256.0), 'layers': {}, 'lanes': lanes, 'outgoing': outgoing,
                                             'incoming': lr.untable(lr.tables(lanes, outgoing))[2]}})
    mf = maps.load_maps(path)
    g = maps.build_lane_graph(mf.lane_tables('boston-seaport'), device=device, name='boston-seaport')
    as_dict = dict(g)
    assert np.array_equal(as_dict['xy'], synth.make_lane_graph()['xy'])
    scenes = []
    for b, n in enumerate((5, 3, 7)):
        px, py, h, s = synth.lane_scene_poses(as_dict, n, 'maps/%d' % b, radius=38.0, centre=(128.0 + 40.0 * (b - 1), 128.0))
        scenes.append([agent(px[i], py[i], h[i], s[i]) for i in range(n)])
    _, st, att, mask, obs, t, ptr, map_idx = make_world(as_dict, scenes)
    plans, failed = [], []
    for lg in (g, as_dict):
        pl = HardcodeNuscPlanner(LaneEnv({'boston-seaport': lg}), PlannerConfig(**CONFIG_DICT['default']))
        pl.on_error = 'report'
        pl.reset(st.to(device), att.to(device), mask.to(device), len(scenes), map_idx)
        before = maps.stats['readbacks']
        plans.append(pl.rollout(torch.from_numpy(obs.copy()).to(device), t, ptr, t, control_all=False).cpu())
        failed.append(pl.failed_scenes())
        assert maps.stats['readbacks'] == before, 'the packed tables are cached by reset(); a rollout reads nothing back'
    assert bool(torch.isfinite(plans[0]).all()) and failed[0] == failed[1] == {}
    assert float((plans[0] - plans[1]).abs().max()) <= 1e-9
    assert float((plans[0][:, -1, :2] - plans[0][:, 0, :2]).norm(dim=1).min()) > 1.0, 'the egos moved'


def test_planner_on_a_device_lane_graph_cpu(emu_ops, tmp_path):
    check_planner('cpu', tmp_path)


@pytest.mark.gpu
def test_planner_on_a_device_lane_graph_gpu(tmp_path):
    check_planner('cuda', tmp_path)


# ------------------------------------------------------------------------------------------------
# 12. the command lines
# ------------------------------------------------------------------------------------------------

def renamed_scenarios(src, dst, name):
    """copies of the scenario files of ``src`` that name the map ``name``"""
    import json
    os.makedirs(dst, exist_ok=True)
    for fn in sorted(os.listdir(src)):
        if fn.endswith('.json'):
            with open(os.path.join(src, fn)) as f:
                jd = json.load(f)
            jd['map'] = name
            with open(os.path.join(dst, fn), 'w') as f:
                json.dump(jd, f)
    return dst


def test_every_driver_takes_maps_and_keeps_its_defaults():
    from strive_amd import (eval_traffic_tracks, refine_traffic_tracks, adv_scenario_gen_tracks, train_traffic, eval_planner, eval_adv_gen,
                            viz_scenario_dir, viz_adv_gen)
    parsers = {'eval_traffic_tracks': lambda a: vars(eval_traffic_tracks.get_parser().parse_args(['--ckpt', 'c'] + a)),
               'refine_traffic_tracks': lambda a: refine_traffic_tracks.parse_cfg(a)[0],
               'adv_scenario_gen_tracks': lambda a: adv_scenario_gen_tracks.parse_cfg(a)[0],
               'train_traffic': lambda a: train_traffic.parse_cfg(a)[0],
               'eval_planner': lambda a: vars(eval_planner.get_parser().parse_args(a)),
               'eval_adv_gen': lambda a: vars(eval_adv_gen.get_parser().parse_args(['--scenarios', 's'] + a)),
               'viz_scenario_dir': lambda a: vars(viz_scenario_dir.get_parser().parse_args(['--scenarios', 's'] + a)),
               'viz_adv_gen': lambda a: vars(viz_adv_gen.get_parser().parse_args(['--scenarios', 's'] + a))}
    for name, parse in parsers.items():
        plain, given = parse([]), parse(['--maps', 'm.npz'])
        assert plain['maps'] is None and given['maps'] == 'm.npz', name
        assert {k: v for k, v in plain.items() if k != 'maps'} == {k: v for k, v in given.items() if k != 'maps'}, name
        for k in ('map_world', 'lane_world', 'tracks'):
            assert plain.get(k) is None, name


def test_maps_conflicts_and_missing_map(tmp_path, capsys):
    from strive_amd import eval_planner, eval_adv_gen, viz_scenario_dir, viz_adv_gen
    from strive_amd.datasets import tracks as tracks_io
    from strive_amd.eval_traffic_tracks import tracks_loader
    path = str(tmp_path / 'm.npz')
    maps.save_maps(path, world_maps(['boston-seaport']))
    g17 = os.path.join(GOLDEN, 'g17_scenarios')
    g18 = os.path.join(GOLDEN, 'g18_scenarios')
    out = str(tmp_path / 'o')
    for main, args in ((eval_planner.main, ['--scenario_dir', g17, '--skip_regular', '--lane_world', 'synthetic']),
                       (eval_adv_gen.main, ['--scenarios', g18, '--eval_quant', '--map_world', 'synthetic']),
                       (viz_scenario_dir.main, ['--scenarios', g17, '--map_world', 'synthetic']),
                       (viz_adv_gen.main, ['--scenarios', g18, '--map_world', 'synthetic'])):
        with pytest.raises(SystemExit, match='--maps and --(map|lane)_world'):
            main(args + ['--maps', path, '--out', out, '--device', 'cpu'])
    # a scenario names a map the file lacks: the run ends before anything is built, with the name
    for main, args in ((eval_planner.main, ['--scenario_dir', g17, '--skip_regular']),
                       (eval_adv_gen.main, ['--scenarios', g18, '--eval_quant']),
                       (viz_scenario_dir.main, ['--scenarios', g17]),
                       (viz_adv_gen.main, ['--scenarios', g18])):
        with pytest.raises(SystemExit, match="no map named 'synthetic-0'.*boston-seaport"):
            main(args + ['--maps', path, '--out', out, '--device', 'cpu'])
    # ... and so does a tracks file
    tr = str(tmp_path / 't.npz')
    tracks_io.save_tracks(tr, synth.make_tracks(n_scenes=2, n_agents=3, T=20))
    with pytest.raises(SystemExit, match="no map named 'synthetic-0'"):
        tracks_loader({'tracks': tr, 'maps': path}, 'cpu')
    with pytest.raises(SystemExit, match='--maps: maps file: cannot read'):
        tracks_loader({'tracks': tr, 'maps': str(tmp_path / 'absent.npz')}, 'cpu')
    capsys.readouterr()


def test_tracks_loader_on_a_maps_file(emu_ops, tmp_path):
    """tracks whose scenes name the maps of a file: the dataset is built on the file's rasters; lane graphs only when asked for"""
    from strive_amd.datasets import tracks as tracks_io
    from strive_amd.eval_traffic_tracks import tracks_loader
    path = str(tmp_path / 'm.npz')
    synth.make_maps_file(path, extent=128.0)
    tr = synth.make_tracks(n_scenes=2, n_agents=3, T=20)
    tr['scene_map'] = ['singapore-onenorth', 'boston-seaport']
    tp = str(tmp_path / 't.npz')
    tracks_io.save_tracks(tp, tr)
    loader, env = tracks_loader({'tracks': tp, 'maps': path}, 'cpu')
    assert env.map_list == ['boston-seaport', 'singapore-onenorth'] and not hasattr(env, 'lane_graphs')
    assert loader.dataset.map_list == env.map_list and tuple(env.nusc_raster.shape[:2]) == (2, 4)
    loader, env = tracks_loader({'tracks': tp, 'maps': path, 'load_lanegraph': True}, 'cpu')
    assert sorted(env.lane_graphs) == sorted(env.map_list) and all(isinstance(g, maps.DeviceLaneGraph) for g in env.lane_graphs.values())


DEV = 'cuda:0'


@pytest.mark.gpu
def test_gpu_adv_scenario_gen_on_a_maps_file(tmp_path):
    """adv_scenario_gen_tracks --maps F --tracks T --planner hardcode (3 iterations, init fits of 2): the planner runs on the file's
    lane graphs (DeviceLaneGraph, not the synthetic dict), files are written, load through read_adv_scenes and name maps of the file."""
    from strive_amd import adv_scenario_gen_tracks as AG
    from strive_amd.datasets import tracks as tracks_io
    from strive_amd.datasets.utils import read_adv_scenes
    from strive_amd.utils import torch as UT
    from util import product_model
    mpath, tpath = str(tmp_path / 'm.npz'), str(tmp_path / 't.npz')
    synth.make_maps_file(mpath)
    tr = synth.make_tracks(n_scenes=2, n_agents=5, T=20)
    tr['scene_map'] = ['boston-seaport', 'boston-seaport']
    tracks_io.save_tracks(tpath, tr)
    m, sd = product_model()
    m.load_state_dict(synth.lane_keeping_weights(sd))
    ckpt = str(tmp_path / 'ckpt.pth')
    UT.save_state(ckpt, m, torch.optim.Adam(m.parameters(), lr=1e-3), cur_epoch=2)
    out = str(tmp_path / 'out')
    seen = []
    orig = AG.run_one_epoch

    def run(source, batch_size, model, map_env, *a, **k):
        seen.append(map_env)
        return orig(source, batch_size, model, map_env, *a, **dict(k, init_iters=(2, 2)))
    AG.run_one_epoch = run
    try:
        written, kept = AG.main(['--config', os.path.join(GOLDEN, 'g23_adv_gen_rule_based.cfg'), '--tracks', tpath, '--maps', mpath, '--ckpt', ckpt,
                                 '--out', out, '--num_iters', '3', '--seq_interval', '3', '--batch_size', '8', '--seed', '7',
                                 '--feasibility_thresh', '40', '--feasibility_vel', '0.05', '--device', DEV, '--on_planner_error', 'drop'],
                                keep_results=True)
    finally:
        AG.run_one_epoch = orig
    env = seen[0]
    assert env.map_list == ['boston-seaport', 'singapore-onenorth'] and isinstance(env.lane_graphs['boston-seaport'], maps.DeviceLaneGraph)
    assert env.lane_graphs['boston-seaport']._packed, 'the planner took the device-built tables'
    files = [(os.path.basename(d), f) for d, _, fs in os.walk(os.path.join(out, 'scenario_results')) for f in fs]
    assert len(files) == sum(written.values()) >= 1
    for d in {d for d, _ in files}:
        got = read_adv_scenes(os.path.join(out, 'scenario_results', d))
        assert got and all(sc['map'] in env.map_list and sc['scene_fut'].shape[1:] == (12, 4) for sc in got)


@pytest.mark.gpu
def test_gpu_eval_planner_and_viz_scenario_dir_on_a_maps_file(tmp_path):
    from strive_amd import eval_planner, viz_scenario_dir
    mpath = str(tmp_path / 'm.npz')
    synth.make_maps_file(mpath)
    scen = renamed_scenarios(os.path.join(GOLDEN, 'g17_scenarios'), str(tmp_path / 'scen'), 'boston-seaport')
    n_scen = len(os.listdir(scen))
    out = str(tmp_path / 'pe')
    eval_planner.main(['--maps', mpath, '--scenario_dir', scen, '--skip_regular', '--out', out, '--device', DEV])
    rows = open(os.path.join(out, 'all_eval_results.csv')).read().strip().splitlines()
    assert len(rows) == 1 + n_scen and os.path.exists(os.path.join(out, 'plan_cfg.json'))
    # the same scenes on the synthetic lane world: the file's lanes clean to the same graph, so the same results are written
    eval_planner.main(['--lane_world', 'synthetic', '--scenario_dir', os.path.join(GOLDEN, 'g17_scenarios'), '--skip_regular',
                       '--out', out + '_synth', '--device', DEV])
    want = open(os.path.join(out + '_synth', 'all_eval_results.csv')).read().strip().splitlines()
    assert want[0] == rows[0] and len(want) == len(rows)
    for a, b in zip(want[1:], rows[1:]):
        a, b = a.split(','), b.split(',')
        assert a[0] == b[0] and np.allclose([float(v) for v in a[1:]], [float(v) for v in b[1:]], rtol=1e-9, atol=1e-9, equal_nan=True), a[0]
    vout = str(tmp_path / 'viz')
    n = viz_scenario_dir.main(['--scenarios', scen, '--out', vout, '--maps', mpath, '--L', '96', '--device', DEV])
    assert n == n_scen and sorted(os.listdir(vout)) == sorted(f[:-5] + '.png' for f in os.listdir(scen))
