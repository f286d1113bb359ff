#!/usr/bin/env python3
"""Fixture g25 (tests/golden/g25_lane_graph.npz): the reference's OWN process_lanegraph and the lane-graph flip of its OWN
NuScenesMapEnv.__init__ (reference src/datasets/nuscenes_utils.py:50-122, src/datasets/map_env.py:22-166), run on four small
lane networks under the four real map names.  Only runs where the reference is mounted; nothing of its source is copied -- the
committed file holds the inputs (lanes + connectivity) and the recorded outputs.

The devkit is stubbed the way make_golden.py stubs it: ``discretize_lane`` returns the stored polyline, ``get_nusc_maps`` returns
stub maps (``lane``, ``lane_connector``, ``arcline_path_3``, ``connectivity``) whose ``get_map_mask`` returns zeros, at a tiny
``pix_per_m`` (the rasters are not what is recorded).

Before anything is written the generator asserts, on the reference's side, that every distance the reference compares with eps
is at least 4 units in the last place away from eps: ties are not what is being tested.

Usage:  python tests/golden/make_golden_maps.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
import make_golden as mg                 # noqa: E402  (the import stand-ins)
import lane_graph_restated as lr         # noqa: E402

EPS = 1e-6
PIX_PER_M = 0.01
# (name, seed, origin): the order of the reference's get_nusc_maps
WORLDS = (('singapore-hollandvillage', 11, (310.0, 2270.0)), ('singapore-queenstown', 12, (1420.0, 905.0)),
          ('boston-seaport', 13, (655.0, 1240.0)), ('singapore-onenorth', 14, (120.0, 1630.0)))


class StubMap(object):
    def __init__(self, lanes, outgoing, incoming):
        tok = ['lane-%03d' % i for i in range(len(lanes))]
        half = len(lanes) // 2
        self.lane = [{'token': t} for t in tok[:half]]
        self.lane_connector = [{'token': t} for t in tok[half:]]
        self.arcline_path_3 = {t: lanes[i] for i, t in enumerate(tok)}
        name = lambda l, k, j: tok[j] if j >= 0 else 'absent-%03d-%d' % (l, k)
        self.connectivity = {tok[l]: {'outgoing': [name(l, k, j) for k, j in enumerate(outgoing[l])],
                                      'incoming': [name(l, k, j) for k, j in enumerate(incoming[l])]} for l in range(len(lanes))}

    def get_map_mask(self, patch_box, patch_angle, layer_names, canvas_size):
        return np.zeros((len(layer_names), int(canvas_size[0]), int(canvas_size[1])), dtype=np.uint8)


def main():
    mg._install_stubs()
    if sys.path[0] != mg.REF_SRC:
        sys.path.insert(0, mg.REF_SRC)
    for name in list(sys.modules):
        if name == 'datasets' or name.startswith('datasets.'):
            del sys.modules[name]
    import importlib
    nutils = importlib.import_module('datasets.nuscenes_utils')
    map_env = importlib.import_module('datasets.map_env')

    worlds = {name: lr.fixture_world(seed, origin) for name, seed, origin in WORLDS}
    stubs = {name: StubMap(*worlds[name]) for name, _, _ in WORLDS}
    nutils.get_nusc_maps = lambda data_folder: dict(stubs)
    nutils.discretize_lane = lambda lane, res: np.concatenate([np.asarray(lane, dtype=np.float64), np.zeros((len(lane), 1))], axis=1)

    compared = []
    norm0 = np.linalg.norm

    def norm(x, *a, **k):
        v = norm0(x, *a, **k)
        compared.extend(np.atleast_1d(v).tolist())
        return v
    np.linalg.norm = norm
    try:
        env = map_env.NuScenesMapEnv('unused', load_lanegraph=True, lanegraph_eps=EPS, pix_per_m=PIX_PER_M, flip_singapore=True)
    finally:
        np.linalg.norm = norm0
    assert list(env.map_list) == [w[0] for w in WORLDS]
    compared = np.asarray(compared)
    margin = np.abs(compared - EPS) / np.spacing(EPS)
    assert margin.min() >= 4.0, 'a distance lies %g ulp from eps' % margin.min()
    print('%d distances compared with eps, the closest %.3g ulp away (%d at or below eps)' % (
        compared.size, margin.min(), int((compared <= EPS).sum())))

    out = {'eps': np.float64(EPS), 'names': np.asarray([w[0] for w in WORLDS], dtype=np.str_),
           'heights': np.asarray([map_env.NUSC_MAP_SIZES[w[0]][0] for w in WORLDS], dtype=np.float64)}
    nfma = nunf = nedge = 0
    for m, (name, _, _) in enumerate(WORLDS):
        t = lr.tables(*worlds[name])
        lg = env.lane_graphs[name]
        for k, v in t.items():
            out['m%d_%s' % (m, k)] = v
        out['m%d_xy' % m] = np.asarray(lg['xy'], dtype=np.float64)
        out['m%d_edges' % m] = np.asarray(lg['edges'], dtype=np.float64)
        out['m%d_edgeixes' % m] = np.asarray(lg['edgeixes'], dtype=np.int64)
        for key in ('out_edges', 'in_edges'):
            ptr = np.concatenate([[0], np.cumsum([len(x) for x in lg[key]])]).astype(np.int64)
            out['m%d_%s_ptr' % (m, key)] = ptr
            out['m%d_%s_idx' % (m, key)] = np.asarray([v for x in lg[key] for v in x], dtype=np.int64)
        assert lg['ee2ix'] == {(int(a), int(b)): k for k, (a, b) in enumerate(lg['edgeixes'].tolist())}
        # which rule do the reference's edge lengths follow?  (positions before the flip: the flip leaves lengths alone)
        flip = name.startswith('singapore')
        r = lr.restate(t, EPS, flip, float(out['heights'][m]))
        u = lr.restate(t, EPS, flip, float(out['heights'][m]), length=lr.length_unfused)
        nedge += lg['edges'].shape[0]
        nfma += int((r['edges'][:, 4] == lg['edges'][:, 4]).sum())
        nunf += int((u['edges'][:, 4] == lg['edges'][:, 4]).sum())
        print('%-26s lanes %3d points %4d -> nodes %4d edges %4d' % (name, len(worlds[name][0]), t['pts'].shape[0], lg['xy'].shape[0],
                                                                     lg['edges'].shape[0]))
    print('edge lengths bit-equal to the reference: sqrt(fma(dy,dy,dx*dx)) %d of %d, sqrt(dx*dx+dy*dy) %d of %d' % (nfma, nedge, nunf, nedge))
    path = os.path.join(HERE, 'g25_lane_graph.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
