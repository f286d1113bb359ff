#!/usr/bin/env python3
"""Lane graph of a maps file: the device build (strive_lane_graph_count / _fill + DeviceLaneGraph.packed, strive_amd/csrc/lane_graph.hip)
against the host path on the same input -- a NumPy restatement of the reference's process_lanegraph (reference
src/datasets/nuscenes_utils.py:28-122) followed by PackedLaneGraph (strive_amd/planners/hardcode_goalcond_nusc.py).

    python tools/lane_graph_bench.py [--device cuda:0] [--out profiles/r28_lane_graph_bench.json]

Two sizes: the synthetic world at 256 m (a few thousand nodes) and one of at least 250 000 nodes.  Both paths start from the lanes of
a loaded maps file (the device path from its offset tables, the host path from its lists) and end with the planner's tables on the
device, synchronised.  The repeats of the two paths alternate in one process; the medians are reported with minimum and maximum.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from strive_amd import synth                                                     # noqa: E402
from strive_amd.datasets import maps                                             # noqa: E402
from strive_amd.planners.hardcode_goalcond_nusc import PackedLaneGraph          # noqa: E402


def process_lanegraph_numpy(lanes, outgoing, incoming, eps):
    """process_lanegraph + process_edges in NumPy, lane by lane and edge by edge as the reference walks them"""
    clean = []
    for xy in lanes:
        kept = np.ones(len(xy), dtype=bool)
        kept[:-1] = np.linalg.norm(xy[1:] - xy[:-1], axis=1) > eps
        assert kept[0]
        clean.append(xy[kept])
    for l in range(len(clean)):
        for o in outgoing[l]:
            if o >= 0 and np.linalg.norm(clean[o][0] - clean[l][-1]) <= eps:
                clean[l] = clean[l][:-1]
                assert clean[l].shape[0] >= 1
    start, xys = [], []
    for ln in clean:
        start.append(len(xys))
        xys.extend(ln.tolist())
    in_edges, out_edges = [[] for _ in xys], [[] for _ in xys]
    for l, ln in enumerate(clean):
        for ix in range(len(ln) - 1):
            out_edges[start[l] + ix].append(start[l] + ix + 1)
        for ix in range(1, len(ln)):
            in_edges[start[l] + ix].append(start[l] + ix - 1)
        for o in outgoing[l]:
            if o >= 0:
                out_edges[start[l] + len(ln) - 1].append(start[o])
        for o in incoming[l]:
            if o >= 0:
                in_edges[start[l]].append(start[o] + len(clean[o]) - 1)
    edges, edgeixes, ee2ix = [], [], {}
    for i in range(len(out_edges)):
        x0, y0 = xys[i]
        for e in out_edges[i]:
            x1, y1 = xys[e]
            diff = np.array([x1 - x0, y1 - y0])
            dist = np.linalg.norm(diff)
            assert dist > eps and (i, e) not in ee2ix
            diff /= dist
            ee2ix[i, e] = len(edges)
            edges.append([x0, y0, diff[0], diff[1], dist])
            edgeixes.append([i, e])
    return {'xy': np.array(xys), 'in_edges': in_edges, 'out_edges': out_edges, 'edges': np.array(edges), 'edgeixes': np.array(edgeixes),
            'ee2ix': ee2ix}


def sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize(device)


def measure(name, extent, repeats, device, xydistmax=2.0, eps=1e-6):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'm.npz')
        synth.make_maps_file(path, names=('boston-seaport',), extent=extent)
        mf = maps.load_maps(path)
    tabs = mf.lane_tables('boston-seaport')
    lanes, outgoing, incoming = mf.lanes('boston-seaport')
    times = {'device_build': [], 'device_packed': [], 'host_process_lanegraph': [], 'host_packed': []}
    sizes = None
    for r in range(repeats + 1):                           # the first round warms both paths up and is not counted
        sync(device)
        t0 = time.perf_counter()
        g = maps.build_lane_graph(tabs, eps=eps, device=device)
        sync(device)
        t1 = time.perf_counter()
        p = g.packed(xydistmax)
        sync(device)
        t2 = time.perf_counter()
        lg = process_lanegraph_numpy(lanes, outgoing, incoming, eps)
        t3 = time.perf_counter()
        hp = PackedLaneGraph(lg, xydistmax, device)
        sync(device)
        t4 = time.perf_counter()
        if r == 0:
            assert (g.N, g.M) == (hp.N, hp.M) and torch.equal(p.t['cell_edges'].view(torch.uint8).reshape(-1), hp.t['cell_edges'])
            sizes = {'lanes': len(lanes), 'points': int(tabs['pts'].shape[0]), 'nodes': g.N, 'edges': g.M,
                     'grid_cells': p.grid['gnx'] * p.grid['gny'], 'grid_entries': int(p.t['cell_edges'].numel())}
            continue
        for k, v in zip(('device_build', 'device_packed', 'host_process_lanegraph', 'host_packed'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            times[k].append(v)
    times['device_total'] = [a + b for a, b in zip(times['device_build'], times['device_packed'])]
    times['host_total'] = [a + b for a, b in zip(times['host_process_lanegraph'], times['host_packed'])]
    row = dict(name=name, extent_m=extent, repeats=repeats, **sizes)
    for k, v in times.items():
        row[k + '_s'] = {'median': statistics.median(v), 'min': min(v), 'max': max(v)}
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default=os.path.join('profiles', 'r28_lane_graph_bench.json'))
    ap.add_argument('--large_extent', type=float, default=2240.0, help='metres; 2240 gives about 268 000 nodes')
    ap.add_argument('--repeats', type=int, nargs=2, default=[7, 3], help='counted repeats of the small and of the large graph')
    cfg = ap.parse_args(argv)
    rows = [measure('small', 256.0, cfg.repeats[0], cfg.device), measure('large', cfg.large_extent, cfg.repeats[1], cfg.device)]
    result = {'device': cfg.device, 'device_name': torch.cuda.get_device_name(cfg.device) if cfg.device.startswith('cuda') else 'host',
              'graphs': rows}
    os.makedirs(os.path.dirname(os.path.abspath(cfg.out)), exist_ok=True)
    with open(cfg.out, 'w') as f:
        json.dump(result, f, indent=1)
    for r in rows:
        print('%s: %d nodes, %d edges: device %.4f s (%.4f .. %.4f), host %.4f s (%.4f .. %.4f)' % (
            r['name'], r['nodes'], r['edges'], r['device_total_s']['median'], r['device_total_s']['min'], r['device_total_s']['max'],
            r['host_total_s']['median'], r['host_total_s']['min'], r['host_total_s']['max']))
    return result


if __name__ == '__main__':
    main()
