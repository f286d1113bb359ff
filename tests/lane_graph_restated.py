"""TEST INFRASTRUCTURE: the lane-graph rules of include/strive_hip.h (strive_lane_graph_count / _fill) restated in plain float64
Python, one lane and one node at a time, in the order of the reference's process_lanegraph / process_edges and the Singapore
flip (reference src/datasets/nuscenes_utils.py:28-122, src/datasets/map_env.py:131-144).  Every distance goes through ``length``,
the stated rule of the device: sqrt(fma(dy, dy, dx*dx)), the fused multiply-add taken from the C library (Python 3.10 has no
math.fma).  tests/test_maps_file.py holds every output byte of the kernels to this, and this to the reference's fixture g25.

Also here: small builders of lane inputs (``tables``) and the worlds the tests and tests/golden/make_golden_maps.py share.
"""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3

LANE_NODE = np.dtype([('n', '<i4'), ('node', '<i4', (4,)), ('pad', '<i4', (3,)), ('len', '<f8', (4,))])


def length(dx, dy):
    """THE LENGTH RULE of strive_amd/csrc/lane_graph.hip"""
    dx, dy = float(dx), float(dy)
    return math.sqrt(_libm.fma(dy, dy, dx * dx))


def length_unfused(dx, dy):
    dx, dy = float(dx), float(dy)
    return math.sqrt(dx * dx + dy * dy)


class Refusal(Exception):
    def __init__(self, status, lane, node=None):
        Exception.__init__(self, 'status %d lane %d node %r' % (status, lane, node))
        self.status, self.lane, self.node = status, lane, node


def tables(lanes, outgoing, incoming=None):
    """lists -> the kernels' input tables.  ``incoming`` None: the inverse of ``outgoing``, in lane order."""
    if incoming is None:
        incoming = [[] for _ in lanes]
        for j, o in enumerate(outgoing):
            for i in o:
                if i >= 0:
                    incoming[i].append(j)
    lanes = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in lanes]

    def csr(lists):
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
        return ptr, np.asarray([v for x in lists for v in x], dtype=np.int32).reshape(-1)
    op, oi = csr(outgoing)
    ip, ii = csr(incoming)
    return dict(pts=np.concatenate(lanes, axis=0), lane_ptr=np.concatenate([[0], np.cumsum([len(p) for p in lanes])]).astype(np.int32),
                out_ptr=op, out_idx=oi, in_ptr=ip, in_idx=ii)


def untable(t):
    nl = len(t['lane_ptr']) - 1
    lanes = [np.asarray(t['pts'], dtype=np.float64)[t['lane_ptr'][i]:t['lane_ptr'][i + 1]] for i in range(nl)]
    out = [[int(v) for v in t['out_idx'][t['out_ptr'][i]:t['out_ptr'][i + 1]]] for i in range(nl)]
    inc = [[int(v) for v in t['in_idx'][t['in_ptr'][i]:t['in_ptr'][i + 1]]] for i in range(nl)]
    return lanes, out, inc


def restate(t, eps=1e-6, flip=False, height=0.0, length=length, decisions=None):
    """-> dict of every table the device builds, or raises Refusal.  ``decisions``: a list that receives every distance that
    was compared with eps."""
    lanes, outgoing, incoming = untable(t)
    note = (lambda d: None) if decisions is None else decisions.append
    # rule 1
    kept, bad = [], None
    for l, xy in enumerate(lanes):
        keep = [True] * len(xy)
        for i in range(len(xy) - 1):
            d = length(xy[i + 1, 0] - xy[i, 0], xy[i + 1, 1] - xy[i, 1])
            note(d)
            keep[i] = d > eps
        if bad is None and len(xy) and not keep[0]:
            bad = l
        kept.append(xy[np.asarray(keep, dtype=bool)])
    if bad is not None:
        raise Refusal(1, bad)
    # rule 2
    first = [k[0] if len(k) else None for k in kept]
    cur = []
    for l, xy in enumerate(kept):
        emptied = len(xy) < 1
        for o in outgoing[l]:
            if emptied:
                break
            if o < 0 or first[o] is None:
                continue
            d = length(first[o][0] - xy[-1, 0], first[o][1] - xy[-1, 1])
            note(d)
            if d <= eps:
                xy = xy[:-1]
                emptied = len(xy) < 1
        if emptied and bad is None:
            bad = l
        cur.append(xy)
    if bad is not None:
        raise Refusal(2, bad)
    # numbering and lists
    start = np.concatenate([[0], np.cumsum([len(x) for x in cur])]).astype(np.int64)
    xy = np.concatenate(cur, axis=0)
    N = xy.shape[0]
    lane_of = np.repeat(np.arange(len(cur)), [len(x) for x in cur])
    out_edges, in_edges = [[] for _ in range(N)], [[] for _ in range(N)]
    for l, x in enumerate(cur):
        s, n = int(start[l]), len(x)
        for k in range(n - 1):
            out_edges[s + k].append(s + k + 1)
        for k in range(1, n):
            in_edges[s + k].append(s + k - 1)
        for o in outgoing[l]:
            if o >= 0:
                out_edges[s + n - 1].append(int(start[o]))
        for o in incoming[l]:
            if o >= 0:
                in_edges[s].append(int(start[o]) + len(cur[o]) - 1)
    # edges (positions before the flip)
    edges, eix = [], []
    for v in range(N):
        short = twice = False
        for k, u in enumerate(out_edges[v]):
            dx, dy = xy[u, 0] - xy[v, 0], xy[u, 1] - xy[v, 1]
            d = length(dx, dy)
            note(d)
            short = short or not d > eps
            twice = twice or u in out_edges[v][:k]
            edges.append([xy[v, 0], xy[v, 1], dx / d if d else np.nan, dy / d if d else np.nan, d])
            eix.append([v, u])
        if short:
            raise Refusal(3, int(lane_of[v]), v)
        if twice:
            raise Refusal(4, int(lane_of[v]), v)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1, 5)
    xy = xy.copy()
    if flip:
        xy[:, 1] = height - xy[:, 1]
        edges[:, 1] = height - edges[:, 1]
        edges[:, 3] *= -1
    # the planner's tables from the final positions

    def records(lists):
        rec = np.zeros((N,), dtype=LANE_NODE)
        ptr = np.zeros((N + 1,), dtype=np.int32)
        idx, lens = [], []
        for v, conn in enumerate(lists):
            rec['n'][v] = len(conn)
            for j, u in enumerate(conn):
                ln = length(xy[u, 0] - xy[v, 0], xy[u, 1] - xy[v, 1])
                if j < 4:
                    rec['node'][v, j], rec['len'][v, j] = u, ln
                idx.append(u)
                lens.append(ln)
            ptr[v + 1] = len(idx)
        return rec, ptr, np.asarray(idx, dtype=np.int32).reshape(-1), np.asarray(lens, dtype=np.float64).reshape(-1)
    succ, sp, si, sl = records(out_edges)
    pred, pp, pi, pl = records(in_edges)
    eix = np.asarray(eix, dtype=np.int64).reshape(-1, 2)
    return dict(xy=xy, in_edges=in_edges, out_edges=out_edges, edges=edges, edgeixes=eix,
                ee2ix={(int(a), int(b)): k for k, (a, b) in enumerate(eix.tolist())},
                succ=succ, pred=pred, succ_ptr=sp, succ_idx=si, succ_len=sl, pred_ptr=pp, pred_idx=pi, pred_len=pl,
                edge_ix=eix.astype(np.int32).reshape(-1))


DEVICE_TABLES = ('xy', 'succ', 'pred', 'succ_ptr', 'succ_idx', 'succ_len', 'pred_ptr', 'pred_idx', 'pred_len', 'edges', 'edge_ix')


def device_view(r):
    """the restated dict's tables as the flat arrays DeviceLaneGraph.host_tables() returns"""
    return {k: np.ascontiguousarray(r[k]).reshape(-1) for k in DEVICE_TABLES}


def ulps(a, b):
    """distance in units in the last place between float64 arrays of equal sign pattern (0 where bit-equal)"""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------------------------------------
# worlds
# ------------------------------------------------------------------------------------------------

def walk(rs, p0, n, step=1.0, turn=0.08):
    """n points from p0, about `step` apart, along a heading that wanders: coordinates with full mantissas"""
    h = rs.uniform(-np.pi, np.pi) + np.cumsum(rs.uniform(-turn, turn, n))
    d = step * rs.uniform(0.8, 1.2, n)
    pts = np.asarray(p0, dtype=np.float64)[None] + np.cumsum(np.stack([d * np.cos(h), d * np.sin(h)], -1), axis=0)
    return np.concatenate([np.asarray(p0, dtype=np.float64)[None], pts[:n - 1]], axis=0)


def with_run(lane, at, count=2, off=1e-8):
    """`count` extra points within `off` of point `at`, inserted before it (the last of the run survives rule 1)"""
    extra = [lane[at] + off * (k + 1) * np.array([0.6, -0.8]) for k in range(count)]
    return np.concatenate([lane[:at], np.asarray(extra), lane[at:]], axis=0)


def fixture_world(seed, origin):
    """One map of fixture g25: ~35 lanes that exercise every rule -- exact and near duplicates in the middle and at the end of a
    lane, one trim, two trims in a row, a two-point lane trimmed to one node with connections on both sides, absent tokens, a
    ring lane that continues into itself, out-degree 9 and in-degree 6, incoming lists that are not in lane order."""
    rs = np.random.RandomState(seed)
    o = np.asarray(origin, dtype=np.float64)
    lanes, out, inc = [], [], []

    def add(pts, outgoing=(), incoming=None):
        lanes.append(np.asarray(pts, dtype=np.float64))
        out.append(list(outgoing))
        inc.append(incoming)
        return len(lanes) - 1
    # a chain of lanes of many lengths; every other one ends ON its successor's first point (one trim), the rest 0.7 m short
    sizes = [2, 3, 5, 8, 13, 70, 4, 6]
    p = o + rs.uniform(0, 50, 2)
    chain = []
    for k, n in enumerate(sizes):
        ln = walk(rs, p, n)
        chain.append(add(ln))
        p = ln[-1] if k % 2 == 0 else ln[-1] + rs.uniform(0.4, 0.6, 2)
    for k, i in enumerate(chain[:-1]):
        out[i] = [chain[k + 1]]
    # after an even lane the next one starts on its last point; lane 1 (3 points) and lane 3 get duplicates
    lanes[chain[2]] = with_run(lanes[chain[2]], 2, count=1, off=0.0)          # an exact repeat mid-lane
    lanes[chain[3]] = with_run(lanes[chain[3]], 4, count=2)                   # three near-equal points mid-lane
    lanes[chain[5]] = with_run(lanes[chain[5]], 66, count=3)                  # a run across point 64 ... 69
    lanes[chain[7]] = with_run(lanes[chain[7]], 5, count=2)                   # a run that ends at the lane's end
    out[chain[-1]] = [-1]                                                     # an absent token
    # two trims in a row: A = [..., q, p]; B starts on p, C starts on q
    A = walk(rs, o + rs.uniform(60, 90, 2), 6)
    a = add(A)
    b = add(walk(rs, A[-1], 4))
    c = add(walk(rs, A[-2], 5))
    out[a] = [b, -1, c]
    # a two-point lane trimmed to one node; two lanes run into it, it runs into two
    D = walk(rs, o + rs.uniform(100, 120, 2), 2)
    d = add(D)
    e = add(walk(rs, D[-1], 3))
    f = add(walk(rs, D[-1] + np.array([0.3, 0.9]), 3))
    g = add(walk(rs, D[0] + np.array([-7.0, 1.5]), 5))
    h = add(walk(rs, D[0] + np.array([-6.0, -2.5]), 4))
    out[d] = [e, f]
    out[g] = [d]
    out[h] = [d]
    inc[d] = [h, g]                                                           # (not in lane order)
    # a ring: the lane ends on its own first point and continues into itself
    ang = np.linspace(0.0, 2 * np.pi, 13)
    ring = o + np.array([150.0, 40.0]) + 9.7 * np.stack([np.cos(ang), np.sin(ang)], -1)
    ring[-1] = ring[0]
    r = add(ring)
    out[r] = [r]
    # a hub of out-degree 9 whose spokes all run into one sink of in-degree 6 (and 3 elsewhere)
    H = walk(rs, o + rs.uniform(170, 190, 2), 4)
    hub = add(H)
    sink = add(walk(rs, H[-1] + np.array([31.0, 2.0]), 3))
    spokes = []
    for k in range(9):
        s = walk(rs, H[-1] + np.array([0.9, 0.45 * (k - 4)]), 4 + k % 3)
        spokes.append(add(s, outgoing=[sink] if k < 6 else [-1]))
    out[hub] = spokes
    inc[sink] = spokes[:6][::-1]
    # incoming lists: the inverse of outgoing in lane order unless given
    for i in range(len(lanes)):
        if inc[i] is None:
            inc[i] = [j for j in range(len(lanes)) if i in out[j]]
    return lanes, out, inc
