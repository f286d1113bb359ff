"""Helpers of tests/test_map_cnn_layers.py (a plain module like loop_util.py): a Python mirror of where the map CNN leaves every
layer's raw output (workspace of strive_map_cnn_fwd / _bench_layer, kept buffer of strive_map_cnn_fwd_keep), the decode of its
layouts, a float64 reference of ONE layer fed the product's own previous output, weight sets and crop families away from the
synthetic default, and the forms (kernel selections) the library can be driven through.  Everything takes a library handle and a
device, so one case runs on the host emulation and on the MI355X."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from strive_amd import _lib as L, params, synth
from oracle import mapenv

# `K`: a raw layer output may differ from the float64 reference of that layer by K times what torch fp32 differs from it on the same
# input.  Twice the worst measured ratio over all layers, forms and default-weight cases, rounded up to a power of two; the ratios
# (host emulation and MI355X) are in profiles/r13_cnn_layer_ratios.md.
K = 16.0

SHAPES = [(16, 125, 125), (32, 61, 61), (64, 29, 29), (64, 14, 14), (128, 6, 6), (128, 2, 2)]
L_OUT = [c * h * w for c, h, w in SHAPES]
NPARTS = [32, 16, 4, 1, 2, 2]          # GroupNorm partial-moment slots per sample and layer: throughput chain / kept buffer
NPMAX = [32, 16, 16, 4, 2, 2]          # slots reserved in the workspace (the small-batch chain writes 16 / 4 for conv3 / conv4)
STAT_SLOTS = sum(NPMAX)
GNSTATS_BYTES = 16                     # struct GNStats { double sum, sq; }
CHUNK_MAX = 1024
GN_EPS = 1e-5


def align(v, a=256):
    return (v + a - 1) // a * a


class WorkspaceMap(object):
    """cnn_run / strive_map_cnn_bench_layer carve the workspace for `per` samples: six activation blocks, then the statistics
    block of per * STAT_SLOTS slots with layer l's slots starting at per * sum(NPMAX[:l]).  Byte offsets."""

    def __init__(self, per):
        self.per = per
        self.act, off = [], 0
        for l in range(6):
            self.act.append(off)
            off += align(per * L_OUT[l] * 4)
        self.stats = off
        self.st = [off + per * sum(NPMAX[:l]) * GNSTATS_BYTES for l in range(6)]
        self.total = off + align(per * STAT_SLOTS * GNSTATS_BYTES)


def workspace_bytes(N):
    return WorkspaceMap(min(max(N, 1), CHUNK_MAX)).total


class KeepMap(object):
    """cnn_keep_carve: six activation blocks of N samples, then six statistics blocks of N * NPARTS[l] slots; strive_map_cnn_keep_bytes
    adds 256 bytes of slack."""

    def __init__(self, N):
        self.per = N
        self.act, self.st, off = [], [], 0
        for l in range(6):
            self.act.append(off)
            off += align(N * L_OUT[l] * 4)
        for l in range(6):
            self.st.append(off)
            off += align(N * NPARTS[l] * GNSTATS_BYTES)
        self.total = off + 256


def chunk_of(lib, N):
    """samples per pass of cnn_run (option cnn_chunk clamped like the library clamps it) = what it carves the workspace for"""
    return min(N, min(max(lib.get_option('cnn_chunk'), 8), CHUNK_MAX))


def last_chunk(lib, N):
    """(first row, rows) of the chunk whose activations the workspace still holds after a call over N samples"""
    ch = chunk_of(lib, N)
    n0 = (N - 1) // ch * ch
    return n0, N - n0


def read_raw(buf, wmap, l, n):
    """bytes of layer l's block for n samples, as the kernels left them (a copy on the host)"""
    return buf[wmap.act[l]:wmap.act[l] + n * L_OUT[l] * 4].cpu().clone()


def read_stats(buf, wmap, l, n, nslots):
    return buf[wmap.st[l]:wmap.st[l] + n * nslots * GNSTATS_BYTES].cpu().clone()


def decode(raw, l, n):
    """raw bytes -> (n, C, H, W) float32 NCHW: conv1 .. conv5 are octet-planar [n][c/8][y][x][c%8], conv6 is NCHW"""
    c, h, w = SHAPES[l]
    x = raw.view(torch.float32)
    if l == 5:
        return x.view(n, c, h, w).clone()
    return x.view(n, c // 8, h, w, 8).permute(0, 1, 4, 2, 3).reshape(n, c, h, w).contiguous()


# ------------------------------------------------------------------------------------------------
# the reference of one layer
# ------------------------------------------------------------------------------------------------
def _p(sd, name, dtype):
    return sd[name].detach().cpu().to(dtype)


def ref_layer(sd, l, x_prev, dtype=torch.float64, batch=32):
    """Layer l in `dtype` on the CPU: GroupNorm (1 group, eps 1e-5, moments of x_prev itself) + ReLU of the previous layer's RAW
    output, then Conv2d(stride 2) l; l = 0 takes the uint8 crop, l = 6 is GroupNorm + ReLU + Linear of conv6's output."""
    out = []
    for i in range(0, x_prev.shape[0], batch):
        x = x_prev[i:i + batch].cpu().to(dtype)
        if l > 0:
            x = F.relu(F.group_norm(x, 1, _p(sd, 'map_conv.%d.weight' % (3 * l - 2), dtype), _p(sd, 'map_conv.%d.bias' % (3 * l - 2), dtype), GN_EPS))
        if l == 6:
            out.append(F.linear(x.reshape(x.shape[0], -1), _p(sd, 'map_feature.weight', dtype), _p(sd, 'map_feature.bias', dtype)))
        else:
            out.append(F.conv2d(x, _p(sd, 'map_conv.%d.weight' % (3 * l), dtype), _p(sd, 'map_conv.%d.bias' % (3 * l), dtype), stride=2))
    return torch.cat(out, 0)


def ref_from(sd, l0, x_prev, dtype=torch.float64):
    """layers l0 .. 6 chained in `dtype` (the rest of the network on top of a raw output of layer l0 - 1)"""
    x = x_prev
    for l in range(l0, 7):
        x = ref_layer(sd, l, x, dtype)
    return x


def scale_floor(net, l):
    """What ONE power of two per layer input costs: the scaled activation is split into two fp16 pieces, so every activation of
    layer l's input carries up to 2^-25 / xscale[l] absolute, however small its channel; pushed through the layer's weights that is
    sum |w| 2^-25 / xscale[l] per output channel.  (C, 1, 1) float64, zero for conv1 (its uint8 input is exact)."""
    if l == 0 or l > 5:
        return 0.0
    w = net.sd['map_conv.%d.weight' % (3 * l)].double()
    return (w.abs().sum(dim=(1, 2, 3)) * 2.0 ** -25 / float(net.cnn.struct.xscale[l])).view(1, -1, 1, 1)


RATIOS = []     # (what, layer, max |product - float64|, e32, ratio): what the last checks measured


def check_layers(net, crop, layers, feat, what, floor=False, feat_rows=None):
    """layers: {l: (n, C, H, W) raw output of the product}; crop: the (n, 4, 256, 256) uint8 input.  Every layer present whose input is
    present too (the crop for l = 0) must be finite and within K * e32[l] of ref_layer on the product's own previous output, where
    e32[l] = max |torch fp32 - float64| of the same layer on the same input; entry-wise maximum, no entry left out.  The feature
    rows `feat_rows` of `feat` are judged on the deepest layer present (conv6 on the kept path, else conv4 through float64
    conv5 + conv6 + Linear).  floor: add scale_floor (weight sets B / C).  Returns the worst ratio."""
    worst = 0.0
    todo = [(l, crop if l == 0 else layers.get(l - 1)) for l in sorted(layers)]
    deep = max(layers)
    todo.append((6, layers[deep]))
    for l, prev in todo:
        if prev is None:
            continue
        if l == 6:
            r64, r32 = ref_from(net.sd, deep + 1, prev), ref_from(net.sd, deep + 1, prev, torch.float32)
            got = feat if feat_rows is None else feat[feat_rows]
            name = 'feature (from conv%d)' % (deep + 1)
        else:
            r64, r32 = ref_layer(net.sd, l, prev), ref_layer(net.sd, l, prev, torch.float32)
            got, name = layers[l], 'conv%d' % (l + 1)
        got = got.cpu().double()
        assert got.shape == r64.shape, '%s %s: shape %s vs %s' % (what, name, tuple(got.shape), tuple(r64.shape))
        assert bool(torch.isfinite(got).all()), '%s %s: not finite' % (what, name)
        e32 = float((r32.double() - r64).abs().max())
        err = (got - r64).abs()
        fl = scale_floor(net, l) if floor else 0.0
        worst_i = int(torch.argmax((err - fl).flatten()))
        e = float((err - fl).flatten()[worst_i])
        ratio = 0.0 if e <= 0.0 else (e / e32 if e32 > 0.0 else float('inf'))
        RATIOS.append((what, name, float(err.max()), e32, ratio))
        print('cnn-ratio | %s | %s | err %.3e | e32 %.3e | ratio %.3f%s' % (what, name, float(err.max()), e32, ratio, ' | floor' if floor and l in range(1, 6) else ''))
        assert e <= K * e32, '%s %s: |product - float64| = %.3e at %s, %.2f x the fp32 reference error %.3e (bound %g x)' % (
            what, name, float(err.flatten()[worst_i]), tuple(int(v) for v in np.unravel_index(worst_i, tuple(err.shape))), ratio, e32, K)
        worst = max(worst, ratio)
    return worst


# ------------------------------------------------------------------------------------------------
# weight sets (counter-based like synth.fill_state_dict: nothing is stored)
# ------------------------------------------------------------------------------------------------
CNN_KEYS = ['map_conv.%d.%s' % (i, n) for i in range(0, 18) if i % 3 != 2 for n in ('weight', 'bias')] + ['map_feature.weight', 'map_feature.bias']
C_VARIANTS = ['C/w1*2^10', 'C/w3*2^-10', 'C/w4*2^10', 'C/w0*2^-10', 'C/g2*2^6']


def weight_set(base_sd, name, key='cnnw'):
    """The map CNN's parameters (a dict of fp32 CPU tensors).  A: the default.  B: trained-like spread -- GroupNorm gamma in [-2, 2]
    with exact zeros, beta in [-1, 1], convolution / Linear rows U(+-1/sqrt(fan_in)) times a per-output-channel 2^U(-8, 3), two
    all-zero output channels and one all-zero input channel per layer, biases up to +-4.  C/w<l>*2^+-10: A with convolution l
    (weights and bias) scaled, so its wscale moves; C/g<l>*2^6: A with GroupNorm l's gamma scaled, so the next layer's xscale drops.
    D: A with conv1's bias exactly zero (the all-zero crop then gives a zero-variance layer output)."""
    sd = {k: base_sd[k].detach().cpu().clone() for k in CNN_KEYS}
    if name == 'A':
        return sd
    if name == 'D':
        sd['map_conv.0.bias'].zero_()
        return sd
    if name.startswith('C/'):
        kind, l, s = name[2], int(name[3]), 2.0 ** int(name.split('^')[1])
        if kind == 'w':
            sd['map_conv.%d.weight' % (3 * l)] *= s
            sd['map_conv.%d.bias' % (3 * l)] *= s
        else:
            sd['map_conv.%d.weight' % (3 * l + 1)] *= s
        return sd
    assert name == 'B', name
    for k in CNN_KEYS:
        shape = tuple(sd[k].shape)
        layer = k.split('.')
        norm = layer[0] == 'map_conv' and int(layer[1]) % 3 == 1
        if norm and layer[-1] == 'weight':
            v = synth.counter_uniform(shape, key + '/B/' + k, -2.0, 2.0)
            v[::7] = 0.0
        elif norm:
            v = synth.counter_uniform(shape, key + '/B/' + k, -1.0, 1.0)
        elif layer[-1] == 'bias':
            v = synth.counter_uniform(shape, key + '/B/' + k, -4.0, 4.0)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = synth.counter_uniform(shape, key + '/B/' + k, -1.0, 1.0) / math.sqrt(fan_in)
            mag = 2.0 ** synth.counter_uniform((shape[0],), key + '/B/mag/' + k, -8.0, 3.0)
            v = v * mag.reshape((-1,) + (1,) * (len(shape) - 1))
            v[1] = 0.0
            v[-1] = 0.0
            v[:, 2] = 0.0
        sd[k] = synth.f32(v).reshape(shape)
    return sd


class Net(object):
    """one weight set packed for one device"""

    def __init__(self, dev, sd, conv2_plain=False):
        self.sd = {k: sd[k].detach().cpu() for k in CNN_KEYS}
        self.cnn = params.pack_cnn({k: v.to(dev) for k, v in self.sd.items()})
        if conv2_plain:
            self.cnn.struct.conv2_plain = 1
        self.dev = dev


# ------------------------------------------------------------------------------------------------
# crops and poses
# ------------------------------------------------------------------------------------------------
CROP_FAMILIES = ['const', 'pixel', 'checker', 'random', 'road']


def road_poses(n, key, lo=40.0, hi=200.0):
    fr = np.zeros((n, 4))
    fr[:, 0] = synth.counter_uniform((n,), key + '/x', lo, hi)
    fr[:, 1] = synth.counter_uniform((n,), key + '/y', lo, hi)
    ang = synth.counter_uniform((n,), key + '/h', -np.pi, np.pi)
    fr[:, 2], fr[:, 3] = np.cos(ang), np.sin(ang)
    return synth.f32(fr).contiguous(), torch.tensor([i % 2 for i in range(n)], dtype=torch.int32)


def road_env():
    import make_golden as mg
    raster, dx = mg.g2_inputs()[:2]
    return synth.SyntheticMapEnv(raster, dx)


def oracle_crop(env, fr, mi):
    return mapenv.map_crop(env.nusc_raster.cpu(), env.nusc_dx.cpu(), fr.cpu(), mi.cpu().long(), env.bounds)


def crop_family(name, key='cnnc'):
    """uint8 (n, 4, 256, 256).  const: all 0 / all 1 / all 255.  pixel: one texel = 255 in an otherwise zero crop -- (0,0), (254,254) (the
    last texel conv1 reads), (255,255) (which it does not), (128,128), each in all four layers, and (128,128) in layer 3 only: the
    outlier that drives a normalised activation towards sqrt(C H W) and the scaled fp16 operand towards its ceiling.  checker: 0 / 255
    boards of period 1 and 2.  random: uniform bytes.  road: two crops of the synthetic road raster."""
    if name == 'const':
        c = torch.zeros((3, 4, 256, 256), dtype=torch.uint8)
        c[1], c[2] = 1, 255
    elif name == 'pixel':
        c = torch.zeros((5, 4, 256, 256), dtype=torch.uint8)
        for i, (y, x) in enumerate([(0, 0), (254, 254), (255, 255), (128, 128)]):
            c[i, :, y, x] = 255
        c[4, 3, 128, 128] = 255
    elif name == 'checker':
        yy, xx = torch.meshgrid(torch.arange(256), torch.arange(256), indexing='ij')
        c = torch.stack([(((yy // p + xx // p) % 2) * 255).to(torch.uint8).expand(4, 256, 256) for p in (1, 2)]).contiguous()
    elif name == 'random':
        c = torch.from_numpy(np.floor(synth.counter_uniform((2, 4, 256, 256), key + '/rnd', 0.0, 256.0)).astype(np.uint8))
    else:
        assert name == 'road', name
        env = road_env()
        c = oracle_crop(env, *road_poses(2, key + '/road'))
    return c.contiguous()


def gather_rasters():
    """(name, raster (M, 4, H, W) uint8, dx (M, 2) float64): pixel (0, 0) of every layer unlike anything else in the raster, so a
    sample that leaves the map (-> pixel (0, 0), crop_dev.h) is visible in conv1's output"""
    out = []
    base, dx2 = synth.make_raster(1024, 1024, M=2)
    for name, dx in (('0.25', [[0.25, 0.25]] * 2), ('0.125', [[0.125, 0.125]] * 2), ('0.25/non-round', [[0.25, 0.2500175], [0.2500325, 0.25]]),
                     ('make_raster', dx2.tolist()), ('1/3', [[1.0 / 3.0, 1.0 / 3.0]] * 2)):
        out.append((name, base.clone(), torch.tensor(dx, dtype=torch.float64)))
    r3, dx3 = synth.make_raster(768, 1280, M=3)
    out.append(('768x1280 x3', r3, dx3))
    for _, r, _ in out:
        for m in range(r.shape[0]):
            for c in range(4):
                r[m, c, 0, 0] = 201 + 10 * m + c
    return out


def gather_poses(raster, dx):
    """(n, 4) fp32 UNNORMALISED poses (x, y, cos, sin) and map indices interleaved over the maps: inside, across each border, wholly
    outside, NaN in each component, +-1e30, and heading 0 / pi/2 at coordinates where g / dx is exactly k + 0.5 for a whole crop row
    when dx is 0.25 or 0.125 (lwise[0] = -17 and wwise[0] = -38.5 are exact: round-half-even ties)."""
    M, _, H, W = raster.shape
    wm, hm = W * float(dx[0, 0]), H * float(dx[0, 1])
    c, s = math.cos(0.7), math.sin(0.7)
    p = [[0.5 * wm, 0.5 * hm, c, s], [0.31 * wm, 0.62 * hm, -s, c],
         [3.0, 0.5 * hm, 1.0, 0.0], [wm - 3.0, 0.5 * hm, 1.0, 0.0], [0.5 * wm, 3.0, c, -s], [0.5 * wm, hm - 3.0, -c, s],
         [-500.0, -500.0, c, s], [wm + 300.0, 0.5 * hm, 0.0, 1.0]]
    for k in range(4):
        q = [0.4 * wm, 0.4 * hm, c, s]
        q[k] = float('nan')
        p.append(q)
    p += [[1e30, 0.5 * hm, c, s], [0.5 * wm, -1e30, c, s], [-1e30, 1e30, 1.0, 0.0]]
    tie = 0.0625 if float(dx[0, 0]) == 0.125 else 0.125
    p += [[27.0 + tie, 58.5 + tie, 1.0, 0.0], [58.5 + tie, 27.0 + tie, 0.0, 1.0]]
    fr = torch.tensor(p, dtype=torch.float32).contiguous()
    return fr, torch.tensor([i % M for i in range(len(p))], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------
# driving the library
# ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def options(monkeypatch, **env):
    """STRIVE_<NAME> variables for the block (tests/conftest.py maps them onto the library's options), the environment as it was after"""
    for k, v in env.items():
        monkeypatch.setenv('STRIVE_' + k.upper(), str(v))
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv('STRIVE_' + k.upper())


FORM_ENV = {'default': {}, 'default_s4': {'cnn_tail_s': 4}, 'throughput': {'cnn_small_batch': 0}, 'throughput_s2': {'cnn_small_batch': 0, 'cnn_tail_s': 2},
             'plain': {'cnn_small_batch': 0, 'conv_ws': 0, 'conv_wsx': 0},
            'conv2_plain': {'cnn_small_batch': 0}, 'kept': {}, 'recompute': {'cnn_small_batch': 0}, 'from_crop': {}}


def sync(dev):
    if str(dev) != 'cpu':
        torch.cuda.synchronize()


class Run(object):
    """One map environment and pose set on one device, and the entry points over it.  pos: NORMALISED poses; mean / std: the
    normaliser the kernels undo ((0, 1): pos is the pose)."""

    def __init__(self, lib, dev, env, fr, mi, mean=(0, 0, 0, 0), std=(1, 1, 1, 1)):
        self.lib, self.dev, self.env = lib, dev, env
        self.mp = params.pack_map(env, dev)
        self.pos, self.mi = fr.to(dev).contiguous(), mi.to(torch.int32).to(dev).contiguous()
        self.mean, self.std = L.f4(mean), L.f4(std)
        self.n = fr.shape[0]
        self.stream = L.stream_ptr(self.pos)

    def buffers(self, n, fill=0):
        wsb = self.lib.query('strive_map_cnn_workspace_bytes', n)
        return torch.full((wsb,), fill, dtype=torch.uint8, device=self.dev), wsb, torch.zeros((n, 64), device=self.dev)

    def fwd(self, net, n=None, ws=None, fill=0):
        n = self.n if n is None else n
        ws_, wsb, feat = self.buffers(n, fill)
        ws = ws_ if ws is None else ws
        self.lib.call('strive_map_cnn_fwd', self.mp.ref(), net.cnn.ref(), L.ptr(self.pos[:n]), self.mean, self.std, L.ptr(self.mi[:n]), n,
                      L.ptr(feat), L.ptr(ws), wsb, self.stream)
        sync(self.dev)
        return ws, feat.cpu()

    def bench_layer(self, net, code, ws, n=None):
        n = self.n if n is None else n
        feat = torch.zeros((n, 64), device=self.dev)
        self.lib.call('strive_map_cnn_bench_layer', self.mp.ref(), net.cnn.ref(), code, L.ptr(self.pos[:n]), self.mean, self.std,
                      L.ptr(self.mi[:n]), n, L.ptr(feat), L.ptr(ws), ws.numel(), self.stream)
        sync(self.dev)
        return feat.cpu()

    def keep(self, net, splits, fill=0xFF):
        """strive_map_cnn_fwd_keep written in calls over the row ranges `splits`; the kept buffer starts as 0xFF bytes"""
        n = self.n
        ws, wsb, feat = self.buffers(n)
        kb = self.lib.query('strive_map_cnn_keep_bytes', n)
        kept = torch.full((kb,), fill, dtype=torch.uint8, device=self.dev)
        for lo, hi in splits:
            self.lib.call('strive_map_cnn_fwd_keep', self.mp.ref(), net.cnn.ref(), L.ptr(self.pos[lo:hi]), self.mean, self.std,
                          L.ptr(self.mi[lo:hi]), hi - lo, L.ptr(feat[lo:hi]), L.ptr(ws), wsb, L.ptr(kept), kb, n, lo, self.stream)
        sync(self.dev)
        return kept, feat.cpu()


def from_crop(lib, dev, net, crop, fill=0):
    n = crop.shape[0]
    wsb = lib.query('strive_map_cnn_workspace_bytes', n)
    ws = torch.full((wsb,), fill, dtype=torch.uint8, device=dev)
    feat = torch.zeros((n, 64), device=dev)
    c = crop.to(dev).contiguous()
    lib.call('strive_map_cnn_fwd_from_crop', net.cnn.ref(), L.ptr(c), n, L.ptr(feat), L.ptr(ws), wsb, L.stream_ptr(c))
    sync(dev)
    return ws, feat.cpu()


def layers_of(buf, wmap, n, which=range(4)):
    return {l: decode(read_raw(buf, wmap, l, n), l, n) for l in which}


def run_form(lib, dev, monkeypatch, form, run, sd):
    """One form over all of run's poses -> (layers {l: NCHW raw output of the rows the buffers still hold}, feature (n, 64),
    (first row, rows) the layers belong to)."""
    net = Net(dev, sd, conv2_plain=(form == 'conv2_plain'))
    n = run.n
    with options(monkeypatch, **FORM_ENV[form]):
        if form == 'kept':
            k = max(1, (2 * n) // 3)
            kept, feat = run.keep(net, [(0, n)] if n == 1 else [(0, k), (k, n)])
            return net, layers_of(kept, KeepMap(n), n, range(6)), feat, (0, n)
        ws, feat = run.fwd(net)
        n0, nl = last_chunk(lib, n)
        wmap = WorkspaceMap(chunk_of(lib, n))
        if form == 'recompute':
            assert n0 == 0, 'strive_map_cnn_bench_layer carves the workspace for N samples: one chunk only'
            for code in (4, 5, 6):
                feat = run.bench_layer(net, code, ws)
            return net, layers_of(ws, wmap, nl, range(3, 6)), feat, (0, n)
        return net, layers_of(ws, wmap, nl), feat, (n0, nl)
