"""The map CNN layer by layer: every raw layer output of every kernel form against a float64 reference of THAT layer fed the
product's own previous output (tests/cnn_layers.py), within K times the error torch fp32 makes on the same input -- entry-wise
maximum, nothing left out -- plus the bit-identity claims of DESIGN section 4 on the raw bytes.  Every case is written once, takes a
library handle and a device, and runs on the host emulation (-m "not gpu") and on the MI355X (-m gpu).  The measured ratios
max |product - float64| / e32 per layer and form, from which K = 16 comes, are in profiles/r13_cnn_layer_ratios.md; every check
prints its figures as `cnn-ratio | ...` lines (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

import cnn_layers as cl
from util import product_model, assert_close
from strive_amd import _lib as L, synth
from strive_amd.constants import state_norm_tensors

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))
DEV = 'cuda:0'
slow = pytest.mark.slow


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'
    return L.get_lib()


@pytest.fixture(scope='module')
def sd():
    return product_model()[1]


# ------------------------------------------------------------------------------------------------
# 1. the mirror of the layouts
# ------------------------------------------------------------------------------------------------
def _mirror_case(lib):
    for n in (1, 8, 97, 512, 1024, 1500):
        assert cl.workspace_bytes(n) == lib.query('strive_map_cnn_workspace_bytes', n), 'workspace of %d samples' % n
        assert cl.KeepMap(n).total == lib.query('strive_map_cnn_keep_bytes', n), 'kept buffer of %d samples' % n


def test_layout_mirror_equals_the_library(emu):
    _mirror_case(emu)


@pytest.mark.gpu
def test_layout_mirror_equals_the_library_gpu(gpu):
    _mirror_case(gpu)


# ------------------------------------------------------------------------------------------------
# 2. per-layer parity of every form
# ------------------------------------------------------------------------------------------------
_FULL = {}


def _full_reference(sd, crop, key):
    """float64 and fp32 features of the whole network on `crop` (cached per pose set: the sizes share one)"""
    if key not in _FULL:
        _FULL[key] = (cl.ref_from(sd, 0, crop), cl.ref_from(sd, 0, crop, torch.float32))
    return _FULL[key]


def _parity_case(lib, dev, monkeypatch, sd, form, n, nmax=None):
    """Road crops through one form: layers against ref_layer on the rows the buffers hold (the last chunk of the workspace, every row
    of the kept buffer); the feature of those rows against float64 GroupNorm + ReLU + rest of the network on the deepest layer read
    (which also pins the layout decode: a wrong decode of conv4 / conv6 cannot reproduce the product's feature).  Rows of earlier chunks have left no activations: their
    features are held to K times the END-TO-END fp32 error (fp32 network vs float64 network on the oracle's crop)."""
    nmax = n if nmax is None else nmax
    env = cl.road_env()
    fr, mi = cl.road_poses(nmax, 'lay/par')
    crop = cl.oracle_crop(env, fr[:n], mi[:n])
    what = '%s | %s | n=%d' % (dev, form, n)
    if form == 'from_crop':
        net = cl.Net(dev, sd)
        ws, feat = cl.from_crop(lib, dev, net, crop)
        (n0, nl) = cl.last_chunk(lib, n)
        layers = cl.layers_of(ws, cl.WorkspaceMap(cl.chunk_of(lib, n)), nl)
    else:
        net, layers, feat, (n0, nl) = cl.run_form(lib, dev, monkeypatch, form, cl.Run(lib, dev, env, fr[:n], mi[:n]), sd)
    cl.check_layers(net, crop[n0:n0 + nl], layers, feat, what, feat_rows=slice(n0, n0 + nl))
    if n0 > 0:
        f64, f32 = _full_reference(net.sd, cl.oracle_crop(env, fr, mi), 'par/%d' % nmax)
        e32 = float((f32[:n].double() - f64[:n]).abs().max())
        err = float((feat.double() - f64[:n]).abs().max())
        print('cnn-ratio | %s | feature, all rows (end to end) | err %.3e | e32 %.3e | ratio %.3f' % (what, err, e32, err / e32))
        assert err <= cl.K * e32, '%s: feature %.3e from the float64 network, %.2f x the fp32 network (%.3e)' % (what, err, err / e32, e32)


EMU_PARITY = [(f, n) for f in ('default', 'throughput', 'plain', 'conv2_plain', 'kept', 'recompute', 'from_crop') for n in (1, 3)] + \
             [('default_s4', 5), ('throughput_s2', 5)]
EMU_PARITY_SLOW = [(f, 9) for f in ('default', 'throughput', 'plain', 'conv2_plain', 'kept', 'recompute', 'from_crop')] + \
                  [('default_s4', 8), ('throughput_s2', 8)]


@pytest.mark.parametrize('form,n', EMU_PARITY + [pytest.param(f, n, marks=slow) for f, n in EMU_PARITY_SLOW])
def test_layer_parity(emu, sd, monkeypatch, form, n):
    _parity_case(emu, 'cpu', monkeypatch, sd, form, n)


GPU_SIZES = [1, 8, 96, 97, 256, 257, 512, 513, 600, 1024, 1025]


@pytest.mark.gpu
@pytest.mark.parametrize('n', GPU_SIZES)
def test_layer_parity_default_chain_gpu(gpu, sd, monkeypatch, n):
    """both sides of every threshold: small batch at 96, one-sample tail at 256, chunk at 512, CNN_CHUNK_MAX at 1024; 600 = a
    512-sample throughput chunk, then an 88-sample small-batch chunk in the same call"""
    _parity_case(gpu, DEV, monkeypatch, sd, 'default', n, nmax=1025)


@pytest.mark.gpu
@pytest.mark.parametrize('form,n', [(f, n) for f, ns in (('throughput', (1, 8, 96)), ('throughput_s2', (5, 96)), ('default_s4', (5, 8)),
                                                          ('plain', (8, 97, 300)), ('conv2_plain', (8, 97)), ('kept', (1, 9, 97, 300)),
                                                          ('recompute', (1, 8, 97, 257, 512)), ('from_crop', (1, 8, 97, 300))) for n in ns])
def test_layer_parity_forms_gpu(gpu, sd, monkeypatch, form, n):
    _parity_case(gpu, DEV, monkeypatch, sd, form, n, nmax=1025)


@pytest.mark.gpu
def test_chunking_does_not_change_the_features_gpu(gpu, sd, monkeypatch):
    """600 samples as nine chunks of 64 and a remainder of 24 (all on the small-batch chain) = the default chunking, bit for bit"""
    env = cl.road_env()
    fr, mi = cl.road_poses(1025, 'lay/par')
    run, net = cl.Run(gpu, DEV, env, fr[:600], mi[:600]), cl.Net(DEV, sd)
    _, want = run.fwd(net)
    with cl.options(monkeypatch, cnn_chunk=64):
        _, got = run.fwd(net)
    assert torch.equal(got, want), 'rows %s differ' % torch.nonzero((got != want).any(1)).flatten().tolist()[:10]


# ------------------------------------------------------------------------------------------------
# bit-identity claims
# ------------------------------------------------------------------------------------------------
def _codes_case(lib, dev, monkeypatch, sd, n):
    """strive_map_cnn_bench_layer codes 1 / 51 (conv2: conv_bf6 / conv_ws), 2 / 52 and 3 / 53 (conv3, conv4: conv_bf6 / conv_wsx) on the
    same input: the activations AND the partial GroupNorm moments they leave are the same bytes."""
    env = cl.road_env()
    fr, mi = cl.road_poses(n, 'lay/codes')
    run, net = cl.Run(lib, dev, env, fr, mi), cl.Net(dev, sd)
    with cl.options(monkeypatch, cnn_small_batch=0):
        ws, _ = run.fwd(net)
    wmap = cl.WorkspaceMap(n)
    for l, (a, b) in ((1, (1, 51)), (2, (2, 52)), (3, (3, 53))):
        out = []
        for code in (a, b):
            ws[wmap.act[l]:wmap.act[l] + n * cl.L_OUT[l] * 4].zero_()
            ws[wmap.st[l]:wmap.st[l] + n * cl.NPARTS[l] * cl.GNSTATS_BYTES].zero_()
            run.bench_layer(net, code, ws)
            out.append((cl.read_raw(ws, wmap, l, n), cl.read_stats(ws, wmap, l, n, cl.NPARTS[l])))
        assert bool(out[0][0].any()) and bool(out[0][1].any()), 'code %d wrote nothing' % a
        assert torch.equal(out[0][0], out[1][0]), 'conv%d activations: codes %d and %d differ' % (l + 1, a, b)
        assert torch.equal(out[0][1], out[1][1]), 'conv%d moments: codes %d and %d differ' % (l + 1, a, b)


def test_specialised_wave_kernels_bit_identical(emu, sd, monkeypatch):
    _codes_case(emu, 'cpu', monkeypatch, sd, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [3, 97, 300])
def test_specialised_wave_kernels_bit_identical_gpu(gpu, sd, monkeypatch, n):
    _codes_case(gpu, DEV, monkeypatch, sd, n)


def _chains_case(lib, dev, monkeypatch, sd, n):
    """small-batch chain vs throughput chain: the raw bytes of conv1 .. conv4 and the feature; then each of them again over a
    workspace of 0xFF bytes: the same bytes in every activation block (nothing is read that was not written); the kept buffer
    likewise (0xFF vs zero filled)."""
    env = cl.road_env()
    fr, mi = cl.road_poses(n, 'lay/chains')
    run, net = cl.Run(lib, dev, env, fr, mi), cl.Net(dev, sd)
    n0, nl = cl.last_chunk(lib, n)
    wmap = cl.WorkspaceMap(cl.chunk_of(lib, n))
    res = {}
    for form, env_ in (('default', {}), ('throughput', {'cnn_small_batch': 0})):
        with cl.options(monkeypatch, **env_):
            for fill in (0, 0xFF):
                ws, feat = run.fwd(net, fill=fill)
                res[form, fill] = [cl.read_raw(ws, wmap, l, nl) for l in range(4)] + [feat]
        for l in range(5):
            assert torch.equal(res[form, 0][l], res[form, 0xFF][l]), '%s chain, %s: depends on what the workspace held' % (
                form, 'conv%d' % (l + 1) if l < 4 else 'feature')
    for l in range(5):
        assert torch.equal(res['default', 0][l], res['throughput', 0][l]), 'small-batch vs throughput chain: %s differs' % (
            'conv%d' % (l + 1) if l < 4 else 'feature')
    k = max(1, n // 2)
    splits = [(0, n)] if n == 1 else [(0, k), (k, n)]
    (k0, f0), (k1, f1) = run.keep(net, splits, fill=0), run.keep(net, splits, fill=0xFF)
    km = cl.KeepMap(n)
    for l in range(6):
        assert torch.equal(cl.read_raw(k0, km, l, n), cl.read_raw(k1, km, l, n)), 'kept conv%d depends on what the buffer held' % (l + 1)
    assert torch.equal(f0, f1)


def test_chains_bit_identical_and_read_nothing_unwritten(emu, sd, monkeypatch):
    _chains_case(emu, 'cpu', monkeypatch, sd, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 8, 96, 600])
def test_chains_bit_identical_and_read_nothing_unwritten_gpu(gpu, sd, monkeypatch, n):
    _chains_case(gpu, DEV, monkeypatch, sd, n)


def _tail_case(lib, dev, monkeypatch, sd, n):
    """fused tail with 1, 2, 4 samples per workgroup: the same feature bits; the conv5 / conv6 outputs it keeps equal those of the
    separate kernels of the training recompute on the same conv4 output within the 2e-6 DESIGN section 4 states."""
    env = cl.road_env()
    fr, mi = cl.road_poses(n, 'lay/tail')
    run, net = cl.Run(lib, dev, env, fr, mi), cl.Net(dev, sd)
    feats = []
    for s in (1, 2, 4):
        with cl.options(monkeypatch, cnn_tail_s=s):
            feats.append(run.fwd(net)[1])
    assert torch.equal(feats[0], feats[1]) and torch.equal(feats[0], feats[2]), 'tail S = 1, 2, 4'
    kept, fk = run.keep(net, [(0, n)])
    with cl.options(monkeypatch, cnn_small_batch=0):
        ws, f1 = run.fwd(net)
        for code in (4, 5, 6):
            fs = run.bench_layer(net, code, ws)
    km, wm = cl.KeepMap(n), cl.WorkspaceMap(n)
    for l in range(4):
        assert torch.equal(cl.read_raw(kept, km, l, n), cl.read_raw(ws, wm, l, n)), 'kept conv%d vs workspace' % (l + 1)
    for l in (4, 5):
        assert_close(cl.decode(cl.read_raw(kept, km, l, n), l, n), cl.decode(cl.read_raw(ws, wm, l, n), l, n), 2e-6, 2e-6,
                     'conv%d kept by the fused tail vs the separate kernel' % (l + 1))
    assert_close(fk, fs, 2e-6, 2e-6, 'feature: fused tail vs separate kernels')


@pytest.mark.parametrize('n', [3, pytest.param(5, marks=slow)])
def test_fused_tail_forms_and_kept_outputs(emu, sd, monkeypatch, n):
    _tail_case(emu, 'cpu', monkeypatch, sd, n)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [5, 8, 97, 300])
def test_fused_tail_forms_and_kept_outputs_gpu(gpu, sd, monkeypatch, n):
    _tail_case(gpu, DEV, monkeypatch, sd, n)


# ------------------------------------------------------------------------------------------------
# 4. weights and crops that leave the comfortable middle
# ------------------------------------------------------------------------------------------------
def _weights_case(lib, dev, monkeypatch, sd, wname, family, forms=('default',)):
    """strive_map_cnn_fwd_from_crop on a crop family under a weight set: finite and within K e32 (B / C: plus the floor of the per-tensor
    power-of-two scaling, cnn_layers.scale_floor) at conv1 .. conv4 and the feature"""
    net = cl.Net(dev, cl.weight_set(sd, wname))
    crop = cl.crop_family(family)
    n = crop.shape[0]
    for form in forms:
        with cl.options(monkeypatch, **cl.FORM_ENV[form]):
            ws, feat = cl.from_crop(lib, dev, net, crop)
        layers = cl.layers_of(ws, cl.WorkspaceMap(n), n)
        cl.check_layers(net, crop, layers, feat, '%s | %s/%s x %s | n=%d' % (dev, wname, form, family, n), floor=wname[0] in 'BC')


WEIGHT_CASES = [('A', f) for f in cl.CROP_FAMILIES] + [('B', f) for f in cl.CROP_FAMILIES] + \
               [(c, f) for c in cl.C_VARIANTS for f in ('road', 'const', 'pixel')] + [('D', f) for f in ('road', 'const', 'pixel')]
EMU_WEIGHT_FAST = {('A', 'pixel'), ('B', 'const'), ('D', 'const'), ('C/g2*2^6', 'pixel')}


@pytest.mark.parametrize('wname,family', [wf if wf in EMU_WEIGHT_FAST else pytest.param(*wf, marks=slow) for wf in WEIGHT_CASES])
def test_weight_sets_and_crop_families(emu, sd, monkeypatch, wname, family):
    _weights_case(emu, 'cpu', monkeypatch, sd, wname, family)


@pytest.mark.gpu
@pytest.mark.parametrize('wname,family', WEIGHT_CASES)
def test_weight_sets_and_crop_families_gpu(gpu, sd, monkeypatch, wname, family):
    _weights_case(gpu, DEV, monkeypatch, sd, wname, family, forms=('default', 'throughput'))


# ------------------------------------------------------------------------------------------------
# 5. the fused gather against the oracle's crop
# ------------------------------------------------------------------------------------------------
def _gather_case(lib, dev, sd, which, norm):
    """conv1's output of the fused crop -> conv1 kernel, one tile per workgroup (strive_map_cnn_fwd, small batch) and four
    (bench-layer code 0), is the bytes conv1 leaves when strive_map_cnn_fwd_from_crop is handed the CPU oracle's crop of the same
    poses."""
    name, raster, dx = cl.gather_rasters()[which]
    env = synth.SyntheticMapEnv(raster, dx)
    fr, mi = cl.gather_poses(raster, dx)
    n = fr.shape[0]
    if norm == 'model':
        mean, std = [t[:4] for t in state_norm_tensors()]
        pos = (fr - mean) / std
        frame = pos * std + mean                      # what the kernels undo: one rounded multiply, one rounded add
    else:
        mean, std, pos, frame = torch.zeros(4), torch.ones(4), fr, fr
    crop = cl.oracle_crop(env, frame, mi)
    assert len(set(int(v) for v in crop.flatten()[::97].tolist())) > 2, 'the crops see pixel (0, 0) and the roads'
    net = cl.Net(dev, sd)
    run = cl.Run(lib, dev, env, pos, mi, mean.tolist(), std.tolist())
    wmap = cl.WorkspaceMap(n)
    ws_c, _ = cl.from_crop(lib, dev, net, crop)
    want = cl.read_raw(ws_c, wmap, 0, n).view(torch.float32).view(n, -1)
    ws_f, _ = run.fwd(net)
    ws_b = torch.zeros_like(ws_f)
    run.bench_layer(net, 0, ws_b)
    for what, ws in (('one tile per workgroup', ws_f), ('four tiles per workgroup', ws_b)):
        got = cl.read_raw(ws, wmap, 0, n).view(torch.float32).view(n, -1)
        bad = torch.nonzero((got.view(torch.int32) != want.view(torch.int32)).any(1)).flatten().tolist()
        assert not bad, 'raster %s, %s normaliser, conv1 %s: poses %s differ from conv1 of the oracle crop' % (name, norm, what, bad)


GATHER_CASES = [(i, nm) for i in range(6) for nm in ('unit', 'model')]


@pytest.mark.parametrize('which,norm', [(5, 'unit')] + [pytest.param(i, nm, marks=slow) for i, nm in GATHER_CASES if (i, nm) != (5, 'unit')])
def test_fused_gather_equals_conv1_of_the_oracle_crop(emu, sd, which, norm):
    _gather_case(emu, 'cpu', sd, which, norm)


@pytest.mark.gpu
@pytest.mark.parametrize('which,norm', GATHER_CASES)
def test_fused_gather_equals_conv1_of_the_oracle_crop_gpu(gpu, sd, which, norm):
    _gather_case(gpu, DEV, sd, which, norm)
