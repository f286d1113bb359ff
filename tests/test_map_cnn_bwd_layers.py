"""The map CNN's backward step by step: what one strive_map_cnn_bwd / _bwd_kept call leaves in its workspace -- dL/d(raw output) of
all six layers, the moments, the GroupNorm sums -- and every block of the flat parameter gradient against a float64 reference of
THAT step fed the product's own upstream adjoint and raw activations (tests/cnn_bwd_layers.py), the matrix-core data gradient
alone through strive_map_cnn_bwd_bench_dgrad, within K_b (e_fmt + e32), entry-wise maximum; only entries whose ReLU mask is
ambiguous are left out of the entry-wise dy check, with their possible contribution added as explicit slack and their number
capped.  Every case is written once, takes a library handle and a device, and runs on the host emulation (-m "not gpu") and on
the MI355X (-m gpu).  The measured ratios, from which K_b comes, are in profiles/r15_cnn_bwd_layer_ratios.md; every check prints
its figures as `cnn-bwd-ratio | ...` lines (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

import cnn_layers as cl
import cnn_bwd_layers as bl
from util import product_model
from strive_amd import _lib as L, synth

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
    for n in (1, 8, 255, 256, 257, 600):
        assert bl.bwd_workspace_bytes(n) == lib.query('strive_map_cnn_bwd_workspace_bytes', n), 'backward workspace of %d samples' % n
    assert bl.GRAD.total == lib.query('strive_map_cnn_param_count')


def test_bwd_layout_mirror_equals_the_library(emu):
    _mirror_case(emu)


@pytest.mark.gpu
def test_bwd_layout_mirror_equals_the_library_gpu(gpu):
    _mirror_case(gpu)


def test_bf16_split_is_the_headers():
    """hi is the nearest bf16 (ties to even), lo the nearest bf16 of the exact rest: v = hi + lo up to 2^-16 |v| (half an ulp of 8 bits, twice), both pieces have
    16 zero low bits"""
    v = synth.f32(synth.counter_uniform((4096,), 'bwd/split', -1.0, 1.0)) * 2.0 ** torch.arange(-40, 24).repeat(64).float()
    v = torch.cat([v, torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 2.0 ** -126])])   # ties: to even
    hi, lo = bl.bf16_split(v)
    assert not bool((hi.view(torch.int32) & 0xFFFF).any()) and not bool((lo.view(torch.int32) & 0xFFFF).any())
    assert bool(((v - hi).abs() <= 2.0 ** -8 * v.abs()).all())
    assert bool(((v.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * v.abs().double()).all())
    assert hi[-5:-1].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0]


# ------------------------------------------------------------------------------------------------
# 2. one call, every step
# ------------------------------------------------------------------------------------------------
def _inputs(n, wname, family, key='bwd/par'):
    """(env, poses, map indices, crops of the CPU oracle at these poses).  road: the synthetic road raster.  const / pixel / checker:
    rasters that are all 0 / all 1 / all 255, zero but for a 3 x 3 block of 255 under every pose, 0 / 255 boards of period 1 and 2 --
    what the oracle's crop makes of them is the layer-0 input"""
    fr, mi = cl.road_poses(n, key)
    if family == 'road':
        env = cl.road_env()
    else:
        assert n == 3
        if family == 'const':
            raster = torch.zeros((3, 4, 1024, 1024), dtype=torch.uint8)
            raster[1], raster[2] = 1, 255
            mi = torch.tensor([0, 1, 2], dtype=torch.int32)
        elif family == 'pixel':
            raster = torch.zeros((1, 4, 1024, 1024), dtype=torch.uint8)
            for x, y in fr[:, :2].tolist():
                px, py = int(round(x / 0.25)), int(round(y / 0.25))
                raster[0, :, py - 1:py + 2, px - 1:px + 2] = 255
            mi = torch.zeros(3, dtype=torch.int32)
        else:
            assert family == 'checker', family
            yy, xx = torch.meshgrid(torch.arange(1024), torch.arange(1024), indexing='ij')
            raster = torch.stack([(((yy // p + xx // p) % 2) * 255).to(torch.uint8).expand(4, 1024, 1024) for p in (1, 2)]).contiguous()
            mi = torch.tensor([0, 1, 0], dtype=torch.int32)
        env = synth.SyntheticMapEnv(raster, torch.tensor([[0.25, 0.25]] * raster.shape[0], dtype=torch.float64))
    crop = cl.oracle_crop(env, fr, mi)
    if family == 'pixel':
        hot = (crop != 0).flatten(1).sum(1)
        assert bool((hot > 0).all()) and bool((hot < 4096).all()), 'pixel crops: %s texels set' % hot.tolist()
    return env, fr, mi, crop


def _step_case(lib, dev, monkeypatch, sd, form, path, n, wname='A', family='road', kind='uniform', twice=False):
    """One call over n <= 256 samples into a zeroed flat gradient; everything copied to the host; then the hook layer by layer."""
    env, fr, mi, crop = _inputs(n, wname, family)
    d_feat = bl.d_feat_of(n, 'bwd/par', kind)
    net = cl.Net(dev, cl.weight_set(sd, wname))
    what = '%s | %s/%s | %s x %s%s | n=%d' % (dev, form, path, wname, family, '' if kind == 'uniform' else ' ' + kind, n)
    judge = bl.Judge(what)
    with cl.options(monkeypatch, **dict(cl.FORM_ENV['recompute' if path == 'recompute' else 'kept'], **bl.FORM_ENV[form])):
        bw = bl.Backward(lib, dev, cl.Run(lib, dev, env, fr, mi), net, d_feat, path)
        flat = bw.call()
        snap = bw.snapshot()
        flat2 = bw.call() if twice else None
        # (the hook runs the matrix-core kernels on the packed weight fragments, which the fp32 data-gradient form never packs)
        hooks = bw.hooks() if form != 'dgrad_igemm' else None
    assert bool(flat.any()), 'nothing was added to the flat gradient'
    acc = bl.check_chunk(judge, net, crop, d_feat, snap, flat, form, hooks)
    judge.done()
    if kind == 'tiny':
        # results must SCALE (bf16 keeps fp32's exponent): the same call with the unscaled d_feat, times 2^-20.  Where the code adds
        # in a fixed order -- G[5] (fc_bwd_kernel, one GroupNorm workgroup per sample) and conv6's weight gradient -- bit for bit;
        # elsewhere within the sum-order error K e32 of the scaled call
        with cl.options(monkeypatch, **dict(cl.FORM_ENV['recompute' if path == 'recompute' else 'kept'], **bl.FORM_ENV[form])):
            bw1 = bl.Backward(lib, dev, cl.Run(lib, dev, env, fr, mi), net, d_feat * 2.0 ** 20, path)
            flat1 = bw1.call() * 2.0 ** -20
            g5 = bw1.snapshot()['G'][5] * 2.0 ** -20
        assert torch.equal(g5.view(torch.int32), snap['G'][5].view(torch.int32)), '%s: G[5] does not scale by 2^-20 bit for bit' % what
        assert torch.equal(bl.GRAD.get(flat1, 'w5').view(torch.int32), bl.GRAD.get(flat, 'w5').view(torch.int32)), '%s: conv6 weight gradient does not scale' % what
        for name, _ in bl.GRAD_KEYS:
            r64, r32, sl, ef = acc[name]
            d = (bl.GRAD.get(flat1, name).double() - bl.GRAD.get(flat, name).double()).abs().max()
            assert float(d) <= bl.k_of('param', name) * float((r32.double() - r64).abs().max()), '%s: %s does not scale with d_feat (%.3e)' % (what, name, float(d))
    if kind == 'row':
        for l in range(6):
            other = [i for i in range(n) if i != n // 2]
            assert not bool(snap['G'][l][other].any()), 'G[%d]: rows of samples without an adjoint are not exactly zero' % l
            assert bool(snap['G'][l][n // 2].any())
    if twice:
        # A second identical call ADDS.  Its contribution is not the first one's bytes: the GroupNorm sums, the bias / gamma / beta
        # sums and the fp32 forms' weight gradients are added with atomics in an order that differs from run to run.  What differs
        # is the order of fp32 sums only (the format error and the ReLU masks are the same in both calls), so the two contributions
        # lie within K e32 of each other -- no e_fmt, no ambiguity slack -- plus the rounding of the addition itself.
        for name, _ in bl.GRAD_KEYS:
            r64, r32, sl, ef = acc[name]
            a, b = bl.GRAD.get(flat, name).double(), bl.GRAD.get(flat2, name).double()
            tol = 2.0 ** -23 * b.abs() + bl.k_of('param', name) * float((r32.double() - r64).abs().max())
            assert bool(((b - 2.0 * a).abs() <= tol).all()), '%s: %s after two calls is not twice the first (worst %.3e)' % (what, name, float((b - 2 * a).abs().max()))
        if form == 'mfma':
            # conv6's weight gradient is reproducible by construction: fc_bwd_kernel writes G[5] without atomics, GroupNorm backward
            # of the 512-entry layer is ONE workgroup per sample (one addition to S), and wgrad_reduce_kernel adds the partial
            # slots in a fixed order -- the two contributions are the same bytes, and doubling is exact
            a, b = bl.GRAD.get(flat, 'w5'), bl.GRAD.get(flat2, 'w5')
            assert torch.equal((2.0 * a).view(torch.int32), b.view(torch.int32)), '%s: conv6 weight gradient: the second call added other bytes' % what


FORMS = ['mfma', 'dgrad_igemm', 'wgrad_igemm', 'wgrad_tile']
EMU_STEP = [(f, p, n) for f in FORMS for p in ('recompute', 'kept') for n in (1, 2, 3)]
EMU_STEP_FAST = {('mfma', 'recompute', 1), ('mfma', 'kept', 3), ('mfma', 'recompute', 2), ('dgrad_igemm', 'kept', 2), ('wgrad_igemm', 'recompute', 1),
                 ('wgrad_tile', 'kept', 2)}
EMU_STEP_SLOW = [(f, p, n) for f in FORMS for p in ('recompute', 'kept') for n in (5, 9)]


@pytest.mark.parametrize('form,path,n', [c if c in EMU_STEP_FAST else pytest.param(*c, marks=slow) for c in EMU_STEP] +
                         [pytest.param(*c, marks=slow) for c in EMU_STEP_SLOW])
def test_backward_steps(emu, sd, monkeypatch, form, path, n):
    _step_case(emu, 'cpu', monkeypatch, sd, form, path, n, twice=(n == 2))


# 1 / 2 / 7 8 9: one sample, one pair, and both sides of the 8-sample units of the conv6 data gradient (2-sample units of conv5's
# and of the conv5 / conv6 weight gradients: odd and even); from 5 samples on a weight-gradient workgroup of conv1 loops over
# several units; 64 / 65 and 255 / 256: partial last groups next to full ones, up to the whole chunk
GPU_SIZES = [1, 2, 7, 8, 9, 64, 65, 255, 256]
GPU_STEP = [('mfma', 'recompute', n) for n in GPU_SIZES] + [('mfma', 'kept', n) for n in (1, 8, 9, 65, 255)] + \
           [(f, 'recompute', n) for f in FORMS[1:] for n in (7, 65, 256)] + [(f, 'kept', 9) for f in FORMS[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize('form,path,n', GPU_STEP)
def test_backward_steps_gpu(gpu, sd, monkeypatch, form, path, n):
    _step_case(gpu, DEV, monkeypatch, sd, form, path, n, twice=(n in (2, 9)))


# ------------------------------------------------------------------------------------------------
# 3. weights, crops and adjoints that leave the comfortable middle
# ------------------------------------------------------------------------------------------------
# set B: zero channels, zero gammas, row magnitudes 2^-8 .. 2^3 -- adjoints that span decades; C/: one layer's scale moved by 2^10;
# D x const: conv1's output of the all-zero crop has zero variance (rstd = 1 / sqrt(eps), the reference's eps = 1e-5)
INPUT_CASES = [('recompute', 3, 'B', 'road', 'uniform'), ('kept', 2, 'B', 'road', 'uniform'), ('kept', 3, 'C/w1*2^10', 'road', 'uniform'),
               ('kept', 3, 'A', 'const', 'uniform'), ('kept', 3, 'A', 'pixel', 'uniform'), ('kept', 3, 'A', 'checker', 'uniform'),
               ('kept', 3, 'D', 'const', 'uniform'), ('recompute', 3, 'A', 'road', 'row'), ('kept', 3, 'A', 'road', 'tiny')]
EMU_INPUT_FAST = {('kept', 2, 'B', 'road', 'uniform'), ('kept', 3, 'D', 'const', 'uniform'), ('recompute', 3, 'A', 'road', 'row')}


@pytest.mark.parametrize('path,n,wname,family,kind', [c if c in EMU_INPUT_FAST else pytest.param(*c, marks=slow) for c in INPUT_CASES])
def test_backward_steps_inputs(emu, sd, monkeypatch, path, n, wname, family, kind):
    _step_case(emu, 'cpu', monkeypatch, sd, 'mfma', path, n, wname, family, kind)


@pytest.mark.gpu
@pytest.mark.parametrize('path,n,wname,family,kind', INPUT_CASES + [('recompute', 9, 'B', 'road', 'uniform'), ('kept', 9, 'A', 'road', 'tiny')])
def test_backward_steps_inputs_gpu(gpu, sd, monkeypatch, path, n, wname, family, kind):
    _step_case(gpu, DEV, monkeypatch, sd, 'mfma', path, n, wname, family, kind)


# ------------------------------------------------------------------------------------------------
# 4. calls whose rows are gone: ranges of a kept buffer, two chunks
# ------------------------------------------------------------------------------------------------
def _range_case(lib, dev, monkeypatch, sd, n):
    """strive_map_cnn_bwd_kept_range in two calls, the last range first: the summed flat gradient against float64 autograd of the
    whole network within K_E2E times the end-to-end fp32 error"""
    env, fr, mi, crop = _inputs(n, 'A', 'road')
    d_feat = bl.d_feat_of(n, 'bwd/par')
    net = cl.Net(dev, cl.weight_set(sd, 'A'))
    judge = bl.Judge('%s | mfma/range | n=%d' % (dev, n))
    bw = bl.Backward(lib, dev, cl.Run(lib, dev, env, fr, mi), net, d_feat, 'range')
    bl.check_total(judge, net.sd, crop, d_feat, bw.call(), 'road/%d' % n)
    judge.done()


@pytest.mark.parametrize('n', [3, pytest.param(5, marks=slow)])
def test_backward_over_ranges_against_the_whole(emu, sd, monkeypatch, n):
    _range_case(emu, 'cpu', monkeypatch, sd, n)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [9])
def test_backward_over_ranges_against_the_whole_gpu(gpu, sd, monkeypatch, n):
    _range_case(gpu, DEV, monkeypatch, sd, n)


# The poses of the two-chunk case are chosen on the references alone.  Of the road poses of TWO_KEY taken one by one, those in
# TWO_DROP have a ReLU plateau within the forward's format error of zero: the float64 gradient of that crop jumps by 4e-5 .. 4.6e-2
# of max |g| under a 2^-19 nudge of the convolution weights (25, 55, 70, 83, 163, 204, 240), or the fp32 twin takes the other side
# and is 4e-3 / 3.6e-2 of max |g| off (213, 226) where the other crops are at 4e-5 .. 2.1e-4.  The first 257 of the rest are used, and
# test_backward_two_chunks_total_gpu asserts both figures for the set (cnn_bwd_layers.conditioning).
TWO_KEY = 'bwd/two'
TWO_DROP = (25, 55, 70, 83, 163, 204, 213, 226, 240)
# (the set: e32 / max |g| 2.9e-4 at conv1's bias, torch fp32's own sums over 4e6 terms, <= 2e-5 from conv2 on; jump 0)
E32REL_MAX, JUMPREL_MAX = 2.0 ** -11, 2.0 ** -16


def _two_inputs():
    n = 257
    fr, mi = cl.road_poses(n + len(TWO_DROP), TWO_KEY)
    keep = [i for i in range(n + len(TWO_DROP)) if i not in TWO_DROP]
    assert len(keep) == n
    fr, mi = fr[keep].contiguous(), mi[keep].contiguous()
    env = cl.road_env()
    return env, fr, mi, cl.oracle_crop(env, fr, mi), bl.d_feat_of(n, TWO_KEY)


def _two_chunks(gpu, sd, monkeypatch):
    env, fr, mi, crop, d_feat = _two_inputs()
    net = cl.Net(DEV, cl.weight_set(sd, 'A'))
    with cl.options(monkeypatch, **cl.FORM_ENV['recompute']):
        bw = bl.Backward(gpu, DEV, cl.Run(gpu, DEV, env, fr, mi), net, d_feat, 'recompute')
        flat = bw.call()
        snap = bw.snapshot(256, 1)
        hooks = bw.hooks(1)
    return net, crop, d_feat, flat, snap, hooks


@pytest.mark.gpu
def test_backward_two_chunks_last_chunk_gpu(gpu, sd, monkeypatch):
    """257 samples: a chunk of 256 and one of a single sample, whose G rows, moments and sums the arena (carved for 256) still
    holds: every step of that sample"""
    net, crop, d_feat, flat, snap, hooks = _two_chunks(gpu, sd, monkeypatch)
    judge = bl.Judge('%s | mfma/recompute | two chunks | n=257' % DEV)
    bl.check_chunk(judge, net, crop[256:], d_feat[256:], snap, None, 'mfma', hooks)
    judge.done()


@pytest.mark.gpu
def test_backward_two_chunks_total_gpu(gpu, sd, monkeypatch):
    """The flat gradient of all 257 samples against float64 autograd of the whole network within K_E2E times the end-to-end fp32
    error; first the inputs: neither the fp32 twin nor the float64 gradient under a 2^-19 nudge may sit on the other side of a
    ReLU plateau (both relative to max |g64| per block), or the comparison would be empty or measure the plateau."""
    net, crop, d_feat, flat, snap, hooks = _two_chunks(gpu, sd, monkeypatch)
    judge = bl.Judge('%s | mfma/recompute | two chunks | n=257' % DEV)
    bl.check_total(judge, net.sd, crop, d_feat, flat, 'road/257')
    e32rel, jumprel = bl.conditioning(net.sd, crop, d_feat, *bl._TOTAL['road/257'])
    print('cnn-bwd-conditioning | n=257 | %s | e32 / max |g| %.2e | jump / max |g| %.2e' % (TWO_KEY, e32rel, jumprel))
    assert e32rel <= E32REL_MAX and jumprel <= JUMPREL_MAX, 'these inputs are no usable end-to-end reference: %.2e, %.2e' % (e32rel, jumprel)
    judge.done()
