"""The small dense networks at their shape and magnitude edges: mlp_fwd_kernel / mlp_bwd_kernel, the scene interaction network
(gnn_node1 / gnn_edge / gnn_node2 and their backward kernels, wjobs_gemm_kernel) and the blocks of csrc/mlp_dev.h under them
(dense_mfma, dense_lds, ln_relu_rows, ln_relu_bwd_rows, wgrad_lds), black box through strive_mlp_fwd / strive_mlp_bwd /
strive_gnn_fwd / strive_gnn_bwd / strive_pack_dense / strive_pack_split_gather, against the float64 references of tests/dense_ref.py.

Every case runs through one body twice: on the host emulation (tests/hipemu, ``ops._lib_for`` patched, scratch and torch.empty
poisoned) and on the MI355X with the product's library (marked gpu).  The bound, its yardsticks (e32, e_fmt) and the factors K are
in dense_ref.py; every check prints a ``RATIO`` line (run with -s), the observed ratios are in profiles/r30_dense_ratios.md.
Decisions -- ReLU masks, arg-max winners -- are asserted ON THE REFERENCE before the device is looked at."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dense_ref as R
from util import poisoned_workspace, nan_empty, product_model
from strive_amd import _lib as L, params, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


_MODELS = {}


def model_sd(NC=2):
    if NC not in _MODELS:
        _MODELS[NC] = product_model(NC=NC)[1]
    return _MODELS[NC]


def on_both(*cases, slow=()):
    """parametrize (case, backend): every case on the emulation and, marked gpu, on the MI355X; ``slow`` = ids of the cases that
    take too long on the emulation for the default set (STRIVE_SLOW=1 runs them)"""
    ps = []
    for c in cases:
        cid = '-'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)
        marks = [pytest.mark.skipif(os.environ.get('STRIVE_SLOW') != '1', reason='STRIVE_SLOW=1 runs it')] if cid in slow else []
        ps.append(pytest.param(c, 'emu', id=cid + '-emu', marks=marks))
        ps.append(pytest.param(c, 'gpu', id=cid + '-gpu', marks=pytest.mark.gpu))
    return pytest.mark.parametrize('case,backend', ps)


class Backend(object):
    """library + device of one run, and the direct calls"""

    def __init__(self, backend, request, monkeypatch):
        from strive_amd import ops
        self.name, self.ops = backend, ops
        if backend == 'emu':
            self.lib = request.getfixturevalue('emu')
            self.dev = 'cpu'
            lib = self.lib
            monkeypatch.setattr(ops, '_lib_for', lambda *tensors: lib)
            monkeypatch.setattr(ops, '_ws_cache', {})
            monkeypatch.setattr(ops, '_workspace', poisoned_workspace(ops))
            monkeypatch.setattr(torch, 'empty', nan_empty())
        else:
            assert torch.cuda.is_available(), 'gpu cases need the MI355X'
            self.lib = L.get_lib()
            self.dev = 'cuda:0'

    def sync(self):
        if self.dev != 'cpu':
            torch.cuda.synchronize()

    def on_dev(self, sd):
        return {k: v.to(self.dev) for k, v in sd.items()}

    def pack_mlp(self, sd, prefix):
        """the device pack: strive_pack_dense on the weights where they are used"""
        return params.pack_mlp(self.on_dev(sd), prefix)

    def mlp_fwd(self, mp, x):
        rows, O = x.shape[0], mp.dims[-1]
        xd = x.to(self.dev).contiguous()
        y = torch.full((rows, O), float('nan'), device=self.dev)
        self.lib.call('strive_mlp_fwd', mp.ref(), L.ptr(xd), rows, L.ptr(y), L.stream_ptr(xd))
        self.sync()
        return y.cpu()

    def mlp_bwd(self, mp, x, dy, dp=None, want_dx=True):
        """-> (dx or None, d_params); ``dp``: a device buffer to accumulate into"""
        rows = x.shape[0]
        xd, dyd = x.to(self.dev).contiguous(), dy.to(self.dev).contiguous()
        n = self.lib.query('strive_mlp_param_count', mp.ref())
        if dp is None:
            dp = torch.zeros(n, device=self.dev)
        assert dp.numel() == n
        dx = torch.full(tuple(x.shape), float('nan'), device=self.dev) if want_dx else None
        self.lib.call('strive_mlp_bwd', mp.ref(), L.ptr(xd), L.ptr(dyd), rows, L.ptr(dx) if want_dx else None, L.ptr(dp), L.stream_ptr(xd))
        self.sync()
        return (dx.cpu() if want_dx else None), dp

    # ---- interaction network: x (N, NS, F), pos (N, NS, 4), sem (N, NC) ----
    def gnn_setup(self, sd, prefix, NC, ptr, NS):
        gp = params.pack_gnn(self.on_dev(sd), prefix, NC)
        sc = params.pack_scenes(torch.tensor(ptr, dtype=torch.long), NS, self.dev)
        return gp, sc

    def gnn_fwd(self, gp, sc, x, pos, sem):
        N, NS, _ = x.shape
        O = gp.struct.mlp_out.dims[gp.struct.mlp_out.nlayers]
        xd, pd, sd_ = x.to(self.dev).contiguous(), pos.to(self.dev).contiguous(), sem.to(self.dev).contiguous()
        wsb = self.lib.query('strive_gnn_workspace_bytes', gp.ref(), sc.ref())
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=self.dev)
        out = torch.full((N, NS, O), float('nan'), device=self.dev)
        self.lib.call('strive_gnn_fwd', gp.ref(), sc.ref(), L.ptr(xd), L.ptr(pd), L.ptr(sd_), L.ptr(out), L.ptr(ws), wsb, L.stream_ptr(xd))
        self.sync()
        return out.cpu()

    def gnn_bwd(self, gp, sc, x, pos, sem, dy, dp=None):
        """workspace of exactly strive_gnn_bwd_workspace_bytes, every byte 0xFF before the call"""
        xd, pd, sd_ = x.to(self.dev).contiguous(), pos.to(self.dev).contiguous(), sem.to(self.dev).contiguous()
        dyd = dy.to(self.dev).contiguous()
        n = self.lib.query('strive_gnn_param_count', gp.ref())
        if dp is None:
            dp = torch.zeros(n, device=self.dev)
        wsb = self.lib.query('strive_gnn_bwd_workspace_bytes', gp.ref(), sc.ref())
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=self.dev)
        dx = torch.full(tuple(x.shape), float('nan'), device=self.dev)
        self.lib.call('strive_gnn_bwd', gp.ref(), sc.ref(), L.ptr(xd), L.ptr(pd), L.ptr(sd_), L.ptr(dyd), L.ptr(dx), L.ptr(dp), L.ptr(ws), wsb,
                      L.stream_ptr(xd))
        self.sync()
        return dx.cpu(), dp


def host_packed_mlp(sd, prefix, dev):
    """the host pack: transposes and fragment tables built on the CPU by the torch layout code (params.dense_fragments), then moved"""
    p = params.Packed(L.StriveMLP())
    s = p.struct
    dims = R.mlp_dims(sd, prefix)
    for k in range(len(dims) - 1):
        w = sd[prefix + '.net.%d.weight' % (3 * k)].float().contiguous()
        s.w[k] = p.hold(w.to(dev))
        s.b[k] = p.hold(sd[prefix + '.net.%d.bias' % (3 * k)].float().contiguous().to(dev))
        s.wt[k] = p.hold(w.t().contiguous().to(dev))
        if w.shape[0] >= 32 and w.shape[1] >= 32:
            sc = params._pow2_scale(float(w.abs().max()))
            s.wsc[k] = sc
            s.wf[k] = p.hold(params.dense_fragments(w, sc).to(dev))
            s.wbf[k] = p.hold(params.dense_fragments(w.t().contiguous(), sc).to(dev))
        if k < len(dims) - 2:
            s.ln_g[k] = p.hold(sd[prefix + '.net.%d.weight' % (3 * k + 1)].float().contiguous().to(dev))
            s.ln_b[k] = p.hold(sd[prefix + '.net.%d.bias' % (3 * k + 1)].float().contiguous().to(dev))
    s.nlayers = len(dims) - 1
    for i, d in enumerate(dims):
        s.dims[i] = d
    p.dims = dims
    return p


def uni(shape, key, lo=-1.0, hi=1.0):
    return synth.f32(synth.counter_uniform(shape, key, lo, hi))


def assert_relu_decided(run, what):
    n, tot = R.relu_ambiguous(run.pres)
    assert n == 0, '%s: precondition on the REFERENCE: %d of %d hidden pre-activations within 2^-18 of 0 (not a kernel failure: ' \
        'pick another key)' % (what, n, tot)


# ================================================================================================
# A. single MLPs: shapes
# ================================================================================================
# (rows, IN, OUT, Linear layers, form).  Rows 1 3 4 5 8 9 17: a last block of one valid row and exact multiples of the 4-row block.
# IN: 31 below the matrix-core threshold; 32, 33, 38, 63 with a K tail; 64, 194, 288 the last padded width that fits; 289 and 512
# fall back to dense_lds.  OUT: 2, 4, 31 dense_lds; 32, 40, 48 an odd tile count (two == false) and c < OUT inside a tile; 64, 128.
# The hidden width is 128 (the kernels' own), so IN varies layer 0 (and the OUT of its input gradient), OUT the last layer (and
# the K of its input gradient: 40 and 48 are K tails there, 2, 4 and 31 fall back).
SHAPES = [
    (1, 31, 64, 2, 'mfma'), (3, 31, 32, 3, 'mfma'),
    (4, 32, 64, 2, 'mfma'), (5, 32, 128, 3, 'mfma'),
    (3, 33, 48, 2, 'mfma'), (8, 33, 64, 3, 'mfma'),
    (5, 38, 2, 3, 'mfma'), (9, 38, 40, 2, 'mfma'),
    (1, 63, 64, 2, 'mfma'), (17, 63, 32, L.MAXL, 'mfma'),
    (4, 64, 64, 3, 'mfma'), (9, 64, 2, 2, 'mfma'), (8, 64, 31, 2, 'mfma'),
    (3, 194, 128, 3, 'mfma'), (5, 194, 4, 2, 'mfma'),
    (8, 288, 64, 2, 'mfma'), (1, 288, 31, 3, 'mfma'),
    (5, 289, 64, 2, 'mfma'), (4, 289, 48, 3, 'mfma'),
    (3, 512, 64, 3, 'mfma'), (17, 512, 40, 2, 'mfma'),
    (1, 32, 4, L.MAXL, 'mfma'),
    (5, 38, 64, 3, 'valu'), (9, 33, 40, 2, 'valu'), (4, 288, 48, L.MAXL, 'valu'), (17, 194, 128, 3, 'valu'),
]


def mlp_case_body(be, monkeypatch, tag, sd, prefix, x, dy, form):
    valu = form == 'valu'
    if valu:
        monkeypatch.setenv('STRIVE_DENSE_VALU', '1')
    r64, r32, rcut = R.mlp_refs(sd, prefix, x, dy, valu)
    assert_relu_decided(r64, tag)
    cut = (lambda f: f(rcut)) if rcut is not None else (lambda f: None)
    mp = be.pack_mlp(sd, prefix)
    y = be.mlp_fwd(mp, x)
    R.check(tag, be.name, 'y', y, r64.y, r32.y, cut(lambda r: r.y))
    dx, dp = be.mlp_bwd(mp, x, dy)
    R.check(tag, be.name, 'dx', dx, r64.dx, r32.dx, cut(lambda r: r.dx))
    for k, blk in R.flat_blocks(sd, prefix, dp.cpu()).items():
        R.check(tag, be.name, 'd ' + k[len(prefix) + 1:], blk, r64.dp[k], r32.dp[k], cut(lambda r: r.dp[k]))
    # d_params accumulates; dx == nullptr is accepted
    _, dp2 = be.mlp_bwd(mp, x, dy, dp=dp, want_dx=False)
    for k, blk in R.flat_blocks(sd, prefix, dp2.cpu()).items():
        R.check(tag, be.name, '2x d ' + k[len(prefix) + 1:], blk, r64.dp[k], r32.dp[k], cut(lambda r: r.dp[k]), times=2.0)
    return mp, r64


@on_both(*SHAPES)
def test_a_mlp_shapes_against_float64(case, backend, request, monkeypatch):
    """forward, dx and every block of the flat gradient (W_l, b_l, gamma_l, beta_l) of a synthetic MLP; a second call without dx
    doubles d_params"""
    rows, IN, OUT, nl, form = case
    be = Backend(backend, request, monkeypatch)
    key = '%s/%d_%d_%d_%d' % (R.MLP_KEY, rows, IN, OUT, nl)
    dims = [IN] + [128] * (nl - 1) + [OUT]
    sd = R.make_mlp_sd('edge_case', dims, key)
    x, dy = uni((rows, IN), key + '/x'), uni((rows, OUT), key + '/dy')
    mlp_case_body(be, monkeypatch, 'A %s' % (case,), sd, 'edge_case', x, dy, form)


PRODUCT_MLPS = R.mlp_prefixes(model_sd())


@on_both(*PRODUCT_MLPS)
def test_a_every_mlp_of_the_product_model(case, backend, request, monkeypatch):
    """every MLP of product_model()'s state dict, enumerated from its keys, on 5 rows (a last block of one row)"""
    sd = model_sd()
    be = Backend(backend, request, monkeypatch)
    dims = R.mlp_dims(sd, case)
    key = '%s/p/%s' % (R.MLP_KEY, case)
    x, dy = uni((5, dims[0]), key + '/x'), uni((5, dims[-1]), key + '/dy')
    mlp_case_body(be, monkeypatch, 'A %s' % case, {k: v for k, v in sd.items() if k.startswith(case + '.')}, case, x, dy, 'mfma')


def test_a_product_model_mlps_are_all_listed():
    assert len(PRODUCT_MLPS) == 14 and 'past_encoder' in PRODUCT_MLPS and 'decoder_net.msg.0.edge_mlp' in PRODUCT_MLPS


@on_both((38, 40, 3), (194, 64, 2))
def test_a_padded_rows_add_nothing(case, backend, request, monkeypatch):
    """rows = 5 in one call against rows = 4 plus rows = 1 in two calls that accumulate: the three padded rows of the last block
    (whose forward activations are non-zero because of the bias) add nothing to weight, bias or LayerNorm gradients; dy = 0 gives
    exactly zero gradients"""
    IN, OUT, nl = case
    be = Backend(backend, request, monkeypatch)
    key = '%s/pad/%d_%d_%d' % (R.MLP_KEY, IN, OUT, nl)
    sd = R.make_mlp_sd('edge_case', [IN] + [128] * (nl - 1) + [OUT], key)
    x, dy = uni((5, IN), key + '/x'), uni((5, OUT), key + '/dy')
    r64, r32, rcut = R.mlp_refs(sd, 'edge_case', x, dy)
    assert_relu_decided(r64, str(case))
    mp = be.pack_mlp(sd, 'edge_case')
    dx5, dp5 = be.mlp_bwd(mp, x, dy)
    dx4, dp41 = be.mlp_bwd(mp, x[:4], dy[:4])
    dx1, dp41 = be.mlp_bwd(mp, x[4:], dy[4:], dp=dp41)
    assert torch.equal(torch.cat([dx4, dx1]), dx5), 'dx of a row depends on the rows of its block'
    tag = 'A pad %s' % (case,)
    b5, b41 = R.flat_blocks(sd, 'edge_case', dp5.cpu()), R.flat_blocks(sd, 'edge_case', dp41.cpu())
    for k in b5:
        R.check(tag, be.name, '5 rows d ' + k[10:], b5[k], r64.dp[k], r32.dp[k], rcut.dp[k])
        R.check(tag, be.name, '4+1 rows d ' + k[10:], b41[k], r64.dp[k], r32.dp[k], rcut.dp[k])
    dx0, dp0 = be.mlp_bwd(mp, x, torch.zeros_like(dy))
    assert float(dx0.abs().max()) == 0.0 and float(dp0.abs().max()) == 0.0, 'dy = 0 must give exactly zero gradients'


# ================================================================================================
# B. single MLPs: magnitudes (the per-row scale of dense_mfma)
# ================================================================================================
MAG_DIMS = {'k64': [64, 128, 64], 'k38': [38, 128, 128, 40]}


def mag_inputs(name, which):
    dims = MAG_DIMS[which]
    key = '%s/mag/%s/%s' % (R.MLP_KEY, name, which)
    sd = R.make_mlp_sd('edge_case', dims, key)
    x, dy = uni((6, dims[0]), key + '/x'), uni((6, dims[-1]), key + '/dy')
    return dims, key, sd, x, dy


@on_both(*[(n, w) for n in ('zero_row', 'denormal_row', 'rows_1e-9_1e+3', 'one_1e4_among_1e-3') for w in ('k64', 'k38')])
def test_b_row_magnitudes_against_float64(case, backend, request, monkeypatch):
    """held to the bound, each row against its OWN largest reference entry where rows differ in magnitude (what dense_mfma's comment
    promises): a row of zeros, a row of denormals, rows scaled by 1e-9 and 1e+3 inside one 4-row block (x in the forward, dy in the
    backward), one entry of 1e4 among entries of 1e-3"""
    name, which = case
    be = Backend(backend, request, monkeypatch)
    dims, key, sd, x, dy = mag_inputs(name, which)
    if name == 'zero_row':
        x[1] = 0.0
        dy[2] = 0.0
    elif name == 'denormal_row':
        x[2] *= 1e-40
        dy[1] *= 1e-40
        assert float(x[2].abs().max()) < 2.0 ** -126 and float(x[2].abs().max()) > 0.0
    elif name == 'rows_1e-9_1e+3':
        x[0] *= 1e-9
        x[1] *= 1e+3
        dy[2] *= 1e-9
        dy[3] *= 1e+3
    else:
        x *= 1e-3
        x[1, 5] = 1e4
        dy *= 1e-3
        dy[2, 7] = 1e4
    r64, r32, rcut = R.mlp_refs(sd, 'edge_case', x, dy)
    assert_relu_decided(r64, str(case))
    mp = be.pack_mlp(sd, 'edge_case')
    tag = 'B %s %s' % case
    R.check(tag, be.name, 'y', be.mlp_fwd(mp, x), r64.y, r32.y, rcut.y, rowwise=True)
    dx, dp = be.mlp_bwd(mp, x, dy)
    R.check(tag, be.name, 'dx', dx, r64.dx, r32.dx, rcut.dx, rowwise=True)
    for k, blk in R.flat_blocks(sd, 'edge_case', dp.cpu()).items():
        R.check(tag, be.name, 'd ' + k[10:], blk, r64.dp[k], r32.dp[k], rcut.dp[k])
    if name == 'zero_row':
        assert float(dx[2].abs().max()) == 0.0, 'a row with dy = 0 has dx = 0'


@on_both('one_weight_2^20', 'zero_weights')
def test_b_weight_magnitudes_in_kind(case, backend, request, monkeypatch):
    """held in kind: finite outputs and gradients, the ratio to the bound printed and recorded but not asserted.  One entry of
    W_0 2^20 times the rest moves ``wsc`` so that the second piece of every other entry is a subnormal fp16; W_1 = 0 has
    wsc = 1 and its output is the bias exactly"""
    be = Backend(backend, request, monkeypatch)
    dims, key, sd, x, dy = mag_inputs(case, 'k38')
    if case == 'one_weight_2^20':
        sd['edge_case.net.0.weight'][3, 4] *= 2.0 ** 20
    else:
        sd['edge_case.net.3.weight'].zero_()
    r64, r32, rcut = R.mlp_refs(sd, 'edge_case', x, dy)
    mp = be.pack_mlp(sd, 'edge_case')
    y = be.mlp_fwd(mp, x)
    dx, dp = be.mlp_bwd(mp, x, dy)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dp).all())
    tag = 'B %s' % case
    R.check(tag, be.name, 'y (in kind)', y, r64.y, r32.y, rcut.y, K=float('inf'))
    R.check(tag, be.name, 'dx (in kind)', dx, r64.dx, r32.dx, rcut.dx, K=float('inf'))
    if case == 'zero_weights':
        assert float(dx.abs().max()) == 0.0, 'no gradient passes a zero matrix'
        blocks = R.flat_blocks(sd, 'edge_case', dp.cpu())
        assert float(blocks['edge_case.net.0.weight'].abs().max()) == 0.0


@on_both(('nan', 1), ('inf', 2), ('-inf', 0), ('3e38', 1), ('3.3e38', 3))
def test_b_row_isolation_inside_a_block(case, backend, request, monkeypatch):
    """NaN / inf in one entry of one row: that row's outputs are non-finite wherever the reference's are, and every other row
    equals, bit for bit, the same call with that row replaced by finite values.  Rows with a finite maximum of 3e38 or more take
    the sc = 1 branch and overflow fp16: only the other rows are asserted (what the kernel returns is in the ratios file)."""
    what, row = case
    be = Backend(backend, request, monkeypatch)
    dims, key, sd, x, dy = mag_inputs('iso', 'k64')
    bad = x.clone()
    if what in ('3e38', '3.3e38'):
        bad[row] = bad[row] / bad[row].abs().max() * float(what)
    else:
        bad[row, 9] = float(what)
    mp = be.pack_mlp(sd, 'edge_case')
    y_ok, y_bad = be.mlp_fwd(mp, x), be.mlp_fwd(mp, bad)
    dx_ok, dp_ok = be.mlp_bwd(mp, x, dy)
    dx_bad, dp_bad = be.mlp_bwd(mp, bad, dy)
    others = [r for r in range(x.shape[0]) if r != row]
    assert torch.equal(y_bad[others], y_ok[others]), 'y of the other rows changed'
    assert torch.equal(dx_bad[others], dx_ok[others]), 'dx of the other rows changed'
    if what in ('3e38', '3.3e38'):
        print('RETURNS %s | %s | row max %s: y finite %d of %d, NaN %d, inf %d; dx finite %d of %d' % (
            be.name, case, what, int(torch.isfinite(y_bad[row]).sum()), y_bad.shape[1], int(torch.isnan(y_bad[row]).sum()),
            int(torch.isinf(y_bad[row]).sum()), int(torch.isfinite(dx_bad[row]).sum()), dx_bad.shape[1]))
    else:
        ref = R.MlpRun(sd, 'edge_case', bad).y
        nonfinite = ~torch.isfinite(ref[row])
        assert bool(nonfinite.any())
        assert bool((~torch.isfinite(y_bad[row]))[nonfinite].all()), 'the row with %s must be non-finite where the reference is' % what


# ================================================================================================
# C. the two packs
# ================================================================================================

@pytest.mark.gpu
@pytest.mark.parametrize('case', [(5, 38, 40, 3), (9, 33, 48, 2), (4, 288, 64, 2), (17, 63, 32, L.MAXL), (3, 512, 31, 3), (1, 194, 48, 3)],
                         ids=lambda c: '-'.join(str(v) for v in c))
def test_c_device_pack_equals_host_pack(case, request, monkeypatch):
    """strive_pack_dense on the device against params.dense_fragments on the CPU, moved: byte-identical fragments, and forward and
    backward agree bit for bit across the two packs"""
    rows, IN, OUT, nl = case
    be = Backend('gpu', request, monkeypatch)
    key = '%s/pack/%d_%d_%d_%d' % (R.MLP_KEY, rows, IN, OUT, nl)
    dims = [IN] + [128] * (nl - 1) + [OUT]
    sd = R.make_mlp_sd('edge_case', dims, key)
    x, dy = uni((rows, IN), key + '/x'), uni((rows, OUT), key + '/dy')
    md, mh = be.pack_mlp(sd, 'edge_case'), host_packed_mlp(sd, 'edge_case', be.dev)
    n_frag = 0
    for l in range(nl):
        w = sd['edge_case.net.%d.weight' % (3 * l)]
        if w.shape[0] >= 32 and w.shape[1] >= 32:
            sc = params._pow2_scale(float(w.abs().max()))
            wd = w.to(be.dev).contiguous()
            M, K = w.shape
            wf = torch.empty((((M + 15) // 16) * ((K + 31) // 32) * 512,), dtype=torch.int32, device=be.dev)
            wbf = torch.empty((((K + 15) // 16) * ((M + 31) // 32) * 512,), dtype=torch.int32, device=be.dev)
            be.lib.call('strive_pack_dense', L.ptr(wd), M, K, sc, None, L.ptr(wf), L.ptr(wbf), L.stream_ptr(wd))
            be.sync()
            assert torch.equal(wf.cpu(), params.dense_fragments(w, sc).reshape(-1)), 'layer %d: forward fragments' % l
            assert torch.equal(wbf.cpu(), params.dense_fragments(w.t().contiguous(), sc).reshape(-1)), 'layer %d: backward fragments' % l
            assert md.struct.wsc[l] == mh.struct.wsc[l] == sc
            n_frag += 1
    assert n_frag >= 1
    assert torch.equal(be.mlp_fwd(md, x), be.mlp_fwd(mh, x)), 'forward differs between the packs'
    (dxd, dpd), (dxh, dph) = be.mlp_bwd(md, x, dy), be.mlp_bwd(mh, x, dy)
    assert torch.equal(dxd, dxh), 'dx differs between the packs'
    # the weight gradients are the same addends in both calls, one per row (LayerNorm) or per 4-row block, summed by atomics in
    # whatever order they arrive: bit for bit with one row, and otherwise within rows * 2^-24 of the sum of their magnitudes,
    # which the block's largest entry times rows bounds from above only loosely -- 2^-20 of it is asked here (rows <= 17)
    if rows == 1:
        assert torch.equal(dpd, dph), 'd_params differs between the packs'
    for k, blk in R.flat_blocks(sd, 'edge_case', dpd.cpu()).items():
        other = R.flat_blocks(sd, 'edge_case', dph.cpu())[k]
        assert float((blk - other).abs().max()) <= 2.0 ** -20 * float(blk.abs().max()), 'd %s differs between the packs' % k


PACK_MK = [(1, 1), (15, 17), (16, 32), (17, 15), (31, 33), (32, 16), (33, 130), (130, 31), (1, 130), (130, 1)]


def read_pieces(frag, M, K):
    """(p0, p1) float64 (MT*16, KS*32) from a fragment table [tile][k-step][piece][lane][8 x fp16]: lane l holds row 16 tile + (l & 15),
    k = 32 step + 8 (l >> 4) + j"""
    MT, KS = (M + 15) // 16, (K + 31) // 32
    h = frag.cpu().contiguous().view(torch.int16).view(torch.float16).reshape(MT, KS, 2, 4, 16, 8).to(torch.float64)
    full = h.permute(2, 0, 4, 1, 3, 5).reshape(2, MT * 16, KS * 32)
    return full[0], full[1]


def pack_input(M, K, key):
    """values on fp16 rounding ties (odd multiples of half an fp16 step after the scale), -0.0, an entry below 2^-40 of the maximum"""
    w = uni((M, K), key, -0.7, 0.7)
    f = w.reshape(-1)
    n = f.numel()
    if n > 1:
        f[1] = -0.0
    if n > 2:
        f[2] = float(f.abs().max()) * 2.0 ** -41
    sc = params._pow2_scale(float(f.abs().max()))
    for i, v in enumerate((1025.5, 2051.0, -1027.5, 1.5 * 2.0 ** -24, 4102.0)):   # ties of the 1-, 2- and 4-steps; a subnormal tie
        if n > 3 + i:
            f[3 + i] = v / sc
    return f.reshape(M, K).contiguous(), sc


@on_both(*PACK_MK)
def test_c_pack_dense_pieces_add_up(case, backend, request, monkeypatch):
    """the two pieces read back from both fragment tables and added in float64: where p0 is a normal fp16, |p0 + p1 - w scale| <=
    2^-22 |w scale|; elsewhere at most 2^-25 absolute (half the fp16 subnormal step); slots beyond (M, K) exactly zero; -0.0 keeps
    its sign in p0"""
    M, K = case
    be = Backend(backend, request, monkeypatch)
    w, sc = pack_input(M, K, 'dense/pack/%d_%d' % (M, K))
    wd = w.to(be.dev)
    wt = torch.full((K, M), float('nan'), device=be.dev)
    wf = torch.full((((M + 15) // 16) * ((K + 31) // 32) * 512,), -1, dtype=torch.int32, device=be.dev)
    wbf = torch.full((((K + 15) // 16) * ((M + 31) // 32) * 512,), -1, dtype=torch.int32, device=be.dev)
    be.lib.call('strive_pack_dense', L.ptr(wd), M, K, sc, L.ptr(wt), L.ptr(wf), L.ptr(wbf), L.stream_ptr(wd))
    be.sync()
    assert torch.equal(wt.cpu(), w.t().contiguous())
    for name, frag, a in (('wf', wf, w), ('wbf', wbf, w.t().contiguous())):
        m, k = a.shape
        p0, p1 = read_pieces(frag, m, k)
        pad = torch.ones_like(p0, dtype=torch.bool)
        pad[:m, :k] = False
        assert float(p0[pad].abs().max() if pad.any() else 0.0) == 0.0 and float(p1[pad].abs().max() if pad.any() else 0.0) == 0.0, \
            '%s: slots beyond (M, K) are not zero' % name
        v = a.double() * sc
        err = (p0[:m, :k] + p1[:m, :k] - v).abs()
        normal = p0[:m, :k].abs() >= 2.0 ** -14
        assert bool((err[normal] <= 2.0 ** -22 * v.abs()[normal]).all()), '%s: a normal entry is off by more than 2^-22 of itself' % name
        assert bool((err[~normal] <= 2.0 ** -25).all()), '%s: a small entry is off by more than 2^-25' % name
        # p0 is the nearest fp16, ties to even
        assert torch.equal(p0[:m, :k], v.float().to(torch.float16).double()), '%s: p0 is not fp16(w scale) to nearest even' % name
        if a.numel() > 1:
            assert bool(torch.signbit(p0[:m, :k].reshape(-1)[a.reshape(-1) == 0.0]).any()), '%s: -0.0 lost its sign' % name
    # the same split through the gather form, identity layout + the zero slot
    n = M * K
    idx = torch.cat([torch.arange(2 * n, dtype=torch.int32), torch.tensor([2 * n], dtype=torch.int32)]).to(be.dev)
    out = torch.full((2 * n + 1,), -1, dtype=torch.int16, device=be.dev)
    be.lib.call('strive_pack_split_gather', L.ptr(wd), n, L.ptr(idx), 2 * n + 1, float(sc), L.ptr(out), L.stream_ptr(wd))
    be.sync()
    g = out.cpu().view(torch.float16).double()
    p0, p1 = read_pieces(wf, M, K)
    assert torch.equal(g[:n].reshape(M, K), p0[:M, :K]) and torch.equal(g[n:2 * n].reshape(M, K), p1[:M, :K]) and float(g[2 * n]) == 0.0, \
        'strive_pack_split_gather and strive_pack_dense split differently'


# ================================================================================================
# D. the scene interaction network
# ================================================================================================
# name -> (state-dict prefix, NC of the model): the three nets of product_model() and a decoder net with five classes
NETS = {'decoder': ('decoder_net', 2), 'prior': ('prior_net', 2), 'posterior': ('posterior_net', 2), 'nc5': ('decoder_net', 5)}
# one ragged batch: source counts 1, 15, 0, 16, 17, 33 -- one, two and three chunks of RB_EDGE = 16 with a partial last one, a
# singleton (arg = -1, aggregate 0) between two others
RAGGED = [2, 16, 1, 17, 18, 34]
TWINS = [3, 5, 18]             # 26 rows: the last 4-row block of the node kernels holds two rows


class wgrad_form(object):
    """the two forms of the GNN weight gradient: deferred products (default) or STRIVE_WGRAD_ATOMICS=1; the library's options are
    re-synchronised after the variable changes, and again on the way out"""

    def __init__(self, lib, form):
        self.lib, self.form = lib, form

    def __enter__(self):
        self.saved = os.environ.get('STRIVE_WGRAD_ATOMICS')
        if self.form == 'atomics':
            os.environ['STRIVE_WGRAD_ATOMICS'] = '1'
        else:
            os.environ.pop('STRIVE_WGRAD_ATOMICS', None)
        self.lib.sync_options_from_env()
        assert self.lib.get_option('wgrad_atomics') == (1 if self.form == 'atomics' else 0)
        return self

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop('STRIVE_WGRAD_ATOMICS', None)
        else:
            os.environ['STRIVE_WGRAD_ATOMICS'] = self.saved
        self.lib.sync_options_from_env()
        return False


def gnn_inputs(net, sizes, NS, variant):
    prefix, NC = NETS[net]
    sd = model_sd(NC)
    fin = sd[prefix + '.mlp_in.net.0.weight'].shape[1]
    O = R.mlp_dims(sd, prefix + '.mlp_out')[-1]
    key = R.GNN_KEYS.get((net, NS, variant), 'dense/gnn/0') + '/%s/%d/%s' % (net, NS, variant)
    x, pos, sem, ptr = R.scene_inputs(sizes, NS, fin, NC, key)
    dy = uni((x.shape[0], NS, O), key + '/dy')
    return sd, prefix, NC, x, pos, sem, ptr, dy


def gnn_refs(sd, prefix, x, pos, sem, ptr, dy):
    return (R.GnnRef(sd, prefix, x, pos, sem, ptr, dy), R.GnnOracle32(sd, prefix, x, pos, sem, ptr, dy),
            R.GnnRef(sd, prefix, x, pos, sem, ptr, dy, cut=True))


def assert_gnn_decided(tag, r64, r32, rcut, ptr, want_positions=None):
    """on the reference alone: no ambiguous ReLU, every max that is not an exact tie beats its runner-up by more than the bound of
    the output, the wanted winner positions occur"""
    e = float((rcut.y - r64.y).abs().max() + (r32.y.double() - r64.y).abs().max())
    thr = R.K_GNN * max(e, R.FLOOR * float(r64.y.abs().max()))
    n_relu, n_close, missing = R.gnn_preconditions(r64, ptr, thr, want_positions)
    m = r64.margin[torch.isfinite(r64.margin) & (r64.margin > R.TIE_EPS)]
    print('MARGIN %s | smallest margin of a max %.3e | threshold %.3e | ambiguous ReLUs %d | close maxes %d | masked entries 0'
          % (tag, float(m.min()) if m.numel() else float('inf'), thr, n_relu, n_close))
    assert n_relu == 0 and n_close == 0 and not missing, \
        '%s: precondition on the REFERENCE: %d ambiguous ReLUs, %d maxes within %.3g of their runner-up, winner positions missing: %s ' \
        '(not a kernel failure: pick another key)' % (tag, n_relu, n_close, thr, missing)


def check_gnn(tag, be, sd, prefix, got_y, got_dx, got_dp, r64, r32, rcut, times=1.0, rows=None):
    if got_y is not None:
        R.check(tag, be.name, 'y', got_y, r64.y, r32.y, rcut.y, K=R.K_GNN)
    if got_dx is not None:
        R.check(tag, be.name, 'dx', got_dx, r64.dx, r32.dx, rcut.dx, K=R.K_GNN)
    if got_dp is not None:
        f64, f32, fc = R.gnn_flat64(sd, prefix, r64), R.gnn_flat64(sd, prefix, r32), R.gnn_flat64(sd, prefix, rcut)
        off = 0
        for k, blk in R.gnn_blocks(sd, prefix, got_dp.cpu()):
            n = blk.numel()
            R.check(tag, be.name, ('%gx ' % times if times != 1.0 else '') + 'd ' + k[len(prefix) + 1:], blk, f64[off:off + n], f32[off:off + n],
                    fc[off:off + n], K=R.K_GNN, times=times)
            off += n


GNN_RAGGED = [('decoder', 1, 'deferred'), ('decoder', 2, 'atomics'), ('prior', 1, 'atomics'), ('posterior', 1, 'deferred'),
              ('nc5', 1, 'deferred'), ('nc5', 2, 'atomics')]


@on_both(*GNN_RAGGED)
def test_d_gnn_ragged_batch_against_float64(case, backend, request, monkeypatch):
    """forward, dx and every block of the flat gradient on the ragged batch, with a workspace of exactly the queried size full of
    0xFF bytes; d_params accumulates over two calls.  The reference's record must show, for the first and for the last agent of the
    34-agent scene (the self-skip `jl >= a - lo` on both sides), winners at the first source, the last source of the first chunk,
    the first of the second chunk and the last source overall."""
    net, NS, form = case
    be = Backend(backend, request, monkeypatch)
    sd, prefix, NC, x, pos, sem, ptr, dy = gnn_inputs(net, RAGGED, NS, 'ragged')
    r64, r32, rcut = gnn_refs(sd, prefix, x, pos, sem, ptr, dy)
    tag = 'D ragged %s NS=%d %s' % case
    assert_gnn_decided(tag, r64, r32, rcut, ptr, {ptr[-2]: (0, 15, 16, 32), ptr[-1] - 1: (0, 15, 16, 32)})
    assert int(r64.win[ptr[2]].max()) == -1 and float(r64.aggr[ptr[2]].abs().max()) == 0.0, 'the singleton scene has no source'
    gp, sc = be.gnn_setup(sd, prefix, NC, ptr, NS)
    check_gnn(tag, be, sd, prefix, be.gnn_fwd(gp, sc, x, pos, sem), None, None, r64, r32, rcut)
    with wgrad_form(be.lib, form):
        dx, dp = be.gnn_bwd(gp, sc, x, pos, sem, dy)
        check_gnn(tag, be, sd, prefix, None, dx, dp, r64, r32, rcut)
        _, dp = be.gnn_bwd(gp, sc, x, pos, sem, dy, dp=dp)
        check_gnn(tag, be, sd, prefix, None, None, dp, r64, r32, rcut, times=2.0)


@on_both(('decoder', 1, 'deferred'), ('posterior', 2, 'atomics'))
def test_d_gnn_exact_ties(case, backend, request, monkeypatch):
    """two agents identical in features, pose and class (in the 18-agent scene the first source chunk holds one, the second the
    other): their messages tie exactly.  The forward is held to the bound; in the backward the gradients summed over the twins
    are, and so is every entry of dx: the first of equal sources takes the gradient (`arg < 0 || v > best`)."""
    net, NS, form = case
    be = Backend(backend, request, monkeypatch)
    sd, prefix, NC, x, pos, sem, ptr, dy = gnn_inputs(net, TWINS, NS, 'twins')
    pairs = [(ptr[0], ptr[0] + 2), (ptr[2] + 1, ptr[3] - 1)]
    for a, b in pairs:
        x[b], pos[b], sem[b] = x[a], pos[a], sem[a]
    r64, r32, rcut = gnn_refs(sd, prefix, x, pos, sem, ptr, dy)
    tag = 'D twins %s NS=%d %s' % case
    assert_gnn_decided(tag, r64, r32, rcut, ptr)
    assert int((r64.margin <= R.TIE_EPS).sum()) > 0, 'no max of the reference is an exact tie'
    gp, sc = be.gnn_setup(sd, prefix, NC, ptr, NS)
    check_gnn(tag, be, sd, prefix, be.gnn_fwd(gp, sc, x, pos, sem), None, None, r64, r32, rcut)
    with wgrad_form(be.lib, form):
        dx, dp = be.gnn_bwd(gp, sc, x, pos, sem, dy)

    def twin_sums(t):
        t = t.clone()
        for a, b in pairs:
            t[a] = t[a] + t[b]
            t[b] = 0.0
        return t
    R.check(tag, be.name, 'dx summed over twins', twin_sums(dx), twin_sums(r64.dx), twin_sums(r32.dx), twin_sums(rcut.dx), K=R.K_GNN)
    # entry by entry: the oracle (scatter amax) splits a tie's gradient evenly between the twins, the kernel hands it to the first,
    # so the fp32 yardstick of the twins' rows is the oracle's error on their SUM, laid on the first twin's row
    o32 = r32.dx.double().clone()
    for a, b in pairs:
        o32[a], o32[b] = o32[a] + o32[b] - r64.dx[b], r64.dx[b]
    R.check(tag, be.name, 'dx', dx, r64.dx, o32, rcut.dx, K=R.K_GNN)
    check_gnn(tag, be, sd, prefix, None, None, dp, r64, r32, rcut)


@on_both(('prior', 'x'), ('decoder', 'all'))
def test_d_gnn_nan_pose(case, backend, request, monkeypatch):
    """NaN in one agent's pose, in x only and in all four components: the output is held against the reference with rel = 0 for
    the NaN components (the agent as a target and as a source), dx is finite everywhere"""
    net, comps = case
    be = Backend(backend, request, monkeypatch)
    sd, prefix, NC, x, pos, sem, ptr, dy = gnn_inputs(net, TWINS, 1, 'nan_' + comps)
    a = ptr[2] + 3
    if comps == 'x':
        pos[a, :, 0] = float('nan')
    else:
        pos[a] = float('nan')
    r64, r32, rcut = gnn_refs(sd, prefix, x, pos, sem, ptr, dy)
    tag = 'D nan %s %s' % case
    assert_gnn_decided(tag, r64, r32, rcut, ptr)
    assert bool(torch.isfinite(r64.y).all())
    gp, sc = be.gnn_setup(sd, prefix, NC, ptr, 1)
    y = be.gnn_fwd(gp, sc, x, pos, sem)
    dx, dp = be.gnn_bwd(gp, sc, x, pos, sem, dy)
    assert bool(torch.isfinite(dx).all()), 'dx is not finite'
    check_gnn(tag, be, sd, prefix, y, dx, dp, r64, r32, rcut)


@on_both(('decoder', 1), ('prior', 2))
def test_d_gnn_scene_alone_and_in_a_batch(case, backend, request, monkeypatch):
    """a 7-agent scene alone against the same scene as the third of five: outputs and dx byte for byte; the weight gradients of
    both calls by the bound (they sum over the batch)"""
    net, NS = case
    be = Backend(backend, request, monkeypatch)
    sizes = [4, 9, 7, 1, 6]
    sd, prefix, NC, x, pos, sem, ptr, dy = gnn_inputs(net, sizes, NS, 'third')
    lo, hi = ptr[2], ptr[3]
    r64, r32, rcut = gnn_refs(sd, prefix, x, pos, sem, ptr, dy)
    tag = 'D third %s NS=%d' % case
    assert_gnn_decided(tag, r64, r32, rcut, ptr)
    gp, sc = be.gnn_setup(sd, prefix, NC, ptr, NS)
    y = be.gnn_fwd(gp, sc, x, pos, sem)
    dx, dp = be.gnn_bwd(gp, sc, x, pos, sem, dy)
    check_gnn(tag, be, sd, prefix, y, dx, dp, r64, r32, rcut)
    xa, pa, sa, da = x[lo:hi].contiguous(), pos[lo:hi].contiguous(), sem[lo:hi].contiguous(), dy[lo:hi].contiguous()
    gp1, sc1 = be.gnn_setup(sd, prefix, NC, [0, hi - lo], NS)
    y1 = be.gnn_fwd(gp1, sc1, xa, pa, sa)
    dx1, dp1 = be.gnn_bwd(gp1, sc1, xa, pa, sa, da)
    assert torch.equal(y1, y[lo:hi]), 'the output of a scene depends on the batch around it'
    assert torch.equal(dx1, dx[lo:hi]), 'dx of a scene depends on the batch around it'
    a64, a32, acut = gnn_refs(sd, prefix, xa, pa, sa, [0, hi - lo], da)
    check_gnn(tag + ' alone', be, sd, prefix, None, None, dp1, a64, a32, acut)
