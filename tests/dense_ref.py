"""Helpers of tests/test_dense_edges.py (a plain module like loss_ref.py and cnn_bwd_layers.py): float64 references of the small
dense networks (MLP, scene interaction network), the input recipes, and the bound -- built from references only:

    |kernel - float64|  <=  K * max(e_fmt + e32, 2^-23 * max|float64|)          per checked tensor, entry-wise maximum

e32   = max |oracle fp32 - float64|: oracle/model.py (``mlp`` / ``interaction_net``) in torch fp32 on the CPU, same inputs.
e_fmt = max |float64 network whose matrix-core products are evaluated on CUT operands - float64 network|.  The cut operands restate
        the comment of dense_mfma (csrc/mlp_dev.h): every activation row times the power of two that brings its largest magnitude
        into [2^14, 2^15), the weights times ``wsc`` (params._pow2_scale), p0 = fp16(v) to nearest even, p1 = fp16(v - p0), and the
        three products p0 q0 + p0 q1 + p1 q0.  A layer is cut exactly where dense_mfma_ok sends it to the matrix cores (``mfma_ok``);
        e_fmt is 0 for the layers that run in dense_lds and for every case packed under STRIVE_DENSE_VALU=1.
K     = twice the worst measured ratio err / max(e_fmt + e32, floor) over every check of every case on the host emulation and on the
        MI355X, rounded up to a power of two (profiles/r30_dense_ratios.md): K_MLP for single MLPs, K_GNN for the interaction network
        end to end.  The yardstick is the reference pair, never the kernel.

Decisions are made on the reference before a device is looked at: ``relu_ambiguous`` counts hidden pre-activations within 2^-18 of 0
(a backward case needs none), ``GnnRef`` records winner, runner-up and margin of every max.  The keys below name the counter streams
(synth.counter_uniform) for which the reference meets those preconditions."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from strive_amd import _lib as L, params, synth
from oracle import model as om

T64 = torch.float64
FLOOR = 2.0 ** -23
RELU_MARGIN = 2.0 ** -18
TIE_EPS = 2.0 ** -40       # two float64 messages this close are a tie (rounding noise of the reference is 2^-50 of a message)
AMBIG_CAP = 1e-3           # at most this share of a tensor's entries may be ambiguous ON THE REFERENCE (the case fails otherwise)

K_MLP = 8.0
K_GNN = 16.0

# counter keys of the backward cases: chosen on the CPU so that no ReLU is ambiguous and (GNN) every max of a scene not built as a
# tie beats its runner-up by more than K_GNN times the bound of the output (tests assert both on the reference)
MLP_KEY = 'dense/mlp/0'
# (net, NS, variant) -> key; 'dense/gnn/0' where not listed.  Found by walking dense/gnn/0, 1, 2, ... with 1.5 times the threshold the
# tests use (the float64 reference rounds differently from one host to the next); one key in a hundred or fewer meets all three
# conditions on the ragged batch (half a million ReLUs, 5 000 to 11 000 maxes);
# none of the first 2 000 does for the posterior net with two samples (a million ReLUs, 22 000 maxes), so that net runs with one
GNN_KEYS = {('decoder', 1, 'ragged'): 'dense/gnn/83', ('decoder', 2, 'ragged'): 'dense/gnn/186', ('prior', 1, 'ragged'): 'dense/gnn/706',
            ('posterior', 1, 'ragged'): 'dense/gnn/178', ('nc5', 1, 'ragged'): 'dense/gnn/55', ('nc5', 2, 'ragged'): 'dense/gnn/162',
            ('prior', 1, 'nan_x'): 'dense/gnn/10', ('prior', 2, 'third'): 'dense/gnn/1'}

RATIOS = []                # (case, backend, what, err, e_fmt, e32, floor, ratio)


# ================================================================================================
# the cut operands of dense_mfma
# ================================================================================================

def mfma_ok(IN, OUT, RB=4):
    """dense_mfma_ok of csrc/mlp_dev.h for a layer that has fragments (params._fill_mlp builds them under the same size rule)"""
    return IN >= 32 and OUT >= 32 and ((IN + 31) & ~31) <= (288 if RB <= 4 else 128)


def row_scale(x):
    """(R, K) float64 -> (R, 1) power of two that brings each row's largest magnitude into [2^14, 2^15); 1 for a zero row and for
    3e38 and beyond; the exponent stays an fp32 one (a denormal row is scaled by 2^127 only)"""
    mx = x.abs().amax(dim=1, keepdim=True)
    ok = (mx > 0) & (mx < 3.0e38)
    _, ex = torch.frexp(torch.where(ok, mx, torch.ones_like(mx)))         # mx = m 2^ex, m in [0.5, 1): floor(log2 mx) = ex - 1
    e = (14 - (ex - 1)).clamp(-126, 127).to(T64)
    return torch.where(ok, torch.pow(torch.full_like(e, 2.0), e), torch.ones_like(e))


def split16(v):
    """two fp16 pieces of a float64 tensor, as float64"""
    p0 = v.to(torch.float16).to(T64)
    p1 = (v - p0).to(torch.float16).to(T64)
    return p0, p1


def cut_matmul(x, w):
    """x (R, K) @ w (O, K)^T on the cut operands"""
    sc = row_scale(x)
    wsc = params._pow2_scale(float(w.abs().max()))
    x0, x1 = split16(x * sc)
    w0, w1 = split16(w * wsc)
    return (x0 @ w0.t() + x0 @ w1.t() + x1 @ w0.t()) / (sc * wsc)


class _Linear(torch.autograd.Function):
    """y = x W^T + b in float64 with the forward product and / or the input-gradient product on cut operands (the weight and
    bias gradients are fp32 vector work in the kernels: never cut)"""

    @staticmethod
    def forward(ctx, x, w, b, cut_f, cut_b):
        ctx.save_for_backward(x, w)
        ctx.cut_b = cut_b
        y = cut_matmul(x, w) if cut_f else x @ w.t()
        return y + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx = cut_matmul(g, w.t().contiguous()) if ctx.cut_b else g @ w
        return dx, g.t() @ x, g.sum(0), None, None


def rule_rows4(l, IN, OUT):
    """which products of layer l of an MLP run by 4-row workgroups (mlp_fwd / mlp_bwd, the node kernels) go to the matrix cores:
    (forward, input gradient -- the same layer with IN and OUT exchanged)"""
    return mfma_ok(IN, OUT, 4), mfma_ok(OUT, IN, 4)


def rule_edge(l, IN, OUT):
    """the edge MLP: 16 source rows per workgroup; layer 0 is factorised into per-node partials on the vector ALUs"""
    return (False, False) if l == 0 else (mfma_ok(IN, OUT, 16), mfma_ok(OUT, IN, 16))


def rule_none(l, IN, OUT):
    return False, False


# ================================================================================================
# MLP
# ================================================================================================

def mlp_keys(sd, prefix):
    """parameter names in named_parameters() order: W_l, b_l and, for hidden layers, gamma_l, beta_l"""
    ks, k = [], 0
    while (prefix + '.net.%d.weight' % (3 * k)) in sd:
        ks += [prefix + '.net.%d.weight' % (3 * k), prefix + '.net.%d.bias' % (3 * k)]
        if (prefix + '.net.%d.weight' % (3 * k + 1)) in sd:
            ks += [prefix + '.net.%d.weight' % (3 * k + 1), prefix + '.net.%d.bias' % (3 * k + 1)]
        k += 1
    return ks


def mlp_prefixes(sd):
    """every MLP of a state dict, from its keys"""
    return sorted({k[:-len('.net.0.weight')] for k in sd if k.endswith('.net.0.weight')})


def mlp_dims(sd, prefix):
    d, k = [], 0
    while (prefix + '.net.%d.weight' % (3 * k)) in sd:
        w = sd[prefix + '.net.%d.weight' % (3 * k)]
        d += ([w.shape[1]] if k == 0 else []) + [w.shape[0]]
        k += 1
    return d


def mlp_ref64(sd, prefix, x, rule=rule_none, pres=None):
    """Linear -> (LayerNorm(eps 1e-5, biased variance) -> ReLU -> Linear)*, in the dtype of ``sd`` / ``x`` (float64); products cut
    where ``rule`` says so.  ``pres``: list that receives the post-LayerNorm pre-activations of the hidden layers."""
    lead = x.shape[:-1]
    h = x.reshape(-1, x.shape[-1])
    k = 0
    while (prefix + '.net.%d.weight' % (3 * k)) in sd:
        w, b = sd[prefix + '.net.%d.weight' % (3 * k)], sd[prefix + '.net.%d.bias' % (3 * k)]
        if k > 0:
            g, be = sd[prefix + '.net.%d.weight' % (3 * k - 2)], sd[prefix + '.net.%d.bias' % (3 * k - 2)]
            pre = F.layer_norm(h, (g.shape[0],), g, be, 1e-5)
            if pres is not None:
                pres.append(pre)
            h = F.relu(pre)
        cf, cb = rule(k, w.shape[1], w.shape[0])
        h = _Linear.apply(h, w, b, cf, cb)
        k += 1
    return h.reshape(lead + (h.shape[-1],))


def make_mlp_sd(prefix, dims, key):
    """synthetic MLP under a made-up prefix: Linear U(+-1/sqrt(fan_in)), LayerNorm weight 1 +- 0.1, bias +- 0.05 (fp32)"""
    sd = {}
    for l in range(len(dims) - 1):
        IN, OUT = dims[l], dims[l + 1]
        a = 1.0 / math.sqrt(IN)
        sd[prefix + '.net.%d.weight' % (3 * l)] = synth.f32(synth.counter_uniform((OUT, IN), '%s/w%d' % (key, l), -a, a))
        sd[prefix + '.net.%d.bias' % (3 * l)] = synth.f32(synth.counter_uniform((OUT,), '%s/b%d' % (key, l), -a, a))
        if l < len(dims) - 2:
            sd[prefix + '.net.%d.weight' % (3 * l + 1)] = synth.f32(1.0 + 0.1 * synth.counter_uniform((OUT,), '%s/g%d' % (key, l), -1.0, 1.0))
            sd[prefix + '.net.%d.bias' % (3 * l + 1)] = synth.f32(0.05 * synth.counter_uniform((OUT,), '%s/e%d' % (key, l), -1.0, 1.0))
    return sd


def to64(sd, grad=False):
    return {k: v.detach().to(T64).clone().requires_grad_(grad) for k, v in sd.items()}


def to32(sd, grad=False):
    return {k: v.detach().to(torch.float32).clone().requires_grad_(grad) for k, v in sd.items()}


def relu_ambiguous(pres, margin=RELU_MARGIN):
    """(ambiguous, total) entries of the hidden pre-activations within ``margin`` of 0"""
    n = sum(int((p.detach().abs() < margin).sum()) for p in pres)
    return n, sum(p.numel() for p in pres)


class MlpRun(object):
    """one evaluation of an MLP with gradients: y, dx, {parameter name: gradient}, hidden pre-activations"""

    def __init__(self, sd, prefix, x, dy=None, rule=rule_none, dtype=T64, oracle=False):
        sdg = {k: v.detach().to(dtype).clone().requires_grad_(dy is not None) for k, v in sd.items() if k.startswith(prefix + '.')}
        xg = x.detach().to(dtype).clone().requires_grad_(dy is not None)
        self.pres = []
        y = om.mlp(sdg, prefix, xg) if oracle else mlp_ref64(sdg, prefix, xg, rule, self.pres)
        self.y = y.detach()
        self.dx, self.dp = None, {}
        if dy is not None:
            (y * dy.to(dtype)).sum().backward()
            self.dx = xg.grad.detach()
            self.dp = {k: (sdg[k].grad if sdg[k].grad is not None else torch.zeros_like(sdg[k])).detach() for k in mlp_keys(sd, prefix)}


def mlp_refs(sd, prefix, x, dy=None, valu=False):
    """(float64, oracle fp32, float64 on cut operands or None) runs of one MLP case"""
    r64 = MlpRun(sd, prefix, x, dy)
    r32 = MlpRun(sd, prefix, x, dy, dtype=torch.float32, oracle=True)
    dims = mlp_dims(sd, prefix)
    any_cut = not valu and any(any(rule_rows4(l, dims[l], dims[l + 1])) for l in range(len(dims) - 1))
    rcut = MlpRun(sd, prefix, x, dy, rule=rule_rows4) if any_cut else None
    return r64, r32, rcut


def flat_blocks(sd, prefix, flat):
    """{parameter name: block} of a flat gradient buffer in named_parameters() order"""
    out, off = {}, 0
    for k in mlp_keys(sd, prefix):
        n = sd[k].numel()
        out[k] = flat[off:off + n].reshape(sd[k].shape)
        off += n
    assert off == flat.numel(), 'flat gradient holds %d entries, the parameters %d' % (flat.numel(), off)
    return out


# ================================================================================================
# the bound
# ================================================================================================

def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def check(case, backend, what, got, r64, r32, rcut=None, K=K_MLP, rowwise=False, times=1.0, mask=None):
    """assert |got - times r64| <= K max(e_fmt + e32, 2^-23 max|r64|) (times: d_params after `times` accumulating calls -- the
    yardstick scales with it); print and record err / (e_fmt + e32).  rowwise: every row against its own bound.  mask: entries
    left out (the caller has counted them against AMBIG_CAP)."""
    g, a, b = _np(got), _np(r64) * times, _np(r32) * times
    c = _np(rcut) * times if rcut is not None else None
    assert g.shape == a.shape, '%s %s: got %s, reference %s' % (case, what, g.shape, a.shape)
    if mask is not None:
        keep = ~_np(mask).astype(bool)
        g, a, b = g[keep], a[keep], b[keep]
        c = c[keep] if c is not None else None
    if g.size == 0:
        return 0.0
    assert np.all(np.isfinite(g)), '%s %s [%s]: non-finite values from the kernel' % (case, what, backend)
    if rowwise:
        rows = [(g[i:i + 1], a[i:i + 1], b[i:i + 1], None if c is None else c[i:i + 1], '%s[row %d]' % (what, i)) for i in range(g.shape[0])]
    else:
        rows = [(g, a, b, c, what)]
    worst = 0.0
    for gg, aa, bb, cc, w in rows:
        e32 = float(np.max(np.abs(bb - aa)))
        e_fmt = float(np.max(np.abs(cc - aa))) if cc is not None else 0.0
        floor = FLOOR * float(np.max(np.abs(aa)))
        err = float(np.max(np.abs(gg - aa)))
        bound = max(e_fmt + e32, floor)
        raw = err / (e_fmt + e32) if e_fmt + e32 > 0.0 else (0.0 if err == 0.0 else float('inf'))
        ratio = err / bound if bound > 0.0 else (0.0 if err == 0.0 else float('inf'))
        RATIOS.append((case, backend, w, err, e_fmt, e32, floor, ratio))
        print('RATIO %s | %s | %s | err %.3e | e_fmt %.3e | e32 %.3e | floor %.3e | err/(e_fmt+e32) %.3f | err/bound %.3f'
              % (case, backend, w, err, e_fmt, e32, floor, raw, ratio))
        assert ratio <= K, '%s %s [%s]: kernel error %.3e is %.2f x max(e_fmt + e32, floor) = %.3e (limit %g)' % (
            case, w, backend, err, ratio, bound, K)
        worst = max(worst, ratio)
    return worst


# ================================================================================================
# the scene interaction network
# ================================================================================================

def edge_index_of(ptr):
    """all ordered pairs (source j -> target i), i != j, inside every scene"""
    src, dst = [], []
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        for i in range(lo, hi):
            for j in range(lo, hi):
                if i != j:
                    src.append(j)
                    dst.append(i)
    return torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)


def rel_pose64(fr, po):
    """pose ``po`` in the frame ``fr`` (..., 4): the rule of rel_pose (csrc/gnn_dev.h) = oracle.geometry.transform2frame; NaN -> 0"""
    dx, dy = po[..., 0] - fr[..., 0], po[..., 1] - fr[..., 1]
    c, s = fr[..., 2], fr[..., 3]
    rel = torch.stack([c * dx + s * dy, -s * dx + c * dy, po[..., 2] * c + po[..., 3] * s, po[..., 3] * c - po[..., 2] * s], dim=-1)
    return torch.where(torch.isnan(rel), torch.zeros_like(rel), rel)


class GnnRef(object):
    """interaction_net of oracle/model.py in float64 (or on cut operands): mlp_in, the edge MLP on [x_i, x_j, sem_i, sem_j, rel_ij]
    (the column order of the edge weight), max aggregation over the sources of each target (0 without a source), the update MLP on
    [x, aggregate, sem], mlp_out.  x (N, NS, F), pos (N, NS, 4), sem (N, NC), ptr: scene offsets.  Records of every max:
    ``win`` (N, NS, D) position of the winner among the target's sources in scene order (-1: none), ``margin`` = winner - runner-up
    (inf with one source), ``aggr``.  With ``dy`` also dx and the parameter gradients (float64 autograd; the first of equal sources takes a
    max's gradient, which is the kernel's rule)."""

    def __init__(self, sd, prefix, x, pos, sem, ptr, dy=None, cut=False):
        names = [k for k in sd if k.startswith(prefix + '.')]
        sdg = {k: sd[k].detach().to(T64).clone().requires_grad_(dy is not None) for k in names}
        xg = x.detach().to(T64).clone().requires_grad_(dy is not None)
        N, NS, Fin = xg.shape
        p64, s64 = pos.detach().to(T64), sem.detach().to(T64)
        r4, re = (rule_rows4, rule_edge) if cut else (rule_none, rule_none)
        self.pres_node, self.pres_edge = [], []
        h = mlp_ref64(sdg, prefix + '.mlp_in', xg, r4, self.pres_node)                    # (N, NS, D)
        D = h.shape[-1]
        NC = s64.shape[1]
        aggr, win, margin, won_rows = [], [], [], []
        for lo, hi in zip(ptr[:-1], ptr[1:]):
            n = hi - lo
            if n < 2:
                aggr.append(torch.zeros((n, NS, D), dtype=T64))
                win.append(torch.full((n, NS, D), -1, dtype=torch.long))
                margin.append(torch.full((n, NS, D), float('inf'), dtype=T64))
                continue
            ii = torch.arange(n).repeat_interleave(n - 1)
            jj = torch.cat([torch.cat([torch.arange(0, i), torch.arange(i + 1, n)]) for i in range(n)])
            rel = rel_pose64(p64[lo + ii], p64[lo + jj])                                 # (E, NS, 4)
            si = s64[lo + ii].unsqueeze(1).expand(-1, NS, NC)
            sj = s64[lo + jj].unsqueeze(1).expand(-1, NS, NC)
            pe = []
            m = mlp_ref64(sdg, prefix + '.msg.0.edge_mlp', torch.cat([h[lo + ii], h[lo + jj], si, sj, rel], dim=-1), re, pe)
            m = m.reshape(n, n - 1, NS, D)
            # the first of equal sources wins and takes the whole gradient (gnn_edge_kernel: `arg < 0 || v > best`)
            # (equal = within TIE_EPS: identical fp32 rows need not come out of a float64 matrix product bit-identical)
            cand = m.detach() >= m.detach().amax(dim=1, keepdim=True) - TIE_EPS
            first = cand & (cand.cumsum(1) == 1)
            v, ix = (m * first).sum(1), first.to(torch.uint8).argmax(dim=1)
            aggr.append(v)
            win.append(ix)
            if n > 2:
                t2 = m.detach().topk(2, dim=1).values
                margin.append(t2[:, 0] - t2[:, 1])
            else:
                margin.append(torch.full((n, NS, D), float('inf'), dtype=T64))
            # pre-activations of the edges that won a channel (the others carry no gradient)
            won = torch.zeros((n, n - 1, NS), dtype=torch.bool)
            won.scatter_(1, ix.permute(0, 2, 1), torch.ones((n, D, NS), dtype=torch.bool))
            self.pres_edge += [p.detach().reshape(n, n - 1, NS, -1)[won] for p in pe]
        self.aggr_t = torch.cat(aggr, 0)
        self.win, self.margin = torch.cat(win, 0), torch.cat(margin, 0)
        sn = s64.unsqueeze(1).expand(N, NS, NC)
        upd = mlp_ref64(sdg, prefix + '.msg.0.update_mlp', torch.cat([h, self.aggr_t, sn], dim=-1), r4, self.pres_node)
        out = mlp_ref64(sdg, prefix + '.mlp_out', upd, r4, self.pres_node)
        self.y, self.aggr = out.detach(), self.aggr_t.detach()
        self.dx, self.dp, self.names = None, None, names
        if dy is not None:
            (out * dy.to(T64)).sum().backward()
            self.dx = xg.grad.detach()
            self.dp = torch.cat([(sdg[k].grad if sdg[k].grad is not None else torch.zeros_like(sdg[k])).reshape(-1) for k in names])
        del self.aggr_t


class GnnOracle32(object):
    """om.interaction_net in torch fp32 on the CPU, same inputs"""

    def __init__(self, sd, prefix, x, pos, sem, ptr, dy=None):
        names = [k for k in sd if k.startswith(prefix + '.')]
        sdg = dict(sd)
        for k in names:
            sdg[k] = sd[k].detach().float().clone().requires_grad_(dy is not None)
        xg = x.detach().float().clone().requires_grad_(dy is not None)
        NS = xg.shape[1]
        ei = edge_index_of(ptr)
        out = om.interaction_net(sdg, prefix, xg if NS > 1 else xg[:, 0], pos if NS > 1 else pos[:, 0], sem, ei)
        out = out if NS > 1 else out.unsqueeze(1)
        self.y = out.detach()
        self.dx = self.dp = None
        self.names = names
        if dy is not None:
            (out * dy.float()).sum().backward()
            self.dx = xg.grad.detach()
            self.dp = torch.cat([(sdg[k].grad if sdg[k].grad is not None else torch.zeros_like(sdg[k])).reshape(-1) for k in names])


def gnn_blocks(sd, prefix, flat):
    """[(parameter name, block)] of the flat gradient: mlp_in | msg.0.edge_mlp | msg.0.update_mlp | mlp_out"""
    out, off = [], 0
    for sub in ('.mlp_in', '.msg.0.edge_mlp', '.msg.0.update_mlp', '.mlp_out'):
        for k in mlp_keys(sd, prefix + sub):
            n = sd[k].numel()
            out.append((k, flat[off:off + n]))
            off += n
    assert off == flat.numel()
    return out


def gnn_flat64(sd, prefix, ref):
    """ref.dp (state-dict order of the prefix) re-ordered into the kernels' flat order"""
    by = {}
    off = 0
    for k in ref.names:
        n = sd[k].numel()
        by[k] = ref.dp[off:off + n]
        off += n
    return torch.cat([by[k] for sub in ('.mlp_in', '.msg.0.edge_mlp', '.msg.0.update_mlp', '.mlp_out') for k in mlp_keys(sd, prefix + sub)])


def scene_inputs(sizes, NS, Fin, NC, key, spread=6.0):
    """x (N, NS, F) in [-1, 1), poses (N, NS, 4) with unit headings inside a `spread` m window, one-hot classes (N, NC), ptr"""
    N = int(sum(sizes))
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    x = synth.f32(synth.counter_uniform((N, NS, Fin), key + '/x', -1.0, 1.0))
    xy = synth.counter_uniform((N, NS, 2), key + '/xy', -spread / 2, spread / 2)
    ang = synth.counter_uniform((N, NS), key + '/h', -math.pi, math.pi)
    pos = synth.f32(np.concatenate([xy, np.cos(ang)[..., None], np.sin(ang)[..., None]], axis=-1))
    cls = (synth.counter_uniform((N,), key + '/c', 0.0, 1.0) * NC).astype(np.int64) % NC
    sem = torch.zeros((N, NC), dtype=torch.float32)
    sem[torch.arange(N), torch.from_numpy(cls)] = 1.0
    return x, pos, sem, ptr


def gnn_preconditions(r64, ptr, thr, want_positions=None):
    """on the REFERENCE alone: (ambiguous ReLUs, maxes whose margin is neither an exact tie nor above ``thr``, winner positions missing
    from ``want_positions`` = {agent row: positions that must win at least one channel})"""
    n_relu, _ = relu_ambiguous(r64.pres_node + r64.pres_edge)
    m = r64.margin
    n_close = int(((m > TIE_EPS) & (m <= thr)).sum())
    missing = []
    for a, want in (want_positions or {}).items():
        have = set(r64.win[a].reshape(-1).tolist())
        missing += [(a, p) for p in want if p not in have]
    return n_relu, n_close, missing
