"""Shared by tests/test_flat_adam.py and tests/test_train_traffic.py: the float64 reference of one Adam step, torch.optim.Adam on the
CPU as the yardstick of what fp32 can do, the input recipes, the segment tables and the bound.

Bound (per tensor, per quantity p / m / v):  |kernel - ref| <= K * max(max |torch.optim.Adam(fp32, CPU) - ref|, 2^-23 max |ref|), K = 16.
"""
import numpy as np
import torch

K = 16.0
TABLE_A = [1, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 70001]
BETAS, EPS = (0.9, 0.999), 1e-8


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


_MODEL_SIZES = {}


def model_sizes(NC=2):
    """numel of the model's parameter tensors in model.parameters() order (174 tensors, 1,092,418 elements for NC = 2)"""
    if NC not in _MODEL_SIZES:
        from strive_amd.models.traffic_model import TrafficModel
        _MODEL_SIZES[NC] = [p.numel() for p in TrafficModel(4, 12, 256, NC).parameters()]
    return _MODEL_SIZES[NC]


def gradients(rng, n):
    """random sign, |g| log-uniform in [1e-6, 1e3], 5 % exact zeros"""
    g = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), n)) * rng.choice([-1.0, 1.0], n)
    g[rng.uniform(size=n) < 0.05] = 0.0
    return g.astype(np.float32)


def make_inputs(n, seed, steps=1):
    """p ~ 0.1 N(0,1); ``steps`` recorded gradients; given moments m, v (for a step that starts at t > 1)"""
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    gs = [gradients(rng, n) for _ in range(steps)]
    m = (0.1 * gradients(rng, n)).astype(np.float32)
    v = (1e-3 * gradients(rng, n).astype(np.float64) ** 2).astype(np.float32)
    return p, gs, m, v


def ref64(p, g, m, v, t, lr, wd, betas=BETAS, eps=EPS):
    """the four formulas in float64 on the given (fp32) values; returns new float64 (p, m, v)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with np.errstate(all='ignore'):
        g = g + wd * p
        m = m + (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def torch_adam(p, gs, m, v, t0, lr, wd, betas=BETAS, eps=EPS):
    """torch.optim.Adam (fp32, CPU, single-tensor form) from the state (m, v) after t0 - 1 steps, over the recorded gradients;
    returns the fp32 (p, m, v) after every step"""
    w = torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=np.float32)))
    opt = torch.optim.Adam([w], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[w] = {'step': torch.tensor(float(t0 - 1)), 'exp_avg': torch.from_numpy(np.array(m, dtype=np.float32)),
                    'exp_avg_sq': torch.from_numpy(np.array(v, dtype=np.float32))}
    out = []
    for g in gs:
        w.grad = torch.from_numpy(np.array(g, dtype=np.float32))
        opt.step()
        st = opt.state[w]
        out.append((w.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()))
    return out


class Kernel(object):
    """strive_adam_flat on flat device (or, emulated, host) tensors"""

    def __init__(self, lib, device, p, m, v, sizes=None):
        from strive_amd import _lib as L
        self.L, self.lib, self.device = L, lib, device
        self.p, self.m, self.v = (torch.from_numpy(np.array(a, dtype=np.float32)).to(device) for a in (p, m, v))
        self.n = int(self.p.numel())
        self.seg = self.table = None
        if sizes is not None:
            self.seg = torch.from_numpy(offsets(sizes)).to(device)
            self.table = torch.full((len(sizes),), 123.0, dtype=torch.float32, device=device)      # (not cleared by the caller)

    def step(self, g, t, lr, wd, betas=BETAS, eps=EPS):
        L = self.L
        g = torch.from_numpy(np.array(g, dtype=np.float32)).to(self.device)
        nseg = 0 if self.seg is None else int(self.table.numel())
        self.lib.call('strive_adam_flat', L.ptr(self.p), L.ptr(g), L.ptr(self.m), L.ptr(self.v), self.n, float(lr), float(betas[0]),
                      float(betas[1]), float(eps), float(wd), 1.0 - betas[0] ** t, 1.0 - betas[1] ** t, L.ptr(self.seg), nseg,
                      L.ptr(self.table), L.stream_ptr(self.p))
        return self

    def values(self):
        return tuple(a.cpu().numpy().copy() for a in (self.p, self.m, self.v))


def worst_ratio(got, torch_vals, ref, sizes, what='', include=None):
    """max over tensors and quantities of |got - ref| / max(max |torch - ref|, 2^-23 max |ref|) over the FINITE reference entries
    (of the elements ``include``, a bool mask, if given); the bound holds iff the result is <= K"""
    off = offsets(sizes)
    worst, where = 0.0, ''
    for name, a, b, r in zip('pmv', got, torch_vals, ref):
        a, b = a.astype(np.float64), b.astype(np.float64)
        for s in range(len(sizes)):
            lo, hi = off[s], off[s + 1]
            fin = np.isfinite(r[lo:hi]) & np.isfinite(b[lo:hi])
            if include is not None:
                fin &= include[lo:hi]
            if not fin.any():
                continue
            rr = r[lo:hi][fin]
            den = max(float(np.abs(b[lo:hi][fin] - rr).max()), 2.0 ** -23 * float(np.abs(rr).max()))
            err = float(np.abs(a[lo:hi][fin] - rr).max())
            ratio = err / den if den > 0.0 else (0.0 if err == 0.0 else float('inf'))
            if not np.isfinite(err):               # a non-finite kernel value where torch's and the reference's are finite
                ratio = float('inf')
            if ratio > worst:
                worst, where = ratio, '%s %s tensor %d' % (what, name, s)
    return worst, where


def absmax_of(p, sizes):
    off = offsets(sizes)
    return np.array([np.abs(p[off[s]:off[s + 1]]).max() if off[s + 1] > off[s] else 0.0 for s in range(len(sizes))], dtype=np.float32)
