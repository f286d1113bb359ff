"""strive_adam_flat (csrc/optim.hip), FlatAdam (strive_amd/optim.py), its wiring into DataParallelTrainer and the max |w| table it
feeds params.py.

Kernel cases run on the host emulation of the same source and, marked ``gpu``, on the MI355X.  The reference is the four Adam
formulas in float64 on the fp32 inputs (tests/adam_ref.py); the bound per tensor and quantity is
|kernel - ref| <= 16 max(max |torch.optim.Adam(fp32, CPU) - ref|, 2^-23 max |ref|).  The worst ratios observed (bound: 16) are kept in
profiles/r23_flat_adam_ratios.md.
"""
import os
import sys

import numpy as np
import pytest
import torch

import adam_ref as AR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

BACKENDS = ['emu', pytest.param('gpu', marks=pytest.mark.gpu)]
TABLES = {'a': AR.TABLE_A, 'b': None, 'c1': [1], 'c3': [1, 2]}
COMBOS = [(wd, lr, t) for wd in (0.0, 0.01) for lr in (1e-3, 1e-5) for t in (1, 2, 1000)]
RATIOS = {}


def _sizes(name):
    return AR.model_sizes(2) if name == 'b' else TABLES[name]


@pytest.fixture(scope='module')
def emu_lib():
    import build as emu_build
    from strive_amd import _lib as L
    return L.StriveLib(emu_build.build(), require_all=True)


@pytest.fixture(params=BACKENDS)
def backend(request):
    """(name, library, device) of the emulated build on host tensors, or of the product's build on the MI355X"""
    if request.param == 'emu':
        return 'emu', request.getfixturevalue('emu_lib'), 'cpu'
    from strive_amd import _lib as L
    return 'gpu', L.get_lib(), 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print('FLAT_ADAM_RATIO %-4s %-28s table %-3s worst %.3f (%s)' % (k + RATIOS[k]))


def _note(backend, kind, table, ratio, where):
    key = (backend, kind, table)
    if key not in RATIOS or ratio > RATIOS[key][0]:
        RATIOS[key] = (ratio, where)
    print('%s %s table %s: worst ratio %.3f at %s (bound %g)' % (backend, kind, table, ratio, where, AR.K))


_INPUTS = {}


def _inputs(name, steps):
    key = (name, steps)
    if key not in _INPUTS:
        n = int(sum(_sizes(name)))
        _INPUTS[key] = AR.make_inputs(n, seed=1000 + 7 * sorted(TABLES).index(name) + steps, steps=steps)
    return _INPUTS[key]


# ------------------------------------------------------------------------------------------------
# the kernel against float64
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table', sorted(TABLES))
def test_single_step_against_float64(backend, table):
    """one step at t = 1, 2, 1000 from given m, v; weight decay 0 and 0.01; lr 1e-3 and 1e-5; and max |p_new| per tensor, bit for
    bit, written into a table the caller did not clear"""
    bname, lib, dev = backend
    sizes = _sizes(table)
    p, (g,), m, v = _inputs(table, 1)
    for wd, lr, t in COMBOS:
        m0, v0 = (np.zeros_like(m), np.zeros_like(v)) if t == 1 else (m, v)
        ref = AR.ref64(p, g, m0, v0, t, lr, wd)
        tor = AR.torch_adam(p, [g], m0, v0, t, lr, wd)[0]
        k = AR.Kernel(lib, dev, p, m0, v0, sizes).step(g, t, lr, wd)
        got = k.values()
        ratio, where = AR.worst_ratio(got, tor, ref, sizes, 'wd %g lr %g t %d' % (wd, lr, t))
        _note(bname, 'single step', table, ratio, where)
        assert ratio <= AR.K, where
        assert np.array_equal(k.table.cpu().numpy(), AR.absmax_of(got[0], sizes)), 'max |w| table, wd %g lr %g t %d' % (wd, lr, t)


@pytest.mark.parametrize('lr,wd', [(1e-3, 0.01), (1e-5, 0.0)])
@pytest.mark.parametrize('table', sorted(TABLES))
def test_trajectory_of_20_steps_against_float64(backend, table, lr, wd):
    """free-running over 20 recorded gradients (they do not depend on p: errors only add up), every quantity after every step; both
    learning rates and both weight decays of the recipe occur (the single steps cover all four combinations)"""
    bname, lib, dev = backend
    sizes = _sizes(table)
    p, gs, _, _ = _inputs(table, 20)
    z = np.zeros_like(p)
    tor = AR.torch_adam(p, gs, z, z, 1, lr, wd)
    k = AR.Kernel(lib, dev, p, z, z, sizes)
    ref = (p.astype(np.float64), z.astype(np.float64), z.astype(np.float64))
    check = range(20) if len(sizes) < 100 else (0, 9, 19)
    for i, g in enumerate(gs):
        ref = AR.ref64(ref[0], g, ref[1], ref[2], i + 1, lr, wd)
        k.step(g, i + 1, lr, wd)
        if i in check:
            got = k.values()
            ratio, where = AR.worst_ratio(got, tor[i], ref, sizes, 'wd %g lr %g step %d' % (wd, lr, i + 1))
            _note(bname, 'trajectory', table, ratio, where)
            assert ratio <= AR.K, where
            assert np.array_equal(k.table.cpu().numpy(), AR.absmax_of(got[0], sizes))


# ------------------------------------------------------------------------------------------------
# per-segment max |w|
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('table', sorted(TABLES))
def test_absmax_table_nan_null_and_determinism(backend, table):
    bname, lib, dev = backend
    sizes = _sizes(table)
    off = AR.offsets(sizes)
    p, (g,), m, v = _inputs(table, 1)
    a = AR.Kernel(lib, dev, p, m, v, sizes).step(g, 2, 1e-3, 0.0)
    b = AR.Kernel(lib, dev, p, m, v, sizes).step(g, 2, 1e-3, 0.0)
    for x, y in zip(a.values() + (a.table.cpu().numpy(),), b.values() + (b.table.cpu().numpy(),)):
        assert x.tobytes() == y.tobytes(), 'two runs differ'
    # no table: the same p, m, v, bit for bit
    c = AR.Kernel(lib, dev, p, m, v, None).step(g, 2, 1e-3, 0.0)
    for x, y in zip(a.values(), c.values()):
        assert x.tobytes() == y.tobytes(), 'seg_absmax = NULL changes the update'
    # a NaN parameter: NaN in its tensor's row, every other row as before
    s = len(sizes) // 2
    pn = p.copy()
    pn[off[s] + (off[s + 1] - off[s]) // 2] = np.nan
    d = AR.Kernel(lib, dev, pn, m, v, sizes).step(g, 2, 1e-3, 0.0)
    tn, t0 = d.table.cpu().numpy(), a.table.cpu().numpy()
    assert np.isnan(tn[s])
    keep = np.arange(len(sizes)) != s
    assert np.array_equal(tn[keep], t0[keep])


# ------------------------------------------------------------------------------------------------
# special values, in kind, against torch.optim.Adam
# ------------------------------------------------------------------------------------------------

def test_special_values_in_kind(backend):
    bname, lib, dev = backend
    sizes = [5, 64, 3, 300]
    n = sum(sizes)
    p, (g,), m, v = AR.make_inputs(n, seed=77)
    special = {'zero': 2, 'huge+': 7, 'huge-': 70, 'tiny': 71, 'nan': 200}
    g[special['zero']] = 0.0
    m[special['zero']] = 0.5                       # (non-zero, so that the quotient m / eps itself is compared with torch's)
    v[special['zero']] = 0.0                       # denominator = eps
    g[special['huge+']], g[special['huge-']] = 1e30, -1e30        # g^2 overflows: v becomes inf
    g[special['tiny']] = 1e-30                     # g^2 underflows
    v[special['tiny']] = 0.0
    g_nonan = g.copy()
    g[special['nan']] = np.nan
    for wd, lr, t in ((0.0, 1e-3, 2), (0.01, 1e-5, 1000)):
        tor = AR.torch_adam(p, [g], m, v, t, lr, wd)[0]
        got = AR.Kernel(lib, dev, p, m, v, sizes).step(g, t, lr, wd).values()
        clean = AR.Kernel(lib, dev, p, m, v, sizes).step(g_nonan, t, lr, wd).values()
        plain = np.ones(n, dtype=bool)
        for name, a, b in zip('pmv', got, tor):
            assert np.array_equal(np.isnan(a), np.isnan(b)), '%s: NaN pattern differs from torch.optim.Adam' % name
            assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), \
                '%s: inf pattern differs from torch.optim.Adam' % name
            plain &= np.isfinite(b)
        assert np.isnan(got[0][special['nan']]) and np.isinf(got[2][special['huge+']]) and np.isinf(got[2][special['huge-']])
        if wd == 0.0:
            z = special['zero']
            assert got[2][z] == 0.0 and got[2][special['tiny']] == 0.0
            # v = 0: the step is (lr / bc1) m_new / eps, 1e8 times the usual size -- a dropped or misplaced eps cannot pass
            assert abs(got[0][z] - p[z]) > 1e3 * lr and abs(got[0][z] - tor[0][z]) <= 4e-7 * abs(tor[0][z])
        # (the float64 reference does not overflow where fp32 does: elements with a non-finite fp32 quantity are compared in kind only)
        ref = AR.ref64(p, g, m, v, t, lr, wd)
        ratio, where = AR.worst_ratio(got, tor, ref, sizes, 'special wd %g' % wd, include=plain)
        _note(bname, 'special values', '-', ratio, where)
        assert ratio <= AR.K, where
        others = np.arange(n) != special['nan']
        for a, c in zip(got, clean):
            assert a[others].tobytes() == c[others].tobytes(), 'a NaN gradient touched its neighbours'


# ------------------------------------------------------------------------------------------------
# FlatAdam
# ------------------------------------------------------------------------------------------------

@pytest.fixture
def emu_ops(emu_lib):
    from strive_amd import _lib as L, ops
    orig = (ops._lib_for, L.get_lib)
    ops._lib_for = lambda *tensors: emu_lib          # CPU tensors + the emulated library: test infrastructure only
    L.get_lib = lambda: emu_lib
    yield emu_lib
    ops._lib_for, L.get_lib = orig


def _small_net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 33))


def _recorded(net, steps, seed):
    rng = np.random.default_rng(seed)
    return [[torch.from_numpy(AR.gradients(rng, p.numel()).reshape(tuple(p.shape))) for p in net.parameters()] for _ in range(steps)]


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy().copy()


def _step_with(opt, net, grads, bound_views=True):
    """one step on the recorded gradients, written into the optimiser's bound views (FlatAdam) or handed over as tensors of their own"""
    bound = bound_views and hasattr(opt, 'grad_flat')
    if bound:
        opt.zero_grad()
    for p, g in zip(net.parameters(), grads):
        if bound:
            p.grad.copy_(g)
        else:
            p.grad = g.clone()
    opt.step()


def test_flat_adam_views_lr_edits_and_bound(emu_ops):
    from strive_amd.optim import FlatAdam
    net, twin = _small_net(), _small_net()
    opt = FlatAdam(net.parameters(), lr=1e-3, weight_decay=0.01)
    ref = torch.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=0.01, foreach=False)
    assert set(opt.param_groups[0]) == set(ref.param_groups[0])
    # parameters and gradients are views at the trainer's offsets (the unpadded concatenation in parameters() order)
    off = 0
    for p in net.parameters():
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * off and p.grad.data_ptr() == opt.grad_flat.data_ptr() + 4 * off
        off += p.numel()
    assert off == opt.numel == sum(p.numel() for p in twin.parameters())
    assert np.array_equal(_flat(net), _flat(twin))
    sizes = [p.numel() for p in net.parameters()]
    grads = _recorded(net, 6, seed=5)
    p64 = _flat(net).astype(np.float64)
    m64, v64 = np.zeros_like(p64), np.zeros_like(p64)
    for i, gl in enumerate(grads):
        if i == 3:                                        # an lr edit between steps takes effect (schedulers, manual edits)
            for o in (opt, ref):
                o.param_groups[0]['lr'] = 1e-5
        lr = 1e-3 if i < 3 else 1e-5
        before = _flat(net)
        _step_with(opt, net, gl, bound_views=(i % 2 == 0))   # odd steps: foreign p.grad tensors, the copying path
        _step_with(ref, twin, gl, bound_views=False)
        gflat = torch.cat([g.reshape(-1) for g in gl]).numpy()
        p64, m64, v64 = AR.ref64(p64, gflat, m64, v64, i + 1, lr, 0.01)
        if i == 3:
            assert float(np.abs(_flat(net) - before).max()) < 1e-4, 'the lr edit was not read'
    st = ref.state_dict()['state']
    tor = (_flat(twin), np.concatenate([st[i]['exp_avg'].reshape(-1).numpy() for i in range(len(sizes))]),
           np.concatenate([st[i]['exp_avg_sq'].reshape(-1).numpy() for i in range(len(sizes))]))
    got = (_flat(net), opt.exp_avg.numpy(), opt.exp_avg_sq.numpy())
    ratio, where = AR.worst_ratio(got, tor, (p64, m64, v64), sizes, 'FlatAdam 6 steps')
    _note('emu', 'FlatAdam vs Adam', 'net', ratio, where)
    assert ratio <= AR.K, where
    assert opt.step_count == 6


def test_flat_adam_state_dict_round_trips_with_torch_adam(emu_ops):
    from strive_amd.optim import FlatAdam
    grads = _recorded(_small_net(), 8, seed=9)
    sizes = [p.numel() for p in _small_net().parameters()]

    def run(first, second):
        """3 steps with optimiser class ``first``, its state dict into class ``second`` on a fresh copy, 5 further steps"""
        make = {'flat': lambda ps: FlatAdam(ps, lr=1e-3), 'torch': lambda ps: torch.optim.Adam(ps, lr=1e-3, foreach=False)}
        net = _small_net()
        o1 = make[first](net.parameters())
        for gl in grads[:3]:
            _step_with(o1, net, gl)
        sd = o1.state_dict()
        net2 = _small_net()
        net2.load_state_dict(net.state_dict())
        o2 = make[second](net2.parameters())
        o2.load_state_dict(sd)
        for gl in grads[3:]:
            _step_with(o2, net2, gl)
        return net2, o2, sd
    p64 = _flat(_small_net()).astype(np.float64)
    m64, v64 = np.zeros_like(p64), np.zeros_like(p64)
    for i, gl in enumerate(grads):
        p64, m64, v64 = AR.ref64(p64, torch.cat([g.reshape(-1) for g in gl]).numpy(), m64, v64, i + 1, 1e-3, 0.0)
    tnet, topt, tsd = run('torch', 'torch')
    st = topt.state_dict()['state']
    tor = (_flat(tnet), np.concatenate([st[i]['exp_avg'].reshape(-1).numpy() for i in range(len(sizes))]),
           np.concatenate([st[i]['exp_avg_sq'].reshape(-1).numpy() for i in range(len(sizes))]))
    for first, second in (('flat', 'torch'), ('torch', 'flat'), ('flat', 'flat')):
        net, opt, sd = run(first, second)
        assert set(sd) == set(tsd) and set(sd['param_groups'][0]) == set(tsd['param_groups'][0])
        assert set(sd['state']) == set(tsd['state']) and set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
        st = opt.state_dict()['state']
        assert float(st[0]['step']) == 8.0
        got = (_flat(net), np.concatenate([st[i]['exp_avg'].reshape(-1).numpy() for i in range(len(sizes))]),
               np.concatenate([st[i]['exp_avg_sq'].reshape(-1).numpy() for i in range(len(sizes))]))
        ratio, where = AR.worst_ratio(got, tor, (p64, m64, v64), sizes, '%s -> %s' % (first, second))
        _note('emu', 'state dict ' + first + '->' + second, 'net', ratio, where)
        assert ratio <= AR.K, where
    # state dict tensors are copies, not views of the flat buffers
    net = _small_net()
    opt = FlatAdam(net.parameters())
    _step_with(opt, net, grads[0])
    sd = opt.state_dict()
    lo, hi = opt.exp_avg.data_ptr(), opt.exp_avg.data_ptr() + 4 * opt.numel
    lo2, hi2 = opt.exp_avg_sq.data_ptr(), opt.exp_avg_sq.data_ptr() + 4 * opt.numel
    for ent in sd['state'].values():
        for key in ('exp_avg', 'exp_avg_sq'):
            assert not (lo <= ent[key].data_ptr() < hi) and not (lo2 <= ent[key].data_ptr() < hi2)
    keep = sd['state'][0]['exp_avg'].clone()
    _step_with(opt, net, grads[1])
    assert torch.equal(sd['state'][0]['exp_avg'], keep)
    # a reference-era integer step loads
    for ent in sd['state'].values():
        ent['step'] = 1
    opt2 = FlatAdam(_small_net().parameters())
    opt2.load_state_dict(sd)
    assert opt2.step_count == 1 and torch.equal(opt2.exp_avg[:keep.numel()].view_as(keep), keep)


def test_flat_adam_refuses_what_it_does_not_do(emu_ops):
    from strive_amd.optim import FlatAdam
    net = _small_net()
    ps = list(net.parameters())
    with pytest.raises(NotImplementedError):
        FlatAdam([{'params': ps[:2]}, {'params': ps[2:]}])
    with pytest.raises(NotImplementedError):
        FlatAdam(ps, amsgrad=True)
    with pytest.raises(NotImplementedError):
        FlatAdam(ps, maximize=True)
    opt = FlatAdam(ps)
    opt.step()
    before = _flat(net)
    ps[1].data = ps[1].data.clone()                           # what model.to(...) does: the storage is not the flat view any more
    with pytest.raises(RuntimeError, match='flat buffer'):
        opt.step()
    assert np.array_equal(_flat(net), before) and opt.step_count == 1


def test_flat_adam_has_no_cpu_path():
    """host tensors without the emulated library have no path, like every operator here"""
    from strive_amd import _lib as L
    from strive_amd.optim import FlatAdam
    net = _small_net()
    before = _flat(net)
    opt = FlatAdam(net.parameters())
    with pytest.raises(L.StriveHipError):
        opt.step()
    assert np.array_equal(_flat(net), before) and opt.step_count == 0


# ------------------------------------------------------------------------------------------------
# trainer wiring (emulator)
# ------------------------------------------------------------------------------------------------

class _StubModel(torch.nn.Module):
    """a model small enough for a trainer step without any kernel: DataParallelTrainer needs FT, parameters and a forward"""
    FT = 2

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(6, 9)
        self.b = torch.nn.Linear(9, 4)

    def forward(self, scene_graph, map_idx, map_env, future_sample=False):
        return {'y': self.b(torch.tanh(self.a(scene_graph.x)))}


class _StubLoss(object):
    loss_weights = {'recon': 1.0, 'kl': 0.5, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0}

    def __call__(self, scene_graph, pred, map_idx=None, map_env=None):
        return {'recon_loss': (pred['y'] ** 2).sum(1), 'kl_loss': pred['y'].abs().sum(1)}


class _StubGraph(object):
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn((3, 6), generator=g)
        self.ptr = torch.tensor([0, 2, 3])
        self.future_vis = torch.ones((3, 2))


def _trainer_steps(model, loss_fn, opt, graphs, map_idx=None, env=None):
    """run the trainer over ``graphs``, recording a clone of the bucket just before every optimiser step"""
    from strive_amd.distributed import DataParallelTrainer
    tr = DataParallelTrainer(model, loss_fn, opt)
    rec, step0 = [], opt.step

    def recording(*a, **k):
        rec.append(tr.bucket[:-1].clone())
        return step0(*a, **k)
    opt.step = recording
    try:
        for gr in graphs:
            assert tr.step(gr, map_idx, env) is not None, tr.last_error
    finally:
        opt.step = step0
    return tr, rec


def _check_trainer_against_standalone(lib, model0_flat, sizes, rec, final_flat, lr):
    """the parameters after the trainer's steps equal strive_adam_flat applied stand-alone to the recorded gradients, bit for bit;
    against torch.optim.Adam on the same gradients they stay within the bound"""
    z = np.zeros_like(model0_flat)
    k = AR.Kernel(lib, 'cpu', model0_flat, z, z, sizes)
    gs = [r.numpy() for r in rec]
    ref = (model0_flat.astype(np.float64), z.astype(np.float64), z.astype(np.float64))
    for i, g in enumerate(gs):
        k.step(g, i + 1, lr, 0.0)
        ref = AR.ref64(ref[0], g, ref[1], ref[2], i + 1, lr, 0.0)
    assert k.values()[0].tobytes() == final_flat.tobytes(), 'the trainer\'s FlatAdam step is not the stand-alone kernel step'
    tor = AR.torch_adam(model0_flat, gs, z, z, 1, lr, 0.0)[-1]
    return AR.worst_ratio(k.values(), tor, ref, sizes, 'trainer, %d steps' % len(gs))


def test_trainer_with_flat_adam_cheap(emu_ops):
    from strive_amd import params
    from strive_amd.optim import FlatAdam
    model = _StubModel()
    start = _flat(model)
    sizes = [p.numel() for p in model.parameters()]
    opt = FlatAdam(model.parameters(), lr=1e-3)
    epoch = params.param_epoch()
    tr, rec = _trainer_steps(model, _StubLoss(), opt, [_StubGraph(1), _StubGraph(2)])
    assert params.param_epoch() == epoch + 2                  # one announcement per step, by the optimiser
    assert opt.grad_flat.data_ptr() == tr.bucket.data_ptr() and all(float(r.abs().max()) > 0 for r in rec)
    for p, v in zip(model.parameters(), tr._views):
        assert p.grad.data_ptr() == v.data_ptr()              # one buffer serves both: nothing is copied
    assert float(tr.bucket[-1]) == 0.0                        # the vote slot is left alone
    ratio, where = _check_trainer_against_standalone(emu_ops, start, sizes, rec, _flat(model), 1e-3)
    _note('emu', 'trainer (stub model)', 'net', ratio, where)
    assert ratio <= AR.K, where
    # any other optimiser: the step is what it was -- the trainer announces the update, once
    for make in (lambda ps: torch.optim.SGD(ps, lr=0.1), lambda ps: torch.optim.Adam(ps, lr=1e-3)):
        model = _StubModel()
        before = _flat(model)
        epoch = params.param_epoch()
        _trainer_steps(model, _StubLoss(), make(model.parameters()), [_StubGraph(1)])
        assert params.param_epoch() == epoch + 1 and not np.array_equal(_flat(model), before)


def _product_setup():
    from util import product_model
    from strive_amd import synth
    from strive_amd.losses.traffic_model import TrafficModelLoss
    TW = {'recon': 1.0, 'kl': 0.004, 'coll_veh_prior': 0.05, 'coll_env_prior': 0.1}
    m, sd = product_model(FT=2)
    m.train()
    batch, map_idx = synth.make_batch([2, 1], key='train/emu', FT=2)
    raster, dx = synth.make_raster(1024, 1024)
    env = synth.SyntheticMapEnv(raster, dx)
    return m, TrafficModelLoss(TW, m.get_normalizer(), m.get_att_normalizer()), batch, map_idx, env


def test_trainer_with_flat_adam_on_the_model(emu_ops):
    """the tests/test_training.py recipe (product_model(FT=2), make_batch([2, 1], FT=2)): two DataParallelTrainer steps with FlatAdam;
    then the weight packs with the max |w| table as the source and with it switched off, bit for bit; then what takes a tensor
    off the table"""
    from strive_amd import params, ops
    from strive_amd.optim import FlatAdam
    m, loss_fn, batch, map_idx, env = _product_setup()
    torch.manual_seed(11)
    start = _flat(m)
    sizes = [p.numel() for p in m.parameters()]
    assert len(sizes) == len(AR.model_sizes(2)) == 174         # (FT = 2: the same tensors, smaller future encoder and decoder head)
    opt = FlatAdam(m.parameters(), lr=1e-5)
    calls, norm0 = [], torch._foreach_norm

    def counting(ts, *a, **k):
        calls.append(len(ts))
        return norm0(ts, *a, **k)
    epoch = params.param_epoch()
    torch._foreach_norm = counting
    try:
        tr, rec = _trainer_steps(m, loss_fn, opt, [batch.clone(), batch.clone()], map_idx, env)
        first_step_norms = len(calls)
    finally:
        torch._foreach_norm = norm0
    assert params.param_epoch() == epoch + 2
    ratio, where = _check_trainer_against_standalone(emu_ops, start, sizes, rec, _flat(m), 1e-5)
    _note('emu', 'trainer (the model)', 'b', ratio, where)
    assert ratio <= AR.K, where
    # the table the last step wrote is exact
    assert np.array_equal(opt.absmax_table.numpy(), AR.absmax_of(_flat(m), sizes))

    # ---- max |w| source: packs with the table and with it switched off ----
    def packs(table_on):
        params._ABSMAX.clear()
        os.environ['STRIVE_ABSMAX_TABLE'] = '1' if table_on else '0'
        del calls[:]
        torch._foreach_norm = counting
        try:
            sd = m.state_dict()
            pk = [params.pack_cnn(sd), params.pack_mlp(sd, 'past_encoder'), params.pack_gnn(sd, 'prior_net', 2)]
        finally:
            torch._foreach_norm = norm0
            del os.environ['STRIVE_ABSMAX_TABLE']
        return [t.clone() for p_ in pk for t in p_.keep if torch.is_tensor(t)], list(pk[0].struct.wscale) + list(pk[0].struct.xscale), len(calls)
    on, s_on, n_on = packs(True)
    off, s_off, n_off = packs(False)
    assert n_on == 0 and n_off > 0, (n_on, n_off)
    assert len(on) == len(off) > 20 and s_on == s_off
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(on, off))

    # ---- what sends a tensor back to the norm path ----
    def served_from_table(tensor):
        params._ABSMAX.clear()
        del calls[:]
        torch._foreach_norm = counting
        try:
            v = params.absmax(tensor)
        finally:
            torch._foreach_norm = norm0
        assert v == float(tensor.detach().abs().max())
        return len(calls) == 0
    w = m.past_encoder.net[0].weight
    assert served_from_table(w)
    with torch.no_grad():
        w.mul_(1.5)                                            # an in-place torch op
    assert not served_from_table(w) and served_from_table(m.past_encoder.net[3].weight)
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})        # load_state_dict copies into every parameter
    assert not served_from_table(m.past_encoder.net[3].weight)
    opt.zero_grad()
    opt.step()                                                # a step makes the table current again
    assert served_from_table(w) and served_from_table(m.past_encoder.net[3].weight)
    w.data[0, 0] = 3.0                                         # a p.data write, announced
    params.parameters_changed()
    assert not served_from_table(w) and not served_from_table(m.past_encoder.net[3].weight)
    m.eval()


@pytest.mark.gpu
def test_lagged_absmax_from_the_table_on_the_gpu():
    """inside lagged_absmax over 5 FlatAdam steps: the bound served for every registered tensor is at least the true max |w| and
    equals the table value the unchanged lag rule prescribes (the read-back of _LAG_DEPTH calls earlier; exact at first sight) plus
    the slack; from the third step on no norm kernel runs for registered tensors"""
    from strive_amd import params
    from strive_amd.optim import FlatAdam
    dev = 'cuda:0'
    params._ABSMAX.clear(); params._LAG.clear(); params._LAG_BATCH.clear()
    net = _small_net().to(dev)
    lr = 1e-2
    opt = FlatAdam(net.parameters(), lr=lr)
    ws = [p for p in net.parameters()]
    grads = _recorded(net, 5, seed=21)
    calls, norm0 = [], torch._foreach_norm

    def counting(ts, *a, **k):
        calls.append(len(ts))
        return norm0(ts, *a, **k)
    slack = 8.0 * lr
    tables, per_step_calls = [], []
    torch._foreach_norm = counting
    try:
        for i, gl in enumerate(grads):
            _step_with(opt, net, [g.to(dev) for g in gl])
            tables.append(opt.absmax_table.cpu().numpy().copy())
            true = np.array([float(p.detach().abs().max()) for p in ws], dtype=np.float32)
            assert np.array_equal(tables[-1], true)
            del calls[:]
            with params.lagged_absmax(slack=slack):
                params.prefetch_absmax([p.detach() for p in ws])
                served = np.array([params.absmax(p.detach()) for p in ws])
            per_step_calls.append(len(calls))
            assert (served >= true.astype(np.float64) - 1e-7).all(), 'step %d: a served bound is below the true max |w|' % i
            want = tables[0].astype(np.float64) if i == 0 else tables[max(i - params._LAG_DEPTH, 0)].astype(np.float64) + slack
            assert np.array_equal(served, want), (i, served, want)
    finally:
        torch._foreach_norm = norm0
        params._ABSMAX.clear(); params._LAG.clear(); params._LAG_BATCH.clear()
    assert per_step_calls[2:] == [0, 0, 0], per_step_calls
