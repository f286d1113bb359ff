"""The scene dataset (strive_amd/datasets/nuscenes_dataset.py, csrc/dataset.hip) against the reference's own ``NuScenesDataset``:
tests/golden/g20_dataset.npz holds what its ``post_process``, ``compile_scenarios`` and ``__getitem__`` returned for the hand-built
tracks set of tests/golden/make_golden_dataset.py (README_g20.md lists the cases).  Every check runs on the host emulation of the
kernels (tests/hipemu) and, marked ``gpu``, on the MI355X.

Tolerances.  The track route has none: ``is_vis``, the kept-agent set, ``ptr, batch, edge_index, sem, past_vis, future_vis, map_idx``
are equal, ``traj`` and ``accel`` are bit-identical in float64 (a NaN where the reference has a NaN; NaN payloads are not compared) and
``past, future, past_gt, future_gt, lw`` bit-identical in fp32 -- on the emulator against the reference and on the GPU against both.
The kernels use + - * / sqrt (IEEE, rounded once under ``fp contract(off)``), ``rint`` and ``fmod`` (both exact), so no column needed
a bound.

The scenario route.  The issue words its bound as "the error of one float64 ``arctan2``".  That premise does not hold for the
reference: its ``read_adv_scenes`` loads ``past`` and ``fut_adv`` with ``torch.tensor(list)``, i.e. as fp32, ``compile_scenarios`` calls
``.numpy()`` on them, and ``np.arctan2`` and ``angle_diff`` of fp32 arrays are evaluated in fp32 (only the division by the float64
time step widens).  The route here does the same on the host, so the bound is derived for the fp32 ``arctan2`` the reference really
runs -- with a float64 one the fixture itself could not be met.  Everything else on that route is IEEE arithmetic on the same inputs, hence bit-identical; only ``arctan2``
may differ between two builds of numpy / libm, by at most one unit in the last place of an angle of magnitude up to pi, u = 2^-22.
The heading rate is ``angle_diff(h[k+1], h[k]) / dt``: two angles, each off by at most u, and the fp32 operations of ``angle_diff`` on
values below 2 pi (ulp 2^-21 = 2 u) can move the result by one more rounding each way: |d hdot| <= (2 u + 2 u) / dt.  Normalised by
the heading-rate deviation (0.055684) and rounded to fp32 this is SCENARIO_HDOT_TOL below; every other float column must be equal.
Where numpy is the version that wrote the fixture (``sc/numpy_version``) the same ``arctan2`` runs and the heading rates must be
bit-identical too; the bound is for any other numpy.  The observed maxima are recorded in profiles/r19_dataset_ratios.md (0).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

from strive_amd import _lib as L                                      # noqa: E402
from strive_amd import ops, synth                                     # noqa: E402
from strive_amd.datasets import tracks as tracks_io                   # noqa: E402
from strive_amd.datasets.nuscenes_dataset import NuScenesDataset      # noqa: E402
from strive_amd.graph import Batch                                    # noqa: E402
import make_golden_dataset as G                                       # noqa: E402
from util import GOLDEN, golden                                       # noqa: E402

FLOAT_FIELDS = ('past', 'future', 'past_gt', 'future_gt', 'lw')
EQUAL_FIELDS = ('sem', 'past_vis', 'future_vis')
DT, STD_HDOT = 0.5, 0.055684
SCENARIO_HDOT_TOL = (4.0 * 2.0 ** -22 / DT) / STD_HDOT * (1.0 + 2.0 ** -20)
SCEN_DIR = os.path.join(GOLDEN, G.SCEN_DIR)


@pytest.fixture(scope='module')
def fix():
    z = golden(G.FIX)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


@pytest.fixture
def emu_ops(emu):
    orig = (ops._lib_for, L.get_lib)
    ops._lib_for = lambda *tensors: emu           # CPU tensors + the emulated library: test infrastructure only
    L.get_lib = lambda: emu
    yield emu
    ops._lib_for, L.get_lib = orig


def fixture_tracks(fix):
    return tracks_io.check_tracks({k: fix['tracks/' + k] for k in tracks_io.KEYS})


_cache = {}


def dataset(fix, cname, device, **kw):
    """The dataset of configuration ``cname`` ('c0', 'c1': track scenes; 'sc': the scenario directory) on ``device``, built once."""
    key = (cname, str(device), tuple(sorted(kw.items())))
    if key not in _cache:
        if cname == 'sc':
            _cache[key] = NuScenesDataset(None, G.fixture_env(True), scenario_path=SCEN_DIR, device=device, **kw)
        else:
            cfg = G.CONFIGS[cname]
            _cache[key] = NuScenesDataset(fixture_tracks(fix), G.fixture_env(cfg['carpark']), require_full_past=cfg['require_full_past'],
                                          seq_interval=cfg['seq_interval'], device=device, **kw)
    return _cache[key]


def tables(ds):
    return {'traj': ds.traj.cpu().numpy(), 'accel': ds.accel.cpu().numpy(), 'is_vis': ds.is_vis.cpu().numpy(), 'kept': ds.kept.cpu().numpy()}


def assert_bits(got, want, what):
    """Bit-identical floats; a NaN where the reference has a NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, '%s: %s %s vs %s %s' % (what, got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), '%s: NaN positions differ in %d entries' % (what, int((gn != wn).sum()))
    iv = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    bad = (got.view(iv) != want.view(iv)) & ~gn
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d entries differ in bits; first at %s: %r vs %r' % (what, int(bad.sum()), i, got[i], want[i]))


def rows_of_kept(fix, cname):
    """Mask over the table rows of the agents the reference kept."""
    tr = fixture_tracks(fix)
    T = np.repeat(np.diff(tr['frame_ptr']), np.diff(tr['agent_ptr']))
    return np.repeat(fix[cname + '/kept'] == 1, T)


def check_tables(fix, cname, tb):
    p = cname + '/'
    assert np.array_equal(tb['kept'], fix[p + 'kept']), 'kept agents'
    rows = rows_of_kept(fix, cname) if cname != 'sc' else np.ones(tb['is_vis'].shape, dtype=bool)
    assert np.array_equal(tb['is_vis'][rows], fix[p + 'is_vis'][rows]), 'is_vis'
    assert_bits(tb['traj'][rows], fix[p + 'traj'][rows], cname + ' traj')
    if cname != 'sc':
        assert_bits(tb['accel'][rows], fix[p + 'accel'][rows], cname + ' accel')


def expected_batch(fix, cname, idx):
    """The fixture's windows ``idx`` collated: dict of arrays."""
    p = cname + '/'
    ptr = fix[p + 'ptr']
    n_all = np.diff(ptr)
    eptr = np.concatenate([[0], np.cumsum(n_all * (n_all - 1))])
    out = {k: np.concatenate([fix[p + k][ptr[i]:ptr[i + 1]] for i in idx]) for k in FLOAT_FIELDS + EQUAL_FIELDS}
    n = n_all[idx]
    out['ptr'] = np.concatenate([[0], np.cumsum(n)])
    out['batch'] = np.repeat(np.arange(len(idx)), n)
    out['edge_index'] = np.concatenate([fix[p + 'edge_index'][:, eptr[i]:eptr[i + 1]] - ptr[i] + out['ptr'][j] for j, i in enumerate(idx)], axis=1)
    out['map_idx'] = fix[p + 'map_idx'][idx]
    return out


def check_batch(g, map_idx, exp, what, float_check=assert_bits):
    assert np.array_equal(g.ptr.cpu().numpy(), exp['ptr']), what + ' ptr'
    assert g.ptr.dtype == torch.long and g.batch.dtype == torch.long and g.edge_index.dtype == torch.long
    assert np.array_equal(g.batch.cpu().numpy(), exp['batch']), what + ' batch'
    assert np.array_equal(g.edge_index.cpu().numpy(), exp['edge_index'].reshape(2, -1)), what + ' edge_index'
    assert np.array_equal(torch.as_tensor(map_idx).reshape(-1).cpu().numpy(), np.asarray(exp['map_idx']).reshape(-1)), what + ' map_idx'
    for k in EQUAL_FIELDS:
        assert g[k].dtype == torch.float32 and np.array_equal(g[k].cpu().numpy(), exp[k]), '%s %s' % (what, k)
    for k in FLOAT_FIELDS:
        float_check(g[k].cpu().numpy(), exp[k], '%s %s' % (what, k))
    assert g.x.shape == g.pos.shape == (exp['ptr'][-1],)


def check_windows(fix, cname, ds, float_check=assert_bits):
    p = cname + '/'
    N = len(fix[p + 'seq_start'])
    assert len(ds) == N
    names = list(fix['tracks/scene_name']) if cname != 'sc' else list(fix['sc/scene_name'])
    assert ds.seq_map == [(str(names[s]), int(i)) for s, i in zip(fix[p + 'seq_scene'], fix[p + 'seq_start'])]
    for i in range(N):                                               # singly, as __getitem__ returns them
        d, m = ds[i]
        assert isinstance(m, int) and 'ptr' not in d and 'batch' not in d
        e = expected_batch(fix, cname, [i])
        d.ptr, d.batch = torch.as_tensor(e['ptr']), torch.as_tensor(e['batch'])
        check_batch(d, [m], e, '%s window %d' % (cname, i), float_check)
    for bs in (1, 3, N):
        got = list(ds.loader(bs))
        assert len(got) == (N + bs - 1) // bs
        for j, (g, mi) in enumerate(got):
            idx = list(range(j * bs, min(N, (j + 1) * bs)))
            assert g.num_graphs == len(idx) and mi.dtype == torch.long
            check_batch(g, mi, expected_batch(fix, cname, idx), '%s batch %d of %d' % (cname, j, bs), float_check)
            info = g.__dict__['_strive_scene_info']                  # primed from the host-known ptr: nothing to read back
            assert torch.equal(info.ptr_cpu, g.ptr.cpu()) and ops.scene_info(g) is info


def scenario_float_check(got, want, what):
    """Bit-identical but for the heading-rate column of the futures (module docstring)."""
    if got.ndim == 3 and got.shape[-1] == 6:
        assert_bits(got[..., :5], want[..., :5], what)
        gn, wn = np.isnan(got[..., 5]), np.isnan(want[..., 5])
        assert np.array_equal(gn, wn), what + ': NaN positions of hdot'
        err = float(np.nanmax(np.abs(got[..., 5].astype(np.float64) - want[..., 5].astype(np.float64)))) if (~gn).any() else 0.0
        print('%s: max |d hdot| (normalised) %.3e, bound %.3e' % (what, err, SCENARIO_HDOT_TOL))
        assert err <= SCENARIO_HDOT_TOL, '%s: hdot off by %.3e (> %.3e)' % (what, err, SCENARIO_HDOT_TOL)
        if str(golden(G.FIX)['sc/numpy_version']) == np.__version__:
            assert_bits(got[..., 5], want[..., 5], what + ' hdot under the numpy that wrote the fixture')
    else:
        assert_bits(got, want, what)


# ------------------------------------------------------------------------------------------------
# no library needed
# ------------------------------------------------------------------------------------------------

def test_tracks_file_round_trip_and_checks(tmp_path, fix):
    tr = fixture_tracks(fix)
    path = str(tmp_path / 'tracks.npz')
    tracks_io.save_tracks(path, tr)
    back = tracks_io.load_tracks(path)
    for k in tracks_io.KEYS:
        assert np.array_equal(np.asarray(back[k]), np.asarray(tr[k])), k
    for key, bad in (('obs_ptr', tr['obs_ptr'][::-1].copy()), ('obs_frame', tr['obs_frame'] + 100), ('lw', tr['lw'][:-1]),
                     ('agent_ptr', np.concatenate([[0, 0], tr['agent_ptr'][2:]])), ('cat', tr['cat'] + 5)):
        with pytest.raises(ValueError):
            tracks_io.check_tracks(dict(tr, **{key: bad}))
    missing = dict(tr)
    del missing['obs']
    with pytest.raises(ValueError):
        tracks_io.check_tracks(missing)


def test_make_tracks_is_deterministic_and_has_every_pattern():
    a, b = synth.make_tracks(n_scenes=3, n_agents=9, T=20, M=2), synth.make_tracks(n_scenes=3, n_agents=9, T=20, M=2)
    for k in tracks_io.KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert a['scene_map'] == ['synthetic-0', 'synthetic-1', 'synthetic-0'] and a['lw'].shape == (30, 2)
    nobs = np.diff(a['obs_ptr'])[:10]
    assert nobs[0] == 20 and nobs[4] == 1 and nobs[2] < 20 and nobs[3] == 17            # ego, single frame, late, gap
    h = a['obs'][a['obs_ptr'][8]:a['obs_ptr'][9], 2]
    assert h.max() > 3.1 and h.min() < -3.1, 'the heading of the wrap pattern crosses +-pi'
    assert np.diff(a['ego_t'][:20]).min() != np.diff(a['ego_t'][:20]).max(), 'timestamps jitter'


def test_unsupported_arguments_raise(fix):
    tr, env = fixture_tracks(fix), G.fixture_env(True)
    with pytest.raises(NotImplementedError, match='devkit'):
        NuScenesDataset(tr, env, use_challenge_splits=True, device='cpu')
    with pytest.raises(NotImplementedError, match='devkit'):
        NuScenesDataset(tr, env, nusc=object(), device='cpu')
    with pytest.raises(ValueError):
        NuScenesDataset(None, env, device='cpu')
    with pytest.raises(ValueError):
        NuScenesDataset(tr, env, categories=['car', 'tram'], device='cpu')
    with pytest.raises(L.StriveHipError):
        NuScenesDataset(tr, env, device='cpu')                      # a host tensor and the product's library: there is no CPU path
    with pytest.raises(NotImplementedError, match='devkit'):
        NuScenesDataset.get_scenes(object.__new__(NuScenesDataset))  # scene splits by name


# ------------------------------------------------------------------------------------------------
# host emulation of the kernels
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cname', ['c0', 'c1'])
def test_post_process_tables_are_the_references(emu_ops, fix, cname):
    check_tables(fix, cname, tables(dataset(fix, cname, 'cpu')))


@pytest.mark.parametrize('cname', ['c0', 'c1'])
def test_every_window_singly_and_in_batches(emu_ops, fix, cname):
    check_windows(fix, cname, dataset(fix, cname, 'cpu'))


def test_scenario_route(emu_ops, fix):
    ds = dataset(fix, 'sc', 'cpu')
    tb = tables(ds)
    assert np.array_equal(tb['kept'], fix['sc/kept']) and np.array_equal(tb['is_vis'], fix['sc/is_vis'])
    assert_bits(tb['traj'][:, :5], fix['sc/traj'][:, :5], 'sc traj')
    check_windows(fix, 'sc', ds, scenario_float_check)
    assert ds.scene2map['sc_0001_plain'] == ('synthetic-1', 1)


def test_tracks_and_scenarios_together(emu_ops, fix):
    cfg = G.CONFIGS['c0']
    ds = NuScenesDataset(fixture_tracks(fix), G.fixture_env(True), scenario_path=SCEN_DIR, device='cpu')
    n0, n1 = len(fix['c0/seq_start']), len(fix['sc/seq_start'])
    assert len(ds) == n0 + n1 and cfg['seq_interval'] == 1
    g, mi = ds.get_batch([n0 - 1, n0, 0])
    e0, e1 = expected_batch(fix, 'c0', [n0 - 1]), expected_batch(fix, 'sc', [0])
    n = [int(e0['ptr'][-1]), int(e1['ptr'][-1])]
    assert g.ptr.tolist()[:3] == [0, n[0], n[0] + n[1]] and mi.tolist()[:2] == [int(e0['map_idx'][0]), int(e1['map_idx'][0])]
    assert_bits(g.past[:n[0]].numpy(), e0['past'], 'track window beside a scenario window')
    scenario_float_check(g.future[n[0]:n[0] + n[1]].numpy(), e1['future'], 'scenario window beside a track window')


def test_the_egos_stored_category_is_ignored(emu_ops, fix):
    tr = fixture_tracks(fix)
    ds = dataset(fix, 'c0', 'cpu')
    for junk in (99, -3):
        cat = tr['cat'].copy()
        cat[tr['agent_ptr'][:-1]] = junk
        other = NuScenesDataset(dict(tr, cat=cat), G.fixture_env(True), device='cpu')
        assert torch.equal(other.kept, ds.kept)
        check_batch(*other.get_batch([0, 8, 9]), expected_batch(fix, 'c0', [0, 8, 9]), 'ego cat %d' % junk)


def test_a_scene_with_more_agents_than_a_workgroup_has_threads(emu_ops, tmp_path):
    """301 agents: the compaction of strive_dataset_gather_batch takes two passes of 256 and carries its running base over; checked
    against a selection made on the host from the dataset's own tables (which the fixture tests pin).  The scene comes in as a
    scenario file, so that the emulator runs the gather kernel only."""
    import json
    from strive_amd.graph import clique_edge_index
    n, T = 301, 18
    f = np.arange(T, dtype=np.float32)
    st = np.zeros((n, T, 6), dtype=np.float32)
    st[:, :, 0] = 20.0 + 0.5 * np.arange(n)[:, None] + f[None]
    st[:, :, 1] = 4.0 + (np.arange(n) % 7)[:, None]
    st[:, :, 2], st[:, :, 4] = 1.0, 2.0
    st[np.arange(n) % 5 == 2, 3] = np.nan                     # not observed at the last past frame of window 0
    st[np.arange(n) % 7 == 3, 4] = np.nan                     # ... of window 1
    st[0] = np.nan_to_num(st[0], nan=1.0)
    d = {'N': n, 'dt': 0.5, 'map': 'synthetic-0', 'lw': [[4.0 + 0.125 * (a % 5), 2.0] for a in range(n)], 'past': st[:, :4].tolist(),
         'fut_adv': st[:, 4:, :4].tolist(), 'attack_t': 3, 'sem': [[1, 0] if a % 3 else [0, 1] for a in range(n)]}
    with open(str(tmp_path / 'big.json'), 'w') as fh:
        json.dump(d, fh)
    raster, dx = synth.make_raster()
    ds = NuScenesDataset(None, synth.SyntheticMapEnv(raster, dx), scenario_path=str(tmp_path), device='cpu')
    assert len(ds) == 2
    traj, vis = ds.traj.numpy().reshape(n, T, 6), ds.is_vis.numpy().reshape(n, T)
    g, mi = ds.get_batch([1, 0])
    rows = []
    for b, sidx in enumerate((1, 0)):
        sel = [a for a in range(n) if a == 0 or not np.isnan(traj[a, sidx + 3]).any()]
        assert 200 < len(sel) < n and sel[-1] > 256 and any(a > 256 for a in set(range(n)) - set(sel)), 'both passes select and skip'
        assert int(g.ptr[b + 1]) - int(g.ptr[b]) == len(sel)
        e0 = sum(m * (m - 1) for m in rows)
        assert torch.equal(g.edge_index[:, e0:e0 + len(sel) * (len(sel) - 1)], clique_edge_index(len(sel)) + int(g.ptr[b]))
        nodes = slice(int(g.ptr[b]), int(g.ptr[b + 1]))
        want = ds.normalizer.normalize(torch.Tensor(traj[sel, sidx:sidx + 16]))
        assert_bits(g.past[nodes].numpy(), want[:, :4].numpy(), 'past of 301 agents')
        assert_bits(g.future[nodes].numpy(), want[:, 4:].numpy(), 'future of 301 agents')
        assert np.array_equal(g.past_vis[nodes].numpy(), vis[sel, sidx:sidx + 4].astype(np.float32))
        assert_bits(g.lw[nodes].numpy(), ds.veh_att_normalizer.normalize(torch.Tensor(ds._lw_host[sel])).numpy(), 'lw of 301 agents')
        assert np.array_equal(g.sem[nodes].argmax(1).numpy(), ds._cat_host[sel]) and (g.batch[nodes] == b).all()
        rows.append(len(sel))
    assert g.edge_index.shape[1] == sum(m * (m - 1) for m in rows) and mi.tolist() == [0, 0]
    assert len(set(ds._cat_host.tolist())) == 2


def test_loader_behaviour(emu_ops, fix):
    ds = dataset(fix, 'c0', 'cpu')
    N = len(ds)
    gen = torch.Generator().manual_seed(5)
    ld = ds.loader(5, shuffle=True, generator=gen)
    first = [g for g, _ in ld]
    sizes = [g.num_graphs for g in first]
    assert sizes == [5, 5, 2] and len(ld) == 3
    # which windows came: a window is identified by its ego's first past state
    egos = {tuple(ds[i][0].past[0, 0].tolist()): i for i in range(N)}
    order = [egos[tuple(g.past[int(p), 0].tolist())] for g in first for p in g.ptr[:-1]]
    assert sorted(order) == list(range(N)) and order != list(range(N)), 'a permutation of the windows'
    assert order == torch.randperm(N, generator=torch.Generator().manual_seed(5)).tolist()
    second = [g for g, _ in ld]                                      # a second iteration works (and draws a new order)
    assert sum(g.num_graphs for g in second) == N
    dl = ds.loader(5, drop_last=True)
    assert len(dl) == 2 and [g.num_graphs for g, _ in dl] == [5, 5]
    assert [g.num_graphs for g, _ in dl] == [5, 5]


def test_noise_and_reduced_categories(emu_ops, fix):
    ds = dataset(fix, 'c0', 'cpu', noise_std=0.05)
    g, _ = ds.get_batch([0, 8], generator=torch.Generator().manual_seed(1))
    h, _ = ds.get_batch([0, 8], generator=torch.Generator().manual_seed(1))
    assert torch.equal(torch.nan_to_num(g.past), torch.nan_to_num(h.past)), "the caller's generator decides the noise"
    assert not torch.equal(torch.nan_to_num(g.past), torch.nan_to_num(g.past_gt)) and float(g.past[:, :, :2].nan_to_num().min()) >= 0.0
    nrm = torch.norm(g.future[:, :, 2:4], dim=-1)
    assert torch.allclose(nrm[~nrm.isnan()], torch.ones(()), atol=1e-6)
    clean = expected_batch(fix, 'c0', [0, 8])
    assert_bits(g.past_gt.numpy(), clean['past_gt'], 'past_gt carries no noise')
    # the same records with every truck stored as a bus: reduce_cats folds the buses back into trucks (the fixture's windows);
    # without 'bus' among the categories they are not asked for and leave the scenes
    buses = dict(fixture_tracks(fix), categories=['car', 'bus'])
    red = NuScenesDataset(buses, G.fixture_env(True), categories=['car', 'truck', 'bus'], reduce_cats=True, device='cpu')
    assert red.categories == ['car', 'truck'] and len(red) == len(ds)
    check_batch(*red.get_batch([0, 9]), expected_batch(fix, 'c0', [0, 9]), 'reduce_cats')
    no_bus = NuScenesDataset(buses, G.fixture_env(True), categories=['car', 'truck'], device='cpu')
    n_truck = int((fix['tracks/cat'][fix['c0/kept'] == 1] == 1).sum())
    assert n_truck > 0 and int(no_bus.kept.sum()) == int(ds.kept.sum()) - n_truck, 'buses are not asked for'
    assert float(no_bus.get_batch([9])[0].sem[:, 1].sum()) == 0.0


# ------------------------------------------------------------------------------------------------
# MI355X
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('cname', ['c0', 'c1'])
def test_gpu_tables_and_windows(emu, fix, cname):
    ds = dataset(fix, cname, 'cuda')
    tb = tables(ds)
    check_tables(fix, cname, tb)
    orig = (ops._lib_for, L.get_lib)
    ops._lib_for, L.get_lib = (lambda *t: emu), (lambda: emu)
    try:
        ref = tables(dataset(fix, cname, 'cpu'))
    finally:
        ops._lib_for, L.get_lib = orig
    assert np.array_equal(tb['kept'], ref['kept']) and np.array_equal(tb['is_vis'], ref['is_vis'])
    assert_bits(tb['traj'], ref['traj'], 'gpu vs emulator traj')              # every row, the dropped agents' included
    assert_bits(tb['accel'], ref['accel'], 'gpu vs emulator accel')
    check_windows(fix, cname, ds)


@pytest.mark.gpu
def test_gpu_scenario_route(fix):
    ds = dataset(fix, 'sc', 'cuda')
    check_windows(fix, 'sc', ds, scenario_float_check)


@pytest.mark.gpu
def test_gpu_run_one_epoch_on_the_loader():
    """test_traffic.run_one_epoch on ``dataset.loader(4)`` of synth.make_tracks with a random-weight model: the per-batch metrics are
    those of the same windows collated on the host with Batch.from_data_list, and no synchronising call happens while the loader is
    being consumed (torch's synchronisation debug mode set to 'error'): run_one_epoch's one read-back comes after the last batch."""
    from strive_amd import test_traffic as TT
    from strive_amd.losses.traffic_model import TrafficModelLoss
    from util import product_model
    dev = torch.device('cuda', 0)
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(dev)
    ds = NuScenesDataset(synth.make_tracks(n_scenes=2, n_agents=7, T=20), env, device=dev)
    assert len(ds) == 8
    model, _ = product_model(device=dev)
    loss_fn = TrafficModelLoss({'recon': 1.0, 'kl': 1.0, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0}).to(dev)

    class HostLoader(object):
        def __iter__(self):
            for i in range(0, len(ds), 4):
                items = [ds[j] for j in range(i, min(len(ds), i + 4))]
                datas = [d.to('cpu') for d, _ in items]
                yield Batch.from_data_list(datas), torch.tensor([m for _, m in items], dtype=torch.long)

    kw = dict(test_recon_coll_rate=True, test_sample_disp_err=True, test_sample_num=2)
    torch.manual_seed(3)
    rec_host = []
    m_host = TT.run_one_epoch(HostLoader(), model, env, loss_fn, dev, None, per_batch=rec_host, **kw)
    torch.manual_seed(3)
    rec_dev = []

    class Guarded(object):
        """Every synchronising call is an error while the loader is being consumed -- its own batch assembly included; the loader
        ends the guarded region: run_one_epoch's one read-back follows the last batch."""

        def __iter__(self):
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode('error')
            try:
                for item in ds.loader(4):
                    yield item
            finally:
                torch.cuda.set_sync_debug_mode(prev)
    m_dev = TT.run_one_epoch(Guarded(), model, env, loss_fn, dev, None, per_batch=rec_dev, **kw)
    assert torch.cuda.get_sync_debug_mode() == 0
    assert len(rec_host) == len(rec_dev) == 2 and m_host.keys() == m_dev.keys()
    for a, b in zip(rec_host, rec_dev):
        assert a.keys() == b.keys()
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(torch.nan_to_num(a[k].float(), nan=-7.0), torch.nan_to_num(b[k].float(), nan=-7.0)), k
    for k in m_host:
        assert m_host[k] == m_dev[k] or (np.isnan(m_host[k]) and np.isnan(m_dev[k])), k


def test_cli_defaults_are_unchanged(tmp_path):
    """Without ``--scenes`` test_traffic exits with its message as before; eval_traffic_tracks needs a source; eval_planner still asks
    for ``--skip_regular`` or ``--tracks``."""
    from strive_amd import eval_planner as EP
    from strive_amd import eval_traffic_tracks as ET
    from strive_amd import test_traffic as TT
    with pytest.raises(SystemExit, match='the nuScenes loader is not part of strive_amd'):
        TT.main(['--ckpt', 'none'])
    cfg = vars(ET.get_parser().parse_args(['--ckpt', 'none']))
    assert cfg['tracks'] is None and cfg['scenario_path'] is None and cfg['batch_size'] == 8
    with pytest.raises(SystemExit, match='--tracks'):
        ET.tracks_loader(cfg, 'cpu')
    with pytest.raises(SystemExit, match='--scenes does not apply'):
        ET.main(['--ckpt', 'none', '--tracks', 'none', '--scenes', 'synthetic'])
    with pytest.raises(SystemExit, match='--num_classes 3'):
        ET.tracks_loader(dict(cfg, tracks='none', num_classes=3), 'cpu')
    with pytest.raises(SystemExit, match='--tracks FILE'):
        EP.main(['--lane_world', 'synthetic', '--out', str(tmp_path / 'o')])


@pytest.mark.gpu
def test_gpu_command_lines_on_a_tracks_file(tmp_path, capsys):
    """``eval_traffic_tracks --tracks FILE --scenario_path DIR`` and ``eval_planner --tracks FILE`` run end to end."""
    from strive_amd import eval_planner as EP
    from strive_amd import eval_traffic_tracks as ET
    from strive_amd.utils import torch as UT
    from util import product_model
    path = str(tmp_path / 'tracks.npz')
    tracks_io.save_tracks(path, synth.make_tracks(n_scenes=1, n_agents=7, T=19))
    m, _ = product_model()
    ckpt = str(tmp_path / 'ckpt.pth')
    UT.save_state(ckpt, m, torch.optim.Adam(m.parameters(), lr=1e-3), cur_epoch=2)
    out = str(tmp_path / 'out')
    em = ET.main(['--ckpt', ckpt, '--out', out, '--tracks', path, '--scenario_path', SCEN_DIR, '--batch_size', '4',
                  '--test_recon_coll_rate'])
    assert np.isfinite(em['Test Mean pos_err']) and 'Test (recon_, _veh) Collision Freq' in em
    pout = str(tmp_path / 'plan')
    EP.main(['--lane_world', 'synthetic', '--tracks', path, '--out', pout])
    capsys.readouterr()
    assert os.path.exists(os.path.join(pout, 'plan_cfg.json')) and len(os.listdir(pout)) > 1
