"""Latent widths other than 32 (``TrafficModel(latent_size=Z)``, the reference drivers' ``--latent_size``): the library takes Z
from the decoder pack (decoder_net's input width 130 + NC + Z), the launch-per-phase kernels read z / dz with row stride Z, and the
scene-resident kernels run every Z from 1 to 64 (scene_rollout.h: KIN = 5, 6 or 7 k-steps of mlp_in's first layer).

Fixture g15_latent.npz (tests/golden/make_golden_latent.py) holds the reference's own outputs at Z = 16 and 64.  CPU tests run the
kernels on the host emulator (tests/hipemu); the GPU tests run on the MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

import make_golden as mg
from util import golden, assert_close, assert_close_frac
from strive_amd import _lib as L, params, synth
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

RT, AT = 1e-4, 2e-5
FIX = 'g15_latent.npz'
ZS = (16, 64)


def latent_model(Z, device='cpu', FT=12):
    from strive_amd.models.traffic_model import TrafficModel
    from strive_amd.datasets.utils import MeanStdNormalizer
    m = TrafficModel(4, FT, 256, 2, latent_size=Z)
    sd = synth.fill_state_dict(m.state_dict(), key='weights')
    m.load_state_dict(sd)
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m.eval()
    return m.to(device), sd


def latent_oracle(sd, Z, FT=12):
    from oracle.model import OracleTrafficModel
    from oracle.geometry import Normalizer
    return OracleTrafficModel(sd, Normalizer(*state_norm_tensors()), Normalizer(*att_norm_tensors()), NUSC_BIKE_PARAMS, FT=FT,
                              NC=2, z_size=Z)


def fix(Z):
    g = golden(FIX)
    return {k[len('z%d/' % Z):]: g[k] for k in g.files if k.startswith('z%d/' % Z)}


def uniform_env(raster, dx, device='cpu'):
    u = torch.zeros((1,) + tuple(raster.shape[1:]), dtype=torch.uint8)
    u[:, 0] = 1
    return synth.SyntheticMapEnv(u, dx.clone()).to(device)


def _case_kw(batch, case):
    if case.startswith('ft'):
        return {'nfuture': int(case[2:])}
    if case == 'ext':
        return {'ext_future': batch.future_gt[batch.ptr[:-1]][:, :, :4].contiguous()}
    return {}


def _case_z(g, case):
    pmu, pvar = torch.from_numpy(g['prior_mu']), torch.from_numpy(g['prior_var'])
    z = synth.make_latents(pmu, pvar, key='g4/z')
    if case == 'ns':
        z = torch.stack([z, synth.make_latents(pmu, pvar, key='g4/z_b')], dim=1)
    return z


def _gz_tol(gw):
    return 1e-6 + 2e-4 * float(np.abs(gw).max())


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


# ------------------------------------------------------------------------------------------------
# CPU: model, oracle, emulated kernels
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('Z', ZS)
def test_constructor_and_state_dict_match_the_reference(Z):
    m, sd = latent_model(Z)
    g = fix(Z)
    assert m.z_size == Z
    assert list(sd.keys()) == list(g['sd_names'])
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == list(g['sd_shapes'])
    assert tuple(sd['prior_net.mlp_out.net.6.weight'].shape) == (2 * Z, 128)
    assert tuple(sd['decoder_net.mlp_in.net.0.weight'].shape) == (128, 130 + 2 + Z)


def test_constructor_refuses_what_the_kernels_do_not_cover():
    from strive_amd.models.traffic_model import TrafficModel
    for Z in (1, 20, 64):
        assert TrafficModel(4, 12, 256, 2, latent_size=Z).z_size == Z
    for Z in (0, 65, 128):
        with pytest.raises(NotImplementedError, match='latent_size'):
            TrafficModel(4, 12, 256, 2, latent_size=Z)
    for kw in ({'past_feat_size': 32}, {'map_feat_size': 128}, {'future_feat_size': 16}):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            TrafficModel(4, 12, 256, 2, **kw)


@pytest.mark.parametrize('Z', ZS)
@pytest.mark.parametrize('case', ['ft1', 'ft12', 'ext', 'ns'])
def test_oracle_matches_the_reference(Z, case):
    """The CPU oracle (oracle/model.py, z_size=Z) against the reference's decode_embedding and its d/dz (fixture)."""
    g = fix(Z)
    _, sd = latent_model(Z)
    orc = latent_oracle(sd, Z)
    batch, map_idx, raster, dx = mg.g4u_inputs()
    env = synth.SyntheticMapEnv(raster, dx)
    with torch.no_grad():
        emb = orc.embed(batch, map_idx, env)
    assert_close(emb['prior_out'][0], g['prior_mu'], RT, AT, 'oracle prior mean')
    z = _case_z(g, case).requires_grad_(True)
    pred = orc.decode(batch, torch.from_numpy(g['map_feat']), torch.from_numpy(g['past_feat']), z, map_idx, env,
                      **_case_kw(batch, case))
    rw = synth.f32(synth.counter_uniform(tuple(pred.shape), 'g15/r' + case, -1.0, 1.0))
    gz, = torch.autograd.grad((pred * rw).sum(), [z])
    assert_close(pred, g['pred_' + case], RT, AT, 'oracle pred_' + case)
    gw = g['gz_' + case]
    assert_close(gz, gw, 2e-3, _gz_tol(gw), 'oracle gz_' + case)


def _emu_rollout(emu, dec, batch, map_idx, mf, pf, z, FT, ext=None, rw_key='emu/z/rw', fill=0):
    """strive_rollout_fwd + strive_rollout_bwd on the emulator; -> traj (R, FT, 4), dz (R, Z), rw"""
    NA = batch.past.shape[0]
    NS = z.shape[1] if z.dim() == 3 else 1
    R, Z = NA * NS, z.shape[-1]
    sc = params.pack_scenes(batch.ptr, NS, 'cpu')
    tb = emu.query('strive_rollout_tape_bytes', dec.ref(), sc.ref(), FT)
    wb = emu.query('strive_rollout_workspace_bytes', dec.ref(), sc.ref(), FT)
    tape, ws = torch.full((tb,), fill, dtype=torch.uint8), torch.full((wb,), fill, dtype=torch.uint8)
    traj = torch.zeros((R, FT, 4))
    zz = z.detach().reshape(R, Z).contiguous()
    mi = map_idx[batch.batch].int().contiguous()
    lw, sem = batch.lw.contiguous(), batch.sem.contiguous()
    emu.call('strive_rollout_fwd', dec.ref(), sc.ref(), L.ptr(batch.past[:, -1, :].contiguous()), L.ptr(lw), L.ptr(sem),
             L.ptr(pf.contiguous()), L.ptr(mf.contiguous()), L.ptr(zz), L.ptr(mi), L.ptr(ext), FT,
             L.ptr(traj), L.ptr(tape), tb, L.ptr(ws), wb, None)
    rw = synth.f32(synth.counter_uniform((R, FT, 4), rw_key, -1.0, 1.0))
    dz = torch.full((R, Z), float('nan'))
    emu.call('strive_rollout_bwd', dec.ref(), sc.ref(), L.ptr(lw), L.ptr(sem), L.ptr(zz), L.ptr(ext), FT,
             L.ptr(rw), L.ptr(dz), L.ptr(tape), tb, L.ptr(ws), wb, None)
    return traj, dz, rw


def _emu_inputs(sizes, Z, key, NS=1):
    batch, map_idx, raster, dx = mg.build_inputs(sizes, key)
    env = uniform_env(raster, dx)
    NA = batch.past.shape[0]
    mf = synth.f32(synth.counter_uniform((NA, 64), key + '/mf', -1, 1))
    pf = synth.f32(synth.counter_uniform((NA, 64), key + '/pf', -1, 1))
    z = synth.f32(synth.counter_normal((NA, NS, Z) if NS > 1 else (NA, Z), key + '/z'))
    return batch, map_idx, env, mf, pf, z


@pytest.mark.parametrize('Z', [16, 20, 64])
@pytest.mark.parametrize('sizes,FT,NS,ext', [([3, 1, 5], 1, 1, False), ([4, 2], 2, 1, True), ([2, 3], 2, 2, False)])
def test_emulated_phase_kernels_equal_the_oracle(emu, Z, sizes, FT, NS, ext, monkeypatch):
    """The launch-per-phase kernels (option scene_kernels = 0) at latent width Z against autograd of the oracle: forward and d/dz,
    with / without ext_future, NS 1 and 2.  Z = 20 is not a multiple of 16 (no tiling assumption may hide there)."""
    monkeypatch.setenv('STRIVE_SCENE_KERNELS', '0')
    _, sd = latent_model(Z)
    orc = latent_oracle(sd, Z)
    batch, map_idx, env, mf, pf, z = _emu_inputs(sizes, Z, 'emu/lz', NS)
    dec = params.pack_decoder(sd, 2, env, 'cpu', orc.get_normalizer(), orc.get_att_normalizer(), NUSC_BIKE_PARAMS)
    sc = params.pack_scenes(batch.ptr, NS, 'cpu')
    assert emu.query('strive_rollout_scene_resident', dec.ref(), sc.ref()) == 0
    extf = batch.future_gt[batch.ptr[:-1]][:, :FT, :4].contiguous() if ext else None
    traj, dz, rw = _emu_rollout(emu, dec, batch, map_idx, mf, pf, z, FT, extf)
    zg = z.clone().requires_grad_(True)
    pred = orc.decode(batch, mf, pf, zg, map_idx, env, ext_future=extf, nfuture=FT)
    R = batch.past.shape[0] * NS
    gz, = torch.autograd.grad((pred.reshape(R, FT, 4) * rw).sum(), [zg])
    assert_close(traj, pred.detach().reshape(R, FT, 4), 1e-4, 1e-5, 'phase kernels fwd (Z = %d)' % Z)
    assert_close(dz, gz.reshape(R, Z), 2e-3, 1e-6 + 1e-4 * float(gz.abs().max()), 'phase kernels d/dz (Z = %d)' % Z)


@pytest.mark.parametrize('Z', ZS)
@pytest.mark.parametrize('sizes,FT,ext', [([3, 1, 5, 2], 1, False), ([16, 9], 1, True), ([4, 2], 2, True)])
def test_emulated_scene_resident_rollout_equals_the_phase_kernels(emu, Z, sizes, FT, ext, monkeypatch):
    """The scene-resident forward step and reverse sweep (scene_rollout.h, KIN = 5 at Z = 16 and 7 at Z = 64, the latent width
    read at run time) against the launch-per-phase kernels: trajectories to fp32 rounding, d/dz to the rounding of the two
    summation orders; the buffers arrive as NaN bytes.  The stepwise sweep (K workgroups per scene, 16 agents: 4 chunks) gives the
    one-launch sweep's bits."""
    _, sd = latent_model(Z)
    orc = latent_oracle(sd, Z)
    batch, map_idx, env, mf, pf, z = _emu_inputs(sizes, Z, 'emu/lzs')
    dec = params.pack_decoder(sd, 2, env, 'cpu', orc.get_normalizer(), orc.get_att_normalizer(), NUSC_BIKE_PARAMS)
    sc = params.pack_scenes(batch.ptr, 1, 'cpu')
    extf = batch.future_gt[batch.ptr[:-1]][:, :FT, :4].contiguous() if ext else None
    out = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('STRIVE_SCENE_KERNELS', mode)
        assert emu.query('strive_rollout_scene_resident', dec.ref(), sc.ref()) == int(mode)
        out[mode] = _emu_rollout(emu, dec, batch, map_idx, mf, pf, z, FT, extf, fill=0xFF)
    (t0, d0, _), (t1, d1, _) = out['0'], out['1']
    assert torch.isfinite(t1).all() and torch.isfinite(d1).all()
    assert_close(t1, t0, 2e-5, 2e-6, 'scene-resident forward (Z = %d)' % Z)
    assert_close(d1, d0, 1e-3, 2e-5 * float(d0.abs().max()), 'scene-resident sweep (Z = %d)' % Z)
    if max(sizes) >= 12:
        monkeypatch.setenv('STRIVE_SWEEP_STEP', '0')
        _, d_one, _ = _emu_rollout(emu, dec, batch, map_idx, mf, pf, z, FT, extf, fill=0xFF)
        monkeypatch.setenv('STRIVE_SWEEP_STEP', '4')
        _, d_k4, _ = _emu_rollout(emu, dec, batch, map_idx, mf, pf, z, FT, extf, fill=0xFF)
        assert torch.equal(d_k4, d_one), 'stepwise sweep (Z = %d) differs from the one-launch sweep' % Z


@pytest.mark.parametrize('Z', ZS)
def test_emulated_scene_tiles_equal_the_phase_kernels(emu, Z, monkeypatch):
    """Scenes of more than 16 agents: the forward step's node phases on the scene kernel in 16-row tiles (option scene_tiles)
    against the launch-per-phase kernels, at latent width Z."""
    _, sd = latent_model(Z)
    orc = latent_oracle(sd, Z)
    batch, map_idx, env, mf, pf, z = _emu_inputs([19, 2], Z, 'emu/lzt')
    dec = params.pack_decoder(sd, 2, env, 'cpu', orc.get_normalizer(), orc.get_att_normalizer(), NUSC_BIKE_PARAMS)
    sc = params.pack_scenes(batch.ptr, 1, 'cpu')
    extf = batch.future_gt[batch.ptr[:-1]][:, :2, :4].contiguous()
    out = {}
    for tiles in ('0', '1'):
        monkeypatch.setenv('STRIVE_SCENE_TILES', tiles)
        assert emu.query('strive_rollout_scene_resident', dec.ref(), sc.ref()) == (2 if tiles == '1' else 0)
        out[tiles] = _emu_rollout(emu, dec, batch, map_idx, mf, pf, z, 2, extf, fill=0xFF)
    (t0, d0, _), (t1, d1, _) = out['0'], out['1']
    assert torch.isfinite(t1).all() and torch.isfinite(d1).all()
    assert_close(t1, t0, 2e-5, 2e-6, 'scene tiles forward (Z = %d)' % Z)
    assert_close(d1, d0, 1e-3, 2e-5 * float(d0.abs().max()), 'per-phase sweep on the scene tiles\' tape (Z = %d)' % Z)


@pytest.mark.parametrize('Z', [1, 16, 20, 32, 33, 64])
@pytest.mark.parametrize('NC', [2, 8])
def test_scene_resident_for_every_width(emu, Z, NC, monkeypatch):
    """strive_rollout_scene_resident: 1 for scenes of <= 16 agents and 2 (tiles) above, for every latent width 1 .. 64 and
    NC <= 8 (mlp_in's first layer: 5, 6 or 7 k-steps); 0 with option scene_kernels = 0."""
    from strive_amd.models.traffic_model import TrafficModel
    monkeypatch.delenv('STRIVE_SCENE_KERNELS', raising=False)
    monkeypatch.delenv('STRIVE_SCENE_TILES', raising=False)
    m = TrafficModel(4, 12, 256, NC, latent_size=Z)
    sd = synth.fill_state_dict(m.state_dict(), key='weights')
    orc = latent_oracle(sd, Z)
    raster = torch.zeros((1, 4, 64, 64), dtype=torch.uint8)
    env = synth.SyntheticMapEnv(raster, torch.tensor([[0.25, 0.25]], dtype=torch.float64))
    dec = params.pack_decoder(sd, NC, env, 'cpu', orc.get_normalizer(), orc.get_att_normalizer(), NUSC_BIKE_PARAMS)
    assert dec.struct.gnn.mlp_in.dims[0] == 130 + NC + Z
    for ptr, want in (([0, 3, 19], 1), ([0, 20, 23], 2)):
        sc = params.pack_scenes(torch.tensor(ptr), 1, 'cpu')
        assert emu.query('strive_rollout_scene_resident', dec.ref(), sc.ref()) == want, (Z, NC, ptr)
    monkeypatch.setenv('STRIVE_SCENE_KERNELS', '0')
    assert emu.query('strive_rollout_scene_resident', dec.ref(), params.pack_scenes(torch.tensor([0, 3]), 1, 'cpu').ref()) == 0


def test_decoder_pack_key_includes_the_latent_width():
    from strive_amd import ops
    m16, _ = latent_model(16)
    m64, _ = latent_model(64)
    batch, map_idx, raster, dx = mg.g4u_inputs()
    env = synth.SyntheticMapEnv(raster, dx)
    k16 = ops._decoder_pack_key(m16, env, 'cpu')
    k64 = ops._decoder_pack_key(m64, env, 'cpu')
    assert k16 != k64


# ------------------------------------------------------------------------------------------------
# GPU (MI355X)
# ------------------------------------------------------------------------------------------------

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gmodels():
    return {Z: latent_model(Z, device=DEV) for Z in ZS}


@pytest.mark.gpu
@pytest.mark.parametrize('Z', ZS)
@pytest.mark.parametrize('case', ['ft1', 'ft12', 'ft16', 'ext', 'ns'])
def test_gpu_rollout_golden(gmodels, Z, case):
    """decode_embedding and d/dz against the REFERENCE (fixture g15, uniform raster) and the oracle: forward 1e-4 relative /
    2e-5 absolute, d/dz 2e-3 relative."""
    m, sd = gmodels[Z]
    g = fix(Z)
    batch, map_idx, raster, dx = mg.g4u_inputs()
    env = synth.SyntheticMapEnv(raster.clone(), dx.clone()).to(DEV)
    bg = batch.clone().to(DEV)
    with torch.no_grad():
        emb_own = m.embed(bg, map_idx.to(DEV), env)
    assert_close(emb_own['map_feat'], g['map_feat'], RT, AT, 'map_feat')
    assert_close(emb_own['prior_out'][0], g['prior_mu'], RT, AT, 'prior mean')
    emb = {'map_feat': torch.from_numpy(g['map_feat']).to(DEV), 'past_feat': torch.from_numpy(g['past_feat']).to(DEV)}
    zg = _case_z(g, case).to(DEV).requires_grad_(True)
    pred = m.decode_embedding(zg, emb, bg, map_idx.to(DEV), env, **_case_kw(bg, case))['future_pred']
    rw = synth.f32(synth.counter_uniform(tuple(pred.shape), 'g15/r' + case, -1.0, 1.0)).to(DEV)
    (pred * rw).sum().backward()
    assert_close(pred, g['pred_' + case], RT, AT, 'Z %d pred_%s' % (Z, case))
    gw = g['gz_' + case]
    assert_close(zg.grad, gw, 2e-3, _gz_tol(gw), 'Z %d gz_%s' % (Z, case))
    orc = latent_oracle(sd, Z)
    zo = _case_z(g, case).requires_grad_(True)
    po = orc.decode(batch, emb['map_feat'].cpu(), emb['past_feat'].cpu(), zo, map_idx, synth.SyntheticMapEnv(raster, dx),
                    **_case_kw(batch, case))
    (po * rw.cpu()).sum().backward()
    assert_close(pred, po, RT, AT, 'Z %d pred_%s vs the oracle' % (Z, case))
    assert_close(zg.grad, zo.grad, 2e-3, _gz_tol(zo.grad.numpy()), 'Z %d gz_%s vs the oracle' % (Z, case))


@pytest.mark.gpu
@pytest.mark.parametrize('Z', ZS)
def test_gpu_rollout_golden_scene_tiles(gmodels, Z):
    """A batch of a 20-agent and a 3-agent scene (the forward's scene tiles; strive_rollout_scene_resident = 2) against the
    reference.  d/dz of the 20-agent scene passes 12 steps of 380-edge max aggregations: at least 99 % of its entries at the tight
    tolerance (a near-tied arg-max may fall the other way), every entry within 2 % of the largest."""
    m, sd = gmodels[Z]
    g = fix(Z)
    batch, map_idx, raster, dx = mg.build_inputs([20, 3], 'g15/big')
    env = uniform_env(raster, dx, DEV)
    bg = batch.clone().to(DEV)
    dec = params.pack_decoder(sd, 2, env, DEV, m.get_normalizer(), m.get_att_normalizer(), NUSC_BIKE_PARAMS)
    assert L.get_lib().query('strive_rollout_scene_resident', dec.ref(), params.pack_scenes(bg.ptr, 1, DEV).ref()) == 2
    with torch.no_grad():
        emb_own = m.embed(bg, map_idx.to(DEV), env)
    assert_close(emb_own['map_feat'], g['big_map_feat'], RT, AT, 'big map_feat')
    emb = {'map_feat': torch.from_numpy(g['big_map_feat']).to(DEV), 'past_feat': torch.from_numpy(g['big_past_feat']).to(DEV)}
    zg = synth.make_latents(emb_own['prior_out'][0].cpu(), emb_own['prior_out'][1].cpu(), key='g15/big/z').to(DEV)
    zg.requires_grad_(True)
    pred = m.decode_embedding(zg, emb, bg, map_idx.to(DEV), env, nfuture=12)['future_pred']
    rw = synth.f32(synth.counter_uniform(tuple(pred.shape), 'g15/rbig', -1.0, 1.0)).to(DEV)
    (pred * rw).sum().backward()
    assert_close(pred, g['big_pred'], RT, AT, 'Z %d big pred' % Z)
    gw = g['big_gz']
    assert_close(zg.grad[20:], gw[20:], 2e-3, _gz_tol(gw[20:]), 'Z %d big gz (3-agent scene)' % Z)
    scale = float(np.abs(gw[:20]).max())
    assert_close_frac(zg.grad[:20], gw[:20], 2e-3, 2e-4 * scale, 0.99, 2e-2 * scale, 'Z %d big gz (20-agent scene)' % Z)


@pytest.mark.gpu
@pytest.mark.parametrize('Z', ZS)
def test_gpu_sample_batched_golden(gmodels, Z):
    m, sd = gmodels[Z]
    g = fix(Z)
    batch, map_idx, raster, dx = mg.build_inputs([4, 2], 'g7')
    env = uniform_env(raster, dx, DEV)
    NA = batch.past.shape[0]
    eps = synth.f32(synth.counter_normal((3, NA, Z), 'g15/eps')).to(DEV)
    saved = m.rsample
    m.rsample = lambda mean, var: mean + eps * torch.sqrt(var)
    try:
        with torch.no_grad():
            so = m.sample_batched(batch.clone().to(DEV), map_idx.to(DEV), env, 3, include_mean=True, nfuture=8)
    finally:
        m.rsample = saved
    assert so['z_samp'].shape[-1] == Z
    assert_close(so['future_pred'], g['samp_future_pred'], RT, AT, 'sample_batched future_pred')
    assert_close(so['z_samp'], g['samp_z_samp'], RT, AT, 'sample_batched z_samp')
    assert_close(so['z_logprob'], g['samp_z_logprob'], 1e-4, 1e-4, 'sample_batched z_logprob')
    assert_close(so['z_mdist'], g['samp_z_mdist'], 1e-4, 1e-5, 'sample_batched z_mdist')


@pytest.mark.gpu
@pytest.mark.parametrize('Z', ZS)
def test_gpu_training_step_golden_and_all_gradients(Z):
    """One training step (forward(future_sample=True), stacked rollouts, TrafficModelLoss, backward) over the uniform raster:
    loss terms and trajectories against the reference; all 174 gradients as relative L2 errors per tensor against the reference's
    (head entries + norms) and against autograd of the oracle."""
    from test_training import _product_step, TW
    from oracle import losses as ol
    m, sd = latent_model(Z, device=DEV)
    g = fix(Z)
    batch, map_idx, raster, dx = mg.g5_inputs(None, None)
    NA = batch.past.shape[0]
    eps_post = synth.f32(synth.counter_normal((NA, Z), 'g15/eps_post'))
    eps_prior = synth.f32(synth.counter_normal((NA, Z), 'g15/eps_prior'))
    env = uniform_env(raster, dx, DEV)
    out, ld, grads, _ = _product_step(m, batch.clone().to(DEV), map_idx.to(DEV), env, eps_post, eps_prior)
    for key in ('future_pred', 'future_samp'):
        assert_close(out[key], g['train_' + key], RT, AT, 'train ' + key)
    for k in ('loss', 'recon_loss', 'kl_loss', 'coll_veh_prior', 'coll_env_prior'):
        assert_close(ld[k], g['train_' + k], 2e-3, 2e-3 if 'env' in k else 1e-5, 'train ' + k)
    assert int(g['train_ngrads']) == 174 and len(grads) == 174 and all(v is not None for v in grads.values())
    worst_h, worst_n = ('', 0.0), ('', 0.0)
    for n, v in grads.items():
        w = torch.from_numpy(g['train_grad/' + n]).double()
        got = v.detach().cpu().reshape(-1)[:w.numel()].double()
        wn = float(g['train_gnorm/' + n])
        rh = float((got - w).norm() / max(float(w.norm()), 1e-30))
        rn = abs(float(v.double().norm()) - wn) / max(wn, 1e-30)
        worst_h, worst_n = max(worst_h, (n, rh), key=lambda x: x[1]), max(worst_n, (n, rn), key=lambda x: x[1])
        assert rh <= 1e-2 and rn <= 1e-2, 'reference gradient %s: head relative L2 %.3g, norm %.3g' % (n, rh, rn)
    print('Z %d training step vs the reference: worst head %s %.3g, worst norm %s %.3g' % ((Z,) + worst_h + worst_n))
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    orc = latent_oracle(sdg, Z)
    env_c = uniform_env(raster, dx)
    oo = orc.forward(batch, map_idx, env_c, eps_post=eps_post, eps_prior=eps_prior)
    ol_d = ol.traffic_model_loss(TW, batch, oo, orc.get_normalizer(), orc.get_att_normalizer(), map_idx, env_c)
    ol_d['loss'].sum().backward()
    want = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items()}
    worst = ('', 0.0)
    for n, w in want.items():
        r = float((grads[n].detach().cpu().double() - w.double()).norm() / max(float(w.double().norm()), 1e-30))
        worst = max(worst, (n, r), key=lambda x: x[1])
    print('Z %d training step: worst gradient vs the oracle %s %.3g (relative L2)' % ((Z,) + worst))
    assert worst[1] <= 2e-3, 'gradient %s vs the oracle: relative L2 %.3g' % worst


@pytest.mark.gpu
@pytest.mark.parametrize('Z', ZS)
def test_gpu_fused_losses_golden(gmodels, Z):
    """AvoidCollLoss and AdvGenLoss (fused loss kernels, D = Z) on the decodes of the g5 batch against the reference: every loss
    term, the trajectories and d(loss)/dz through the rollout."""
    from strive_amd.losses.adv_gen_nusc import AvoidCollLoss, AdvGenLoss
    from strive_amd.utils.adv_gen_optim import collate_tgt_other_z
    m, sd = gmodels[Z]
    g = fix(Z)
    batch, map_idx, raster, dx = mg.g5_inputs(None, None)
    env = uniform_env(raster, dx, DEV)
    bg, mi = batch.clone().to(DEV), map_idx.to(DEV)
    with torch.no_grad():
        emb = m.embed(bg, mi, env)
    emb = {k: (tuple(t.detach() for t in v) if isinstance(v, tuple) else v.detach()) for k, v in emb.items()}
    NA = bg.past.shape[0]
    ego = torch.zeros((NA,), dtype=torch.bool, device=DEV)
    ego[bg.ptr[:-1]] = True
    nu = m.get_normalizer().unnormalize
    veh_att = m.get_att_normalizer().unnormalize(bg.lw)
    mapixes = mi[bg.batch]
    prior = emb['prior_out']
    z0 = synth.make_latents(prior[0].cpu(), prior[1].cpu(), key='g5/z').to(DEV)

    z = z0.clone().requires_grad_(True)
    pred = m.decode_embedding(z, emb, bg, mi, env, nfuture=16)['future_pred']
    ld = AvoidCollLoss(mg.REFINE_WEIGHTS, veh_att, mapixes, env, z0.clone() * 0.9, veh_coll_buffer=0.2)(nu(pred), z, prior)
    ld['loss'].backward()
    assert_close(pred, g['avoid_pred'], RT, AT, 'Z %d avoid pred' % Z)
    for k, v in ld.items():
        assert_close(v, g['avoid_' + k], 2e-3, 2e-3 if 'env' in k else 1e-4, 'Z %d AvoidCollLoss %s' % (Z, k))
    assert_close(z.grad, g['avoid_gz'], 2e-3, _gz_tol(g['avoid_gz']), 'Z %d AvoidCollLoss d/dz' % Z)

    other_z = z0[~ego].clone().requires_grad_(True)
    zc = collate_tgt_other_z(bg, z0[ego].clone(), other_z)
    planner = bg.future_gt[ego][:, :, :4]
    pred = m.decode_embedding(zc, emb, bg, mi, env, ext_future=planner)['future_pred']
    lf = AdvGenLoss(mg.ADV_WEIGHTS, veh_att, mapixes, env, other_z.detach().clone() * 0.9, bg.ptr, veh_coll_buffer=0.1,
                    crash_loss_min_time=2, crash_loss_min_infront=0.0)
    ld = lf(nu(pred), nu(planner), other_z, (prior[0][~ego], prior[1][~ego]))
    ld['loss'].backward()
    assert_close(pred, g['adv_pred'], RT, AT, 'Z %d adv pred' % Z)
    for k, v in ld.items():
        assert_close(v, g['adv_' + k], 2e-3, 2e-3 if 'env' in k else 2e-4, 'Z %d AdvGenLoss %s' % (Z, k))
    assert_close(other_z.grad, g['adv_gz'], 2e-3, _gz_tol(g['adv_gz']), 'Z %d AdvGenLoss d/dz' % Z)


def _refine_inputs():
    batch, map_idx, _, _ = mg.build_inputs(mg.G12_SIZES, 'g12', window=14.0)
    raster, dx = mg.loop_rasters('u')
    eps = synth.f32(synth.counter_normal((1, batch.past.shape[0], 16), 'g15/refine_eps'))
    return batch, map_idx, raster, dx, eps


@pytest.mark.gpu
def test_gpu_refine_function_golden(gmodels):
    """strive_amd.refine_traffic_optim at Z = 16 (prior sample injected, Adam, 3 iterations) against the reference's own
    function (fixture g15, uniform raster): the tolerances of test_loops.test_refine_function_matches_the_reference_function."""
    from strive_amd.refine_traffic_optim import refine_traffic_optim
    m, sd = gmodels[16]
    g = fix(16)
    batch, map_idx, raster, dx, eps = _refine_inputs()
    env = synth.SyntheticMapEnv(raster.clone(), dx.clone()).to(DEV)
    saved = m.rsample
    try:
        m.rsample = lambda mean, var: mean + eps.to(mean.device) * torch.sqrt(var)
        init_pred, z, res, _ = refine_traffic_optim(batch.clone().to(DEV), map_idx.to(DEV), env, m, mg.REFINE_WEIGHTS, 3, 6, 6,
                                                    True, 0.05)
    finally:
        m.rsample = saved
    assert z.shape[-1] == 16
    assert_close(init_pred, g['refine/init_future_pred'], 1e-4, 2e-5, 'refine init_future_pred')
    frac = float(np.mean(np.abs(z.detach().cpu().numpy() - g['refine/z']) <= 2e-3))
    assert frac >= 0.97, 'only %.3f of the latent entries within 2e-3' % frac
    assert_close(res, g['refine/result_traj'], 0, 5e-3, 'refine result_traj')


@pytest.mark.gpu
@pytest.mark.parametrize('Z', ZS)
def test_gpu_refine_loop_graph_replay_equals_eager(gmodels, Z, monkeypatch):
    """The refine closure at the headline size (32 x 16 agents, FT 16: the scene-resident kernels) at latent width Z: finite, and
    replayed as a HIP graph it gives what the eager iterations give (max abs 0.0)."""
    from strive_amd.refine_traffic_optim import refine_traffic_optim
    from strive_amd.utils import graphed as gmod
    import strive_amd.refine_traffic_optim as rmod
    m, sd = gmodels[Z]
    monkeypatch.setattr(gmod, 'adam_kwargs', lambda graphed: {'capturable': True})
    monkeypatch.setattr(rmod, 'adam_kwargs', lambda graphed: {'capturable': True})
    batch, map_idx = synth.make_batch([16] * 32, key='gc/graph', map_extent=(512.0, 512.0))
    raster = torch.zeros((1, 4, 4096, 4096), dtype=torch.uint8)
    raster[:, 0] = 1
    env = synth.SyntheticMapEnv(raster, torch.tensor([[0.25, 0.25]], dtype=torch.float64)).to(DEV)
    with torch.no_grad():
        emb = m.embed(batch.clone().to(DEV), map_idx.to(DEV), env)
    z0 = synth.make_latents(emb['prior_out'][0].cpu(), emb['prior_out'][1].cpu(), key='gc/graph/z')
    dec = params.pack_decoder(sd, 2, env, DEV, m.get_normalizer(), m.get_att_normalizer(), NUSC_BIKE_PARAMS)
    assert L.get_lib().query('strive_rollout_scene_resident', dec.ref(), params.pack_scenes(batch.ptr, 1, DEV).ref()) == 1

    def run(graph):
        monkeypatch.setenv('STRIVE_HIP_GRAPH', '1' if graph else '0')
        _, z, final, _ = refine_traffic_optim(batch.clone().to(DEV), map_idx.to(DEV), env, m, mg.REFINE_WEIGHTS, 8, 16, 16, True,
                                              0.05, z_init=z0.clone().to(DEV))
        return z.detach().cpu().clone(), z.grad.detach().cpu().clone(), final.detach().cpu()
    zg, gg, fg = run(True)
    ze, ge, fe = run(False)
    for t in (zg, gg, fg):
        assert torch.isfinite(t).all()
    assert float((zg - z0).abs().max()) > 1e-3, 'the iterations moved the latents'
    d = max(float((zg - ze).abs().max()), float((gg - ge).abs().max()), float((fg - fe).abs().max()))
    print('Z %d refine loop, graph replay vs eager: max abs %.3g' % (Z, d))
    assert d == 0.0, 'graph replay vs eager: %.3g apart' % d


@pytest.mark.gpu
def test_gpu_dropin_adversarial_closure_at_latent_size_16():
    """Through dropin.install(): the reference's import names build TrafficModel(latent_size=16) (what the drivers do for
    --latent_size 16), and one adversarial closure -- decode with the planner's future, AdvGenLoss, backward -- gives the
    reference's loss terms and d/dz (fixture g15)."""
    from test_dropin_reference import _names_installed
    g = fix(16)
    with _names_installed():
        from models.traffic_model import TrafficModel
        from datasets.utils import MeanStdNormalizer
        from losses.adv_gen_nusc import AdvGenLoss
        from utils.adv_gen_optim import collate_tgt_other_z
        from utils.scenario_gen import detach_embed_info
        m = TrafficModel(4, 12, 256, 2, latent_size=16)
        m.load_state_dict(synth.fill_state_dict(m.state_dict(), key='weights'))
        m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
        m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
        m.set_bicycle_params(NUSC_BIKE_PARAMS)
        m = m.eval().to(DEV)
        batch, map_idx, raster, dx = mg.g5_inputs(None, None)
        env = uniform_env(raster, dx, DEV)
        bg, mi = batch.clone().to(DEV), map_idx.to(DEV)
        with torch.no_grad():
            emb = detach_embed_info(m.embed(bg, mi, env))
        NA = bg.past.shape[0]
        ego = torch.zeros((NA,), dtype=torch.bool, device=DEV)
        ego[bg.ptr[:-1]] = True
        prior = emb['prior_out']
        z0 = synth.make_latents(prior[0].cpu(), prior[1].cpu(), key='g5/z').to(DEV)
        other_z = z0[~ego].clone().requires_grad_(True)
        zc = collate_tgt_other_z(bg, z0[ego].clone(), other_z)
        planner = bg.future_gt[ego][:, :, :4]
        pred = m.decode_embedding(zc, emb, bg, mi, env, ext_future=planner)['future_pred']
        nu = m.get_normalizer().unnormalize
        lf = AdvGenLoss(mg.ADV_WEIGHTS, m.get_att_normalizer().unnormalize(bg.lw), mi[bg.batch], env, other_z.detach().clone() * 0.9,
                        bg.ptr, veh_coll_buffer=0.1, crash_loss_min_time=2, crash_loss_min_infront=0.0)
        ld = lf(nu(pred), nu(planner), other_z, (prior[0][~ego], prior[1][~ego]))
        ld['loss'].backward()
    assert_close(pred, g['adv_pred'], RT, AT, 'drop-in adv pred')
    for k, v in ld.items():
        assert_close(v, g['adv_' + k], 2e-3, 2e-3 if 'env' in k else 2e-4, 'drop-in AdvGenLoss %s' % k)
    assert_close(other_z.grad, g['adv_gz'], 2e-3, _gz_tol(g['adv_gz']), 'drop-in AdvGenLoss d/dz')
