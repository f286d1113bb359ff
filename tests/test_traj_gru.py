"""The GRU trajectory encoders (``TrafficModel(traj_encoder='gru')``, reference src/models/traffic_model.py:93-119, 453-523): each
encoder call is ONE launch of csrc/traj_gru.hip over all frames and all 4 layers, rows in tiles of 16; the training step keeps the
gates and states and runs strive_traj_gru_bwd.

Fixture g16_gru.npz (tests/golden/make_golden_gru.py) holds the reference's own outputs; tests/gru_oracle.py restates the two
encoders from the equations (float32 / float64, autograd).  CPU tests run the kernels on the host emulator (tests/hipemu); the GPU
tests run on the MI355X.

Tolerances: features and trajectories rtol 1e-4 / atol 2e-5 (the reference's own fp32 encoders sit 3.5e-8 / 6.4e-8 from a float64
evaluation, the features are 0.14 to 0.26 in size); the 18 gradient tensors of an encoder relative L2 <= 1e-4 per tensor against
float64 autograd of the restatement (the bound of tests/test_training.py on the uniform raster); d/dz and the training step against
the fixture as tests/test_latent_size.py bounds its own cases of the same shape."""
import os
import sys

import numpy as np
import pytest
import torch

import make_golden as mg
import gru_oracle as go
from util import golden, assert_close
from strive_amd import _lib as L, params, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

RT, AT = 1e-4, 2e-5
GRAD_L2 = 1e-4
FIX = 'g16_gru.npz'
TILE = 16                       # rows per workgroup of traj_gru.hip: NA 1 / 9 / 17 = one row, a partial tile, one row past a tile
DEV = 'cuda:0'


def uniform_env(raster, dx, device='cpu'):
    u = torch.zeros((1,) + tuple(raster.shape[1:]), dtype=torch.uint8)
    u[:, 0] = 1
    return synth.SyntheticMapEnv(u, dx.clone()).to(device)


def _gz_tol(gw):
    return 1e-6 + 2e-4 * float(np.abs(gw).max())


def _embed_inputs(tag):
    if tag == 'g4u':
        batch, map_idx, raster, dx = mg.g4u_inputs()
    elif tag == 'big':
        batch, map_idx, raster, dx = mg.build_inputs([20, 3], 'g15/big')
    else:
        batch, map_idx, raster, dx = mg.build_inputs(mg.G4B_SIZES, 'g4b', NC=5)
    return go.with_gaps(batch), map_idx, raster, dx


def _model_args(tag):
    return (5, 'weights5') if tag == 'nc5' else (2, 'weights')


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    return L.StriveLib(emu_build.build(), require_all=True)


@pytest.fixture(scope='module')
def raw():
    """Inputs of the raw-kernel tests, built once: the state dicts of the NC = 2 and NC = 5 models (input widths 11 and 14) and the
    assembled sequences of a 9 + 8 agent batch with visibility gaps: T = 4 the past, T = 12 the future, T = 1 its first frame."""
    out = {}
    for NC, key in ((2, 'weights'), (5, 'weights5')):
        _, sd = go.gru_product_model(NC=NC, key=key)
        batch, _ = synth.make_batch([9, 8], key='gru/raw%d' % NC, NC=NC)
        go.with_gaps(batch)
        batch.future_vis[5, :] = 0.0
        b = batch
        xs = {4: go.encoder_input(b.past, b.past, b.past_vis, b.lw, b.sem),
              12: go.encoder_input(b.past, b.future, b.future_vis, b.lw, b.sem)}
        xs[1] = xs[12][:, :1].contiguous()
        assert xs[4].shape == (17, 4, NC + 9) and float((xs[12][:, :, 6] == 0).sum()) > 12
        out[NC + 9] = (sd, xs)
    return out


def _enc_of(T):
    return ('past_encoder', 'past_out_layer') if T == 4 else ('future_encoder', 'future_out_layer')


def _pack(sd, T, device='cpu'):
    enc, outl = _enc_of(T)
    return params.pack_traj_gru({k: v.to(device) for k, v in sd.items() if k.startswith((enc, outl))}, enc, outl)


def _ref64(sd, T, x, d_feat=None):
    enc, outl = _enc_of(T)
    names, ps = go.gru_params(sd, enc, outl, torch.float64, d_feat is not None)
    feat = go.gru_features(ps, x.double())
    if d_feat is None:
        return feat.detach()
    return feat.detach(), names, torch.autograd.grad((feat * d_feat.double()).sum(), ps)


def _lib_fwd(lib, pk, x, keep=False):
    NA, T, _ = x.shape
    feat = torch.full((NA, 64), float('nan'), device=x.device)
    if not keep:
        lib.call('strive_traj_gru_fwd', pk.ref(), L.ptr(x), NA, T, L.ptr(feat), L.stream_ptr(x))
        return feat
    kb = lib.query('strive_traj_gru_keep_bytes', pk.ref(), NA, T)
    kept = torch.full((kb,), 0xFF, dtype=torch.uint8, device=x.device)
    lib.call('strive_traj_gru_fwd_keep', pk.ref(), L.ptr(x), NA, T, L.ptr(feat), L.ptr(kept), kb, L.stream_ptr(x))
    return feat, kept


def _lib_bwd(lib, pk, x, kept, d_feat):
    NA, T, _ = x.shape
    n = lib.query('strive_traj_gru_param_count', pk.ref())
    dp = torch.zeros((n,), device=x.device)
    lib.call('strive_traj_gru_bwd', pk.ref(), NA, T, L.ptr(kept), kept.numel(), L.ptr(d_feat), L.ptr(dp), L.stream_ptr(x))
    return dp


def _check_grads(dp, names, want, what):
    off, worst = 0, ('', 0.0)
    for n, w in zip(names, want):
        got = dp[off:off + w.numel()].detach().cpu().double().view(w.shape)
        off += w.numel()
        rel = float((got - w).norm() / max(float(w.norm()), 1e-30))
        worst = max(worst, (n, rel), key=lambda e: e[1])
    assert off == dp.numel()
    print('%s: worst gradient %s relative L2 %.3g' % ((what,) + worst))
    assert worst[1] <= GRAD_L2, '%s: gradient %s relative L2 %.3g' % ((what,) + worst)


# ------------------------------------------------------------------------------------------------
# CPU: model, restatement, emulated kernels
# ------------------------------------------------------------------------------------------------

def test_constructor_and_state_dict_match_the_reference():
    from strive_amd.models.traffic_model import TrafficModel
    m, sd = go.gru_product_model()
    g = golden(FIX)
    assert m.traj_encoder_type == 'gru' and m.past_in_size == m.future_in_size == 11
    assert len(sd) == 182 and list(sd.keys()) == list(g['sd_names'])
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == list(g['sd_shapes'])
    TrafficModel(4, 12, 256, 2, traj_encoder='gru').load_state_dict(sd)
    with pytest.raises(NotImplementedError, match='output_bicycle'):
        TrafficModel(4, 12, 256, 2, traj_encoder='gru', output_bicycle=False)
    with pytest.raises(NotImplementedError, match='traj_encoder'):
        TrafficModel(4, 12, 256, 2, traj_encoder='lstm')
    assert len(TrafficModel(4, 12, 256, 2).state_dict()) == 174


@pytest.mark.parametrize('tag', ['g4u', 'big', 'nc5'])
def test_restatement_matches_the_reference(tag):
    g = golden(FIX)
    NC, key = _model_args(tag)
    _, sd = go.gru_product_model(NC=NC, key=key)
    batch = _embed_inputs(tag)[0]
    for which in ('past', 'future'):
        for dt in (torch.float32, torch.float64):
            assert_close(go.encode(sd, which, batch, dt), g['%s_%s_feat' % (tag, which)], RT, AT, '%s %s_feat %s' % (tag, which, dt))


@pytest.fixture(scope='module')
def emu_runs(emu, raw):
    """plain forward, kept forward and the float64 restatement of every raw case, computed once"""
    runs = {}
    for W in (11, 14):
        sd, xs = raw[W]
        for T in (1, 4, 12):
            pk = _pack(sd, T)
            want = _ref64(sd, T, xs[T])
            for NA in (1, 9, 17):
                if W == 14 and (NA, T) not in ((17, 4), (9, 12)):
                    continue                      # the second input width adds nothing per shape: a past and a future case
                x = xs[T][:NA].contiguous()
                feat = _lib_fwd(emu, pk, x)
                fk, kept = _lib_fwd(emu, pk, x, keep=True)
                runs[(W, NA, T)] = (pk, x, feat, fk, kept, want[:NA])
    return runs


@pytest.mark.parametrize('W,NA,T', [(11, NA, T) for NA in (1, 9, 17) for T in (1, 4, 12)] + [(14, 17, 4), (14, 9, 12)])
def test_emulated_forward_equals_the_restatement(emu_runs, W, NA, T):
    pk, x, feat, fk, kept, want = emu_runs[(W, NA, T)]
    assert bool(torch.isfinite(feat).all())
    assert_close(feat, want, RT, AT, 'emulated strive_traj_gru_fwd W %d NA %d T %d' % (W, NA, T))
    assert torch.equal(fk, feat), 'the kept forward returns the plain forward\'s bytes'


@pytest.mark.parametrize('T', [1, 4, 12])
def test_rows_do_not_depend_on_the_batch(emu_runs, T):
    assert torch.equal(emu_runs[(11, 17, T)][2][:9], emu_runs[(11, 9, T)][2])
    assert torch.equal(emu_runs[(11, 9, T)][2][:1], emu_runs[(11, 1, T)][2])


@pytest.mark.parametrize('W,NA,T', [(11, 9, 1), (11, 17, 1), (11, 9, 12), (11, 17, 12), (14, 17, 4)])
def test_emulated_backward_equals_autograd_of_the_restatement(emu, raw, emu_runs, W, NA, T):
    pk, x, feat, fk, kept, _ = emu_runs[(W, NA, T)]
    d_feat = synth.f32(synth.counter_uniform((NA, 64), 'gru/dfeat', -1.0, 1.0))
    dp = _lib_bwd(emu, pk, x, kept.clone(), d_feat)
    _, names, want = _ref64(raw[W][0], T, x, d_feat)
    assert len(want) == 18
    _check_grads(dp, names, want, 'emulated strive_traj_gru_bwd W %d NA %d T %d' % (W, NA, T))
    # d_params is accumulated into
    dp2 = torch.ones_like(dp)
    emu.call('strive_traj_gru_bwd', pk.ref(), NA, T, L.ptr(kept.clone()), kept.numel(), L.ptr(d_feat), L.ptr(dp2), None)
    assert_close(dp2 - 1.0, dp, 0, 1e-6 * max(1.0, float(dp.abs().max())), 'accumulation')


def test_refusals(emu, raw):
    sd, xs = raw[11]
    pk = _pack(sd, 4)
    feat = torch.full((17, 64), 7.0)
    with pytest.raises(L.StriveHipError, match='T = 0'):
        emu.call('strive_traj_gru_fwd', pk.ref(), L.ptr(xs[4]), 17, 0, L.ptr(feat), None)
    pk.struct.in_size = 33
    with pytest.raises(L.StriveHipError, match='input width 33'):
        emu.call('strive_traj_gru_fwd', pk.ref(), L.ptr(xs[4]), 17, 4, L.ptr(feat), None)
    with pytest.raises(L.StriveHipError, match='input width 33'):
        emu.call('strive_traj_gru_bwd', pk.ref(), 17, 4, L.ptr(feat), 0, L.ptr(feat), L.ptr(feat), None)
    assert float(feat.min()) == 7.0, 'nothing was launched'
    sd33 = {k: v for k, v in sd.items() if k.startswith('past_')}
    sd33['past_encoder.weight_ih_l0'] = torch.zeros((384, 33))
    with pytest.raises(NotImplementedError, match='input width 33'):
        params.pack_traj_gru(sd33, 'past_encoder', 'past_out_layer')
    from strive_amd.models.traffic_model import TrafficModel
    with pytest.raises(NotImplementedError, match='32 inputs'):
        TrafficModel(4, 12, 256, 24, traj_encoder='gru')


def test_model_encoders_on_the_emulator_match_the_reference(emu, monkeypatch):
    """encode_past / encode_future of the model itself (input assembly, pack, the pack cache) with the emulated library in the
    product library's place, against the reference's features; a changed parameter rebuilds the pack."""
    from strive_amd import ops
    monkeypatch.setattr(ops, '_lib_for', lambda *tensors: emu)
    monkeypatch.setattr(L, 'get_lib', lambda: emu)
    g = golden(FIX)
    m, sd = go.gru_product_model()
    batch = _embed_inputs('g4u')[0]
    with torch.no_grad():
        pf, ff = m.encode_past(batch), m.encode_future(batch)
    assert pf.shape == (9, 64) and ff.shape == (9, 64)
    assert_close(pf, g['g4u_past_feat'], RT, AT, 'past_feat')
    assert_close(ff, g['g4u_future_feat'], RT, AT, 'future_feat')
    pk = ops.traj_gru_pack(m, 'past')
    assert ops.traj_gru_pack(m, 'past') is pk
    with torch.no_grad():
        m.past_out_layer.bias.add_(1.0)
        assert ops.traj_gru_pack(m, 'past') is not pk
        assert_close(m.encode_past(batch), g['g4u_past_feat'] + 1.0, RT, AT, 'past_feat after an in-place parameter update')


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('NA,T', [(1, 1), (17, 12)])
def test_gpu_raw_forward_and_backward(raw, NA, T):
    sd, xs = raw[11]
    lib = L.get_lib()
    pk = _pack(sd, T, DEV)
    x = xs[T][:NA].contiguous().to(DEV)
    feat = _lib_fwd(lib, pk, x)
    fk, kept = _lib_fwd(lib, pk, x, keep=True)
    d_feat = synth.f32(synth.counter_uniform((NA, 64), 'gru/dfeat', -1.0, 1.0))
    dp = _lib_bwd(lib, pk, x, kept, d_feat.to(DEV))
    want, names, gw = _ref64(sd, T, xs[T][:NA], d_feat)
    assert_close(feat, want, RT, AT, 'strive_traj_gru_fwd NA %d T %d' % (NA, T))
    assert torch.equal(fk, feat)
    _check_grads(dp, names, gw, 'strive_traj_gru_bwd NA %d T %d' % (NA, T))


@pytest.fixture(scope='module')
def gmodel():
    return go.gru_product_model(device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['g4u', 'big', 'nc5'])
def test_gpu_embed_golden(gmodel, tag):
    g = golden(FIX)
    NC, key = _model_args(tag)
    m = gmodel[0] if NC == 2 else go.gru_product_model(NC=NC, key=key, device=DEV)[0]
    batch, map_idx, raster, dx = _embed_inputs(tag)
    env = uniform_env(raster, dx, DEV)
    with torch.no_grad():
        emb = m.embed(batch.clone().to(DEV), map_idx.to(DEV), env)
        ff = m.encode_future(batch.clone().to(DEV))
    assert_close(emb['past_feat'], g[tag + '_past_feat'], RT, AT, tag + ' past_feat')
    assert_close(ff, g[tag + '_future_feat'], RT, AT, tag + ' future_feat')
    assert_close(emb['map_feat'], g[tag + '_map_feat'], RT, AT, tag + ' map_feat')
    for k, i, n in (('prior_out', 0, 'prior_mu'), ('prior_out', 1, 'prior_var'), ('posterior_out', 0, 'post_mu'), ('posterior_out', 1, 'post_var')):
        assert_close(emb[k][i], g['%s_%s' % (tag, n)], RT, AT, '%s %s' % (tag, n))


@pytest.mark.gpu
def test_gpu_decode_embedding_golden(gmodel):
    m, sd = gmodel
    g = golden(FIX)
    batch, map_idx, raster, dx = _embed_inputs('g4u')
    env = uniform_env(raster, dx, DEV)
    bg = batch.clone().to(DEV)
    with torch.no_grad():
        emb = m.embed(bg, map_idx.to(DEV), env)
    z = synth.make_latents(torch.from_numpy(g['g4u_prior_mu']), torch.from_numpy(g['g4u_prior_var']), key='g4/z').to(DEV).requires_grad_(True)
    pred = m.decode_embedding(z, {'map_feat': emb['map_feat'], 'past_feat': emb['past_feat']}, bg, map_idx.to(DEV), env, nfuture=12)['future_pred']
    rw = synth.f32(synth.counter_uniform(tuple(pred.shape), 'g16/rft12', -1.0, 1.0)).to(DEV)
    (pred * rw).sum().backward()
    assert_close(pred, g['pred_ft12'], RT, AT, 'pred_ft12')
    assert_close(z.grad, g['gz_ft12'], 2e-3, _gz_tol(g['gz_ft12']), 'gz_ft12')


@pytest.mark.gpu
def test_gpu_sample_batched_golden(gmodel):
    m, sd = gmodel
    g = golden(FIX)
    batch, map_idx, raster, dx = mg.build_inputs([4, 2], 'g7')
    go.with_gaps(batch)
    env = uniform_env(raster, dx, DEV)
    eps = synth.f32(synth.counter_normal((3, batch.past.shape[0], 32), 'g16/eps')).to(DEV)
    saved = m.rsample
    m.rsample = lambda mean, var: mean + eps * torch.sqrt(var)
    try:
        with torch.no_grad():
            so = m.sample_batched(batch.clone().to(DEV), map_idx.to(DEV), env, 3, include_mean=True, nfuture=8)
    finally:
        m.rsample = saved
    assert_close(so['future_pred'], g['samp_future_pred'], RT, AT, 'sample_batched future_pred')
    assert_close(so['z_samp'], g['samp_z_samp'], RT, AT, 'sample_batched z_samp')
    assert_close(so['z_logprob'], g['samp_z_logprob'], 1e-4, 1e-4, 'sample_batched z_logprob')
    assert_close(so['z_mdist'], g['samp_z_mdist'], 1e-4, 1e-5, 'sample_batched z_mdist')


@pytest.mark.gpu
def test_gpu_training_step_golden_and_all_gradients(monkeypatch):
    """One training step over the uniform raster: loss terms and trajectories against the reference; all 182 gradients against the
    reference's (head entries + norms) and against autograd of the oracle with the restated encoders (the bounds of
    tests/test_latent_size.py); and the 36 tensors of the two encoders, given the adjoints of past_feat / future_feat that reached
    them, against float64 autograd of the restatement at relative L2 1e-4."""
    from test_training import _product_step, TW
    from oracle import losses as ol
    from strive_amd import ops
    m, sd = go.gru_product_model(device=DEV)
    g = golden(FIX)
    batch, map_idx, raster, dx = mg.g5_inputs(None, None)
    go.with_gaps(batch)
    NA = batch.past.shape[0]
    eps_post = synth.f32(synth.counter_normal((NA, 32), 'g16/eps_post'))
    eps_prior = synth.f32(synth.counter_normal((NA, 32), 'g16/eps_prior'))
    env = uniform_env(raster, dx, DEV)
    seen = {}
    orig = ops.encode_traj_gru

    def spy(model, which, gg, traj, vis):
        feat = orig(model, which, gg, traj, vis)
        feat.register_hook(lambda d, which=which: seen.__setitem__(which, d.detach().cpu().clone()))
        return feat
    monkeypatch.setattr(ops, 'encode_traj_gru', spy)
    out, ld, grads, _ = _product_step(m, batch.clone().to(DEV), map_idx.to(DEV), env, eps_post, eps_prior)
    for key in ('future_pred', 'future_samp'):
        assert_close(out[key], g['train_' + key], RT, AT, 'train ' + key)
    for k in ('loss', 'recon_loss', 'kl_loss', 'coll_veh_prior', 'coll_env_prior'):
        assert_close(ld[k], g['train_' + k], 2e-3, 2e-3 if 'env' in k else 1e-5, 'train ' + k)
    assert int(g['train_ngrads']) == 182 and len(grads) == 182 and all(v is not None for v in grads.values())
    for n, v in grads.items():
        w = torch.from_numpy(g['train_grad/' + n]).double()
        got = v.detach().cpu().reshape(-1)[:w.numel()].double()
        wn = float(g['train_gnorm/' + n])
        rh = float((got - w).norm() / max(float(w.norm()), 1e-30))
        rn = abs(float(v.double().norm()) - wn) / max(wn, 1e-30)
        assert rh <= 1e-2 and rn <= 1e-2, 'reference gradient %s: head relative L2 %.3g, norm %.3g' % (n, rh, rn)
    # the two encoders alone, float64
    assert set(seen) == {'past', 'future'}
    for which in ('past', 'future'):
        traj, vis = (batch.past, batch.past_vis) if which == 'past' else (batch.future, batch.future_vis)
        x = go.encoder_input(batch.past.double(), traj.double(), vis.double(), batch.lw.double(), batch.sem.double())
        names, ps = go.gru_params(sd, which + '_encoder', which + '_out_layer', torch.float64, True)
        want = torch.autograd.grad((go.gru_features(ps, x) * seen[which].double()).sum(), ps)
        for n, w in zip(names, want):
            r = float((grads[n].detach().cpu().double() - w).norm() / max(float(w.norm()), 1e-30))
            assert r <= GRAD_L2, 'encoder gradient %s vs float64 autograd of the restatement: relative L2 %.3g' % (n, r)
    # the whole step against the oracle
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    orc = go.gru_oracle_model(sdg)
    env_c = uniform_env(raster, dx)
    oo = orc.forward(batch, map_idx, env_c, eps_post=eps_post, eps_prior=eps_prior)
    ol_d = ol.traffic_model_loss(TW, batch, oo, orc.get_normalizer(), orc.get_att_normalizer(), map_idx, env_c)
    ol_d['loss'].sum().backward()
    worst = ('', 0.0)
    for n, v in sdg.items():
        w = v.grad if v.grad is not None else torch.zeros_like(v)
        r = float((grads[n].detach().cpu().double() - w.double()).norm() / max(float(w.double().norm()), 1e-30))
        worst = max(worst, (n, r), key=lambda e: e[1])
    print('training step: worst gradient vs the oracle %s %.3g (relative L2)' % worst)
    assert worst[1] <= 2e-3, 'gradient %s vs the oracle: relative L2 %.3g' % worst


@pytest.mark.gpu
def test_gpu_dropin_refine_closure_with_gru_encoders():
    """Through dropin.install(): the reference's import names build TrafficModel(traj_encoder='gru'); a refine closure (decode,
    AvoidCollLoss, backward, Adam) runs 3 iterations with finite latents, and a second run repeats iteration 1 bit for bit."""
    from test_dropin_reference import _names_installed
    from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors
    with _names_installed():
        from models.traffic_model import TrafficModel
        from datasets.utils import MeanStdNormalizer
        from losses.adv_gen_nusc import AvoidCollLoss
        from utils.scenario_gen import detach_embed_info
        m = TrafficModel(4, 12, 256, 2, traj_encoder='gru')
        m.load_state_dict(synth.fill_state_dict(m.state_dict(), key='weights'))
        m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
        m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
        m.set_bicycle_params(NUSC_BIKE_PARAMS)
        m = m.eval().to(DEV)
        batch, map_idx, raster, dx = mg.g5_inputs(None, None)
        go.with_gaps(batch)
        env = uniform_env(raster, dx, DEV)
        bg, mi = batch.clone().to(DEV), map_idx.to(DEV)

        def run():
            with torch.no_grad():
                emb = detach_embed_info(m.embed(bg, mi, env))
            assert emb['past_feat'].shape == (bg.past.shape[0], 64)
            z0 = synth.make_latents(emb['prior_out'][0].cpu(), emb['prior_out'][1].cpu(), key='g5/z').to(DEV)
            z = z0.clone().requires_grad_(True)
            opt = torch.optim.Adam([z], lr=0.05)
            lf = AvoidCollLoss(mg.REFINE_WEIGHTS, m.get_att_normalizer().unnormalize(bg.lw), mi[bg.batch], env, z0.clone() * 0.9,
                               veh_coll_buffer=0.2)
            trace = []
            for _ in range(3):
                opt.zero_grad()
                pred = m.decode_embedding(z, emb, bg, mi, env, nfuture=6)['future_pred']
                lf(m.get_normalizer().unnormalize(pred), z, emb['prior_out'])['loss'].backward()
                opt.step()
                trace.append(z.detach().cpu().clone())
            return z0.cpu(), trace
        z0, a = run()
        _, b = run()
    assert all(bool(torch.isfinite(t).all()) for t in a)
    assert float((a[2] - z0).abs().max()) > 1e-3, 'the iterations moved the latents'
    assert torch.equal(a[0], b[0]), 'iteration 1 of a second run differs'
