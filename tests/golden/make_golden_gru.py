#!/usr/bin/env python3
"""Generate tests/golden/g16_gru.npz: the reference's model with the GRU trajectory encoders (``traj_encoder='gru'``), run by the
reference.

Like make_golden_latent.py (whose layout it follows) this runs the reference itself in the build container and stores only its
outputs.  The model is the reference's ``TrafficModel(4, 12, 256, NC, traj_encoder='gru')`` with ``synth.fill_state_dict`` weights
(key 'weights'; 'weights5' for NC = 5), the suite's normalisers and bicycle parameters, over a UNIFORM raster (layer 0 = 1
everywhere).  The synthetic scenes are fully visible, so every batch gets the visibility gaps of tests/gru_oracle.with_gaps: frames
missing in the past and in the future, and one agent whose past is invisible throughout.

Contents:
  sd_names, sd_shapes            the 182 state_dict names and shapes
  <c>_map_feat, <c>_past_feat, <c>_future_feat, <c>_prior_mu, <c>_prior_var, <c>_post_mu, <c>_post_var
                                 embed() for c = g4u (the g4u scenes, sizes 3, 5, 1), big (a 20-agent and a 3-agent scene,
                                 build_inputs key 'g15/big') and nc5 (NC = 5 model on build_inputs(G4B_SIZES, 'g4b', NC=5))
  pred_ft12, gz_ft12             decode_embedding FT 12 on the g4u scenes and d(sum(pred * r))/dz (latents key 'g4/z', r key 'g16/rft12')
  samp_*                         sample_batched NS 3, include_mean, nfuture 8, eps injected (key 'g16/eps', shape (3, NA, 32)) on
                                 build_inputs([4, 2], 'g7')
  train_*                        one training step: forward(future_sample=True) with injected eps (keys 'g16/eps_post',
                                 'g16/eps_prior') on the g5 batch; the TrafficModelLoss terms (weights of train_traffic.cfg),
                                 future_pred / future_samp, and for each of the 182 parameters the first GRAD_HEAD entries of its
                                 flattened gradient (train_grad/<name>) and the L2 norm of the whole gradient (train_gnorm/<name>)

Usage:  python tests/golden/make_golden_gru.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                         # noqa: E402
from make_golden import import_reference, g4u_inputs, build_inputs, ref_map_env   # noqa: E402
from make_golden_latent import uniform_raster, TRAIN_WEIGHTS, GRAD_HEAD, BIG_SIZES, SAMP_SIZES    # noqa: E402
from gru_oracle import with_gaps                                 # noqa: E402
from strive_amd import synth                                     # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors    # noqa: E402

Z = 32


def ref_gru_model(R, NC=2, key='weights'):
    m = R.traffic_model.TrafficModel(4, 12, 256, NC, traj_encoder='gru')
    sd = synth.fill_state_dict(m.state_dict(), key=key)
    m.load_state_dict(sd)
    m.set_normalizer(R.dutils.MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(R.dutils.MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m.eval()
    return m, sd


def embed_case(R, tm, out, tag, batch, map_idx, raster, dx):
    env = ref_map_env(R, uniform_raster(raster), dx)
    with torch.no_grad():
        emb = tm.embed(batch, map_idx, env)
        out[tag + '_future_feat'] = mg.npy(tm.encode_future(batch))
    emb = R.scenario_gen.detach_embed_info(emb)
    out[tag + '_map_feat'] = mg.npy(emb['map_feat'])
    out[tag + '_past_feat'] = mg.npy(emb['past_feat'])
    out[tag + '_prior_mu'], out[tag + '_prior_var'] = mg.npy(emb['prior_out'][0]), mg.npy(emb['prior_out'][1])
    out[tag + '_post_mu'], out[tag + '_post_var'] = mg.npy(emb['posterior_out'][0]), mg.npy(emb['posterior_out'][1])
    return emb, env


def g16_gru(R):
    out = {}
    tm, sd = ref_gru_model(R)
    out['sd_names'] = np.asarray(list(sd.keys()))
    out['sd_shapes'] = np.asarray([','.join(str(d) for d in v.shape) for v in sd.values()])

    batch, map_idx, raster, dx = g4u_inputs()
    with_gaps(batch)
    emb, env = embed_case(R, tm, out, 'g4u', batch, map_idx, raster, dx)
    z = synth.make_latents(emb['prior_out'][0], emb['prior_out'][1], key='g4/z').requires_grad_(True)
    pred = tm.decode_embedding(z, emb, batch, map_idx, env, nfuture=12)['future_pred']
    rw = synth.f32(synth.counter_uniform(tuple(pred.shape), 'g16/rft12', -1.0, 1.0))
    gz, = torch.autograd.grad((pred * rw).sum(), [z])
    out['pred_ft12'], out['gz_ft12'] = mg.npy(pred), mg.npy(gz)

    batch, map_idx, raster, dx = build_inputs(BIG_SIZES, 'g15/big')
    embed_case(R, tm, out, 'big', with_gaps(batch), map_idx, raster, dx)

    tm5, _ = ref_gru_model(R, NC=5, key='weights5')
    batch, map_idx, raster, dx = build_inputs(mg.G4B_SIZES, 'g4b', NC=5)
    embed_case(R, tm5, out, 'nc5', with_gaps(batch), map_idx, raster, dx)

    batch, map_idx, raster, dx = build_inputs(SAMP_SIZES, 'g7')
    with_gaps(batch)
    env = ref_map_env(R, uniform_raster(raster), dx)
    NA = batch.past.shape[0]
    eps = synth.f32(synth.counter_normal((3, NA, Z), 'g16/eps'))
    tm.rsample = lambda mean, var: mean + eps * torch.sqrt(var)
    with torch.no_grad():
        so = tm.sample_batched(batch, map_idx, env, 3, include_mean=True, nfuture=8)
    for k in ('future_pred', 'z_samp', 'z_logprob', 'z_mdist'):
        out['samp_' + k] = mg.npy(so[k])

    tm, _ = ref_gru_model(R)
    batch, map_idx, raster, dx = build_inputs(mg.G5_SIZES, 'g5', window=14.0)
    with_gaps(batch)
    env = ref_map_env(R, uniform_raster(raster), dx)
    NA = batch.past.shape[0]
    tm.train()
    seq = [synth.f32(synth.counter_normal((NA, Z), 'g16/eps_post')), synth.f32(synth.counter_normal((NA, Z), 'g16/eps_prior'))]
    tm.rsample = lambda mean, var: mean + seq.pop(0) * torch.sqrt(var)
    net_out = tm(batch, map_idx, env, future_sample=True)
    tloss = R.tm_losses.TrafficModelLoss(TRAIN_WEIGHTS, tm.get_normalizer(), tm.get_att_normalizer())
    ld = tloss(batch, net_out, map_idx, env)
    ld['loss'].sum().backward()
    for k, v in ld.items():
        out['train_%s' % k] = mg.npy(v)
    out['train_future_pred'] = mg.npy(net_out['future_pred'])
    out['train_future_samp'] = mg.npy(net_out['future_samp'])
    grads = {n: p.grad for n, p in tm.named_parameters()}
    out['train_ngrads'] = np.asarray(sum(1 for g in grads.values() if g is not None))
    for n, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), n
        out['train_grad/' + n] = mg.npy(g.reshape(-1)[:GRAD_HEAD])
        out['train_gnorm/' + n] = np.asarray(float(g.double().norm()))
    mg.save('g16_gru.npz', **out)


if __name__ == '__main__':
    torch.set_num_threads(8)
    g16_gru(import_reference())
