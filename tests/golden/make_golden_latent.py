#!/usr/bin/env python3
"""Generate tests/golden/g15_latent.npz: the reference's model at latent widths other than 32 (``--latent_size``), run by the
reference.

Like make_golden_direct.py (whose case layout it follows) and make_golden.py (whose import stand-ins and input builders it uses),
this runs the reference itself in the build container and stores only its outputs.  The model is the reference's
``TrafficModel(4, FT, 256, 2, latent_size=Z)`` with ``synth.fill_state_dict`` weights (key 'weights'), the suite's normalisers and
bicycle parameters.  Every case runs over a UNIFORM raster (layer 0 = 1 everywhere), so every map crop is the same image and no
crop can flip between two fp32 rollouts.

Contents, for Z = 16 and Z = 64 under the prefix ``z<Z>/`` (``r`` = a counter-uniform array of pred's shape, key noted):
  sd_names, sd_shapes            the 174 state_dict names and shapes (prior_net / posterior_net's last layer 2Z wide, decoder_net's
                                 first layer 130 + NC + Z)
  map_feat, past_feat, prior_mu, prior_var
                                 embed() of the g4u scenes (sizes 3, 5, 1)
  pred_<c>, gz_<c>               decode_embedding on the g4u scenes and d(sum(pred * r))/dz (latents: make_latents key 'g4/z'), for
                                 c = ft1, ft12, ft16 (nfuture; r key 'g15/r<c>'), ext (ext_future = the egos' GT future, FT 12),
                                 ns (NS = 2, second sample key 'g4/z_b')
  big_*                          one decode FT 12 + d/dz on a batch of a 20-agent and a 3-agent scene (build_inputs key 'g15/big';
                                 latents key 'g15/big/z', r key 'g15/rbig'): the scene-tile path of the forward
  samp_*                         sample_batched NS 3, include_mean, nfuture 8, eps injected (key 'g15/eps', shape (3, NA, Z)) on
                                 build_inputs([4, 2], 'g7')
  train_*                        one training step: forward(future_sample=True) with injected eps (keys 'g15/eps_post',
                                 'g15/eps_prior') on build_inputs(G5_SIZES, 'g5', window=14) over the uniform raster; the
                                 TrafficModelLoss terms (weights of train_traffic.cfg), future_pred / future_samp, and for every one
                                 of the 174 parameters the first GRAD_HEAD entries of its flattened gradient (train_grad/<name>) and
                                 the L2 norm of the whole gradient (train_gnorm/<name>)
  avoid_*                        AvoidCollLoss (REFINE_WEIGHTS, buffer 0.2) on a 16-step decode of the g5 batch (latents key
                                 'g5/z'): every loss term, pred and d(loss)/dz
  adv_*                          AdvGenLoss (ADV_WEIGHTS, ego-planner mode, buffer 0.1, min time 2, in front 0.0) on a decode with
                                 ext_future = the egos' GT future: every loss term, pred and d(loss)/d(other_z)
  refine/*                       (Z = 16 only) the reference's own refine_traffic_optim() (its function body executed from its file),
                                 Adam, 3 iterations, samp / save future length 6, lr 0.05, on the g12 batch with the prior sample
                                 injected (key 'g15/refine_eps', shape (1, NA, 16)): init_future_pred, z, result_traj

Usage:  python tests/golden/make_golden_latent.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                         # noqa: E402
from make_golden import import_reference, g4u_inputs, build_inputs, ref_map_env   # noqa: E402
from strive_amd import synth                                     # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors    # noqa: E402

ZS = (16, 64)
FTS = (1, 12, 16)
BIG_SIZES = [20, 3]
SAMP_SIZES = [4, 2]
GRAD_HEAD = 96
REFINE_Z = 16
TRAIN_WEIGHTS = {'recon': 1.0, 'kl': 0.004, 'coll_veh_prior': 0.05, 'coll_env_prior': 0.1}


def uniform_raster(raster):
    u = torch.zeros((1,) + tuple(raster.shape[1:]), dtype=torch.uint8)
    u[:, 0] = 1
    return u


def ref_latent_model(R, Z, FT=12):
    m = R.traffic_model.TrafficModel(4, FT, 256, 2, latent_size=Z)
    sd = synth.fill_state_dict(m.state_dict(), key='weights')
    m.load_state_dict(sd)
    m.set_normalizer(R.dutils.MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(R.dutils.MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m.eval()
    return m, sd


def decode_case(tm, emb, batch, map_idx, env, z, rkey, **kw):
    z = z.clone().requires_grad_(True)
    pred = tm.decode_embedding(z, emb, batch, map_idx, env, **kw)['future_pred']
    rw = synth.f32(synth.counter_uniform(tuple(pred.shape), rkey, -1.0, 1.0))
    gz, = torch.autograd.grad((pred * rw).sum(), [z])
    return mg.npy(pred), mg.npy(gz)


def latent_cases(R, Z):
    out = {}
    tm, sd = ref_latent_model(R, Z)
    out['sd_names'] = np.asarray(list(sd.keys()))
    out['sd_shapes'] = np.asarray([','.join(str(d) for d in v.shape) for v in sd.values()])

    batch, map_idx, raster, dx = g4u_inputs()
    env = ref_map_env(R, uniform_raster(raster), dx)
    with torch.no_grad():
        emb = R.scenario_gen.detach_embed_info(tm.embed(batch, map_idx, env))
    out['map_feat'] = mg.npy(emb['map_feat'])
    out['past_feat'] = mg.npy(emb['past_feat'])
    out['prior_mu'] = mg.npy(emb['prior_out'][0])
    out['prior_var'] = mg.npy(emb['prior_out'][1])
    z1 = synth.make_latents(emb['prior_out'][0], emb['prior_out'][1], key='g4/z')
    z2 = torch.stack([z1, synth.make_latents(emb['prior_out'][0], emb['prior_out'][1], key='g4/z_b')], dim=1)
    ext = batch.future_gt[batch.ptr[:-1]][:, :, :4]
    cases = [('ft%d' % f, z1, {'nfuture': f}) for f in FTS] + [('ext', z1, {'ext_future': ext}), ('ns', z2, {})]
    for name, z, kw in cases:
        out['pred_' + name], out['gz_' + name] = decode_case(tm, emb, batch, map_idx, env, z, 'g15/r' + name, **kw)

    # a 20-agent scene
    batch, map_idx, raster, dx = build_inputs(BIG_SIZES, 'g15/big')
    env = ref_map_env(R, uniform_raster(raster), dx)
    with torch.no_grad():
        emb = R.scenario_gen.detach_embed_info(tm.embed(batch, map_idx, env))
    zb = synth.make_latents(emb['prior_out'][0], emb['prior_out'][1], key='g15/big/z')
    out['big_map_feat'] = mg.npy(emb['map_feat'])
    out['big_past_feat'] = mg.npy(emb['past_feat'])
    out['big_pred'], out['big_gz'] = decode_case(tm, emb, batch, map_idx, env, zb, 'g15/rbig', nfuture=12)

    # sample_batched NS 3 with injected eps
    batch, map_idx, raster, dx = build_inputs(SAMP_SIZES, 'g7')
    env = ref_map_env(R, uniform_raster(raster), dx)
    NA = batch.past.shape[0]
    eps = synth.f32(synth.counter_normal((3, NA, Z), 'g15/eps'))
    tm.rsample = lambda mean, var: mean + eps * torch.sqrt(var)
    with torch.no_grad():
        so = tm.sample_batched(batch, map_idx, env, 3, include_mean=True, nfuture=8)
    for k in ('future_pred', 'z_samp', 'z_logprob', 'z_mdist'):
        out['samp_' + k] = mg.npy(so[k])

    # the two fused losses on the dense g5 batch
    batch, map_idx, raster, dx = build_inputs(mg.G5_SIZES, 'g5', window=14.0)
    env = ref_map_env(R, uniform_raster(raster), dx)
    with torch.no_grad():
        emb = R.scenario_gen.detach_embed_info(tm.embed(batch, map_idx, env))
    NA = batch.past.shape[0]
    ego_mask = torch.zeros((NA,), dtype=torch.bool)
    ego_mask[batch.ptr[:-1]] = True
    veh_att = tm.get_att_normalizer().unnormalize(batch.lw)
    mapixes = map_idx[batch.batch]
    z = synth.make_latents(emb['prior_out'][0], emb['prior_out'][1], key='g5/z').requires_grad_(True)
    pred = tm.decode_embedding(z, emb, batch, map_idx, env, nfuture=16)['future_pred']
    lf = R.adv_losses.AvoidCollLoss(mg.REFINE_WEIGHTS, veh_att, mapixes, env, z.clone().detach() * 0.9, veh_coll_buffer=0.2)
    ld = lf(tm.get_normalizer().unnormalize(pred), z, emb['prior_out'])
    ld['loss'].backward()
    for k, v in ld.items():
        out['avoid_' + k] = mg.npy(v)
    out['avoid_pred'] = mg.npy(pred)
    out['avoid_gz'] = mg.npy(z.grad)

    z = synth.make_latents(emb['prior_out'][0], emb['prior_out'][1], key='g5/z')
    other_z = z[~ego_mask].clone().requires_grad_(True)
    tgt_z = z[ego_mask].clone()
    zc = R.adv_optim.collate_tgt_other_z(batch, tgt_z, other_z)
    planner = batch.future_gt[ego_mask][:, :, :4]
    pred = tm.decode_embedding(zc, emb, batch, map_idx, env, ext_future=planner)['future_pred']
    lf = R.adv_losses.AdvGenLoss(mg.ADV_WEIGHTS, veh_att, mapixes, env, other_z.clone().detach() * 0.9, batch.ptr,
                                 veh_coll_buffer=0.1, crash_loss_min_time=2, crash_loss_min_infront=0.0)
    oprior = (emb['prior_out'][0][~ego_mask], emb['prior_out'][1][~ego_mask])
    ld = lf(tm.get_normalizer().unnormalize(pred), tm.get_normalizer().unnormalize(planner), other_z, oprior)
    ld['loss'].backward()
    for k, v in ld.items():
        out['adv_' + k] = mg.npy(v)
    out['adv_pred'] = mg.npy(pred)
    out['adv_gz'] = mg.npy(other_z.grad)

    # one training step
    tm, _ = ref_latent_model(R, Z)
    batch, map_idx, raster, dx = build_inputs(mg.G5_SIZES, 'g5', window=14.0)
    env = ref_map_env(R, uniform_raster(raster), dx)
    NA = batch.past.shape[0]
    tm.train()
    for p in tm.parameters():
        p.grad = None
    seq = [synth.f32(synth.counter_normal((NA, Z), 'g15/eps_post')), synth.f32(synth.counter_normal((NA, Z), 'g15/eps_prior'))]
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
        out['train_grad/' + n] = mg.npy(g.reshape(-1)[:GRAD_HEAD])
        out['train_gnorm/' + n] = np.asarray(float(g.double().norm()))
    return out


def refine_inputs():
    batch, map_idx, _, _ = build_inputs(mg.G12_SIZES, 'g12', window=14.0)
    raster, dx = mg.loop_rasters('u')
    eps = synth.f32(synth.counter_normal((1, batch.past.shape[0], REFINE_Z), 'g15/refine_eps'))
    return batch, map_idx, raster, dx, eps


def refine_case(R):
    """the reference's own refine_traffic_optim() at latent width REFINE_Z (as make_golden.g12_refine_fn, Adam branch)"""
    import tqdm
    src = open(os.path.join(mg.REF_SRC, 'refine_traffic_optim.py')).read()
    body = src[src.index('def refine_traffic_optim('):src.index('def run_one_epoch(')]
    ns = {'torch': torch, 'optim': torch.optim, 'tqdm': tqdm, 'detach_embed_info': R.scenario_gen.detach_embed_info,
          'AvoidCollLoss': R.adv_losses.AvoidCollLoss}
    exec(compile(body, 'reference:refine_traffic_optim.py', 'exec'), ns)
    tm, _ = ref_latent_model(R, REFINE_Z)
    batch, map_idx, raster, dx, eps = refine_inputs()
    env = ref_map_env(R, raster, dx)
    tm.rsample = lambda mean, var: mean + eps * torch.sqrt(var)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
        init_pred, z, res, _ = ns['refine_traffic_optim'](batch, map_idx, env, tm, mg.REFINE_WEIGHTS, 3, 6, 6, True, 0.05)
    return {'refine/init_future_pred': mg.npy(init_pred), 'refine/z': mg.npy(z), 'refine/result_traj': mg.npy(res)}


def g15_latent(R):
    out = {}
    for Z in ZS:
        for k, v in latent_cases(R, Z).items():
            out['z%d/%s' % (Z, k)] = v
    for k, v in refine_case(R).items():
        out['z%d/%s' % (REFINE_Z, k)] = v
    mg.save('g15_latent.npz', **out)


if __name__ == '__main__':
    torch.set_num_threads(8)
    g15_latent(import_reference())
