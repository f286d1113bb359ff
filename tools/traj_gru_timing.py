#!/usr/bin/env python3
"""GRU trajectory encoder (traj_encoder='gru'): the HIP path (strive_traj_gru_fwd / _fwd_keep + _bwd, csrc/traj_gru.hip) against
torch's own nn.GRU(in, 128, num_layers=4) + nn.Linear(128, 64) with the same weights and inputs on the same GPU -- what the
reference runs (src/models/traffic_model.py:477-486).

Per size (NA agents x T frames, input width 11): forward alone, and forward + backward (weight gradients of all 18 tensors), each the
median of --reps timed runs after --warmup untimed ones, timed with events on the stream, one event pair around --inner back-to-back
calls (a single call is shorter than the event resolution); min / max over the runs are reported as the spread.  Then embed() and
one 4 x 16-agent training step (forward(future_sample=True), TrafficModelLoss, backward) with the MLP and with the GRU encoders.

Usage:  python tools/traj_gru_timing.py [--reps 20] [--warmup 5] [--inner 10] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from strive_amd import synth, ops, params, _lib as L                     # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors   # noqa: E402
from strive_amd.datasets.utils import MeanStdNormalizer                 # noqa: E402
from strive_amd.losses.traffic_model import TrafficModelLoss            # noqa: E402
from strive_amd.models.traffic_model import TrafficModel                # noqa: E402

DEV = torch.device('cuda', 0)
SIZES = [(64, 4), (64, 12), (512, 12)]
TW = {'recon': 1.0, 'kl': 0.004, 'coll_veh_prior': 0.05, 'coll_env_prior': 0.1}


def timed(fn, reps, warmup, inner):
    """ms per call of fn: median, min, max over ``reps`` runs of ``inner`` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def model(enc):
    m = TrafficModel(4, 12, 256, 2, traj_encoder=enc)
    m.load_state_dict(synth.fill_state_dict(m.state_dict(), key='weights'))
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    return m.to(DEV)


def encoder_case(m, NA, T, a):
    lib = L.get_lib()
    gru = torch.nn.GRU(11, 128, 4, batch_first=True).to(DEV)
    lin = torch.nn.Linear(128, 64).to(DEV)
    gru.load_state_dict(m.future_encoder.state_dict())
    lin.load_state_dict(m.future_out_layer.state_dict())
    x = synth.f32(synth.counter_uniform((NA, T, 11), 'timing/x', -1.0, 1.0)).to(DEV)
    d_feat = synth.f32(synth.counter_uniform((NA, 64), 'timing/d', -1.0, 1.0)).to(DEV)
    pk = ops.traj_gru_pack(m, 'future')
    feat = torch.empty((NA, 64), device=DEV)
    kb = lib.query('strive_traj_gru_keep_bytes', pk.ref(), NA, T)
    kept = torch.empty((kb,), dtype=torch.uint8, device=DEV)
    dp = torch.zeros((lib.query('strive_traj_gru_param_count', pk.ref()),), device=DEV)
    st = L.stream_ptr(x)
    tps = list(gru.parameters()) + list(lin.parameters())

    def hip_fwd():
        lib.call('strive_traj_gru_fwd', pk.ref(), L.ptr(x), NA, T, L.ptr(feat), st)

    def hip_fwd_bwd():
        lib.call('strive_traj_gru_fwd_keep', pk.ref(), L.ptr(x), NA, T, L.ptr(feat), L.ptr(kept), kb, st)
        lib.call('strive_traj_gru_bwd', pk.ref(), NA, T, L.ptr(kept), kb, L.ptr(d_feat), L.ptr(dp), st)

    def torch_fwd():
        with torch.no_grad():
            return lin(gru(x)[0][:, -1])

    def torch_fwd_bwd():
        torch.autograd.grad((lin(gru(x)[0][:, -1]) * d_feat).sum(), tps)

    hip_fwd()
    err = float((feat - torch_fwd()).abs().max())
    r = {'hip_fwd': timed(hip_fwd, a.reps, a.warmup, a.inner), 'torch_fwd': timed(torch_fwd, a.reps, a.warmup, a.inner),
         'hip_fwd_bwd': timed(hip_fwd_bwd, a.reps, a.warmup, a.inner), 'torch_fwd_bwd': timed(torch_fwd_bwd, a.reps, a.warmup, a.inner),
         'max_abs_diff_fwd': err}
    return r


def model_case(enc, a):
    m = model(enc)
    batch, map_idx = synth.make_batch([16] * 4, key='timing/train', map_extent=(512.0, 512.0))
    raster, dx = synth.make_raster(2048, 2048)
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    batch, map_idx = batch.to(DEV), map_idx.to(DEV)
    lf = TrafficModelLoss(TW, m.get_normalizer(), m.get_att_normalizer())

    def embed():
        with torch.no_grad():
            m.embed(batch, map_idx, env)

    def step():
        for p in m.parameters():
            p.grad = None
        out = m(batch, map_idx, env, future_sample=True)
        lf(batch, out, map_idx=map_idx, map_env=env)['loss'][0].backward()
    m.eval()
    r = {'embed': timed(embed, a.reps, a.warmup, 1)}
    m.train()
    r['train_step'] = timed(step, a.reps, a.warmup, 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'inner': a.inner}
    m = model('gru')
    for NA, T in SIZES:
        out['NA%d_T%d' % (NA, T)] = encoder_case(m, NA, T, a)
    for enc in ('mlp', 'gru'):
        out['model_' + enc] = model_case(enc, a)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
