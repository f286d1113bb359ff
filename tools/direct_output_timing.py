#!/usr/bin/env python3
"""ms per refine closure (decode_embedding(nfuture=16) + AvoidCollLoss + backward, reference src/refine_traffic_optim.py:184-220)
at the headline size (32 scenes x 16 agents) for three models:
  direct     TrafficModel(output_bicycle=False): the launch-per-phase rollout kernels in their direct mode
  bike_phase the bicycle model with option scene_kernels = 0: the same kernel family
  bike       the bicycle model as shipped (scene-resident kernels)
Same weights (but the last decoder layer), same batch, textured raster; eager closures timed with events (no graph replay).

Usage:  python tools/direct_output_timing.py [--iters 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from strive_amd import synth, _lib as L                                  # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors   # noqa: E402
from strive_amd.datasets.utils import MeanStdNormalizer                 # noqa: E402
from strive_amd.losses.adv_gen_nusc import AvoidCollLoss                # noqa: E402
from strive_amd.models.traffic_model import TrafficModel                # noqa: E402
from strive_amd.utils.scenario_gen import detach_embed_info             # noqa: E402

REFINE_WEIGHTS = {'coll_veh': 100.0, 'coll_env': 100.0, 'init_z': 0.01, 'motion_prior': 1.0}
DEV = 'cuda:0'


def model(bicycle):
    m = TrafficModel(4, 12, 256, 2, output_bicycle=bicycle)
    m.load_state_dict(synth.fill_state_dict(m.state_dict(), key='weights'))
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    if bicycle:
        m.set_bicycle_params(NUSC_BIKE_PARAMS)
    return m.eval().to(DEV)


def time_closure(m, batch, map_idx, env, iters, warmup):
    with torch.no_grad():
        emb = detach_embed_info(m.embed(batch, map_idx, env))
    z = synth.make_latents(emb['prior_out'][0].cpu(), emb['prior_out'][1].cpu(), key='timing/z').to(DEV).requires_grad_(True)
    lf = AvoidCollLoss(REFINE_WEIGHTS, m.get_att_normalizer().unnormalize(batch.lw), map_idx[batch.batch], env, z.clone().detach(),
                       veh_coll_buffer=0.2)

    def closure():
        z.grad = None
        pred = m.decode_embedding(z, emb, batch, map_idx, env, nfuture=16)['future_pred']
        ld = lf(m.get_normalizer().unnormalize(pred), z, emb['prior_out'])
        ld['loss'].backward()
    for _ in range(warmup):
        closure()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        closure()
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(z.grad).all()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    batch, map_idx = synth.make_batch([16] * 32, key='gc/graph', map_extent=(512.0, 512.0))
    raster, dx = synth.make_raster(2048, 2048)
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    batch, map_idx = batch.to(DEV), map_idx.to(DEV)
    lib = L.get_lib()
    out = {'direct': time_closure(model(False), batch, map_idx, env, a.iters, a.warmup)}
    bike = model(True)
    lib.set_option('scene_kernels', 0)
    try:
        out['bike_phase'] = time_closure(bike, batch, map_idx, env, a.iters, a.warmup)
    finally:
        lib.sync_options_from_env()
    out['bike'] = time_closure(bike, batch, map_idx, env, a.iters, a.warmup)
    print(json.dumps({k: round(v, 3) for k, v in out.items()}))


if __name__ == '__main__':
    main()
