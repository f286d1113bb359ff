#!/usr/bin/env python3
"""ms per refine closure (decode_embedding(nfuture=16) + AvoidCollLoss + backward, reference src/refine_traffic_optim.py:184-220)
at the headline size (32 scenes x 16 agents) for the bicycle model at latent widths 16, 32 (shipped) and 64, each with the
scene-resident kernels (the default) and with option scene_kernels = 0 (the launch-per-phase kernels).  Weights from
synth.fill_state_dict per width, same batch, textured raster; eager closures timed with events (no graph replay).

Usage:  python tools/latent_size_timing.py [--iters 50] [--warmup 10] [--widths 16,32,64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from strive_amd import synth, _lib as L                                  # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors   # noqa: E402
from strive_amd.datasets.utils import MeanStdNormalizer                 # noqa: E402
from strive_amd.models.traffic_model import TrafficModel                # noqa: E402
from direct_output_timing import time_closure, DEV                      # noqa: E402


def model(Z):
    m = TrafficModel(4, 12, 256, 2, latent_size=Z)
    m.load_state_dict(synth.fill_state_dict(m.state_dict(), key='weights'))
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    return m.eval().to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--widths', default='16,32,64')
    a = ap.parse_args()
    batch, map_idx = synth.make_batch([16] * 32, key='gc/graph', map_extent=(512.0, 512.0))
    raster, dx = synth.make_raster(2048, 2048)
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    batch, map_idx = batch.to(DEV), map_idx.to(DEV)
    lib = L.get_lib()
    out = {}
    for Z in [int(w) for w in a.widths.split(',')]:
        m = model(Z)
        out['z%d' % Z] = time_closure(m, batch, map_idx, env, a.iters, a.warmup)
        lib.set_option('scene_kernels', 0)
        try:
            out['z%d_phase' % Z] = time_closure(m, batch, map_idx, env, a.iters, a.warmup)
        finally:
            lib.sync_options_from_env()
    print(json.dumps({k: round(v, 3) for k, v in out.items()}))


if __name__ == '__main__':
    main()
