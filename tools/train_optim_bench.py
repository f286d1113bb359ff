"""What FlatAdam buys in the training step: ms per step and host enqueue per step of DataParallelTrainer.step with torch.optim.Adam
and with strive_amd.optim.FlatAdam, in ONE process, alternating, at the benchmark's training shape (bench.py --workload train:
4 scenes x 16 agents, FT 12, NC 2, TRAIN_WEIGHTS, lr 1e-5).

    python tools/train_optim_bench.py [--repeats 5] [--steps 30] [--warmup 10] [--out FILE]

Per repeat and optimiser: ``steps`` steps between two device synchronisations; ms per step = wall time / steps, host enqueue per
step = the time the host spends inside ``step()`` (it returns once everything is enqueued).  Prints one JSON line with every
repeat, the medians and the spread (max - min) of the repeats.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

TRAIN_WEIGHTS = {'recon': 1.0, 'kl': 0.004, 'coll_veh_prior': 0.05, 'coll_env_prior': 0.1}      # train_traffic.cfg:17-21


def make_trainer(kind, device, env, scenes, agents):
    from strive_amd import synth
    from strive_amd.constants import NUSC_BIKE_PARAMS, att_norm_tensors, state_norm_tensors
    from strive_amd.datasets.utils import MeanStdNormalizer
    from strive_amd.distributed import DataParallelTrainer
    from strive_amd.losses.traffic_model import TrafficModelLoss
    from strive_amd.models.traffic_model import TrafficModel
    from strive_amd.optim import FlatAdam
    m = TrafficModel(4, 12, 256, 2)
    m.load_state_dict(synth.fill_state_dict(m.state_dict()))
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m = m.to(device).train()
    batch, map_idx = synth.make_batch([agents] * scenes, key='bench/train/optim')
    opt = FlatAdam(m.parameters(), lr=1e-5) if kind == 'flat' else torch.optim.Adam(m.parameters(), lr=1e-5)
    tr = DataParallelTrainer(m, TrafficModelLoss(dict(TRAIN_WEIGHTS), m.get_normalizer(), m.get_att_normalizer()), opt)
    g, mi = batch.to(device), map_idx.to(device)

    def step():
        if tr.step(g, mi, env) is None:
            raise RuntimeError('training step was skipped: %r' % (tr.last_error,))
    return step


def measure(step, steps):
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        h0 = time.perf_counter()
        step()
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return 1e3 * wall / steps, 1e3 * host / steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--scenes', type=int, default=4)
    ap.add_argument('--agents', type=int, default=16)
    ap.add_argument('--device', type=str, default='cuda:0')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        raise SystemExit('at least 5 repeats per optimiser')
    from strive_amd import synth
    device = torch.device(args.device)
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(device)
    kinds = ('torch', 'flat')
    steps = {}
    for k in kinds:
        torch.manual_seed(0)
        steps[k] = make_trainer(k, device, env, args.scenes, args.agents)
        for _ in range(args.warmup):
            steps[k]()
    runs = {k: [] for k in kinds}
    for r in range(args.repeats):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):          # alternating, and alternating who goes first
            runs[k].append(measure(steps[k], args.steps))
    out = {'workload': 'DataParallelTrainer.step, %d scenes x %d agents, FT 12, NC 2, TRAIN_WEIGHTS, lr 1e-5' % (args.scenes, args.agents),
           'device': torch.cuda.get_device_name(device), 'steps_per_repeat': args.steps, 'warmup_steps': args.warmup, 'repeats': args.repeats}
    for k in kinds:
        ms, host = [a for a, _ in runs[k]], [b for _, b in runs[k]]
        out[k] = {'ms_per_step': [round(v, 4) for v in ms], 'host_enqueue_ms_per_step': [round(v, 4) for v in host],
                  'median_ms_per_step': round(statistics.median(ms), 4), 'median_host_enqueue_ms_per_step': round(statistics.median(host), 4),
                  'spread_ms_per_step': round(max(ms) - min(ms), 4), 'spread_host_enqueue_ms_per_step': round(max(host) - min(host), 4)}
    out['flat_minus_torch_median_ms_per_step'] = round(out['flat']['median_ms_per_step'] - out['torch']['median_ms_per_step'], 4)
    out['flat_minus_torch_median_host_enqueue_ms'] = round(out['flat']['median_host_enqueue_ms_per_step'] -
                                                           out['torch']['median_host_enqueue_ms_per_step'], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    return out


if __name__ == '__main__':
    main()
