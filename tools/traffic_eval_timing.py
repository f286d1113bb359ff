#!/usr/bin/env python3
"""Wall time of the model-evaluation metrics on 32 scenes x 16 agents, 12 steps, NS 3 and NS 20, inputs on the device, warm-up first,
device synchronised before and after every timed call; wall time (the existing functions read results back, so that is what
compares) and the time between two events recorded around the call:
  (a) the three existing functions compute_disp_err + compute_coll_rate_env(ego_only=True) + compute_coll_rate_veh
  (b) the ONE traffic_eval_metrics call (disp, env, veh)
  (c) one run_one_epoch batch with the shared embed against the same batch through the three separate model calls (8 scenes x 8
      agents, NS 3, all four quantitative flags)
Information only, no gate.

Usage:  python tools/traffic_eval_timing.py [--reps 7] [--out profiles/r18_traffic_eval_timing.md]
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from strive_amd import synth                                              # noqa: E402
from strive_amd import test_traffic as TT                                 # noqa: E402
from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors   # noqa: E402
from strive_amd.datasets.utils import MeanStdNormalizer                  # noqa: E402
from strive_amd.losses import traffic_model as TM                        # noqa: E402
from strive_amd.models.traffic_model import TrafficModel                 # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps):
    """(median, min, max) of the wall time and the median of the time between two events recorded around the call, ms."""
    fn()
    fn()
    out, ev = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out), statistics.median(ev)


def injected(batch, NS, T=12):
    """Predictions around the scenes' own futures, as tests/golden/make_golden.py builds g11's."""
    NA = batch.past.shape[0]
    base = batch.future_gt[:, :T, :4].unsqueeze(1).expand(NA, NS, T, 4)
    off = synth.f32(synth.counter_uniform((NA, NS, 1, 2), 'timing/off', -0.06, 0.06))
    drift = synth.f32(synth.counter_uniform((NA, NS, 1, 2), 'timing/drift', -0.01, 0.01)) * torch.arange(T).view(1, 1, T, 1)
    pred = base.clone()
    pred[..., :2] = pred[..., :2] + off + drift
    return pred.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sn, an = MeanStdNormalizer(*state_norm_tensors()), MeanStdNormalizer(*att_norm_tensors())
    raster, dx = synth.make_raster()
    env = synth.SyntheticMapEnv(raster, dx).to(DEV)
    rows = []
    batch, mi = synth.make_batch([16] * 32, key='timing')
    batch, mi = batch.to(DEV), mi.to(DEV)
    for NS in (3, 20):
        pred = {'future_pred': injected(batch.clone().to('cpu'), NS).to(DEV)}

        def existing():
            TM.compute_disp_err(batch, pred, sn)
            TM.compute_coll_rate_env(batch, mi, pred, env, sn, an, ego_only=True)
            TM.compute_coll_rate_veh(batch, pred, sn, an)

        def one_call():
            TT.traffic_eval_metrics(pred['future_pred'], batch.ptr, batch.lw, sn, an, gt=batch.future_gt, map_env=env, mapix=mi, disp=True,
                                    veh=True, env=True, env_ego_only=True)
        rows.append(('(a) three existing functions, NS %d' % NS,) + timed(existing, a.reps))
        rows.append(('(b) one `traffic_eval_metrics` call, NS %d' % NS,) + timed(one_call, a.reps))

    m = TrafficModel(4, 12, 256, 2)
    m.load_state_dict(synth.fill_state_dict(m.state_dict()))
    m.set_normalizer(sn)
    m.set_att_normalizer(an)
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m = m.eval().to(DEV)
    loss_fn = TM.TrafficModelLoss({'recon': 1.0, 'kl': 1.0, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0})
    sb, smi = synth.make_batch([8] * 8, key='timing/model')
    sb, smi = sb.to(DEV), smi.to(DEV)
    flags = dict(test_recon_coll_rate=True, test_sample_disp_err=True, test_sample_coll_rate=True, test_sample_num=3)

    def shared():
        TT.run_one_epoch([(sb, smi)], m, env, loss_fn, DEV, '.', **flags)

    def separate():
        with torch.no_grad():
            p = m(sb, smi, env, use_post_mean=True)
            loss_fn(sb, p)
            loss_fn.compute_err(sb, p, sn)
            r = {'future_pred': m.reconstruct(sb, smi, env)['future_pred'].unsqueeze(1)}
            TM.compute_coll_rate_env(sb, smi, r, env, sn, an, ego_only=True)
            TM.compute_coll_rate_veh(sb, r, sn, an)
            s = m.sample_batched(sb, smi, env, 3, include_mean=False)
            TM.compute_disp_err(sb, s, sn)
            TM.compute_coll_rate_env(sb, smi, s, env, sn, an, ego_only=True)
            TM.compute_coll_rate_veh(sb, s, sn, an)
    import contextlib
    import io
    rows.append(('(c) one batch, three model calls + the existing functions',) + timed(separate, a.reps))
    with contextlib.redirect_stdout(io.StringIO()):                 # (the report lines of run_one_epoch)
        rows.append(('(c) one batch through `run_one_epoch` (shared embed, two metric launches, its one read-back and its report)',) + timed(shared, a.reps))

    text = ['# Model evaluation: wall time (information only, no gate)', '',
            '`tools/traffic_eval_timing.py` on %s: (a), (b) 32 scenes x 16 agents, 12 steps, injected predictions; (c) 8 scenes x 8 agents,' % torch.cuda.get_device_name(0),
            'NS 3, all four quantitative flags.  Inputs on the device, two warm-up calls, %d timed calls each, device synchronised around' % a.reps,
            'every call.  Wall: median (min .. max) of the host clock, which is what compares here -- the existing functions read their',
            'results back and do host work between launches; events: median of the time between two events recorded around the call.',
            '', '| what | wall ms | events ms |', '|---|---|---|']
    text += ['| %s | %.3f (%.3f .. %.3f) | %.3f |' % r for r in rows]
    print('\n'.join(text))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
