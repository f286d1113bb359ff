"""Scenario-generation helpers on the hot path (reference src/utils/scenario_gen.py:19-28)."""
import torch

# The names strive_amd.dropin lays over the reference's utils/scenario_gen.py.  The metric helpers below are not among them:
# they pool sums and counts (PooledMetric), while the reference's own tools keep lists under the same names and must keep theirs.
__all__ = ['detach_embed_info', 'determine_feasibility_nusc', 'prepare_output_dict']


def detach_embed_info(embed_info_attached):
    out = {}
    for k, v in embed_info_attached.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.detach()
        elif isinstance(v, tuple):
            out[k] = (v[0].detach(), v[1].detach())
    return out


def determine_feasibility_nusc(samples, normalizer, feasibility_thresh, feasibility_time=0, feasibility_vel=0.0,
                               feasibility_infront_min=None, check_non_drivable_separation=True, map_env=None, map_idx=None):
    """Is a scene a plausible seed for scenario generation?  (reference src/utils/scenario_gen.py:30-107)
    ``samples`` (NA,NS,FT,4) NORMALISED futures of ONE scene, agent 0 = ego.  An agent is feasible if, in some sample
    and step >= ``feasibility_time``, it comes within ``feasibility_thresh`` metres of the ego (optionally only counting
    steps where it is in front of the ego), the closest approach is not across non-drivable area, and it moves faster
    than ``feasibility_vel`` per step somewhere.  Returns (feasible, closest step, closest distance), each (NA-1,);
    three Nones for an ego-only scene."""
    import torch
    from ..datasets import nuscenes_utils as nutils
    if samples.size(0) == 1:
        return None, None, None
    if feasibility_infront_min is not None and not (-1 <= feasibility_infront_min <= 1):
        raise AssertionError('feasibility_infront_min must lie in [-1, 1]')
    s = normalizer.unnormalize(samples)
    ego, oth = s[0:1], s[1:]
    NA, NS, FT, _ = oth.size()
    t0 = feasibility_time
    dist = torch.norm(ego[..., :2] - oth[..., :2], dim=-1)[:, :, t0:]                 # (NA, NS, FT')
    if feasibility_infront_min is not None:
        to_agent = oth[:, :, t0:, :2] - ego[:, :, t0:, :2]
        to_agent = to_agent / torch.norm(to_agent, dim=-1, keepdim=True)
        infront = torch.sum(to_agent * ego[:, :, t0:, 2:4], dim=-1) >= feasibility_infront_min
        dist = torch.where(infront, dist, torch.full_like(dist, float('inf')))
    best_over_samples, best_sample = torch.min(dist, dim=1)                           # (NA, FT')
    feasible_dist, step = torch.min(best_over_samples, dim=1)
    step = step + t0
    feasible = (dist < feasibility_thresh).sum(dim=[1, 2]) > 0
    if check_non_drivable_separation:
        ar = torch.arange(NA, device=samples.device)
        samp = best_sample[ar, step - t0]
        agent_xy = oth[ar, samp, step][:, :2]
        ego_xy = ego.expand(NA, NS, FT, 4)[ar, samp, step][:, :2]
        blocked = nutils.check_line_layer(map_env.nusc_raster[:, 0], map_env.nusc_dx, agent_xy, ego_xy, map_idx.expand(NA))
        feasible = torch.logical_and(feasible, ~blocked)
    vel = torch.norm(oth[:, :, 1:, :2] - oth[:, :, :-1, :2], dim=-1)
    feasible = torch.logical_and(feasible, vel.amax(dim=(1, 2)) > feasibility_vel)
    return feasible, step, feasible_dist


def prepare_output_dict(scene_graph, map_idx, map_env, dt, model, init_fut_traj, adv_fut_traj, sol_fut_traj=None,
                        attack_agt=None, attack_t=None, adv_z=None, sol_z=None, prior_distrib=None,
                        attack_bike_params=None, internal_ego_traj=None):
    """The scenario wire format consumed by the eval / clustering / viz tools (reference src/utils/scenario_gen.py:189-254):
    a JSON-ready dict with keys ``N, dt, map, lw, sem, past, fut_init, fut_adv`` and, when given, ``fut_internal_ego,
    fut_sol, attack_agt, attack_t, z_adv, z_sol, z_prior{mean,var}, attack_bike_prof``.  Trajectories and ``lw`` are
    stored UNNORMALISED as nested lists."""
    nrm = model.get_normalizer()

    def world(t):
        return nrm.unnormalize(t).cpu().numpy().tolist()

    def plain(t):
        return t.detach().cpu().numpy().tolist()
    out = {'N': int(init_fut_traj.size(0)), 'dt': dt, 'map': map_env.map_list[map_idx]}
    out['lw'] = plain(model.get_att_normalizer().unnormalize(scene_graph.lw))
    out['sem'] = plain(scene_graph.sem)
    out['past'] = world(scene_graph.past_gt)
    out['fut_init'] = world(init_fut_traj)
    out['fut_adv'] = world(adv_fut_traj)
    if internal_ego_traj is not None:
        out['fut_internal_ego'] = world(internal_ego_traj)
    if sol_fut_traj is not None:
        out['fut_sol'] = world(sol_fut_traj)
    if attack_agt is not None:
        out['attack_agt'] = int(attack_agt)
    if attack_t is not None:
        out['attack_t'] = int(attack_t)
    if adv_z is not None:
        out['z_adv'] = plain(adv_z)
    if sol_z is not None:
        out['z_sol'] = plain(sol_z)
    if prior_distrib is not None:
        out['z_prior'] = {'mean': plain(prior_distrib[0]), 'var': plain(prior_distrib[1])}
    if attack_bike_params is not None:
        out['attack_bike_prof'] = plain(attack_bike_params)
    return out


class PooledMetric(object):
    """Running total and count of one metric's per-frame values.  The reference keeps every value in a list and prints
    ``np.mean`` of it; the evaluation kernel hands back per-scene sums and counts, and ``total / count`` is that pooled mean
    (the mean over all frames of all scenes, not a mean of per-scene means)."""
    __slots__ = ('total', 'count')

    def __init__(self, total=0.0, count=0):
        self.total, self.count = float(total), int(count)

    def add(self, total, count):
        self.total += float(total)
        self.count += int(count)

    def mean(self):
        return self.total / self.count if self.count > 0 else float('nan')

    def __len__(self):
        return self.count

    def __repr__(self):
        return 'PooledMetric(mean=%r, count=%d)' % (self.mean(), self.count)


def log_metric_sum(metric_dict, stat_str, total, count):
    """``log_metric`` for values that arrive already summed (the evaluation kernel's per-scene sums and frame counts)."""
    if stat_str not in metric_dict:
        metric_dict[stat_str] = PooledMetric()
    metric_dict[stat_str].add(total, count)
    return metric_dict


def log_metric(metric_dict, stat_str, metric_np):
    """Add the values ``metric_np`` to the metric ``stat_str`` (reference src/utils/scenario_gen.py:120-124; pooled as a sum and
    a count instead of a growing list)."""
    import numpy as np
    v = np.asarray(metric_np, dtype=np.float64).reshape(-1)
    return log_metric_sum(metric_dict, stat_str, float(v.sum()), v.size)


def log_freq_stat(freq_dict_cnt, freq_dict_total, stat_str, cnt_add, tot_add):
    """Add ``cnt_add`` occurrences out of ``tot_add`` trials to ``stat_str`` (reference src/utils/scenario_gen.py:126-132)."""
    if stat_str not in freq_dict_cnt:
        freq_dict_cnt[stat_str] = 0
        freq_dict_total[stat_str] = 0
    freq_dict_cnt[stat_str] += cnt_add
    freq_dict_total[stat_str] += tot_add
    return freq_dict_cnt, freq_dict_total


def print_metrics(metrics, freq_metrics_cnt, freq_metrics_total, log=print):
    """One ``name = value`` line per metric (pooled mean) and per frequency (count / total), in insertion order (reference
    src/utils/scenario_gen.py:134-138)."""
    for k, v in metrics.items():
        log('%s = %f' % (k, v.mean()))
    for k, v in freq_metrics_cnt.items():
        log('%s = %f' % (k, float(v) / freq_metrics_total[k]))


def optim_result_calls(out_path, scene_graph_ptr, future_pred, attack_agt, crop_t, viz_bounds, bidx, ow_gt, show_gt, show_gt_idx,
                       colored=True):
    """The two viz_scene_graph calls of viz_optim_results (reference src/utils/scenario_gen.py:160-187): the overview with
    trajectories, then the frames under ``<out_path>_vid``."""
    from .. import render
    colors = None
    if colored:
        NA = int(scene_graph_ptr[bidx + 1]) - int(scene_graph_ptr[bidx])
        colors = render.get_adv_coloring(NA, attack_agt, 0)
    common = dict(bidx=bidx, future_pred=future_pred, show_gt=show_gt, show_gt_idx=show_gt_idx, viz_bounds=viz_bounds, crop_t=crop_t,
                  center_viz=crop_t is None, car_colors=colors, ow_gt=ow_gt)
    return [dict(common, out_path=out_path, viz_traj=True, make_video=False),
            dict(common, out_path=out_path + '_vid', viz_traj=False, make_video=True)]


def viz_optim_results(out_path, scene_graph, map_idx, map_env, model, future_pred, planner_name, attack_agt, crop_t,
                      viz_bounds=[-60.0, -60.0, 60.0, 60.0], bidx=0, ow_gt=None, show_gt=False, show_gt_idx=None):
    """Overview and frames of an optimised scene (reference src/utils/scenario_gen.py:149-187, same arguments; ``attack_agt`` is
    local to scene ``bidx``): both viz_scene_graph calls in one table launch, one render launch and one read-back."""
    from ..datasets import nuscenes_utils as nutils
    from ..scene_draw import host_ptr
    calls = optim_result_calls(out_path, host_ptr(scene_graph), future_pred, attack_agt, crop_t, viz_bounds, bidx, ow_gt, show_gt,
                               show_gt_idx)
    return nutils.viz_scene_graphs(scene_graph, map_idx, map_env, calls, model.get_normalizer(), model.get_att_normalizer())
