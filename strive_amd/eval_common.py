"""Host pieces shared by the evaluation drivers (eval_planner, eval_adv_gen, test_traffic): the scenario-directory reader and
what the drivable-area check of the metric kernels needs (strive_amd/csrc/eval_metrics.hip)."""
import glob
import json
import os

import torch

LIN_MAX = 128                     # largest sampling grid of the drivable-area check along either axis


def scene_jsons(scene_path):
    """(name, parsed JSON) of every ``*.json`` of a directory, sorted by name; a file that holds ``null`` comes as (name, None)."""
    for path in sorted(glob.glob(os.path.join(scene_path, '*.json'))):
        with open(path, 'r') as f:
            yield os.path.basename(path)[:-5], json.load(f)


_lin_tabs = {}


def lin_table(dev):
    """fp32 ``torch.linspace(-1, 1, k)`` for k = 1..LIN_MAX one after the other (table k starts at k (k - 1) / 2), uploaded once
    per device: the kernel picks the grid size on the device, after the collision time is known."""
    t = _lin_tabs.get(str(dev))
    if t is None:
        t = torch.cat([torch.linspace(-1.0, 1.0, k) for k in range(1, LIN_MAX + 1)]).to(dev)
        _lin_tabs[str(dev)] = t
    return t


class PackEnv(object):
    """What the map packer reads of a map environment; crop geometry the evaluation does not use gets the reference's defaults."""

    def __init__(self, env):
        self.nusc_raster, self.nusc_dx = env.nusc_raster, env.nusc_dx
        self.bounds = list(getattr(env, 'bounds', [-17.0, -38.5, 60.0, 38.5]))
        self.L, self.W = getattr(env, 'L', 256), getattr(env, 'W', 256)


def pack_env(map_env):
    pe = map_env.__dict__.get('_strive_eval_env')
    if pe is None or pe.nusc_raster is not map_env.nusc_raster:
        pe = PackEnv(map_env)
        map_env.__dict__['_strive_eval_env'] = pe
    return pe
