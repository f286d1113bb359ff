"""Host pieces shared by the evaluation drivers (eval_planner, eval_adv_gen, test_traffic): the scenario-directory reader and
what the drivable-area check of the metric kernels needs (strive_amd/csrc/eval_metrics.hip)."""
import glob
import json
import os

import torch

from . import _lib as L

LIN_MAX = 128                     # largest sampling grid of the drivable-area check along either axis


# ------------------------------------------------------------------------------------------------
# what every wrapper of a metric kernel does with its arguments
# ------------------------------------------------------------------------------------------------

def traj_arg(traj, who):
    """The trajectories of a verdict call, (NA,1,T,4) or (NA,T,4), as contiguous fp32 (NA,T,4); ``who`` names the caller in the error."""
    traj = traj.detach()
    if traj.dim() == 4 and traj.shape[1] == 1:
        traj = traj[:, 0]
    if traj.dim() != 3 or traj.shape[2] != 4:
        raise ValueError('%s expects final_result_traj (NA,1,T,4)' % who)
    return traj.to(torch.float32).contiguous()


def i32(t, dev, shape=None):
    """Offsets, map indices or flags as a contiguous int32 tensor on ``dev``, reshaped to ``shape`` if one is given."""
    t = torch.as_tensor(t).to(device=dev, dtype=torch.int32)
    return (t if shape is None else t.reshape(shape)).contiguous()


def outputs(out, dev, spec):
    """A copy of the caller's ``out`` dict (or a new one) in which every ``(key, shape, dtype, fill)`` of ``spec`` that the caller did
    not supply is a new tensor on ``dev`` holding ``fill``."""
    out = {} if out is None else dict(out)
    for key, shape, dtype, fill in spec:
        out.setdefault(key, torch.full(shape, fill, dtype=dtype, device=dev))
    return out


def host_stats(state_normalizer, att_normalizer):
    """The four ``float[4]`` arguments of an entry point from the two normalisers, converted ONCE (a normaliser built from device
    tensors would otherwise be read back on every call)."""
    sn, an = state_normalizer, att_normalizer
    return (L.f4(sn.mean_vals[:4].tolist()), L.f4(sn.std_vals[:4].tolist()),
            L.f4(an.mean_vals[:2].tolist() + [0.0, 0.0]), L.f4(an.std_vals[:2].tolist() + [1.0, 1.0]))


def model_stats(model):
    """``host_stats`` of a model's two normalisers, kept on the model until it is given other normalisers."""
    sn, an = model.get_normalizer(), model.get_att_normalizer()
    ent = model.__dict__.get('_strive_verdict_stats')
    if ent is None or ent[0] is not sn or ent[1] is not an:
        ent = (sn, an, host_stats(sn, an))
        model.__dict__['_strive_verdict_stats'] = ent
    return ent[2]


def check_status(codes, text, what, positions=None):
    """Raise for the first scene a kernel refused (``codes``: the status vector on the host; ``text``: the driver's table of the
    codes; ``what``: the entry point; ``positions``: the scenes' names, else their index in the call)."""
    for b, code in enumerate(codes):
        if code != 0:
            raise ValueError('scene %s: %s (status %d of %s)' % (positions[b] if positions is not None else b,
                                                                 text.get(int(code), 'refused'), code, what))


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
