"""Restatement of the GRU trajectory encoders (``TrafficModel(traj_encoder='gru')``, reference src/models/traffic_model.py:93-119,
453-523) in plain torch, from the equations alone: runnable in float32 and float64, differentiable by autograd.

Each encoder is a 4-layer GRU with hidden size 128 over the frames of every agent (zero initial state, gate order r, z, n) followed
by a Linear(128, 64) on the top layer's state after the last frame:
    r = sigmoid(W_ir x + b_ir + W_hr h + b_hr),  z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),  h' = (1 - z) * n + z * h
The input of frame t is [x, y, hx, hy, s, hdot | vis | l, w | sem(NC)]: the pose in the frame of the last past step, the first six
values zeroed where vis == 0 (vis, lw and sem never are).  Test infrastructure only."""
import torch

LAYERS, HID = 4, 128


def transform2frame(frame, poses):
    c, s = frame[:, 2:3], frame[:, 3:4]
    dx, dy = poses[..., 0] - frame[:, 0:1], poses[..., 1] - frame[:, 1:2]
    pc, ps = poses[..., 2], poses[..., 3]
    return torch.stack([c * dx + s * dy, -s * dx + c * dy, pc * c + ps * s, ps * c - pc * s], dim=-1)


def encoder_input(past, traj, vis, lw, sem):
    """(NA, T, NC + 9) sequence of one encoder: ``traj`` (NA, T, 6) and ``vis`` (NA, T) are the past or the future."""
    NA, T, _ = traj.shape
    local = torch.cat([transform2frame(past[:, -1, :4], traj[:, :, :4]), traj[:, :, 4:]], dim=2)
    local = torch.where((vis == 0.0).unsqueeze(-1), torch.zeros_like(local), local)
    return torch.cat([local, vis.unsqueeze(-1), lw.unsqueeze(1).expand(NA, T, 2), sem.unsqueeze(1).expand(NA, T, sem.shape[1])], dim=-1)


def gru_params(sd, enc, out, dtype=torch.float64, requires_grad=False):
    """the 18 tensors of one encoder in named_parameters() order, as leaves of ``dtype``"""
    names = ['%s.%s_l%d' % (enc, k, l) for l in range(LAYERS) for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    names += [out + '.weight', out + '.bias']
    return names, [sd[n].detach().clone().to(dtype).requires_grad_(requires_grad) for n in names]


def gru_features(ps, x):
    """ps: the 18 tensors (gru_params); x (NA, T, in) -> (NA, 64)"""
    NA, T, _ = x.shape
    h = [x.new_zeros((NA, HID)) for _ in range(LAYERS)]
    for t in range(T):
        inp = x[:, t]
        for l in range(LAYERS):
            wih, whh, bih, bhh = ps[4 * l:4 * l + 4]
            gi = inp @ wih.t() + bih
            gh = h[l] @ whh.t() + bhh
            r = torch.sigmoid(gi[:, :HID] + gh[:, :HID])
            z = torch.sigmoid(gi[:, HID:2 * HID] + gh[:, HID:2 * HID])
            n = torch.tanh(gi[:, 2 * HID:] + r * gh[:, 2 * HID:])
            h[l] = (1.0 - z) * n + z * h[l]
            inp = h[l]
    return h[-1] @ ps[16].t() + ps[17]


def encode(sd, which, batch, dtype=torch.float64):
    """past_feat / future_feat of a batch (``which`` = 'past' or 'future') with the state_dict's encoder"""
    traj, vis = (batch.past, batch.past_vis) if which == 'past' else (batch.future, batch.future_vis)
    x = encoder_input(batch.past.to(dtype), traj.to(dtype), vis.to(dtype), batch.lw.to(dtype), batch.sem.to(dtype))
    _, ps = gru_params(sd, which + '_encoder', which + '_out_layer', dtype)
    return gru_features(ps, x)


def gru_oracle_model(sd, NC=2, FT=12):
    """The CPU oracle (oracle/model.py) with its two trajectory encoders replaced by the restatement above, in the dtype of ``sd``"""
    from oracle.model import OracleTrafficModel
    from oracle.geometry import Normalizer
    from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors

    class GRUOracle(OracleTrafficModel):
        def _encode_traj(self, prefix, g, traj, vis):
            which = prefix.split('_')[0]
            x = encoder_input(g.past, traj, vis, g.lw, g.sem).detach()
            names, _ = gru_params(self.sd, which + '_encoder', which + '_out_layer')
            return gru_features([self.sd[n] for n in names], x)
    return GRUOracle(sd, Normalizer(*state_norm_tensors()), Normalizer(*att_norm_tensors()), NUSC_BIKE_PARAMS, FT=FT, NC=NC)


def gru_product_model(NC=2, FT=12, device='cpu', key='weights'):
    from strive_amd import synth
    from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors
    from strive_amd.models.traffic_model import TrafficModel
    from strive_amd.datasets.utils import MeanStdNormalizer
    m = TrafficModel(4, FT, 256, NC, traj_encoder='gru')
    sd = synth.fill_state_dict(m.state_dict(), key=key)
    m.load_state_dict(sd)
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m.eval()
    return m.to(device), sd


def with_gaps(batch):
    """Visibility gaps in a fully visible synthetic batch (in place): agent 0 loses past frame 1 and future frames 3 and 7, agent 1
    future frames from 9 on, and the LAST agent's past is invisible throughout."""
    batch.past_vis[0, 1] = 0.0
    batch.future_vis[0, 3] = 0.0
    batch.future_vis[0, 7] = 0.0
    if batch.past.shape[0] > 2:
        batch.future_vis[1, 9:] = 0.0
    batch.past_vis[-1, :] = 0.0
    return batch
