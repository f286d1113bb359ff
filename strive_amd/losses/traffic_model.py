"""Training-time loss with the reference's names (reference src/losses/traffic_model.py:20-295).

Values and gradients w.r.t. the predictions come from the same HIP collision kernels as the optimisation-time
losses (autograd Functions in strive_amd.ops) plus elementwise torch glue; together with ``TrafficModel.forward``
(which builds the parameter-gradient graph) ``loss_dict['loss'][0].backward()`` trains the model like the reference's
loop (src/train_traffic.py:103-131).
"""
import torch
from torch import nn

from .common import kl_normal, log_normal
from . import adv_gen_nusc as _opt

ENV_COLL_THRESH = 0.05
VEH_COLL_THRESH = 0.02


class VehCollLoss(nn.Module):
    """Every valid in-scene pair contributes (zero when not colliding); returns (penalties, num_pairs)
    (reference :166-238)."""

    def __init__(self, veh_att, batch, ptr, num_circ=5, buffer_dist=0.0):
        super(VehCollLoss, self).__init__()
        self.inner = _opt.VehCollLoss(veh_att, num_circ=num_circ, buffer_dist=buffer_dist, ptr=ptr)
        sizes = self.inner.info.sizes.to(torch.long)
        self.num_pairs = torch.sum(sizes * sizes - sizes).to(veh_att.device)
        # the valid (i != j) slots as an index tensor, built once: pen[:, bool_mask] synchronises on every call, forward and backward
        self.valid_idx = torch.nonzero(self.inner.valid).flatten()

    def forward(self, traj):
        pen, mask = self.inner.block_penalties(traj)
        pen = torch.where(mask, pen, torch.zeros_like(pen))
        return pen.index_select(1, self.valid_idx).reshape(-1), self.num_pairs


class EnvCollLoss(nn.Module):
    """Dense (NA,T) penalties, zero where no collision point exists (reference :240-295)."""

    def __init__(self, veh_att, mapixes, map_env, T):
        super(EnvCollLoss, self).__init__()
        self.inner = _opt.EnvCollLoss(veh_att, mapixes, map_env)
        self.T = T

    def forward(self, traj):
        NA = traj.size(0)
        assert traj.size(1) == self.T
        pen, valid = self.inner.valid_penalties(traj)
        return torch.where(valid, pen, torch.zeros_like(pen)).view(NA, self.T)


class TrafficModelLoss(nn.Module):
    """(reference :20-118)"""

    def __init__(self, loss_weights, state_normalizer=None, att_normalizer=None):
        super(TrafficModelLoss, self).__init__()
        self.loss_weights = loss_weights
        self.state_normalizer = state_normalizer
        self.att_normalizer = att_normalizer

    @staticmethod
    def _sig(t):
        return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), str(t.device))

    def _batch_constants(self, scene_graph, map_idx, map_env, T):
        """What depends on the batch only -- the visible-frame index and targets, the two collision modules (circle tables, slot
        maps, grid size) -- is built once per batch and kept on the graph object.  The reference builds the modules inside every
        forward (:79-101); here that cost a dozen host synchronisations per training step (tools/sync_audit.py train)."""
        w = self.loss_weights
        key = (self._sig(scene_graph.ptr), self._sig(scene_graph.lw), self._sig(scene_graph.future_vis), self._sig(scene_graph.future_gt),
               self._sig(map_idx), id(map_env), T, w['coll_veh_prior'] > 0.0, w['coll_env_prior'] > 0.0,
               # (the collision modules freeze the unnormalised vehicle sizes: new attribute statistics = new modules)
               self._sig(getattr(self.att_normalizer, 'mean_vals', None)), self._sig(getattr(self.att_normalizer, 'std_vals', None)))
        ent = scene_graph.__dict__.get('_strive_train_consts')
        if ent is not None and ent[0] == key:
            return ent[1]
        c = {}
        vis = (scene_graph.future_vis == 1.0).reshape(-1)
        c['vis_idx'] = torch.nonzero(vis).flatten()
        c['gt'] = scene_graph.future_gt.reshape(-1, scene_graph.future_gt.size(-1)).index_select(0, c['vis_idx'])[:, :4].contiguous()
        if w['coll_veh_prior'] > 0.0:
            c['veh'] = VehCollLoss(self.att_normalizer.unnormalize(scene_graph.lw), scene_graph.batch, scene_graph.ptr)
        if w['coll_env_prior'] > 0.0 and map_idx is not None and map_env is not None:
            ego = scene_graph.ptr[:-1].to(scene_graph.lw.device)
            c['ego'] = ego
            c['env'] = EnvCollLoss(self.att_normalizer.unnormalize(scene_graph.lw[ego]), map_idx, map_env, T)
        scene_graph.__dict__['_strive_train_consts'] = (key, c)
        return c

    def forward(self, scene_graph, pred, map_idx=None, map_env=None):
        w = self.loss_weights
        T = pred['future_pred'].size(1)
        c = self._batch_constants(scene_graph, map_idx, map_env, T)
        if tuple(pred['future_pred'].shape[:2]) != tuple(scene_graph.future_vis.shape[:2]):
            # (the reference's boolean mask pred[vis == 1] raises on such a mismatch; the cached index would silently pick wrong rows)
            raise IndexError('future_pred %s does not match future_vis %s' % (tuple(pred['future_pred'].shape), tuple(scene_graph.future_vis.shape)))
        pf = pred['future_pred'].reshape(-1, pred['future_pred'].size(-1)).index_select(0, c['vis_idx'])
        recon = -log_normal(pf, c['gt'], torch.ones_like(pf))
        pm, pv = pred['prior_out']
        qm, qv = pred['posterior_out']
        kl = kl_normal(qm, qv, pm, pv)
        loss = w['recon'] * recon.mean() + w['kl'] * kl.mean()
        out = {'recon_loss': recon, 'kl_loss': kl}
        if w['coll_veh_prior'] > 0.0 and 'future_samp' in pred:
            pens, npairs = c['veh'](self.state_normalizer.unnormalize(pred['future_samp']))
            cv = torch.sum(pens) / npairs
            loss = loss + w['coll_veh_prior'] * cv
            out['coll_veh_prior'] = cv.view((1,))
        if w['coll_env_prior'] > 0.0 and 'future_samp' in pred:
            assert map_idx is not None and map_env is not None
            ce = c['env'](self.state_normalizer.unnormalize(pred['future_samp'].index_select(0, c['ego'])))
            loss = loss + w['coll_env_prior'] * ce.mean()
            out['coll_env_prior'] = ce.view(-1)
        out['loss'] = loss.view((1,))
        return out


    def dense_terms(self, scene_graph, pred):
        """``forward`` without its compaction, for loops that must not synchronise (strive_amd/test_traffic.py): the same terms with
        ``recon_loss`` DENSE, (NA,T), beside the mask of the frames ``forward`` keeps.  ``forward`` selects the visible frames
        through an index built with ``torch.nonzero`` -- a read-back the first time it sees a batch object; here the reconstruction
        mean is a masked sum over all frames divided by the number of visible ones.  Returns ``(terms, masks)``: ``terms`` in
        ``forward``'s key order, ``masks[key]`` where only part of ``terms[key]`` counts.  Only for predictions without
        ``future_samp`` (the prior-sample collision terms need ``forward``)."""
        if 'future_samp' in pred:
            raise ValueError('dense_terms covers the reconstruction and KL terms only; call forward for the collision terms')
        w = self.loss_weights
        fp = pred['future_pred']
        if tuple(fp.shape[:2]) != tuple(scene_graph.future_vis.shape[:2]):
            raise IndexError('future_pred %s does not match future_vis %s' % (tuple(fp.shape), tuple(scene_graph.future_vis.shape)))
        vis = scene_graph.future_vis == 1.0
        recon = -log_normal(fp, scene_graph.future_gt[..., :4], torch.ones_like(fp))
        pm, pv = pred['prior_out']
        qm, qv = pred['posterior_out']
        kl = kl_normal(qm, qv, pm, pv)
        rmean = torch.where(vis, recon, torch.zeros_like(recon)).sum() / vis.sum()
        loss = w['recon'] * rmean + w['kl'] * kl.mean()
        return {'recon_loss': recon, 'kl_loss': kl, 'loss': loss.view((1,))}, {'recon_loss': vis}

    def compute_err(self, scene_graph, pred, normalizer):
        """Interpretable errors the training / test loops log (reference :120-164): position error (m) and heading error
        (degrees) per visible frame, NLL and Mahalanobis distance of the posterior mean under the prior per agent."""
        vis = scene_graph.future_vis == 1.0
        gt = normalizer.unnormalize(scene_graph.future_gt)[vis]
        pf = normalizer.unnormalize(pred['future_pred'])[vis]
        pos_err = torch.norm(gt[:, :2] - pf[:, :2], dim=-1)
        gh = gt[:, 2:4] / torch.norm(gt[:, 2:4], dim=-1, keepdim=True)
        ph = pf[:, 2:4] / torch.norm(pf[:, 2:4], dim=-1, keepdim=True)
        ang_err = torch.rad2deg(torch.acos(torch.sum(gh * ph, dim=-1).clamp(-1, 1)))
        pm, pv = pred['prior_out']
        qm = pred['posterior_out'][0]
        return {'pos_err': pos_err, 'ang_err': ang_err, 'z_logprob': log_normal(qm, pm, pv),
                'z_mdist': torch.norm((qm - pm) / torch.sqrt(pv), dim=-1)}


ENV_COLL_THRESH = 0.05   # up to 5 % of a vehicle may be off the road (reference :17)


def compute_coll_rate_env(scene_graph, map_idx, pred, map_env, state_normalizer, att_normalizer, ego_only=False):
    """Which sampled rollouts leave the drivable area?  ``pred`` (NA,NS,FT,4) NORMALISED (or a dict holding
    ``future_pred``); NaN frames never count (reference :366-419).  Returns the reference's dict with
    ``did_collide`` (NA,NS) bool."""
    from ..datasets import nuscenes_utils as nutils
    from ..datasets.utils import get_ego_inds
    fut = pred if isinstance(pred, torch.Tensor) else pred['future_pred']
    NA, NS, FT, _ = fut.size()
    veh_att = scene_graph.lw
    mapixes = map_idx[scene_graph.batch]
    if ego_only:
        ego = torch.from_numpy(get_ego_inds(scene_graph)).to(fut.device)
        fut, veh_att, mapixes = fut[ego], veh_att[ego], mapixes[ego]
        NA = fut.size(0)
    flat = state_normalizer.unnormalize(fut).reshape(NA * NS * FT, 4)
    att = att_normalizer.unnormalize(veh_att).view(NA, 1, 1, 2).expand(NA, NS, FT, 2).reshape(NA * NS * FT, 2)
    mix = mapixes.view(NA, 1, 1).expand(NA, NS, FT).reshape(NA * NS * FT)
    valid = ~torch.isnan(flat.sum(-1))
    frac = torch.ones((NA * NS * FT,), dtype=torch.float32, device=fut.device)
    if bool(valid.any()):
        frac[valid] = nutils.check_on_layer(map_env.nusc_raster[:, 0], map_env.nusc_dx, flat[valid], att[valid], mix[valid])
    coll = (frac.view(NA, NS, FT) < (1.0 - ENV_COLL_THRESH)).sum(dim=2) >= 1
    return {'num_coll_map': float(coll.sum().item()), 'num_traj_map': float(NS * NA), 'did_collide': coll}


def compute_coll_rate_env_from_traj(pred_future, veh_att, mapixes, map_env):
    """The same test on UNNORMALISED trajectories: ``pred_future`` (NA,NS,FT,4), ``veh_att`` (NA,2) in metres, ``mapixes`` (NA)
    (reference :421-463, what the scenario-evaluation tools call on stored scenarios)."""
    from ..datasets import nuscenes_utils as nutils
    NA, NS, FT, _ = pred_future.size()
    flat = pred_future.reshape(NA * NS * FT, 4)
    att = veh_att.view(NA, 1, 1, 2).expand(NA, NS, FT, 2).reshape(NA * NS * FT, 2)
    mix = mapixes.view(NA, 1, 1).expand(NA, NS, FT).reshape(NA * NS * FT)
    valid = ~torch.isnan(flat.sum(-1))
    frac = torch.ones((NA * NS * FT,), dtype=torch.float32, device=pred_future.device)
    if bool(valid.any()):
        frac[valid] = nutils.check_on_layer(map_env.nusc_raster[:, 0], map_env.nusc_dx, flat[valid], att[valid], mix[valid])
    coll = (frac.view(NA, NS, FT) < (1.0 - ENV_COLL_THRESH)).sum(dim=2) >= 1
    return {'num_coll_map': float(coll.sum().item()), 'num_traj_map': float(NS * NA), 'did_collide': coll}


def compute_disp_err(scene_graph, pred, normalizer):
    """Sample-based displacement errors of the EGO of every scene (reference :297-364): ``pred['future_pred']`` (NA,NS,FT',4)
    NORMALISED against ``scene_graph.future_gt`` over the common horizon.  Returns per scene the best-of-NS average / final
    position error (m), the same for the heading (degrees) and the average pairwise distance between the samples."""
    fut = pred['future_pred']
    gt = scene_graph.future_gt
    T = min(int(fut.size(2)), int(gt.size(1)))
    ego = scene_graph.ptr[:-1].to(fut.device)
    g = normalizer.unnormalize(gt[:, :T]).index_select(0, ego).unsqueeze(1)            # (B,1,T,6)
    p = normalizer.unnormalize(fut[:, :, :T]).index_select(0, ego)                      # (B,NS,T,4)
    B, NS = p.size(0), p.size(1)
    dist = torch.norm(g[..., :2] - p[..., :2], dim=-1)                                  # (B,NS,T)
    spread = torch.norm(p[:, :, None, :, :2] - p[:, None, :, :, :2], dim=-1)            # (B,NS,NS,T); zero on the diagonal
    apd = spread.sum(dim=(1, 2)).sum(dim=-1) / (NS * (NS - 1) * T)
    unit = lambda v: v / torch.norm(v, dim=-1, keepdim=True)
    ang = torch.rad2deg(torch.acos(torch.sum(unit(g[..., 2:4]) * unit(p[..., 2:4]), dim=-1).clamp(-1, 1)))
    return {'pos_minADE': dist.mean(dim=-1).min(dim=1)[0], 'pos_minFDE': dist[:, :, -1].min(dim=1)[0],
            'ang_minADE': ang.mean(dim=-1).min(dim=1)[0], 'ang_minFDE': ang[:, :, -1].min(dim=1)[0], 'APD': apd}


VEH_COLL_THRESH = 0.02   # IoU above which two boxes count as collided (reference :18)


def compute_coll_rate_veh(scene_graph, pred, state_normalizer, att_normalizer):
    """Which sampled rollouts collide with another agent?  ``pred`` (NA,NS,FT,4) NORMALISED (or a dict holding
    ``future_pred``).  Like the reference (:465-545) every connected pair is checked once and charged to its LOWER-indexed
    agent: ``did_collide[i, s]`` iff the box of agent i overlaps (IoU > 0.02) the box of some connected agent j > i at some
    step of sample s; NaN frames never count.  The reference walks samples x pairs x steps through shapely polygons on the
    host; here all (pair, sample, step) boxes go through ONE launch of the exact clipping kernel (ops.rect_iou)."""
    from .. import ops
    fut = pred if isinstance(pred, torch.Tensor) else pred['future_pred']
    NA, NS, FT, _ = fut.size()
    dev = fut.device
    traj = state_normalizer.unnormalize(fut)
    lw = att_normalizer.unnormalize(scene_graph.lw)
    ei = scene_graph.edge_index.to(dev)
    keep = ei[0] > ei[1]
    aj, ai = ei[0][keep], ei[1][keep]
    did = torch.zeros((NA, NS), dtype=torch.bool, device=dev)
    Pn = int(aj.numel())
    if Pn > 0:
        n = Pn * NS * FT
        a = traj.index_select(0, ai)[..., :4].reshape(n, 4)
        b = traj.index_select(0, aj)[..., :4].reshape(n, 4)
        la = lw.index_select(0, ai).view(Pn, 1, 1, 2).expand(Pn, NS, FT, 2).reshape(n, 2)
        lb = lw.index_select(0, aj).view(Pn, 1, 1, 2).expand(Pn, NS, FT, 2).reshape(n, 2)
        hit = (ops.rect_iou(a, la, b, lb).view(Pn, NS, FT) > VEH_COLL_THRESH).any(dim=2)      # NaN compares False
        did.index_put_((ai.view(Pn, 1).expand(Pn, NS)[hit], torch.arange(NS, device=dev).view(1, NS).expand(Pn, NS)[hit]),
                       torch.ones((int(hit.sum()),), dtype=torch.bool, device=dev))
    host = did.cpu().numpy().astype(bool)
    return {'num_coll_veh': float(host.sum()), 'num_traj_veh': float(NS * NA), 'did_collide': host}
