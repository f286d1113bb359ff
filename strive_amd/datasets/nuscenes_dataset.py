"""The scene dataset with the reference's name and arguments (reference src/datasets/nuscenes_dataset.py:65-704), on device-resident
tables: everything of ``NuScenesDataset`` that follows the devkit.

``compile_data`` reads the nuScenes tables through the devkit, which is not here; its output -- the per-scene records -- comes from a
tracks file instead (``datasets/tracks.py``).  ``post_process`` is one HIP launch over all agents of all
scenes (strive_dataset_post_process), the agent counts of all windows a second one (strive_dataset_window_counts, read back once),
and every batch a third (strive_dataset_gather_batch): window selection, agent selection, normalisation, the clique graph and
the DataLoader collation, with no host work per agent and no synchronisation.  Scenario directories (``compile_scenarios``, :231-290)
are host glue that fills the same tables.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .. import ops, params
from ..graph import Data, Batch
from . import nuscenes_utils as nutils
from . import tracks as tracks_io
from .utils import MeanStdNormalizer, NUSC_NORM_STATS, read_adv_scenes

ALL_CATS = ['car', 'truck', 'bus', 'motorcycle', 'trailer', 'cyclist', 'pedestrian', 'emergency', 'construction']
REDUCE_CATS = {'car': 'car', 'truck': 'truck', 'bus': 'truck', 'motorcycle': 'motorcycle', 'trailer': 'truck', 'cyclist': 'cyclist',
               'pedestrian': 'pedestrian', 'emergency': 'car', 'construction': 'truck'}
MAX_GRID = 4096          # largest check_on_layer grid side the linspace tables are built for

_DEVKIT = 'needs the nuScenes devkit, which is not part of strive_amd: a tracks file is one split of pre-compiled records'


class _Loader(object):
    """Re-iterable over ``(Batch, map_idx)``: every batch is one strive_dataset_gather_batch launch."""

    def __init__(self, dataset, batch_size, shuffle, drop_last, generator):
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.generator = dataset, int(batch_size), shuffle, drop_last, generator

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for i in range(0, n, self.batch_size):
            idx = order[i:i + self.batch_size]
            if self.drop_last and len(idx) < self.batch_size:
                return
            yield self.dataset.get_batch(idx)


class NuScenesDataset(object):
    def __init__(self, data_path, map_env, version='mini', split='train', categories=['car', 'truck'], npast=4, nfuture=12, nusc=None,
                 noise_std=0.0, flip_singapore=True, seq_interval=1, randomize_val=False, val_size=200, scenario_path=None,
                 require_full_past=False, use_challenge_splits=False, reduce_cats=False, device=None):
        """``data_path``: a tracks file (or an already loaded tracks dict), or None together with a ``scenario_path``.  The other
        arguments are the reference's (:66-105); ``version``, ``split``, ``flip_singapore``, ``randomize_val`` and ``val_size`` describe
        how the devkit's tables are split and flipped, which a tracks file has behind it.  ``device``: where the tables and every
        batch live (default: the current ROCm device)."""
        assert version in ['mini', 'trainval']
        assert split in ['train', 'val', 'test']
        if nusc is not None:
            raise NotImplementedError('a pre-loaded NuScenes object ' + _DEVKIT)
        if use_challenge_splits:
            raise NotImplementedError('use_challenge_splits ' + _DEVKIT)
        self.version, self.split, self.data_path = version, split, data_path
        self.use_nusc = data_path is not None
        self.map_env = map_env
        self.map_list = map_env.map_list
        self.dt = 0.5
        self.noise_std = noise_std
        self.npast, self.nfuture, self.seq_len = npast, nfuture, npast + nfuture
        self.flip_singapore, self.seq_interval = flip_singapore, seq_interval
        self.randomize_val, self.val_size = randomize_val, val_size
        self.scenario_path = scenario_path
        if scenario_path is None and not self.use_nusc:
            raise ValueError('data_path may only be None together with a scenario_path')
        if npast < 1 or nfuture < 1 or seq_interval < 1:
            raise ValueError('npast, nfuture and seq_interval must be positive')
        self.require_full_past = bool(require_full_past)
        self.use_challenge_splits = False
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

        wanted = list(categories)
        for cat in wanted:
            if cat not in ALL_CATS:
                raise ValueError('Unrecognized category %s!' % cat)
        self._cat_of = {c: (REDUCE_CATS[c] if reduce_cats else c) for c in wanted}      # stored name -> the model's category
        self.categories = sorted(set(self._cat_of.values())) if reduce_cats else wanted
        iden = torch.eye(len(self.categories), dtype=torch.int)
        self.cat2vec = {c: iden[i] for i, c in enumerate(self.categories)}
        self.vec2cat = {tuple(iden[i].tolist()): c for i, c in enumerate(self.categories)}
        if 'car' not in self.cat2vec:
            raise ValueError("the ego is a 'car' (reference :613): categories must contain it")

        ninfo = NUSC_NORM_STATS[tuple(sorted(self.categories))]
        self.normalizer = MeanStdNormalizer(
            torch.Tensor([ninfo['lscale'][0], ninfo['lscale'][0], ninfo['h'][0], ninfo['h'][0], ninfo['s'][0], ninfo['hdot'][0]]),
            torch.Tensor([ninfo['lscale'][1], ninfo['lscale'][1], ninfo['h'][1], ninfo['h'][1], ninfo['s'][1], ninfo['hdot'][1]]))
        self.veh_att_normalizer = MeanStdNormalizer(torch.Tensor([ninfo['l'][0], ninfo['w'][0]]), torch.Tensor([ninfo['l'][1], ninfo['w'][1]]))
        self.norm_info = ninfo
        self._norm = L.StriveNorm()
        for i in range(6):
            self._norm.state_mean[i] = float(self.normalizer.mean_vals[i])
            self._norm.state_std[i] = float(self.normalizer.std_vals[i])
        for i in range(2):
            self._norm.att_mean[i] = float(self.veh_att_normalizer.mean_vals[i])
            self._norm.att_std[i] = float(self.veh_att_normalizer.std_vals[i])

        self.seq_map = []
        self.scene2map = {}
        self._build_tables(self._read_tracks(data_path) if self.use_nusc else None,
                           self.compile_scenarios(scenario_path) if scenario_path is not None else [])
        self.data_len = len(self.seq_map)

    # ------------------------------------------------------------------------------------------------
    # the reference's accessors
    # ------------------------------------------------------------------------------------------------
    def get_state_normalizer(self):
        return self.normalizer

    def get_att_normalizer(self):
        return self.veh_att_normalizer

    def __len__(self):
        return self.data_len

    def get_scenes(self):
        """Scene splits by name (reference :292-341) come from the devkit's ``create_splits_scenes``."""
        raise NotImplementedError('scene splits by name (get_scenes) ' + _DEVKIT)

    # ------------------------------------------------------------------------------------------------
    # construction
    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def _read_tracks(data_path):
        return tracks_io.check_tracks(data_path) if isinstance(data_path, dict) else tracks_io.load_tracks(data_path)

    def compile_scenarios(self, scenario_path):
        """Scenario files as scenes (reference :231-290), host numpy: [(name, map name, traj (NA,T,6) float64, is_vis (NA,T), lw (NA,2),
        category names)].  Speeds and heading rates of the future come from finite differences of the stored poses; the heading
        angle is an ``arctan2``, which is why this stays on the host."""
        out = []
        for scene in read_adv_scenes(scenario_path):
            lw = scene['veh_att'].numpy()
            past, fut = scene['scene_past'].numpy(), scene['scene_fut'].numpy()        # fp32, as the reference holds them
            NA = lw.shape[0]
            k = [self.vec2cat[tuple(row)] for row in scene['sem'].numpy().tolist()] if 'sem' in scene else ['car'] * NA
            k[0] = 'car'                                                                # the ego (:613)
            # the future's speeds and heading rates: differences over (last past pose, future poses), first entry dropped
            poses = np.concatenate((past[:, -1:, :4], fut), axis=1)
            t = self.dt * np.arange(poses.shape[1])
            heading = np.arctan2(poses[..., 3], poses[..., 2])                          # fp32 in, fp32 out
            traj = np.full((NA, past.shape[1] + fut.shape[1], 6), np.nan, dtype=np.float64)
            traj[:, :past.shape[1]] = past
            traj[:, past.shape[1]:, :4] = fut
            for a in range(NA):
                traj[a, past.shape[1]:, 4] = np.linalg.norm(nutils.velocity(poses[a, :, :2], t)[1:], axis=1)
                traj[a, past.shape[1]:, 5] = nutils.heading_change_rate(heading[a], t)[1:]
            vis = (~np.isnan(traj.sum(axis=2))).astype(np.int32)
            vis[0] = 1                                                                  # the ego counts as visible throughout
            out.append((scene['name'], scene['map'], traj, vis, lw.astype(np.float64), k))
        return out

    def _build_tables(self, tr, scenarios):
        dev = self.device
        i32 = lambda a: params.upload(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)), dev)      # noqa: E731
        i64 = lambda a: params.upload(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)), dev)      # noqa: E731
        f64 = lambda a: params.upload(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)), dev)    # noqa: E731
        car = self.categories.index('car')

        # ---- host side of the track scenes ----
        S1 = A1 = 0
        names, scene_map, scene_T, agent_ptr, cat, lw = [], [], [], [0], [], np.zeros((0, 2))
        if tr is not None:
            S1, A1 = len(tr['scene_name']), tr['lw'].shape[0]
            names = list(tr['scene_name'])
            scene_map = [self.map_list.index(m) for m in tr['scene_map']]
            scene_T = np.diff(tr['frame_ptr']).tolist()
            agent_ptr = tr['agent_ptr'].tolist()
            # per stored category: the model's category column, or -1 where it is not asked for; the egos' stored index is
            # ignored (it may hold anything), an ego is a car
            column = np.asarray([self.categories.index(self._cat_of[c]) if c in self._cat_of else -1 for c in tr['categories']] + [car])
            src = tr['cat'].astype(np.int64)
            src[tr['agent_ptr'][:-1]] = len(tr['categories'])
            cat = column[src]
            use = (cat >= 0).astype(np.int32)
            cat = np.maximum(cat, 0).tolist()
            lw = tr['lw']
            for s, name in enumerate(names):
                self.scene2map[name] = (tr['scene_map'][s], scene_map[s])
                self.seq_map.extend((name, i) for i in range(0, scene_T[s] - self.seq_len, self.seq_interval))
        # ---- scenario scenes follow in the same tables ----
        for name, mname, traj, vis, slw, k in scenarios:
            if name in self.scene2map:
                raise ValueError('scenario %s has the name of an earlier scene' % name)
            names.append(name)
            scene_map.append(self.map_list.index(mname))
            scene_T.append(traj.shape[1])
            agent_ptr.append(agent_ptr[-1] + traj.shape[0])
            cat.extend(self.categories.index(c) for c in k)
            lw = np.concatenate([lw, slw], axis=0)
            self.scene2map[name] = (mname, scene_map[-1])
            self.seq_map.extend((name, i) for i in range(0, traj.shape[1] - self.seq_len, 1))
        S, A = len(names), len(cat)
        self._scene_index = {n: i for i, n in enumerate(names)}
        per_agent_T = np.repeat(np.asarray(scene_T, dtype=np.int64), np.diff(agent_ptr))
        row_ptr = np.concatenate([[0], np.cumsum(per_agent_T)])
        R = int(row_ptr[-1])
        self._scene_map_host = np.asarray(scene_map, dtype=np.int64)
        self._cat_host, self._lw_host = np.asarray(cat, dtype=np.int64), np.asarray(lw, dtype=np.float64).reshape(-1, 2)

        keep = self._keep = []

        def hold(t):
            keep.append(t)
            return t.data_ptr()

        traj_t = torch.empty((R, 6), dtype=torch.float64, device=dev)
        accel_t = torch.full((R, 2), float('nan'), dtype=torch.float64, device=dev)
        vis_t = torch.zeros((R,), dtype=torch.int32, device=dev)
        kept_t = torch.ones((A,), dtype=torch.int32, device=dev)
        tb = self._tables = L.StriveSceneTables()
        tb.S, tb.A, tb.R = S, A, R
        tb.agent_ptr, tb.scene_T, tb.scene_map = hold(i32(agent_ptr)), hold(i32(scene_T)), hold(i32(scene_map))
        tb.row_ptr, tb.cat, tb.lw = hold(i64(row_ptr[:-1] if A else row_ptr)), hold(i32(cat)), hold(f64(lw.reshape(-1, 2)))
        tb.traj, tb.accel, tb.is_vis, tb.kept = hold(traj_t), hold(accel_t), hold(vis_t), hold(kept_t)
        self.traj, self.accel, self.is_vis, self.kept = traj_t, accel_t, vis_t, kept_t
        self._row_ptr, self._agent_ptr = row_ptr, np.asarray(agent_ptr, dtype=np.int64)

        lib = ops._lib_for(traj_t)
        if tr is not None and A1 > 0:
            self._post_process(lib, tr, use, S1, A1, hold, i32, i64, f64)
        if scenarios:
            r0 = int(row_ptr[A1])
            traj_t[r0:] = f64(np.concatenate([t.reshape(-1, 6) for _, _, t, _, _, _ in scenarios], axis=0))
            vis_t[r0:] = i32(np.concatenate([v.reshape(-1) for _, _, _, v, _, _ in scenarios], axis=0))

        # ---- the agent count of every window: one launch, one read-back ----
        N = len(self.seq_map)
        seq = np.asarray([(self._scene_index[n], i) for n, i in self.seq_map], dtype=np.int32).reshape(-1, 2)
        self._seq = i32(seq)
        keep.append(self._seq)
        self._seq_scene = seq[:, 0].astype(np.int64)
        counts = torch.zeros((N,), dtype=torch.int32, device=dev)
        if N > 0:
            lib.call('strive_dataset_window_counts', C.byref(tb), L.ptr(self._seq), N, self.npast, self.nfuture, int(self.require_full_past),
                     L.ptr(counts), ops._stream(counts))
        self._counts = counts.cpu().numpy().astype(np.int64)
        if N > 0 and self._counts.min() < 1:
            raise L.StriveHipError('strive_dataset_window_counts: a window lies outside its scene')

    def _post_process(self, lib, tr, use, S1, A1, hold, i32, i64, f64):
        dev = self.device
        env = self.map_env
        pk = ops._map_pack(env, dev)
        layer_map = getattr(env, 'layer_map', None) or {}
        carpark = int(layer_map['carpark_area']) if 'carpark_area' in layer_map else -1
        if carpark == 0:
            raise ValueError('layer 0 is the drivable layer; carpark_area cannot be layer 0')
        mdx = float(torch.mean(env.nusc_dx))
        ego = np.zeros((A1,), dtype=bool)
        ego[tr['agent_ptr'][:-1]] = True
        sides = np.rint(tr['lw'][~ego] / mdx) if (~ego).any() else np.zeros((0, 2))
        nmax = int(sides.max()) if sides.size else 0
        if nmax > MAX_GRID or (sides.size and sides.min() < 0):
            raise ValueError('vehicle sizes give a sampling grid of %d samples a side (the limit is %d)' % (nmax, MAX_GRID))
        lin = torch.cat([torch.linspace(-1.0, 1.0, n) for n in range(nmax + 1)] + [torch.zeros((1,))])
        lin_off = np.concatenate([[0], np.cumsum(np.arange(nmax + 1))])[:nmax + 1]
        t = self._tracks_struct = L.StriveTracks()
        t.S, t.A, t.O = S1, A1, tr['obs'].shape[0]
        t.frame_ptr, t.ego_t, t.agent_ptr = hold(i32(tr['frame_ptr'])), hold(i64(tr['ego_t'])), hold(i32(tr['agent_ptr']))
        t.scene_map = self._tables.scene_map
        t.agent_scene = hold(i32(np.repeat(np.arange(S1), np.diff(tr['agent_ptr']))))
        t.use, t.lw = hold(i32(use)), hold(f64(tr['lw']))
        t.obs_ptr, t.obs_frame, t.obs = hold(i32(tr['obs_ptr'])), hold(i32(tr['obs_frame'])), hold(f64(tr['obs'].reshape(-1, 5)))
        lin_d, off_d = params.upload(lin.contiguous(), dev), i32(lin_off)
        ws_bytes = max(int(self._tables.R) * 8 * 8, 8)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        lib.call('strive_dataset_post_process', C.byref(t), pk.ref(), C.byref(self._tables), carpark, mdx, L.ptr(off_d), L.ptr(lin_d), nmax,
                 L.ptr(ws), ws_bytes, ops._stream(ws))
        self._keep.extend([lin_d, off_d, ws, pk])

    # ------------------------------------------------------------------------------------------------
    # batches
    # ------------------------------------------------------------------------------------------------
    def batch_ptr(self, idx):
        """Host ``ptr`` (B+1) of the batch of windows ``idx``: known without touching the device."""
        return np.concatenate([[0], np.cumsum(self._counts[np.asarray(idx, dtype=np.int64)])])

    def get_batch(self, idx, generator=None):
        """``(Batch, map_idx (B,) long)`` of the windows ``idx``, assembled on the device by one launch."""
        idx = [int(i) for i in idx]
        B = len(idx)
        if B == 0:
            raise ValueError('an empty batch')
        for i in idx:
            if i < 0 or i >= self.data_len:
                raise IndexError('window %d of %d' % (i, self.data_len))
        dev = self.device
        ptr = self.batch_ptr(idx)
        n = np.diff(ptr)
        eptr = np.concatenate([[0], np.cumsum(n * (n - 1))])
        NA, E = int(ptr[-1]), int(eptr[-1])
        meta_cpu = torch.from_numpy(np.stack([np.asarray(idx + [0], dtype=np.int64), ptr.astype(np.int64), eptr.astype(np.int64)]))
        meta = params.upload(meta_cpu, dev)
        PT, FT, NC = self.npast, self.nfuture, len(self.categories)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)       # noqa: E731
        g = Batch(x=f32(NA), pos=f32(NA), edge_index=torch.empty((2, E), dtype=torch.long, device=dev), past=f32(NA, PT, 6),
                  past_gt=f32(NA, PT, 6), future=f32(NA, FT, 6), future_gt=f32(NA, FT, 6), sem=f32(NA, NC), lw=f32(NA, 2),
                  past_vis=f32(NA, PT), future_vis=f32(NA, FT))
        g.batch = torch.empty((NA,), dtype=torch.long, device=dev)
        g.ptr = meta[1]
        g.num_graphs = B
        map_idx = torch.empty((B,), dtype=torch.long, device=dev)
        lib = ops._lib_for(g.past)
        lib.call('strive_dataset_gather_batch', C.byref(self._tables), L.ptr(self._seq), L.ptr(meta), B, PT, FT, NC,
                 int(self.require_full_past), C.byref(self._norm), L.ptr(g.past), L.ptr(g.past_gt), L.ptr(g.future), L.ptr(g.future_gt),
                 L.ptr(g.lw), L.ptr(g.sem), L.ptr(g.past_vis), L.ptr(g.future_vis), L.ptr(g.batch), L.ptr(map_idx),
                 L.ptr(g.edge_index), E, ops._stream(g.past))
        if self.noise_std > 0:
            self._add_noise(g, generator)
        ops.prime_scene_info(g, meta_cpu[1].clone(), clique_by_construction=True)
        return g, map_idx

    def _add_noise(self, g, generator):
        """Gaussian noise on the observed states (reference :666-676): torch ops after the launch, under the caller's generator."""
        def randn(t):
            return torch.randn(t.shape, generator=generator, device=t.device, dtype=t.dtype)
        g.past += randn(g.past) * self.noise_std
        g.future += randn(g.future) * self.noise_std
        for t in (g.past, g.future):
            t[:, :, 2:4] = t[:, :, 2:4] / torch.norm(t[:, :, 2:4], dim=-1, keepdim=True)
            t[:, :, :2] = torch.clamp(t[:, :, :2], min=0.0)
        g.lw += randn(g.lw) * self.noise_std

    def __getitem__(self, idx):
        """``(Data, map_idx)`` of one window with the reference's keys and dtypes (:689-704), on the dataset's device."""
        if idx < 0:
            idx += self.data_len
        g, _ = self.get_batch([idx])
        d = Data(**{k: g[k] for k in ('x', 'pos', 'edge_index', 'past', 'past_gt', 'future', 'future_gt', 'sem', 'lw', 'past_vis', 'future_vis')})
        return d, int(self._scene_map_host[self._seq_scene[idx]])

    def loader(self, batch_size, shuffle=False, drop_last=False, generator=None):
        """What ``DataLoader(dataset, batch_size, shuffle, drop_last)`` yields in the reference, ``(Batch, map_idx)``, straight from the
        gather kernel; ``generator``: a host torch.Generator for the shuffle only.  With ``noise_std > 0`` the loader's batches draw
        their noise from the device's default generator (seed it with ``torch.manual_seed``); ``get_batch(idx, generator=...)`` takes
        a device generator of the caller's."""
        return _Loader(self, batch_size, shuffle, drop_last, generator)
