"""strive_amd/train_traffic.py: the host logic of the training driver with a stub model / loss / loader (no kernels), and the driver
end to end on a tracks file -- on the MI355X, and (``slow``) on the host emulation."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CFG = os.path.join(GOLDEN, 'g21_train_traffic.cfg')


# ------------------------------------------------------------------------------------------------
# stubs: everything DataParallelTrainer.step and run_one_epoch touch, in plain torch
# ------------------------------------------------------------------------------------------------

class StubGraph(object):
    def __init__(self, n, seed, boom=None):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn((n, 6), generator=g)
        self.ptr = torch.tensor([0, n])
        self.future_vis = torch.ones((n, 2))
        self.boom = boom

    def to(self, device):
        return self


class StubModel(torch.nn.Module):
    FT = 2

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(6, 4)

    def get_normalizer(self):
        return None

    def forward(self, scene_graph, map_idx, map_env, future_sample=False):
        if scene_graph.boom is not None:
            raise scene_graph.boom
        return {'y': self.a(scene_graph.x)}


class StubLoss(object):
    """per-element terms of a different length per batch; ``eval_losses``: the values 'loss' takes in successive validation batches"""

    def __init__(self, eval_losses=None):
        self.loss_weights = {'recon': 1.0, 'kl': 0.004, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0}
        self.eval_losses = list(eval_losses) if eval_losses is not None else None
        self.seen = []

    def __call__(self, scene_graph, pred, map_idx=None, map_env=None):
        y = pred['y']
        out = {'recon_loss': (y ** 2).sum(1), 'kl_loss': y.abs().sum(1)}
        if not torch.is_grad_enabled() and self.eval_losses is not None:
            out['loss'] = torch.tensor([self.eval_losses.pop(0)])
        else:
            out['loss'] = (y ** 2).reshape(-1).detach() * 3.0 + 1.0          # one value per element: batches of different sizes
        self.seen.append(out['loss'].detach().double().numpy().copy())
        return out

    def compute_err(self, scene_graph, pred, normalizer):
        return {'pos_err': pred['y'].detach().abs().reshape(-1)}


def _loader(sizes, boom_at=None, boom=None):
    return [(StubGraph(n, 10 + i, boom if i == boom_at else None), torch.zeros((1,), dtype=torch.long)) for i, n in enumerate(sizes)]


def _cfg(tmp_path, **kw):
    cfg = {'out': str(tmp_path), 'epochs': 7, 'kl_anneal_end': 4, 'loss_kl': 0.004, 'val_every': 2, 'save_every': 3, 'print_every': 0}
    cfg.update(kw)
    return cfg


def _lines(tmp_path):
    return open(os.path.join(str(tmp_path), 'log.txt')).read().splitlines()


def _run_loop(tmp_path, cfg, model, loss, opt, train, val, **kw):
    from strive_amd import train_traffic as T
    with open(os.path.join(str(tmp_path), 'log.txt'), 'w') as log:
        return T.train_loop(cfg, model, loss, opt, train, val, None, None, 'cpu', log, **kw)


def test_kl_schedule_best_loss_reset_and_checkpoint_arithmetic(tmp_path):
    from strive_amd.utils.torch import compute_kl_weight, load_state
    model = StubModel()
    # validations at epochs 0, 2, 4, 6: 5 (best), 3 (best), 4 (best again: the tracking was reset at kl_anneal_end = 4), 6 (not)
    loss = StubLoss(eval_losses=[5.0, 3.0, 4.0, 6.0])
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    cfg = _cfg(tmp_path)
    steps, best = _run_loop(tmp_path, cfg, model, loss, opt, _loader([3, 2]), _loader([2]))
    lines = _lines(tmp_path)
    assert steps == 7 * 2 and best == 4.0                           # step_counter: one scene per stepped batch
    assert [l for l in lines if l.startswith('KL weight')] == ['KL weight %f...' % compute_kl_weight(e, 4, 0.004) for e in range(7)]
    assert [float(l.split()[2][:-3]) for l in lines if l.startswith('KL weight')] == pytest.approx([0.0, 0.001, 0.002, 0.003, 0.004, 0.004, 0.004])
    assert loss.loss_weights['kl'] == 0.004
    assert lines.count('Using KL annealing...') == 1 and lines.count('KL ANNEALING FINISHED: resetting val loss tracking...') == 1
    assert lines.index('KL ANNEALING FINISHED: resetting val loss tracking...') == lines.index('Starting epoch 4...') + 2
    assert lines.count('Validating...') == 4 and lines.count('Lowest eval loss so far! Saving checkpoint...') == 3
    assert lines.count('Saving checkpoint...') == 3                 # epochs 0, 3, 6
    assert sorted(os.listdir(os.path.join(str(tmp_path), 'checkpoints'))) == [
        'best_eval_model.pth', 'epoch_00000000_model.pth', 'epoch_00000003_model.pth', 'epoch_00000006_model.pth', 'latest_model.pth']
    ck = os.path.join(str(tmp_path), 'checkpoints')
    fresh = StubModel()
    assert load_state(os.path.join(ck, 'best_eval_model.pth'), fresh) == (4, 4.0)
    assert load_state(os.path.join(ck, 'latest_model.pth'), fresh) == (6, 4.0)
    assert load_state(os.path.join(ck, 'epoch_00000003_model.pth'), fresh) == (3, 3.0)
    load_state(os.path.join(ck, 'latest_model.pth'), fresh)
    assert all(torch.equal(fresh.state_dict()[k], v) for k, v in model.state_dict().items())
    # resume at the checkpoint's epoch (the reference's range(ckpt_epoch, epochs)), with its best loss
    ep, best0 = load_state(os.path.join(ck, 'latest_model.pth'), fresh)
    loss2 = StubLoss(eval_losses=[3.5, 9.0])
    _run_loop(tmp_path, _cfg(tmp_path, epochs=9), fresh, loss2, torch.optim.SGD(fresh.parameters(), lr=0.01), _loader([3]), _loader([2]),
              ckpt_epoch=ep, ckpt_eval_loss=best0)
    lines = _lines(tmp_path)
    assert [l for l in lines if l.startswith('Starting epoch')] == ['Starting epoch 6...', 'Starting epoch 7...', 'Starting epoch 8...']
    assert lines.count('Lowest eval loss so far! Saving checkpoint...') == 1        # 3.5 < 4.0 at epoch 6; 9.0 at epoch 8 is not
    # without a validation loader nothing validates
    _run_loop(tmp_path, _cfg(tmp_path, epochs=2), StubModel(), StubLoss(), torch.optim.SGD(model.parameters(), lr=0.01), _loader([3]), None)
    assert 'Validating...' not in _lines(tmp_path)


def test_a_runtime_error_skips_the_batch_and_anything_else_propagates(tmp_path):
    from strive_amd import train_traffic as T
    model = StubModel()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    loss = StubLoss()
    with open(os.path.join(str(tmp_path), 'log.txt'), 'w') as log:
        before = [p.detach().clone() for p in model.parameters()]
        steps, mean = T.run_one_epoch(_loader([3], 0, RuntimeError('injected failure')), model, None, loss, 'cpu', str(tmp_path),
                                      train=True, optimizer=opt, step_counter=5, log=log)
        assert steps == 5 and np.isnan(mean) and all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        steps, mean = T.run_one_epoch(_loader([3, 2, 4], 1, RuntimeError('injected failure')), model, None, loss, 'cpu', str(tmp_path),
                                      train=True, optimizer=opt, step_counter=5, log=log)
        assert steps == 7 and np.isfinite(mean)
        # validation skips it too
        with torch.no_grad():
            steps, _ = T.run_one_epoch(_loader([3, 2], 0, RuntimeError('injected failure')), model, None, loss, 'cpu', str(tmp_path),
                                       train=False, step_counter=7, log=log)
        assert steps == 7
        with pytest.raises(KeyError):
            T.run_one_epoch(_loader([3, 2], 1, KeyError('not a RuntimeError')), model, None, loss, 'cpu', str(tmp_path), train=True,
                            optimizer=opt, log=log)
        with pytest.raises(ValueError):
            T.run_one_epoch(_loader([3]), model, None, loss, 'cpu', str(tmp_path), train=True, optimizer=None, log=log)
    lines = _lines(tmp_path)
    assert lines.count('Caught error in training batch injected failure!') == 3 and lines.count('Skipping') == 3


@pytest.mark.parametrize('train', [True, False])
def test_epoch_means_are_means_over_concatenated_elements(tmp_path, train):
    from strive_amd import train_traffic as T
    model = StubModel()
    loss = StubLoss()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    with open(os.path.join(str(tmp_path), 'log.txt'), 'w') as log:
        _, mean = T.run_one_epoch(_loader([1, 7, 2]), model, None, loss, 'cpu', str(tmp_path), train=train,
                                  optimizer=opt if train else None, log=log)
    want = float(np.mean(np.concatenate(loss.seen)))
    of_batch_means = float(np.mean([s.mean() for s in loss.seen]))
    assert abs(mean - want) <= 1e-12 * abs(want) and abs(want - of_batch_means) > 1e-3 * abs(want)
    lines = _lines(tmp_path)
    prefix = 'Train' if train else 'Eval'
    assert [l.split(' = ')[0] for l in lines if ' Epoch Mean ' in l] == [prefix + ' Epoch Mean ' + k for k in ('recon_loss', 'kl_loss', 'loss', 'pos_err')]


def test_dense_error_terms_equal_compute_err():
    """run_one_epoch forms TrafficModelLoss's error terms dense with the visibility mask (no boolean indexing, no read-back): their
    masked float64 sums and counts in the accumulators equal those of compute_err's compacted terms, with frames that are not
    visible -- one of them NaN in the ground truth -- left out"""
    from strive_amd import synth, test_traffic as TT, train_traffic as T
    from strive_amd.constants import state_norm_tensors
    from strive_amd.datasets.utils import MeanStdNormalizer
    from strive_amd.losses.traffic_model import TrafficModelLoss
    batch, _ = synth.make_batch([3, 2], key='train_traffic/err', FT=5)
    NA = batch.past.shape[0]
    batch.future_vis[0, 1:3] = 0.0
    batch.future_vis[4, 4] = 0.0
    batch.future_gt[0, 2] = float('nan')
    assert 0 < int((batch.future_vis == 1.0).sum()) < batch.future_vis.numel()
    g = torch.Generator().manual_seed(4)
    rnd = lambda *shape: torch.randn(shape, generator=g)
    pred = {'future_pred': batch.future_gt[..., :4].nan_to_num(0.0) + 0.3 * rnd(NA, 5, 4), 'prior_out': (rnd(NA, 32), rnd(NA, 32).abs() + 0.1),
            'posterior_out': (rnd(NA, 32), rnd(NA, 32).abs() + 0.1)}
    norm = MeanStdNormalizer(*state_norm_tensors())
    loss_fn = TrafficModelLoss({'recon': 1.0, 'kl': 1.0, 'coll_veh_prior': 0.0, 'coll_env_prior': 0.0})
    want = loss_fn.compute_err(batch, pred, norm)
    got, masks = T._err_terms(loss_fn, batch, pred, norm)
    assert list(got) == list(want) and set(masks) == {'pos_err', 'ang_err'}
    acc = TT._Accumulators(torch.device('cpu'))
    for k, v in got.items():
        acc.add(k, v, masks.get(k))
    for k, w in want.items():
        assert bool(torch.isfinite(w).all()) and int(acc.counts[k]) == w.numel(), k
        assert abs(float(acc.sums[k]) - float(w.double().sum())) <= 1e-12 * float(w.double().abs().sum()), k
    assert float(acc.sums['pos_err']) > 0.0 and float(acc.sums['ang_err']) > 0.0


def test_config_file(tmp_path):
    from strive_amd import train_traffic as T
    cfg, ignored = T.parse_cfg(['--config', CFG])
    assert ignored == ['data_dir', 'data_version']
    assert (cfg['out'], cfg['data_noise_std'], cfg['batch_size'], cfg['epochs'], cfg['lr']) == ('./out/train_traffic_out', 0.01, 4, 200, 1e-5)
    assert (cfg['loss_kl'], cfg['kl_anneal_end'], cfg['loss_recon'], cfg['loss_veh_coll_prior'], cfg['loss_env_coll_prior']) == (0.004, 20, 1.0, 0.05, 0.1)
    # the reference's defaults where the file is silent
    assert (cfg['val_every'], cfg['save_every'], cfg['print_every'], cfg['weight_decay'], cfg['past_len'], cfg['future_len']) == (3, 3, 10, 0.0, 4, 12)
    assert (cfg['map_obs_size_pix'], cfg['latent_size'], cfg['num_classes'], cfg['scenario_dir'], cfg['ckpt']) == (256, 32, 2, None, None)
    assert cfg['optim'] == T.DEFAULT_OPTIM
    # the command line overrides the file
    cfg, _ = T.parse_cfg(['--config', CFG, '--lr', '3e-4', '--epochs', '2', '--out', 'elsewhere', '--agent_types', 'car', 'truck', 'bus'])
    assert (cfg['lr'], cfg['epochs'], cfg['out'], cfg['batch_size'], cfg['num_classes']) == (3e-4, 2, 'elsewhere', 4, 3)
    # without a file: the parser's defaults
    assert T.parse_cfg([])[0]['lr'] == 1e-5
    bad = tmp_path / 'bad.cfg'
    bad.write_text('# a comment\nlr: 1e-4   # trailing comment\nno_such_key: 3\n')
    with pytest.raises(ValueError, match='no_such_key'):
        T.parse_cfg(['--config', str(bad)])
    ok = tmp_path / 'ok.cfg'
    ok.write_text('lr: 1e-4   # trailing comment\n\nnum_workers: 8\nmap_layers: [drivable_area, carpark_area]\nwandb_project: x\nagent_types: [car, truck]\n')
    cfg, ignored = T.parse_cfg(['--config', str(ok)])
    assert cfg['lr'] == 1e-4 and ignored == ['num_workers', 'map_layers', 'wandb_project'] and cfg['agent_types'] == ['car', 'truck']
    noline = tmp_path / 'noline.cfg'
    noline.write_text('lr 1e-4\n')
    with pytest.raises(ValueError, match='key: value'):
        T.parse_cfg(['--config', str(noline)])


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------

LINE_KINDS = ('Args: ', 'Using device ', 'Num model params: ', 'Using KL annealing...', 'Starting epoch 0...', 'KL weight ', 'Epoch time: ',
              'Validating...', 'Lowest eval loss so far! Saving checkpoint...', 'Saving checkpoint...', 'Train Epoch Mean loss = ',
              'Eval Epoch Mean loss = ', 'Train Epoch Mean pos_err = ')


def _end_to_end(tmp_path, device, optim, tracks, extra, epochs, model_kw, capsys=None):
    """train ``epochs`` epochs, check the log, the checkpoints and the evaluation of the last one, then resume for one more epoch"""
    from strive_amd import eval_traffic_tracks, train_traffic as T
    from strive_amd.datasets import tracks as tracks_io
    from strive_amd.models.traffic_model import TrafficModel
    from strive_amd.utils.torch import load_state
    path = str(tmp_path / 'tracks.npz')
    tracks_io.save_tracks(path, tracks)
    out = str(tmp_path / ('out_' + optim))
    init = {}
    make0 = T.make_optimizer

    def recording(kind, model, lr, wd):
        init.update({n: p.detach().clone() for n, p in model.named_parameters()})
        return make0(kind, model, lr, wd)
    args = ['--tracks', path, '--val_tracks', path, '--out', out, '--val_every', '1', '--save_every', '1', '--data_noise_std', '0.01',
            '--optim', optim, '--device', device] + extra
    T.make_optimizer = recording
    try:
        T.main(args + ['--epochs', str(epochs)])
    finally:
        T.make_optimizer = make0
    log = open(os.path.join(out, 'train_log.txt')).read()
    for kind in LINE_KINDS:
        assert ('\n' + kind) in ('\n' + log), 'no `%s` line in the log' % kind
    assert 'Caught error' not in log, log
    ck = os.path.join(out, 'checkpoints')
    names = ['best_eval_model.pth', 'latest_model.pth'] + ['epoch_%08d_model.pth' % e for e in range(epochs)]
    assert sorted(os.listdir(ck)) == sorted(names)
    for name in names:
        m = TrafficModel(*model_kw).to(device)
        o = torch.optim.Adam(m.parameters(), lr=1e-5)
        ep, best = load_state(os.path.join(ck, name), m, optimizer=o, map_location=device)
        assert 0 <= ep < epochs and np.isfinite(best)
        assert len(o.state_dict()['state']) == len(list(m.parameters())) == 174
    sd = torch.load(os.path.join(ck, 'latest_model.pth'), map_location='cpu')
    assert sd['epoch'] == epochs - 1
    for n, p0 in init.items():
        p1 = sd['model'][n]
        assert bool(torch.isfinite(p1).all()), n
        # (a run that ends with epoch 0 has trained at KL weight 0 -- compute_kl_weight(0, ...) -- and the prior network's only other
        #  gradient comes from the collision terms of the prior sample, which may all be zero: it need not have moved)
        if epochs > 1 or not n.startswith('prior_net.'):
            assert not torch.equal(p1, p0.cpu()), 'parameter %s did not move' % n
    ev = eval_traffic_tracks.main(['--ckpt', os.path.join(ck, 'latest_model.pth'), '--tracks', path, '--out', str(tmp_path / ('eval_' + optim)),
                                   '--device', device] + _eval_args(extra))
    assert np.isfinite(ev['Test Mean loss'])
    # resume: starts at the checkpoint's epoch (the reference's range(ckpt_epoch, epochs)) and runs exactly one epoch beyond it,
    # with the OTHER optimiser class reading the checkpoint's optimiser state
    other = 'torch' if optim == 'flat' else 'flat'
    T.main(args[:args.index('--optim')] + ['--optim', other, '--device', device] + extra +
           ['--epochs', str(epochs + 1), '--ckpt', os.path.join(ck, 'latest_model.pth')])
    resumed = open(os.path.join(out, 'train_log.txt')).read()[len(log):]
    assert re.findall(r'^Starting epoch (\d+)\.\.\.$', resumed, re.M) == [str(epochs - 1), str(epochs)]
    assert 'Loaded checkpoint from epoch %d' % (epochs - 1) in resumed
    assert os.path.exists(os.path.join(ck, 'epoch_%08d_model.pth' % epochs))
    assert torch.load(os.path.join(ck, 'latest_model.pth'), map_location='cpu')['epoch'] == epochs


def _eval_args(extra):
    """the model-shape arguments of the training command line that eval_traffic_tracks takes too"""
    out, it = [], iter(extra)
    for a in it:
        v = next(it)
        if a in ('--future_len', '--past_len', '--batch_size'):
            out += [a, v]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('optim', ['flat', 'torch'])
def test_gpu_train_traffic_end_to_end(tmp_path, optim):
    from strive_amd import synth
    _end_to_end(tmp_path, 'cuda:0', optim, synth.make_tracks(n_scenes=2, n_agents=4, T=24), ['--batch_size', '4'], 2,
                (4, 12, 256, 2))


@pytest.fixture
def emu_everywhere():
    import build as emu_build
    from strive_amd import _lib as L, ops
    emu = L.StriveLib(emu_build.build(), require_all=True)
    orig = (ops._lib_for, L.get_lib)
    ops._lib_for = lambda *tensors: emu           # CPU tensors + the emulated library: test infrastructure only
    L.get_lib = lambda: emu
    yield emu
    ops._lib_for, L.get_lib = orig


@pytest.mark.slow
def test_emulated_train_traffic_end_to_end(tmp_path, emu_everywhere):
    """one epoch of two batches of at most 3 agents at FT 2 through the host emulation of the same kernels"""
    from strive_amd import synth
    _end_to_end(tmp_path, 'cpu', 'flat', synth.make_tracks(n_scenes=2, n_agents=2, T=7), ['--batch_size', '1', '--future_len', '2'], 1,
                (4, 2, 256, 2))
