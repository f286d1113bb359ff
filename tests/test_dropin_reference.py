"""Drop-in check of the boundary, ``strive_amd.dropin.install``, in both of its modes.

Next to a checkout of the reference (``install(reference_src=...)``): the hot-path packages are replaced by this package's,
the mixed modules are the reference's files with this package's functions laid over them, everything else stays the reference's
own file, and the loop drivers are this package's or (``loops='reference'``) the reference's.  The reference is not part of this
repository, so these tests write a small synthetic ``src/`` tree of the same layout (stub modules of their own, nothing of the
reference) and check which owner every name resolves to, and that a loop function living in that tree runs through the
reference's import names on this package's HIP-backed modules.

Without a checkout (``install()``): the names resolve to this package alone, and ``run_adv_gen_optim`` reached through them
gives what the reference's OWN function gave on the same scene (fixture g13, tests/golden/make_golden.py::g13_dropin, generated
by running the reference).

No GPU here, so the C ABI behind those modules is the host-emulation build of the same .hip sources (tests/hipemu) -- these
tests are about names, signatures, dict keys, tensor shapes, autograd plumbing and the numbers coming out, not about speed."""
import contextlib
import io
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))

ROOTS = ('models', 'losses', 'utils', 'datasets', 'planners', 'torch_geometric')


@contextlib.contextmanager
def _names_installed(**kw):
    """dropin.install(**kw) for the duration of the block; the import names it defined are forgotten afterwards."""
    from strive_amd import dropin
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] in ROOTS}
    try:
        yield dropin.install(**kw)
    finally:
        for k in list(sys.modules):
            if k.split('.')[0] in ROOTS:
                del sys.modules[k]
        sys.modules.update(saved)


@pytest.fixture(scope='module')
def emu():
    import build as emu_build
    from strive_amd import _lib as L, ops
    lib = L.StriveLib(emu_build.build(), require_all=True)
    orig = (ops._lib_for, L.get_lib)
    ops._lib_for = lambda *tensors: lib           # CPU tensors + the emulated library: test infrastructure only
    L.get_lib = lambda: lib
    yield lib
    ops._lib_for, L.get_lib = orig


@pytest.fixture(scope='module')
def dropin_env(emu):
    with _names_installed() as names:
        yield names


# the synthetic reference tree: the layout of the reference's src/ (utils/, datasets/), stub modules written for this test
SYNTHETIC_SRC = {
    'utils/__init__.py': '',
    'utils/logger.py': 'class Logger(object):\n    pass\n',
    'utils/scenario_gen.py': (
        'def detach_embed_info(embed_info):\n'
        '    raise AssertionError("laid over by strive_amd.utils.scenario_gen")\n\n\n'
        'def log_metric(*args, **kwargs):\n'
        '    return "kept"\n'),
    'utils/init_optim.py': 'def run_init_optim(*args, **kwargs):\n    return "synthetic"\n',
    'utils/sol_optim.py': 'def run_find_solution_optim(*args, **kwargs):\n    return "synthetic"\n',
    # a loop function on the reference's side: it only knows the reference's import names
    'utils/adv_gen_optim.py': (
        'import torch\n'
        'from losses.adv_gen_nusc import AvoidCollLoss\n'
        'from utils.scenario_gen import detach_embed_info\n\n\n'
        'def run_adv_gen_optim(*args, **kwargs):\n'
        '    return "synthetic"\n\n\n'
        'def refine_iterations(model, scene_graph, map_idx, map_env, z_init, weights, num_iters, lr):\n'
        '    with torch.no_grad():\n'
        '        emb = detach_embed_info(model.embed(scene_graph, map_idx, map_env))\n'
        '    z = z_init.clone().detach().requires_grad_(True)\n'
        '    opt = torch.optim.Adam([z], lr=lr)\n'
        '    loss_fn = AvoidCollLoss(weights, model.get_att_normalizer().unnormalize(scene_graph.lw), map_idx[scene_graph.batch],\n'
        '                            map_env, z_init.clone().detach(), veh_coll_buffer=0.2)\n'
        '    for _ in range(num_iters):\n'
        '        opt.zero_grad()\n'
        '        pred = model.decode_embedding(z, emb, scene_graph, map_idx, map_env, nfuture=model.FT)["future_pred"]\n'
        '        loss = loss_fn(model.get_normalizer().unnormalize(pred), z, emb["prior_out"])\n'
        '        loss["loss"].backward()\n'
        '        opt.step()\n'
        '    return z.detach(), emb\n'),
    'datasets/__init__.py': '',
    'datasets/utils.py': (
        'class MeanStdNormalizer(object):\n'
        '    pass\n\n\n'
        'def kept_helper():\n'
        '    return "kept"\n'),
    # imports a name of a module overlaid before it (dependency order)
    'datasets/nuscenes_utils.py': (
        'from datasets.utils import MeanStdNormalizer\n\n\n'
        'def get_map_obs(*args, **kwargs):\n'
        '    raise AssertionError("laid over by strive_amd.datasets.nuscenes_utils")\n\n\n'
        'def kept_helper():\n'
        '    return "kept"\n'),
    'datasets/map_env.py': 'class NuScenesMapEnv(object):\n    pass\n',
}


@pytest.fixture
def reference_tree(tmp_path):
    src = tmp_path / 'src'
    for rel, text in SYNTHETIC_SRC.items():
        (src / rel).parent.mkdir(parents=True, exist_ok=True)
        (src / rel).write_text(text)
    return str(src)


def _in_tree(mod, src):
    return os.path.abspath(mod.__file__).startswith(os.path.abspath(src) + os.sep)


def _assert_reference_mode_owners(src, names):
    import models.traffic_model, models.interaction_net, losses.adv_gen_nusc, losses.traffic_model   # noqa: E401
    import utils.transforms, utils.logger, utils.scenario_gen, datasets.utils, datasets.nuscenes_utils, datasets.map_env  # noqa: E401
    import torch_geometric.data
    from strive_amd import graph
    # replaced entirely
    assert models.traffic_model.__name__ == 'strive_amd.models.traffic_model'
    assert models.interaction_net.__name__ == 'strive_amd.models.interaction_net'
    assert losses.adv_gen_nusc.__name__ == 'strive_amd.losses.adv_gen_nusc'
    assert losses.traffic_model.__name__ == 'strive_amd.losses.traffic_model'
    assert utils.transforms.__name__ == 'strive_amd.utils.transforms'
    assert torch_geometric.data.Batch is graph.Batch
    # the reference's own files, everything off the hot path
    assert _in_tree(utils.logger, src) and _in_tree(datasets.map_env, src)
    # the reference's files with ours laid over the same names, theirs kept
    for mod, ours in ((utils.scenario_gen, 'strive_amd.utils.scenario_gen'), (datasets.utils, 'strive_amd.datasets.utils'),
                      (datasets.nuscenes_utils, 'strive_amd.datasets.nuscenes_utils')):
        assert _in_tree(mod, src), mod.__file__
        assert mod.__strive_amd_overlay__ == ours
    assert utils.scenario_gen.detach_embed_info.__module__ == 'strive_amd.utils.scenario_gen'
    assert utils.scenario_gen.log_metric() == 'kept' and utils.scenario_gen.log_metric.__module__ == 'utils.scenario_gen'
    assert datasets.utils.MeanStdNormalizer.__module__ == 'strive_amd.datasets.utils'
    assert datasets.utils.kept_helper() == 'kept'
    assert datasets.nuscenes_utils.get_map_obs.__module__ == 'strive_amd.datasets.nuscenes_utils'
    assert datasets.nuscenes_utils.kept_helper() == 'kept'
    # datasets.utils is overlaid before datasets.nuscenes_utils is executed: its import of MeanStdNormalizer got ours
    assert vars(datasets.nuscenes_utils)['MeanStdNormalizer'].__module__ == 'strive_amd.datasets.utils'
    assert set(names) >= {'models.traffic_model', 'losses.adv_gen_nusc', 'utils.scenario_gen', 'datasets.utils',
                          'datasets.nuscenes_utils', 'utils.init_optim', 'utils.adv_gen_optim', 'utils.sol_optim'}


def test_names_resolve_to_the_right_owner(emu, reference_tree):
    """install(reference_src=..., loops='reference'): replaced, overlaid and kept modules, and the reference's own loop drivers,
    whose module-level imports of the reference's names reach this package."""
    with _names_installed(reference_src=reference_tree, loops='reference') as names:
        _assert_reference_mode_owners(reference_tree, names)
        import utils
        import utils.init_optim, utils.adv_gen_optim, utils.sol_optim   # noqa: E401
        from strive_amd.losses import adv_gen_nusc
        for mod in (utils.init_optim, utils.adv_gen_optim, utils.sol_optim):
            assert _in_tree(mod, reference_tree), mod.__file__                   # the reference's own files
        assert utils.adv_gen_optim.run_adv_gen_optim() == 'synthetic'
        assert utils.adv_gen_optim.AvoidCollLoss is adv_gen_nusc.AvoidCollLoss
        assert utils.adv_gen_optim.detach_embed_info.__module__ == 'strive_amd.utils.scenario_gen'
        assert utils.adv_gen_optim is sys.modules['utils.adv_gen_optim']


def test_names_resolve_with_this_packages_loops(emu, reference_tree):
    """install(reference_src=...) with the default loops='strive_amd': the same owners, the loop drivers are this package's."""
    with _names_installed(reference_src=reference_tree) as names:
        _assert_reference_mode_owners(reference_tree, names)
        import utils
        import utils.init_optim, utils.adv_gen_optim, utils.sol_optim   # noqa: E401
        for mod in (utils.init_optim, utils.adv_gen_optim, utils.sol_optim):
            assert mod.__name__.startswith('strive_amd.utils.'), mod.__name__
            assert getattr(utils, mod.__name__.rsplit('.', 1)[1]) is mod
        assert utils.adv_gen_optim.run_adv_gen_optim.__module__ == 'strive_amd.utils.adv_gen_optim'


def test_install_refuses_bad_arguments(tmp_path):
    from strive_amd import dropin
    with pytest.raises(ValueError):
        dropin.install(loops='reference')                       # the reference's loops need the reference's tree
    with pytest.raises(ValueError):
        dropin.install(loops='other')
    with pytest.raises(FileNotFoundError):
        dropin.install(reference_src=str(tmp_path))             # no utils/ and datasets/ there


def test_reference_side_loop_runs_on_the_hip_modules(emu, reference_tree):
    """A loop function of the reference's tree (loops='reference'), which knows only the reference's import names, runs on this
    package's HIP-backed TrafficModel and AvoidCollLoss: 2 Adam iterations on the drop-in scene, against the oracle's refine loop."""
    import make_golden as mg
    from strive_amd import synth
    from oracle import loops as oloops
    from util import assert_close
    with _names_installed(reference_src=reference_tree, loops='reference'):
        import utils.adv_gen_optim as theirs
        m, sd, batch, map_idx, env = _setup()
        assert type(m).__module__ == 'strive_amd.models.traffic_model'
        with torch.no_grad():
            pm, pv = m.embed(batch, map_idx, env)['prior_out']
        z0 = synth.make_latents(pm, pv, key='dropin/z')
        z, emb = theirs.refine_iterations(m, batch, map_idx, env, z0, mg.REFINE_WEIGHTS, 2, 0.05)
    assert z.shape == z0.shape and torch.isfinite(z).all()
    orc = _oracle(sd, mg.DROPIN_FT)
    with torch.no_grad():
        emb_o = orc.embed(batch, map_idx, env)
    assert_close(emb['map_feat'], emb_o['map_feat'], 1e-4, 2e-5, 'map_feat')
    z_o = oloops.refine_loop(orc, batch, map_idx, env, emb_o, z0, mg.REFINE_WEIGHTS, 2, 0.05, mg.DROPIN_FT)
    # (each iteration moves every entry by ~lr = 0.05)
    assert_close(z, z_o, 0, 1e-4, 'z after 2 iterations of the reference-side loop against the oracle')


def _setup():
    import make_golden as mg
    from models.traffic_model import TrafficModel                 # resolves to strive_amd's
    from datasets.utils import MeanStdNormalizer                   # resolves to strive_amd's (both modes)
    from strive_amd import synth
    from strive_amd.constants import NUSC_BIKE_PARAMS, state_norm_tensors, att_norm_tensors
    m = TrafficModel(4, mg.DROPIN_FT, 256, 2)
    sd = synth.fill_state_dict(m.state_dict())
    m.load_state_dict(sd)
    m.set_normalizer(MeanStdNormalizer(*state_norm_tensors()))
    m.set_att_normalizer(MeanStdNormalizer(*att_norm_tensors()))
    m.set_bicycle_params(NUSC_BIKE_PARAMS)
    m.eval()
    batch, map_idx, raster, dx = mg.g13_inputs()
    env = synth.SyntheticMapEnv(raster, dx)
    return m, sd, batch, map_idx, env


def test_default_install_names_resolve_to_this_package(dropin_env):
    """install() without a checkout: every name is this package's; the reference's other files do not exist."""
    import models.traffic_model, losses.adv_gen_nusc, utils.adv_gen_optim, utils.sol_optim, utils.init_optim   # noqa: E401
    import utils.scenario_gen, datasets.nuscenes_utils, datasets.utils, planners.hardcode_goalcond_nusc        # noqa: E401
    import torch_geometric.data
    assert models.traffic_model.__name__ == 'strive_amd.models.traffic_model'
    assert losses.adv_gen_nusc.__name__ == 'strive_amd.losses.adv_gen_nusc'
    for mod in (utils.adv_gen_optim, utils.sol_optim, utils.init_optim):
        assert mod.__name__.startswith('strive_amd.utils.'), mod.__name__        # this package's loop drivers
    assert utils.scenario_gen.detach_embed_info.__module__ == 'strive_amd.utils.scenario_gen'
    assert datasets.nuscenes_utils.get_map_obs.__module__ == 'strive_amd.datasets.nuscenes_utils'
    assert datasets.utils.MeanStdNormalizer.__module__ == 'strive_amd.datasets.utils'
    assert planners.hardcode_goalcond_nusc.HardcodeNuscPlanner.__module__ == 'strive_amd.planners.hardcode_goalcond_nusc'
    from strive_amd import graph
    assert torch_geometric.data.Batch is graph.Batch
    with pytest.raises(ImportError):             # off the hot path: the reference's own file, which is not part of this package
        import utils.logger                      # noqa: F401
    assert set(dropin_env) >= {'models.traffic_model', 'losses.adv_gen_nusc', 'utils.adv_gen_optim'}


def _oracle(sd, FT):
    from util import oracle_model
    return oracle_model(sd, FT=FT)


def _weights():
    import make_golden as mg
    return mg.LOOP_WEIGHTS


def test_dropin_adv_loop_matches_the_reference_loop(dropin_env):
    """run_adv_gen_optim ('ego' planner) reached through the reference's import name, one iteration on 3 agents with FT = 2:
    the same numbers as the reference's own function on that scene (fixture g13) and as the oracle's restatement of the loop."""
    import utils.adv_gen_optim as adv
    from utils.scenario_gen import detach_embed_info
    from oracle import loops as oloops
    from util import assert_close, golden
    ref = golden('g13_dropin.npz')
    m, sd, batch, map_idx, env = _setup()
    with torch.no_grad():
        emb = detach_embed_info(m.embed(batch, map_idx, env))
    NA = batch.past.shape[0]
    ego = torch.zeros((NA,), dtype=torch.bool)
    ego[batch.ptr[:-1]] = True
    pm, pv = emb['prior_out']
    tp, op = (pm[ego], pv[ego]), (pm[~ego], pv[~ego])
    z0 = emb['posterior_out'][0].clone()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        z, fin, out, agt, tt = adv.run_adv_gen_optim(z0, 0.05, _weights(), m, batch, env, map_idx, 1, emb, 'ego', tp, op, 0, 0.0)
    assert z.shape == (NA, 32) and fin.shape == (NA, 1, 2, 4) and len(agt) == 1 and torch.isfinite(z).all()
    assert_close(emb['map_feat'], ref['map_feat'], 1e-4, 2e-5, 'map_feat against the reference')
    assert_close(z0, ref['z0'], 1e-4, 2e-5, 'posterior mean against the reference')
    # one Adam step moves every entry by lr = 0.05: 1e-4 catches a step of another size or a differently weighted loss term
    assert_close(z.detach(), ref['z'], 0, 1e-4, 'z after one iteration against the reference')
    assert_close(fin, ref['final_result_traj'], 0, 1e-4, 'final_result_traj against the reference')
    assert [int(a) for a in agt] == ref['min_agt'].tolist(), 'attacking agent'
    assert [int(t) for t in tt] == ref['min_t'].tolist(), 'time of the closest approach'
    orc = _oracle(sd, fin.shape[2])
    with torch.no_grad():
        emb_o = orc.embed(batch, map_idx, env)
    assert_close(emb['map_feat'], emb_o['map_feat'], 1e-4, 2e-5, 'map_feat')
    z_o = oloops.adv_loop(orc, batch, map_idx, env, emb_o, emb_o['posterior_out'][0].clone(), _weights(), 1, 0.05,
                          (emb_o['prior_out'][0][ego], emb_o['prior_out'][1][ego]),
                          (emb_o['prior_out'][0][~ego], emb_o['prior_out'][1][~ego]), feasibility_time=0, feasibility_infront_min=0.0)
    # (one Adam step moves every entry by ~lr in the direction of its gradient sign: agreement means the two-rollout
    # complementary-detach closure, the losses and the backward produced the same gradient signs)
    assert float(((z.detach() - z0) * (z_o - z0) > 0).float().mean()) > 0.98
    assert_close(z.detach(), z_o, 0, 0.11, 'z after one iteration against the oracle')


@pytest.mark.slow
def test_dropin_init_sol_and_refine_run_on_the_hip_modules(dropin_env):
    """install() without a checkout: run_init_optim -> run_find_solution_optim through the reference's import names, and this
    package's refine_traffic_optim(), on the emulated HIP modules: shapes and finite results (their numbers are pinned against the
    reference's own functions by tests/test_loops.py, fixtures g6_loops and g12)."""
    import utils.init_optim as init_optim
    import utils.sol_optim as sol_optim
    from utils.scenario_gen import detach_embed_info
    from strive_amd.refine_traffic_optim import refine_traffic_optim
    import make_golden as mg
    m, sd, batch, map_idx, env = _setup()
    with torch.no_grad():
        emb = detach_embed_info(m.embed(batch, map_idx, env))
    NA = batch.past.shape[0]
    ego = torch.zeros((NA,), dtype=torch.bool)
    ego[batch.ptr[:-1]] = True
    pm, pv = emb['prior_out']
    tp, op = (pm[ego], pv[ego]), (pm[~ego], pv[~ego])
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
        z1, traj1, _ = init_optim.run_init_optim(emb['posterior_out'][0].clone(), batch.future_gt[:, :, :4], batch.future_vis, 0.05,
                                                 _weights(), m, batch, env, map_idx, 1, emb, emb['prior_out'])
        fin = traj1.unsqueeze(1)
        z3, sol, _ = sol_optim.run_find_solution_optim(z1.detach(), fin, 2, 0.05, _weights(), m, batch, env, map_idx, 1, emb, tp, op)
    assert traj1.shape == (NA, 2, 4) and sol.shape == (NA, 1, 2, 4) and torch.isfinite(z3).all()
    with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
        init_pred, z, res, emb2 = refine_traffic_optim(batch, map_idx, env, m, mg.REFINE_WEIGHTS, 1, 2, 2, True, 0.05)
    assert init_pred.shape == (NA, 2, 4) and res.shape == (NA, 1, 2, 4) and torch.isfinite(z).all()
