"""The rule-based planner, rule by rule and table edge by table edge (strive_amd/csrc/planner.hip against oracle/planner.py).

tests/test_planner.py compares finished plans on worlds that leave most of the planner's rules unreached
(profiles/r27_planner_rule_ratios.md has the counts).  Here every world is built so that ONE rule decides, the ORACLE's own record
(planner_worlds.record_rollout) is asserted to show that rule with a margin before the device is looked at, and the device is
compared through its plan AND through the tables it leaves in its workspace (strive_planner_workspace_layout):

  a. the profile-choice and action rules;                       d. lane graphs that exercise the chain walk and the cumulative sum;
  b. the gap kernel against a float64 restatement of its inputs; e. profile / time / prediction table sizes at their limits;
  c. predicted trajectories and duplicate marks;                f. a scene alone against the same scene in a 128-scene batch.

Every case runs through the host emulation of the kernels and, marked gpu, on the MI355X, on the same worlds.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hipemu'))
os.environ['STRIVE_POISON_WS'] = '1'          # the planner's workspace starts as garbage in every test of this file

import planner_worlds as pw
from planner_worlds import agent
from oracle import planner as oplan
from strive_amd import synth
from strive_amd import _lib as L
from strive_amd.planners.hardcode_goalcond_nusc import CONFIG_DICT

ATOL = 1e-9
EPS = np.finfo(np.float64).eps
RATIOS = {}             # worst observed figures of this run, printed by the last test (profiles/r27_planner_rule_ratios.md)


def note(name, value):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(value))


@pytest.fixture(params=['emu', pytest.param('gpu', marks=pytest.mark.gpu)])
def backend(request):
    """(library, device): the emulated library on CPU tensors, or the product's on the MI355X"""
    if request.param == 'emu':
        with pw.emulated_ops() as emu:
            yield emu, 'cpu'
    else:
        yield L.get_lib(), 'cuda:0'


# ------------------------------------------------------------------------------------------------
# worlds
# ------------------------------------------------------------------------------------------------

LANE_Y = 100.0


def straight_lane(n=200, step=2.0, x0=20.0):
    return pw.lane_graph([pw.polyline((x0, LANE_Y), 0.0, n, step)], [[]])


def cfg_of(name='default', **over):
    return dict(CONFIG_DICT[name], **over)


T16 = np.array([1.0, 2.0, 3.0])              # nstep 15: sixteen planner steps
T3 = np.array([0.2, 0.4])                    # nstep 2: three planner steps, the tables are those of step 2


def ego_at(x=60.0, y=LANE_Y, h=0.0, s=8.0, **kw):
    return agent(x, y, h, s, **kw)


def rule_world(rule):
    """(world, config, planner_t) of one decision rule"""
    lg = straight_lane()
    cfg, tq = cfg_of(), T16
    if rule == 'some_unsafe':                 # a slower lead vehicle in the ego's lane
        sc = [ego_at(), agent(88.0, LANE_Y, 0.0, 2.0)]
    elif rule == 'wide_ego':                  # ... and an ego wider than long (the l < w swap of its circles)
        sc = [ego_at(l=2.0, w=4.4), agent(88.0, LANE_Y, 0.0, 2.0)]
    elif rule == 'none_safe':                 # a parked car right ahead of a fast ego
        sc = [ego_at(s=12.0), agent(88.0, LANE_Y, 0.0, 0.0)]
        tq = T3
    elif rule == 'overlap':                   # a box on top of the ego: gap < 0 at t = 0 for every profile
        sc = [ego_at(), agent(61.5, LANE_Y + 0.5, 0.3, 0.0)]
        tq = T3
    elif rule == 'prefer_stop':               # the ego off every lane, a parked car ahead of it but clear of its path
        sc = [ego_at(y=LANE_Y + 8.0, s=6.0), agent(90.0, LANE_Y + 14.0, 0.0, 0.0)]
    elif rule == 'far':                       # everyone beyond interacdist
        sc = [ego_at(), agent(250.0, LANE_Y, 0.0, 8.0), agent(60.0, LANE_Y + 90.0, 1.0, 0.0)]
        tq = T3
    elif rule == 'exact70':                   # a wrong-way driver in the ego's lane, at step 0 exactly 70.0 m ahead
        sc = [ego_at(), agent(130.0, LANE_Y, np.pi, 8.0)]
        tq = T3
    elif rule == 'crossing':                  # a parked car 72 m ahead of an ego doing 8 m/s: it comes inside interacdist on the way
        sc = [ego_at(), agent(132.0, LANE_Y + 5.0, 0.0, 0.0)]
    elif rule == 'at_rest':                   # an ego at rest behind a parked car
        sc = [ego_at(s=0.0), agent(66.0, LANE_Y, 0.0, 0.0)]
        tq = T3
    else:
        raise KeyError(rule)
    return pw.make_world(lg, [sc]), cfg, tq


def hairpin_world():
    """the lane doubles back 1.5 m ahead of the ego: the route pose one step ahead lies on the return leg, ahead of the ego but
    heading the other way -- the sign of the route step differs from the sign of s_next"""
    x0, y0 = 200.0, 50.0
    out = pw.polyline((x0 - 30.0, y0), 0.0, 32, 1.0)                   # ... (x0, y0), (x0 + 1, y0)
    back = pw.polyline((x0 + 1.0, y0 + 0.3), np.pi, 200, 2.0)
    back[1:, 0] += 1.0                                                  # (x0 + 1, y0 + .3), (x0, y0 + .3), (x0 - 2, ...), ...
    lg = pw.lane_graph([np.concatenate([out, back])], [[]])
    sc = [agent(x0 + 0.2, y0, 0.0, 6.9)]
    return pw.make_world(lg, [sc]), cfg_of(), T3


# ------------------------------------------------------------------------------------------------
# oracle first, then the device, then the comparison
# ------------------------------------------------------------------------------------------------

def oracle_case(world, cfg, tq):
    orc = pw.oracle_planner(world, cfg)
    return pw.record_rollout(orc, world[4], world[5], world[6], tq)


def device_case(backend, world, cfg, tq, traj_cap=None):
    """(plan on the host, tables of the workspace, the planner) of one device rollout"""
    lib, device = backend
    dev = pw.device_planner(world, cfg, device, traj_cap)
    dev.defer_check = True
    got = dev.rollout(torch.from_numpy(world[4].copy()).to(device), world[5], world[6], tq, control_all=False)
    assert dev.check() == {}
    return got.cpu(), pw.device_tables(lib, dev, world[6], tq), dev


def rule_choice(cfg, prof, gap, J, prefer_stop):
    """the profile-choice rule (plot_plan_info, reference :768-801) applied to tables: index of the chosen profile"""
    reach = prof[:, 2]
    if J == 0:
        return int(np.argmax(reach))
    risk = pw.risks_of(oplan.PlannerConfig(**cfg), gap)
    ok = [i for i in range(len(risk)) if risk[i] < cfg['col_plim']]
    if not ok:
        return int(np.argmin(risk))
    sel = [reach[i] for i in ok]
    return ok[int(np.argmin(sel) if prefer_stop else np.argmax(sel))]


def compare(world, cfg, tq, want, rec, got, tabs, scenes=None):
    """plan, and per scene the tables of the LAST planner step, against the oracle's record of that step"""
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=ATOL)
    note('plan', np.abs(got.numpy() - want.numpy()).max())
    P, NT, K = tabs['P'], tabs['NT'], tabs['K']
    assert K == len(rec[0]) and P == len(rec[0][-1]['prof']) and NT == cfg['nsteps'] + 1
    for b, sc in enumerate(rec):
        if scenes is not None and b not in scenes:
            continue
        r = sc[-1]
        prof = tabs['prof'][b, :P]
        np.testing.assert_allclose(prof, r['prof'], rtol=0, atol=ATOL)
        assert bool(tabs['prefer_stop'][b]) == r['prefer_stop']
        assert int(tabs['part_cnt'][b, :tabs['nchunk']].sum()) == r['J'], 'near trajectories of scene %d' % b
        gap = pw.device_gap(tabs, b)
        if r['J'] == 0:
            assert np.all(np.isposinf(gap))
        else:
            np.testing.assert_allclose(gap, r['gap'], rtol=0, atol=ATOL)
            note('gap vs oracle', np.abs(gap - r['gap']).max())
        # the chosen profile: the rule restated on the device's tables, and what the ego then did (where two profiles share
        # (s1, acc) the action is the same: that pair is what is compared)
        p = rule_choice(cfg, prof, gap, r['J'], r['prefer_stop'])
        assert abs(prof[p, 0] - r['s1']) <= ATOL and abs(prof[p, 1] - r['acc']) <= ATOL, (b, p, r['chosen'])
        px, py, ph = r['control']
        np.testing.assert_allclose(tabs['poses'][b, K - 1], [px, py, np.cos(ph), np.sin(ph)], rtol=0, atol=ATOL)
        ex, ey = r['ego'][0], r['ego'][1]
        assert abs(tabs['ego'][b, 3] - oplan.signed_speed(ex, ey, px, py, ph, cfg['dt'])) <= ATOL
        assert abs(tabs['ego'][b, 3] - r['s_next']) < 1e-6


def test_workspace_layout_view(backend):
    """the layout view: offsets ascend, are 256-byte aligned and lie inside what workspace_bytes asks for; too small an output
    array is an error; nchunk follows clamp(512 / B, 4, 32) at the default table"""
    lib, device = backend
    for B, nchunk in ((1, 32), (36, 14), (128, 4), (200, 4)):
        world = pw.make_world(straight_lane(), [[ego_at(x=60.0 + b)] for b in range(B)])
        dev = pw.device_planner(world, cfg_of(), device)
        lay, NR = pw.workspace_layout(lib, dev, world[6], T3)
        assert (lay['K'], lay['cap'], lay['ENT'], lay['P'], lay['NT']) == (3, 512, 5 + 3 * 26, 25, 26)
        assert (lay['nchunk'], lay['MAXK'], lay['MAXPROF'], lay['NCHUNK']) == (nchunk, 384, 64, 32)
        big = [lay[n] for n in ('wstate', 'present', 'traj', 'traj_cnt', 'ego', 'route', 'prof', 'circ', 'part', 'poses')]
        assert big[0] == 0 and all(a <= b_ for a, b_ in zip(big, big[1:])) and len(set(big[2:])) == len(big) - 2 and all(o % 256 == 0 for o in big) and big[-1] < lay['total']
        assert lay['scene_bad'] == lay['traj_cnt'] + 4 * B * 3 and lay['route_nk'] == lay['scene_bad'] + 4 * B
        assert lay['prefer_stop'] == lay['route_nk'] + 4 * B and lay['part_cnt'] == lay['prefer_stop'] + 4 * B
        assert lay['part_cnt'] + 4 * B * 32 <= lay['ego']
        row_obj, row_scene, NR = dev._row_maps(world[6])
        import ctypes as C
        desc = dev._descriptor(row_obj, row_scene, NR)
        assert lay['total'] + 256 == lib.query('strive_planner_workspace_bytes', C.byref(desc), 2, 512)
    with pytest.raises(L.StriveHipError, match='STRIVE_PLANNER_NLAYOUT'):
        pw.workspace_layout(lib, dev, world[6], T3, n_out=23)


# ------------------------------------------------------------------------------------------------
# a. decision rules
# ------------------------------------------------------------------------------------------------

def branches(rec, b=0):
    return [(r['branch'], r['prefer_stop']) for r in rec[b]]


@pytest.mark.parametrize('rule', ['some_unsafe', 'wide_ego', 'none_safe', 'overlap', 'prefer_stop', 'far', 'exact70', 'crossing', 'at_rest',
                                  'hairpin'])
def test_decision_rule(backend, rule):
    world, cfg, tq = hairpin_world() if rule == 'hairpin' else rule_world(rule)
    want, rec = oracle_case(world, cfg, tq)
    br, acts, J = branches(rec), [r['act'] for r in rec[0]], [r['J'] for r in rec[0]]
    # the coverage condition, on the oracle
    if rule in ('some_unsafe', 'wide_ego'):
        assert br.count(('some_unsafe', False)) >= 10
        assert len(set(r['chosen'] for r in rec[0])) >= 2, 'the value of a risk decides: more than one profile is chosen over the steps'
    elif rule == 'none_safe':
        assert br == [('none_safe', False)] * 3 and all(len(np.unique(r['risk'])) > 1 for r in rec[0])
    elif rule == 'overlap':
        assert br == [('none_safe', False)] * 3
        assert all(np.all(r['risk'] == 1.0) and r['gap'][:, 0].max() < 0 and r['chosen'] == 0 for r in rec[0]), 'the tie is the subject'
    elif rule == 'prefer_stop':
        assert all(b_ in (('all_safe', True), ('some_unsafe', True)) for b_ in br) and min(J) > 0
        assert all(r['chosen'] == int(np.argmin(r['reach'])) for r in rec[0]) and 'dn0' in acts and 'route' in acts
    elif rule == 'far':
        assert br == [('no_others', False)] * 3 and len(world[6]) == 2 and world[6][1] == 2, 'two objects, both far'
    elif rule == 'exact70':
        st = world[1].numpy().astype(np.float64)
        assert np.sqrt((st[0, 0] - st[1, 0]) ** 2 + (st[0, 1] - st[1, 1]) ** 2) == cfg['interacdist'] == 70.0
        assert J[0] == 2 and br[0] == ('some_unsafe', False)
        assert rec[0][0]['chosen'] != int(np.argmax(rec[0][0]['reach'])), 'counting it as far would choose another profile'
    elif rule == 'crossing':
        assert J[0] == 0 and J[-1] > 0 and 0 < J.index(2) < len(J) - 1
    elif rule == 'at_rest':
        assert acts == ['dn0'] * 3 and all(r['s_next'] == 0.0 and r['s1'] == 0.0 and r['ego'][3] == 0.0 for r in rec[0])
        assert br == [('none_safe', False)] * 3 and all(len(np.unique(r['risk'])) > 1 for r in rec[0])
    elif rule == 'hairpin':
        assert acts[0] == 'sign' and rec[0][0]['s_next'] > 0
    if rule == 'wide_ego':
        assert rec[0][0]['ego'][4] < rec[0][0]['ego'][5]
    pw.assert_unambiguous(rec, allow_tie=rule == 'overlap')
    got, tabs, _ = device_case(backend, world, cfg, tq)
    compare(world, cfg, tq, want, rec, got, tabs)


# ------------------------------------------------------------------------------------------------
# b. the gap kernel against a float64 restatement of its own inputs
# ------------------------------------------------------------------------------------------------

GAP_CFG = cfg_of(predsfacs=[1.0])           # others off every lane + one predicted speed profile: one trajectory per object
DECISIVE = dict(x=84.0, y=LANE_Y + 3.4, h=0.0, s=0.0, l=4.4, w=2.0)       # parked beside the ego's lane, 1.4 m clear of its path


def gap_scene(J, far=True):
    """ego on the lane + J objects off every lane: J - 1 fillers 20 m and more beside the ego's path (turning, moving, some wider
    than long; the second one beyond interacdist if there are 31 or more) and, LAST, the one parked right beside the ego's path"""
    sc = [ego_at()]
    for i in range(J - 1):
        col, row = i % 40, i // 40
        l, w = 3.8 + 0.1 * (i % 7), 1.7 + 0.1 * (i % 4)
        if i % 11 == 5:
            l, w = w, l
        y = LANE_Y + 22.0 + 2.5 * row + (200.0 if (far and i == 1 and J >= 31) else 0.0)
        sc.append(agent(40.0 + 1.5 * col, y, (0.37 * i) % (2 * np.pi), 0.8 * (i % 4), l=l, w=w))
    if J >= 1:
        sc.append(agent(**DECISIVE))
    return sc


def batch_of(scene, B, at):
    """`scene` as scene `at` of B, the others ego-only"""
    return [scene if b == at else [ego_at(x=40.0 + 0.5 * b, s=4.0 + 0.05 * b)] for b in range(B)]


def single_gaps(tabs, world, b, cfg, j):
    """(P, NT) restated gap of trajectory j alone, and of all the other near trajectories"""
    one = dict(tabs)
    K = tabs['K']
    one['traj'] = tabs['traj'].copy()
    one['traj_cnt'] = tabs['traj_cnt'].copy()
    one['traj'][b, K - 1, 0] = tabs['traj'][b, K - 1, j]
    one['traj_cnt'][b, K - 1] = 1
    rest = dict(tabs)
    rest['traj'] = tabs['traj'].copy()
    rest['traj'][b, K - 1, j, 0:2] = 1e9          # (beyond the interaction distance: left out)
    return pw.gap_restated(one, world, b, cfg['interacdist'])[0], pw.gap_restated(rest, world, b, cfg['interacdist'])[0]


def check_gap_tables(world, cfg, tabs, b, J, emulated, decisive=True):
    """part / part_cnt of scene b's last step against the restatement; -> worst |difference| / bound"""
    K = tabs['K']
    assert int(tabs['traj_cnt'][b, K - 1]) == J
    want, nnear, idx = pw.gap_restated(tabs, world, b, cfg['interacdist'])
    assert int(tabs['part_cnt'][b, :tabs['nchunk']].sum()) == nnear
    got = pw.device_gap(tabs, b)
    if nnear == 0:
        assert np.all(np.isposinf(got))
        return 0.0
    ent = tabs['traj'][b, K - 1, :J]
    scale = max(1.0, np.abs(tabs['circ'][b]).max(), np.abs(ent[idx][:, 5:].reshape(len(idx), -1, 3)[:, :, :2]).max())
    bound = 16 * EPS * scale
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    ratio = float(np.abs(got - want).max() / bound)
    print('gap table of J=%d, nchunk=%d: worst |device - float64 restatement| = %.3g = %.3g x bound' % (J, tabs['nchunk'], np.abs(got - want).max(), ratio))
    note('gap ratio', ratio)
    assert ratio <= 1.0
    if decisive:
        # the object nearest the ego's path: its gap IS the table's minimum somewhere, so losing it cannot go unnoticed
        j = [i for i in range(J) if np.array_equal(ent[i, 0:4], np.array([DECISIVE[k] for k in ('x', 'y', 'l', 'w')], dtype=np.float32).astype(np.float64))]
        assert len(j) == 1
        if emulated:            # (the emulator runs the route workgroups in order; on the GPU the slot order is the atomic counter's)
            assert j[0] == J - 1, 'the last slot of the last chunk that holds any'
        alone, rest = single_gaps(tabs, world, b, cfg, j[0])
        assert np.any((np.abs(got - alone) <= bound) & (alone < rest - 1e-3))
    return ratio


GAP_CASES = [(1, 0, 0, None), (1, 0, 1, None), (1, 0, 31, None), (1, 0, 32, None), (1, 0, 33, None), (1, 0, 512, None), (1, 0, 513, 600),
             (128, 77, 3, None), (128, 77, 4, None), (128, 77, 5, None), (128, 77, 63, None), (128, 77, 64, None), (128, 77, 65, None),
             (128, 77, 129, None), (36, 20, 225, None)]
NCHUNK_OF = {1: 32, 36: 14, 128: 4}


@pytest.mark.parametrize('B,at,J,cap', GAP_CASES, ids=['B%d-J%d' % (c[0], c[2]) for c in GAP_CASES])
def test_gap_kernel_against_float64_restatement(backend, B, at, J, cap):
    """chunking (nchunk 32 / 14 / 4), staging rounds of 16 with full and partial tails, the near count"""
    scene = gap_scene(J)
    world = pw.make_world(straight_lane(), batch_of(scene, B, at))
    want, rec = oracle_case(world, GAP_CFG, T3)
    assert [r['J'] for r in rec[at]] == [J - (1 if J >= 31 else 0)] * 3, 'one trajectory per near object'
    if J >= 1:
        # on the oracle: without the last object another profile is chosen
        w2 = pw.make_world(straight_lane(), [scene[:-1]])
        _, rec2 = oracle_case(w2, GAP_CFG, T3)
        assert rec2[0][0]['chosen'] != rec[at][0]['chosen'] and rec2[0][-1]['chosen'] != rec[at][-1]['chosen']
    pw.assert_unambiguous(rec)
    got, tabs, _ = device_case(backend, world, GAP_CFG, T3, traj_cap=cap)
    assert tabs['nchunk'] == NCHUNK_OF[B]
    per = (min(J, tabs['cap']) + tabs['nchunk'] - 1) // tabs['nchunk']
    if J == 513:
        assert per == 17, 'a second staging round of one trajectory'
    compare(world, GAP_CFG, T3, want, rec, got, tabs)
    check_gap_tables(world, GAP_CFG, tabs, at, J, backend[1] == 'cpu', decisive=J >= 1)
    for b in (0, B - 1):
        if b != at:
            check_gap_tables(world, GAP_CFG, tabs, b, 0, backend[1] == 'cpu', decisive=False)


# ------------------------------------------------------------------------------------------------
# f. alone against batched
# ------------------------------------------------------------------------------------------------

def test_alone_against_scene_77_of_128(backend):
    """nchunk 32 against 4: the plan and the minimum over the chunks do not depend on the chunking, bit for bit"""
    world1, cfg, tq = rule_world('some_unsafe')
    lead = [ego_at(), agent(88.0, LANE_Y, 0.0, 2.0)]
    world128 = pw.make_world(straight_lane(), batch_of(lead, 128, 77))
    want, rec = oracle_case(world1, cfg, tq)
    assert branches(rec).count(('some_unsafe', False)) >= 10
    got1, tabs1, _ = device_case(backend, world1, cfg, tq)
    got128, tabs128, _ = device_case(backend, world128, cfg, tq)
    assert (tabs1['nchunk'], tabs128['nchunk']) == (32, 4)
    np.testing.assert_allclose(got1.numpy(), want.numpy(), rtol=0, atol=ATOL)
    assert torch.equal(got1[0], got128[77])
    assert np.array_equal(pw.device_gap(tabs1, 0), pw.device_gap(tabs128, 77))
    assert np.array_equal(tabs1['prof'][0], tabs128['prof'][77]) and np.array_equal(tabs1['circ'][0], tabs128['circ'][77])


# ------------------------------------------------------------------------------------------------
# c. predicted trajectories, world states and duplicate marks
# ------------------------------------------------------------------------------------------------

def branching_world(sizes=(9, 6), key='rules/branch'):
    """scenes on the synthetic lane graph (crossings with a straight and a right-turn successor): objects whose routes fork inside
    the horizon, one off every lane, one parked, one reversing, one that leaves early (test_planner.random_world)"""
    from test_planner import random_world
    return random_world(list(sizes), key)


def check_world_and_trajectories(world, cfg, rec, tabs, dev):
    """wstate / present against _advance, traj / traj_cnt per (scene, step) against _predict_others as multisets"""
    row_obj, row_scene, NR = dev._row_maps(world[6])
    row_obj, row_scene = row_obj.cpu().numpy(), row_scene.cpu().numpy()
    first = dev._world['ptr_np']
    K, NT = tabs['K'], tabs['NT']
    for r in range(NR):
        b = int(row_scene[r])
        name = '%04d' % (int(row_obj[r]) - int(first[b]))
        for k in range(K):
            here = name in rec[b][k]['world']
            assert bool(tabs['present'][r, k]) == here, (r, k)
            if here:
                np.testing.assert_allclose(tabs['wstate'][r, k], rec[b][k]['world'][name], rtol=0, atol=ATOL)
                note('world state', np.abs(tabs['wstate'][r, k] - np.array(rec[b][k]['world'][name])).max())
    for b in range(len(rec)):
        for k in range(K):
            J = int(tabs['traj_cnt'][b, k])
            assert J <= tabs['cap']
            ent = tabs['traj'][b, k, :J]
            ex, ey = rec[b][k]['ego'][0:2]
            d = np.sqrt((ex - ent[:, 0]) ** 2 + (ey - ent[:, 1]) ** 2)
            assert not np.any(np.abs(d - cfg['interacdist']) < pw.MARGIN), 'an object sits on the interaction boundary'
            ent = ent[d <= cfg['interacdist']]
            oth = np.transpose(rec[b][k]['others'], (1, 0, 2))                         # (J, NT, 5) x, y, h, l, w
            assert len(ent) == len(oth), (b, k, len(ent), len(oth))
            assert sum(n for name, n in rec[b][k]['nroutes'].items() if name != 'ego') * len(cfg['predsfacs']) * len(cfg['predafacs']) == J
            if len(oth) == 0:
                continue
            pts = ent[:, 5:].reshape(len(ent), NT, 3)
            dv = np.concatenate([pts[:, :, 0], pts[:, :, 1], np.cos(pts[:, :, 2]), np.sin(pts[:, :, 2]), ent[:, 2:4]], axis=1)
            ov = np.concatenate([oth[:, :, 0], oth[:, :, 1], np.cos(oth[:, :, 2]), np.sin(oth[:, :, 2]), oth[:, 0, 3:5]], axis=1)
            diff = np.abs(dv[:, None, :] - ov[None, :, :]).max(axis=2)                 # (device, oracle)
            free = np.ones(len(ov), dtype=bool)
            for i in range(len(dv)):                   # equal trajectories are equal to 1e-9 on both sides: first free partner
                cand = np.nonzero(free & (diff[i] <= ATOL))[0]
                assert len(cand) > 0, 'scene %d step %d: device trajectory %d has no partner (closest %.3g)' % (b, k, i, diff[i][free].min())
                free[cand[0]] = False
                note('trajectory', diff[i, cand[0]])


def check_duplicate_marks(tabs, times=None):
    """every marked point has, in its (scene, step), an entry of the same object with the bit-identical point and a clear bit;
    -> marked points (at the given times)"""
    K, NT = tabs['K'], tabs['NT']
    marked = 0
    for b in range(tabs['traj'].shape[0]):
        for k in range(K):
            J = int(tabs['traj_cnt'][b, k])
            ent = tabs['traj'][b, k, :J]
            if J == 0:
                continue
            assert np.all(ent[:, 4] == np.floor(ent[:, 4])) and ent[:, 4].min() >= 0 and ent[:, 4].max() < 2.0 ** NT
            mask = ent[:, 4].astype(np.uint64)
            bits = ent.view(np.int64)
            for j in np.nonzero(mask)[0]:
                for t in range(NT):
                    if not (int(mask[j]) >> t) & 1:
                        continue
                    same = np.all(bits[:, 0:4] == bits[j, 0:4], axis=1) & np.all(bits[:, 5 + 3 * t:8 + 3 * t] == bits[j, 5 + 3 * t:8 + 3 * t], axis=1)
                    clear = ((mask >> np.uint64(t)) & np.uint64(1)) == 0
                    assert np.any(same & clear), 'scene %d step %d entry %d time %d is marked without an unmarked twin' % (b, k, j, t)
                    marked += times is None or t in times
    return marked


def test_trajectories_world_states_and_duplicate_marks(backend):
    world, cfg, tq = branching_world(), cfg_of(), T16[:2]
    want, rec = oracle_case(world, cfg, tq)
    assert max(max(r['nroutes'].values()) for sc in rec for r in sc) >= 2, 'routes fork'
    assert len(set(len(r['world']) for r in rec[0])) > 1, 'an object leaves the world on the way'
    got, tabs, dev = device_case(backend, world, cfg, tq)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=ATOL)
    check_world_and_trajectories(world, cfg, rec, tabs, dev)
    marked = check_duplicate_marks(tabs)
    print('duplicate marks: %d marked points' % marked)
    assert marked >= 100
    # the gap kernel leaves the marked points out: its table must still be the minimum over ALL points
    for b in range(len(rec)):
        check_gap_tables(world, cfg, tabs, b, int(tabs['traj_cnt'][b, -1]), backend[1] == 'cpu', decisive=False)


# ------------------------------------------------------------------------------------------------
# e. table sizes
# ------------------------------------------------------------------------------------------------

SIZE_CFGS = {
    'P1xNT3': dict(nsteps=2, plannspeeds=1, planaccfacs=[1.0]),                    # 3 threads: the ego kernel is wider than the gap kernel
    'P32xNT32': dict(nsteps=31, plannspeeds=4, planaccfacs=[0.5, 1.0]),            # 1024 threads exactly, bit 31 of the duplicate mask
    'P64xNT16': dict(nsteps=15, plannspeeds=8),                                    # MAXPROF
    'npred8': dict(predsfacs=[0.25, 0.5, 0.75, 1.0], predafacs=[0.5, 1.0]),        # MAXPRED
}


@pytest.mark.parametrize('name', sorted(SIZE_CFGS))
def test_table_sizes(backend, name):
    cfg = cfg_of(**SIZE_CFGS[name])
    world, _, _ = rule_world('some_unsafe')
    want, rec = oracle_case(world, cfg, T3)
    pw.assert_unambiguous(rec)
    assert rec[0][-1]['J'] == len(cfg['predsfacs']) * len(cfg['predafacs'])
    got, tabs, dev = device_case(backend, world, cfg, T3)
    P = len(cfg['planaccfacs']) * cfg['plannspeeds'] ** 2
    assert (tabs['P'], tabs['NT']) == (P, cfg['nsteps'] + 1)
    compare(world, cfg, T3, want, rec, got, tabs)
    check_gap_tables(world, cfg, tabs, 0, rec[0][-1]['J'], backend[1] == 'cpu', decisive=False)
    check_world_and_trajectories(world, cfg, rec, tabs, dev)
    if name in ('P32xNT32', 'npred8'):
        # ... and on the branching world: trajectories of every prediction, marks up to the last time
        world = branching_world((9,))
        want, rec = oracle_case(world, cfg, T3)
        got, tabs, dev = device_case(backend, world, cfg, T3)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=ATOL)
        check_world_and_trajectories(world, cfg, rec, tabs, dev)
        check_gap_tables(world, cfg, tabs, 0, int(tabs['traj_cnt'][0, -1]), backend[1] == 'cpu', decisive=False)
        last = check_duplicate_marks(tabs, times=(cfg['nsteps'],))
        print('%s: %d marked points at t = %d' % (name, last, cfg['nsteps']))
        assert last >= 1


def test_table_limits_are_refused(backend):
    """NT = 33, more than 64 profiles (81: a product of 1..4 factors and a square cannot be 65) and more than 1024 threads
    (64 x 17 = 1088: 1025 = 25 x 41 needs NT = 41 or P = 205, which the first two checks refuse) each with their message"""
    lib, device = backend
    world, _, _ = rule_world('some_unsafe')
    for over, msg in ((dict(nsteps=32), r'nsteps \+ 1 must be <= 32'), (dict(plannspeeds=9), 'at most 64 ego speed profiles'),
                      (dict(plannspeeds=8, nsteps=16), 'profiles x times exceed one workgroup'),
                      (dict(predsfacs=[0.4, 0.6, 0.8], predafacs=[0.5, 0.7, 1.0]), 'at most 8 predicted speed profiles')):
        dev = pw.device_planner(world, cfg_of(**over), device)
        with pytest.raises(L.StriveHipError, match=msg):
            dev.rollout(torch.from_numpy(world[4].copy()).to(device), world[5], world[6], T3, control_all=False)
        with pytest.raises(L.StriveHipError, match=msg):
            pw.workspace_layout(lib, dev, world[6], T3)


# ------------------------------------------------------------------------------------------------
# d. lane graphs that exercise the chain walk and the cumulative sum
# ------------------------------------------------------------------------------------------------

def main_lane_with_stubs(n, step, forks=(), merges=(), stub=3, x0=20.0, perm=False):
    """A main lane of n consecutive node ids along +x with side lanes: ``forks`` = [(node, count)] short dead-end lanes leaving that
    node (so it has 1 + count successors, the main lane first), ``merges`` = [(node, count)] short lanes arriving at it.  The side
    lanes leave and arrive at right angles, so that no pose on the main lane is matched to them."""
    spac = np.broadcast_to(np.asarray(step, dtype=np.float64), (n - 1,))
    main = pw.polyline((x0, LANE_Y), 0.0, n, spac)
    cuts = sorted(set([v + 1 for v, _ in forks if v + 1 < n] + [v for v, _ in merges if v > 0]))
    bounds = [0] + cuts + [n]
    lanes = [main[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    assert all(len(l) >= 1 for l in lanes)
    npieces = len(lanes)
    outgoing = [[i + 1] if i + 1 < npieces else [] for i in range(npieces)]
    piece_ending_at = {b - 1: i for i, b in enumerate(bounds[1:])}
    piece_starting_at = {a: i for i, a in enumerate(bounds[:-1])}
    for v, count in forks:
        for c in range(count):
            side = -1.0 if c % 2 else 1.0
            p0 = main[v] + np.array([0.3 * (c // 2), side * 0.5])
            lanes.append(pw.polyline(p0, side * np.pi / 2, stub, 0.5))
            outgoing.append([])
            outgoing[piece_ending_at[v]].append(len(lanes) - 1)
    for v, count in merges:
        for c in range(count):
            side = -1.0 if c % 2 else 1.0
            p0 = main[v] + np.array([-0.3 * (c // 2), side * 0.5 * stub])
            lanes.append(pw.polyline(p0, -side * np.pi / 2, stub, 0.5))
            outgoing.append([piece_starting_at[v]])
    lg = pw.lane_graph(lanes, outgoing)
    assert np.array_equal(lg['xy'][:n], main)
    return pw.permuted(lg, pw.scatter_permutation(lg['xy'].shape[0])) if perm else lg


def route_inputs(cfg, s):
    tmax = cfg['nsteps'] * cfg['preddt']
    back = 1.0 if s > 0 else 1.0 + abs(s) * tmax
    fwd = 1.0 + cfg['smax'] * tmax if s < 0 else max(1.0 + cfg['smax'] * tmax, 1.0 + s * tmax)
    return back, fwd


def oracle_routes(lg, cfg, pose):
    """(routes, np of every route as routes_through counts its nodes, number of matches, kept edges) of the oracle"""
    x, y, h, s = pose
    G = oplan.LaneGraph(lg)
    e_all, p_all = G.match(x, y, h, 1.0 - np.cos(np.radians(cfg['cdistang'])), cfg['xydistmax'])
    e, p = G.cluster(x, y, e_all, p_all)
    back, fwd = route_inputs(cfg, s)
    routes = oplan.routes_through(G, e, p, back, fwd, cfg['xydistmax'], np.array([x, y]), h)
    need_f, need_b = fwd + oplan.SBUFFER + cfg['xydistmax'], back + oplan.SBUFFER + cfg['xydistmax']
    nps, chains = [], []
    for v0, v1 in e:
        fc, bc = G.chains(int(v1), G.succ, need_f), G.chains(int(v0), G.pred, need_b)
        chains.append((fc, bc))
        for fv, fl in fc:
            for bv, bl in bc:
                nps.append(len(fv) + len(bv) + (fl <= need_f) + (bl <= need_b))
    return routes, nps, len(e_all), e, chains


def device_routes(backend, lg, cfg, pose, maxr=64):
    """strive_planner_routes -> (status (8), number of routes, [(s (nk), knots (nk, 4))])"""
    import ctypes as C
    lib, device = backend
    world = pw.make_world(lg, [[agent(*pose)]])
    dev = pw.device_planner(world, cfg, device)
    row_obj, row_scene, NR = dev._row_maps(world[6])
    desc = dev._descriptor(row_obj, row_scene, NR)
    maxk = 384
    nr = torch.zeros((1,), dtype=torch.int32, device=device)
    nk = torch.zeros((maxr,), dtype=torch.int32, device=device)
    kn = torch.zeros((maxr, maxk, 5), dtype=torch.float64, device=device)
    status = torch.zeros((8,), dtype=torch.int32, device=device)
    p4 = torch.tensor([float(v) for v in pose], dtype=torch.float64, device=device)
    lib.call('strive_planner_routes', C.byref(desc), 0, L.ptr(p4), maxr, maxk, L.ptr(nr), L.ptr(nk), L.ptr(kn), L.ptr(status), L.stream_ptr(p4))
    nk, kn = nk.cpu().numpy(), kn.cpu().numpy()
    n = int(nr.cpu())
    return status.cpu().numpy(), n, [(kn[r, :nk[r], 0], kn[r, :nk[r], 1:]) for r in range(min(n, maxr))]


def compare_routes(backend, lg, cfg, pose, want):
    status, n, got = device_routes(backend, lg, cfg, pose)
    assert int(np.abs(status).sum()) == 0, status
    assert n == len(want)
    for (s, kn), route in zip(got, want):
        assert len(s) == len(route.t)
        np.testing.assert_allclose(s, route.t, rtol=0, atol=1e-10)
        np.testing.assert_allclose(kn, route.y, rtol=0, atol=1e-10)
        note('knot', max(np.abs(s - route.t).max(), np.abs(kn - route.y).max()))


def on_edge(lg, v, s, along=0.2, off=0.0):
    """pose on the edge from main-lane node v to v + 1 (lanes of main_lane_with_stubs run along +x)"""
    return (float(lg['xy'][v, 0]) + along, LANE_Y + off, 0.02, s)


WINDOW_CFG = cfg_of(smax=5.0)               # a short forward horizon leaves room in the 320-node table for a long backward walk


@pytest.mark.parametrize('case', ['fwd_once', 'fwd_twice', 'bwd_once', 'bwd_twice'])
def test_chain_walk_windows_and_forks_at_their_edges(backend, case):
    """one lane of consecutive ids: the 64-node register window is refilled once / twice, forwards and backwards, with a fork
    (forwards) or a merge (backwards) at window positions 0, 63 and 64"""
    n, p = 240, 100 if case.startswith('fwd') else 200
    if case.startswith('fwd'):
        cfg, s = cfg_of(), 6.0
        step = 1.0 if case == 'fwd_once' else 0.5
        lg = main_lane_with_stubs(n, step, forks=[(p + 1, 1), (p + 64, 2), (p + 65, 1)])
        need = route_inputs(cfg, s)[1] + 6.0
    else:
        cfg = WINDOW_CFG
        s = -10.0 if case == 'bwd_once' else -12.2          # (137 nodes back: the backward tables hold 160 in all, side lanes included)
        lg = main_lane_with_stubs(n, 0.5, merges=[(p, 1), (p - 63, 2), (p - 64, 1)])
        need = route_inputs(cfg, s)[0] + 6.0
    pose = on_edge(lg, p, s)
    want, nps, nmatch, kept, chains = oracle_routes(lg, cfg, pose)
    assert len(kept) == 1 and tuple(kept[0]) == (p, p + 1), 'the walks start at nodes p + 1 (forwards) and p (backwards)'
    fc, bc = chains[0]
    walk = fc[0][0] if case.startswith('fwd') else bc[0][0]
    refills = (len(walk) - 1) // 64                  # the walk leaves its first window after 64 nodes
    assert refills == (1 if case.endswith('once') else 2), (len(walk), need)
    assert len(fc if case.startswith('fwd') else bc) == 5 and len(want) == 5
    compare_routes(backend, lg, cfg, pose, want)


def fan(p0, h0, count, spread, nodes, step):
    hs = h0 + np.linspace(-spread, spread, count) if count > 1 else [h0]
    return [pw.polyline(np.asarray(p0) + step * np.array([np.cos(h), np.sin(h)]), h, nodes, step) for h in hs]


def fan_graph(second, preds=1):
    """a trunk along +x that forks 6 ways; branch i forks again second[i] ways; `preds` lanes arrive at the trunk's first node"""
    trunk = pw.polyline((20.0, LANE_Y), 0.0, 12, 2.0)
    lanes, outgoing = [trunk], [[]]
    for br in fan(trunk[-1], 0.0, 6, 0.6, 2, 10.0):
        lanes.append(br)
        outgoing.append([])
        outgoing[0].append(len(lanes) - 1)
    for i, cnt in enumerate(second):
        b = 1 + i
        h = np.arctan2(*(lanes[b][-1] - lanes[b][0])[::-1])
        for leaf in fan(lanes[b][-1], h, cnt, 0.08, 9, 10.0):
            lanes.append(leaf)
            outgoing.append([])
            outgoing[b].append(len(lanes) - 1)
    for lane in fan(trunk[0], np.pi, preds, 0.5, 6, 2.0):
        lanes.append(lane[::-1])
        outgoing.append([0])
    return pw.lane_graph(lanes, outgoing)


@pytest.mark.parametrize('leaves', [48, 49])
def test_overflow_connection_lists_and_the_chain_limit(backend, leaves):
    """junctions with 6 and 8 (9) successors and 5 predecessors: connections beyond the fourth come from the CSR lists.  48 forward
    chains fit the table, the 49th raises the chain flag"""
    second = [8] * 6
    second[3] += leaves - 48
    lg = fan_graph(second, preds=5)
    assert max(len(o) for o in lg['out_edges']) == max(second) and sorted(len(o) for o in lg['out_edges'])[-7] == 6
    assert max(len(i) for i in lg['in_edges']) == 5
    cfg = cfg_of()
    pose = (26.3, LANE_Y + 0.1, 0.0, -1.0)          # reversing slowly: the backward walk (11 m) reaches the five arriving lanes
    want, nps, nmatch, kept, chains = oracle_routes(lg, cfg, pose)
    assert len(kept) == 1 and len(chains[0][0]) == leaves and len(chains[0][1]) == 5 and len(want) == 5 * leaves
    status, n, got = device_routes(backend, lg, cfg, pose, maxr=256)
    if leaves == 49:
        assert status[2] == 1 and status[[0, 1, 3, 4, 5, 6, 7]].sum() == 0, status
        return
    assert int(np.abs(status).sum()) == 0 and n == len(want), (status, n)
    for (s, kn), route in zip(got, want):
        assert len(s) == len(route.t)
        np.testing.assert_allclose(s, route.t, rtol=0, atol=1e-10)
        np.testing.assert_allclose(kn, route.y, rtol=0, atol=1e-10)
        note('knot', max(np.abs(s - route.t).max(), np.abs(kn - route.y).max()))


DEAD_ENDS = {            # (nodes of the lane, node the matched edge starts at, speed): which ends are extended
    'ahead': (200, 197, 6.0), 'one_ahead': (200, 198, 6.0), 'behind': (200, 1, 6.0), 'at_the_start': (200, 0, 6.0),
    'both': (6, 3, 6.0), 'two_nodes': (2, 0, 6.0), 'both_reversing': (30, 8, -4.0),
}


@pytest.mark.parametrize('case', sorted(DEAD_ENDS))
def test_dead_ends(backend, case):
    """ext_f, ext_b and the shift by one; in 'two_nodes' the lane IS the matched edge: the backward extension's direction is read
    from nodes 1 and 2 of the table, and node 2 is the last one"""
    n, p, s = DEAD_ENDS[case]
    lg = main_lane_with_stubs(n, 2.0)
    cfg = cfg_of()
    pose = on_edge(lg, p, s, along=0.7, off=0.4)
    want, nps, nmatch, kept, chains = oracle_routes(lg, cfg, pose)
    back, fwd = route_inputs(cfg, s)
    (fv, fl), (bv, bl) = chains[0][0][0], chains[0][1][0]
    ext_f, ext_b = fl <= fwd + 6.0, bl <= back + 6.0
    assert (ext_f, ext_b) == {'ahead': (True, False), 'one_ahead': (True, False), 'behind': (False, True), 'at_the_start': (False, True)}.get(case, (True, True))
    if case == 'two_nodes':
        assert nps == [4] and len(fv) == len(bv) == 1
    if case == 'one_ahead':
        assert len(fv) == 1
    compare_routes(backend, lg, cfg, pose, want)


CUMSUM_SPACINGS = (6.5, 6.0, 5.5, 2.95, 2.85, 2.8, 1.95, 1.9)


def test_cumulative_sum_batches(backend):
    """seq_cumsum adds up the node distances in batches of 16 behind two single terms, the next batch prefetched: node counts np
    with (np - 2) % 16 in {0, 1, 15} and (np - 2) // 16 in {0, 1, >= 2}, as the oracle counts them.  (np = 2 and np = 3 cannot
    occur: a chain walk takes at least one step or ends at a dead end, which adds the extension node -- the two-node lane of
    test_dead_ends has np = 4, the smallest there is.)"""
    cfg = cfg_of()
    cases = []
    for d in CUMSUM_SPACINGS:
        n = int(400 / d)
        lg = main_lane_with_stubs(n, d)
        pose = on_edge(lg, n // 2, 6.0, along=0.3 * d, off=-0.3)
        want, nps, _, _, _ = oracle_routes(lg, cfg, pose)
        cases.append((lg, pose, want, nps[0]))
    nps = [c[3] for c in cases]
    assert nps == [17, 18, 19, 33, 34, 35, 49, 50]
    assert set((v - 2) % 16 for v in nps) == {0, 1, 15} and set(min((v - 2) // 16, 2) for v in nps) == {0, 1, 2}
    for lg, pose, want, _ in cases:
        compare_routes(backend, lg, cfg, pose, want)


def test_tied_matches_beyond_sixteen(backend):
    """More than 16 matches, the two closest at exactly the same distance (the pose sits on a node).  The reference orders matches
    with np.argsort's default kind, which is not stable (and not the same on every CPU) once ties exist; the device keeps the first
    of the tied matches in edge order.  Whichever of the two edges the oracle keeps, they are consecutive pieces of one lane and the
    route through either is the same curve: the knots agree."""
    lg = main_lane_with_stubs(300, 0.2)
    cfg = cfg_of()
    pose = (float(lg['xy'][150, 0]), LANE_Y, 0.0, 6.0)
    want, nps, nmatch, kept, chains = oracle_routes(lg, cfg, pose)
    G = oplan.LaneGraph(lg)
    e, pts = G.match(pose[0], pose[1], pose[2], 1.0 - np.cos(np.radians(cfg['cdistang'])), cfg['xydistmax'])
    d = np.linalg.norm(np.array([[pose[0], pose[1]]]) - pts, axis=1)
    assert nmatch == len(e) > 16 and int((d == d.min()).sum()) == 2 and len(kept) == 1
    assert tuple(kept[0]) in ((149, 150), (150, 151))
    compare_routes(backend, lg, cfg, pose, want)


def test_permuted_node_ids(backend):
    """the synthetic graph with scattered node ids: no edge joins consecutive ids, so the chain walk never finds a plain run and
    takes the general step (and reloads its window) at every node.  Routes knot by knot, then a rollout."""
    from test_planner import random_world
    lg0 = synth.make_lane_graph()
    n = lg0['xy'].shape[0]
    perm = pw.scatter_permutation(n, stride=11)
    lg = pw.permuted(lg0, perm)
    assert np.all(np.abs(lg['edgeixes'][:, 0] - lg['edgeixes'][:, 1]) > 1)
    assert np.all(np.diff(lg['edgeixes'][:, 0]) >= 0), 'the edge table follows the new ids'
    cfg = cfg_of('final_tuned_val_1')
    xy = lg0['xy']
    poses = [(xy[40, 0] + 0.3, xy[40, 1] - 0.4, None, 6.0), (xy[200, 0], xy[200, 1] + 0.8, None, 0.0), (xy[333, 0] - 0.5, xy[333, 1], None, -3.0),
             (xy[75, 0], xy[75, 1], None, 27.0)]
    nbranch = 0
    for x, y, h, s in poses:
        v = int(np.argmin(np.linalg.norm(xy - np.array([[x, y]]), axis=1)))
        d = xy[lg0['out_edges'][v][0]] - xy[v] if lg0['out_edges'][v] else xy[v] - xy[lg0['in_edges'][v][0]]
        pose = (float(x), float(y), float(np.arctan2(d[1], d[0])) + 0.05, s)
        want, _, _, _, _ = oracle_routes(lg, cfg, pose)
        want0, _, _, _, _ = oracle_routes(lg0, cfg, pose)
        assert len(want) == len(want0)
        nbranch += len(want) > 1
        compare_routes(backend, lg, cfg, pose, want)
    assert nbranch >= 2
    world = list(random_world([7, 4], 'rules/perm'))
    world[0] = lg
    world = tuple(world)
    want, rec = oracle_case(world, cfg_of(), T16[:2])
    assert max(max(r['nroutes'].values()) for sc in rec for r in sc) >= 2
    got, tabs, dev = device_case(backend, world, cfg_of(), T16[:2])
    compare(world, cfg_of(), T16[:2], want, rec, got, tabs)
    check_world_and_trajectories(world, cfg_of(), rec, tabs, dev)


def test_zz_print_worst_figures(backend):
    """(not a check: the worst figures of this run, for profiles/r27_planner_rule_ratios.md; run with -s)"""
    for k in sorted(RATIOS):
        print('worst %-16s %.3g' % (k, RATIOS[k]))


def test_first_point_behind_a_fork_decides_a_gap(backend):
    """An object whose routes fork at a crossing, and an ego standing where the turning route passes: for some (profile, time)
    the table's minimum is the FIRST point at which the turning trajectory is no longer a marked duplicate of the straight one.
    Reading the marks shifted by one time step would drop exactly that point."""
    lg = synth.make_lane_graph()
    world = pw.make_world(lg, [[agent(126.0, 134.0, -np.pi / 2, 0.0), agent(110.0, 126.0, 0.0, 8.0)]])
    cfg = cfg_of()
    want, rec = oracle_case(world, cfg, T3)
    assert rec[0][-1]['nroutes']['0001'] >= 2 and rec[0][-1]['J'] >= 4
    got, tabs, dev = device_case(backend, world, cfg, T3)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=ATOL)
    K, NT, P = tabs['K'], tabs['NT'], tabs['P']
    J = int(tabs['traj_cnt'][0, K - 1])
    ent = tabs['traj'][0, K - 1, :J]
    mask = ent[:, 4].astype(np.uint64)
    per = np.array([single_gaps(tabs, world, 0, cfg, j)[0] for j in range(J)])           # (J, P, NT) gap of every trajectory alone
    bits = ent.view(np.int64)
    decided = 0
    for j in range(J):
        m = int(mask[j])
        if m == 0 or m == (1 << NT) - 1:
            continue
        assert m & (m + 1) == 0, 'the marks of a trajectory are a prefix: the points before the fork'
        t0 = m.bit_length()                       # the first unmarked point
        other = [i for i in range(J) if not np.array_equal(bits[i, 5 + 3 * t0:8 + 3 * t0], bits[j, 5 + 3 * t0:8 + 3 * t0])]
        decided += int(np.sum(per[j, :, t0] < per[other][:, :, t0].min(axis=0) - 1e-3))
    assert decided >= 1, 'no (profile, time) at which the first point behind a fork is the closest'
    check_gap_tables(world, cfg, tabs, 0, J, backend[1] == 'cpu', decisive=False)
    check_duplicate_marks(tabs)
