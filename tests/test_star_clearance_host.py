"""K3b under the clearance objective on the CPU: the sequential form star_clearance_ref.py over the shared cases of
star_clearance_cases.py -- the node-set invariance against rrtstar_ref, the self-consistency of what it returns against the
clearance report's reference, the saturated band against path-length RRT*, the mix of branches the cases reach -- and the C ABI of
the new entries without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import motion_clearance_ref as MC
import star_clearance_cases as CC
import star_clearance_ref as SR
from simplify_ref import dist, so2_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mopa_plan_star_clearance_batch", "mopa_plan_star_clearance"]
CASES = [(env, band) for env, (_, _, bands) in CC.SIZES.items() for band in bands]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_sizes():
    assert CC.SIZES[CC.PUSHER][0] >= 8 and CC.SIZES[CC.PUSH][0] >= 4
    assert all(iters <= 300 for _, iters, _ in CC.SIZES.values())
    assert CC.SIZES[CC.LIFT][0] <= 4 and CC.SIZES[CC.LIFT][1] <= 150


@pytest.mark.parametrize("env,band", CASES)
def test_node_set_is_the_path_length_planners(oracle_mod, env, band):
    """fails without star_clearance_ref: status, nodes, trapped, full, goal nodes and first goal iteration are rrtstar_ref's"""
    ref, pl = CC.reference(oracle_mod, env, band), CC.path_length_reference(oracle_mod, env)
    assert np.array_equal(ref[2], pl[2]), "status"
    for c in (0, 1, 4, 5, 7):
        assert np.array_equal(ref[5][:, c], pl[4][:, c]), f"info column {c}"
    for r, p in zip(ref[6], pl[5]):
        assert r.events["trapped"] == p.events["trapped"] and r.events["full"] == p.events["full"]
        if r.tree is not None:
            assert np.array_equal(_bits(r.tree[0]), _bits(p.tree[0])), "node set"
            # one first evaluation per appended or trapped iteration, then the parent walk's and the rewire step's
            assert r.info[2] == (r.info[1] - 1 + r.events["trapped"]) + r.info[8] + r.info[9]
        else:
            assert r.info[2] == 0


@pytest.mark.parametrize("env,band", CASES)
def test_results_are_self_consistent(oracle_mod, env, band):
    pi, orc = CC.scene_of(oracle_mod, env)
    path, plen, status, clearance, length, info, res = CC.reference(oracle_mod, env, band)
    so2 = so2_flags(orc.model, orc.active_idx)
    act = np.asarray(orc.active_idx)
    want = MC.path_clearance(pi, orc, path, plen, band)["clearance"]
    assert (status == 0).any()
    for e, r in enumerate(res):
        if r.status != 0:
            assert plen[e] == 0 and clearance[e] == -math.inf and length[e] == math.inf
            continue
        assert _bits([clearance[e]])[0] == _bits([want[e]])[0], f"query {e}: clearance is not path_clearance's"
        total = 0.0
        for j in range(len(r.rows) - 1):
            total = total + dist(r.rows[j][act], r.rows[j + 1][act], so2)
            assert bool(orc.check_motion(r.rows[0], r.rows[j][act], r.rows[j + 1][act], 0.005)[0]), f"query {e}: segment {j} is blocked"
        assert _bits([length[e]])[0] == _bits([total])[0], f"query {e}: length"
    for r in res:
        if r.tree is None:
            continue
        Q, parent, inc, edge, Cn, Ln, goals = r.tree
        for c in range(1, len(Q)):
            p = int(parent[c])
            assert Cn[c] == min(Cn[p], edge[c]) and Ln[c] == Ln[p] + inc[c], f"node {c}: the key is not its chain's"


def test_saturated_band_is_path_length_rrt_star(oracle_mod):
    """band 0 on Push: where no evaluated motion came below the band, rows and length are rrtstar_ref's rows and cost"""
    ref, pl = CC.reference(oracle_mod, CC.PUSH, 0.0), CC.path_length_reference(oracle_mod, CC.PUSH)
    sat = [e for e, r in enumerate(ref[6]) if r.status == 0 and r.events["unsaturated"] == 0]
    assert len(sat) >= 2
    for e in sat:
        assert np.array_equal(_bits(ref[6][e].rows), _bits(pl[5][e].rows)) and _bits([ref[4][e]])[0] == _bits([pl[3][e]])[0]
        assert ref[3][e] == 0.0 and np.array_equal(ref[5][e][:8][[0, 1, 3, 4, 5, 6, 7]], pl[4][e][[0, 1, 3, 4, 5, 6, 7]])


def test_cases_reach_the_branches(oracle_mod):
    """over the case set at 1 cm; the last two are reached as well (DESIGN.md lists what is not)"""
    tot = {}
    for env, (_, _, bands) in CC.SIZES.items():
        assert 0.01 in bands
        for r in CC.reference(oracle_mod, env, 0.01)[6]:
            for k, v in r.events.items():
                if isinstance(v, int):
                    tot[k] = tot.get(k, 0) + v
    print(tot)
    for k in ("parent_not_path_length", "bound_cut", "rewire_raise", "desc", "rewire_shorten", "best_goal_not_earliest", "trapped", "unsaturated"):
        assert tot[k] >= 1, k
    assert tot["unsaturated"] < tot["evals"]


def test_lift_evaluates_the_can_in_band(oracle_mod):
    """the MESH instantiation is exercised: some evaluated state has a pair of the can as its nearest pair in band"""
    from geom_ref import MESH
    pi, _ = CC.scene_of(oracle_mod, CC.LIFT)
    pg = np.asarray(pi.model.pair_geom).reshape(-1, 2)
    gt = np.asarray(pi.model.geom_type)
    seen = set().union(*(r.events["pairs"] for r in CC.reference(oracle_mod, CC.LIFT, 0.01)[6]))
    assert any((gt[pg[p]] == MESH).any() for p in seen)


def test_symbols_are_declared_exported_and_bound():
    """fails on a library without the feature"""
    from mopa_rl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mopa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mopa_[a-z_0-9]+)\s*\(", txt))
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/mopa_hip.h"
        assert hasattr(L, s), f"{s} is not exported"
        assert s in _lib.EXPORTED_SYMBOLS
    assert _lib.STAR_CLEARANCE_INFO_COLS == SR.INFO_COLS == 11


def test_null_and_argument_errors_are_status_codes():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    prm = _lib.MopaStarParams(10, 11, 8, 0, 0, None, None, 0.05, 0.0, 1.1, 0)
    assert L.mopa_plan_star_clearance_batch(None, None, None, 0, C.byref(prm), 0.01, None, None, None, None, None, None, None) == 1
    assert b"null" in L.mopa_last_error()
    assert L.mopa_plan_star_clearance(None, None, None, C.byref(prm), 0.01, None, None, None, None, None, None) == 1
    assert L.mopa_star_params_size() == C.sizeof(_lib.MopaStarParams)
