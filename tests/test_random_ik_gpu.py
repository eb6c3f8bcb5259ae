"""The IK kernels off the Sawyer (k_ik_solve, k_ik_site_pose, k_ik_displacement_pos) on the chains of tests/random_ik.py -- eight
movable joints (the last row and column of the unrolled 8 x 8 Cholesky live), slide columns and a site rotation under an orientation
target, jointless prefixes, a fixed joint on the chain, movable joints off it, a free joint on it -- 130 problems per chain (two waves
and two lanes of a third), against oracle/mopa_oracle.c bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import random_ik as RI  # noqa: E402
import random_scenes as RS  # noqa: E402
from test_env_tables_gpu import _fma, _quat2mat  # noqa: E402

pytestmark = pytest.mark.gpu

E = RI.E_GPU


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def setups(oracle_mod):
    """per chain, built once: the kernel-side solver, the oracle, the states and the targets (read-only)"""
    import torch
    from scipy.spatial.transform import Rotation
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    from mopa_rl_amd.ik import BatchIK
    made = {}

    def get(name):
        if name not in made:
            c = RI.chain(name)
            m = c.model
            ik = BatchIK(m, "tip", c.joints, device=torch.cuda.current_device())
            orc = oracle_mod.OracleScene(m, c.pi.passive_joint_idx, c.pi.ignored_contacts, RS.CONTACT_THRESHOLD)
            q = RI.rows(c, E, seed=51)
            qt = RI.perturbed(c, q, seed=51)
            poses = [RI.site_pose_ref(c, row) for row in qt]
            tgt = RI.far_targets(np.array([p for p, _ in poses]), seed=51)
            xyzw = Rotation.from_matrix(np.array([R for _, R in poses])).as_quat()
            tq = RI.target_quats(np.ascontiguousarray(xyzw[:, [3, 0, 1, 2]]), seed=51)
            made[name] = dict(c=c, ik=ik, orc=orc, q=q, tgt=tgt, tq=tq)
        return made[name]

    yield get
    for s in made.values():
        s["ik"].close()


@pytest.mark.parametrize("name", list(RI.CHAINS))
def test_solve_is_the_oracle_bit_for_bit(setups, name):
    import torch
    S = setups(name)
    c, ik, orc, q, tgt, tq = (S[k] for k in ("c", "ik", "orc", "q", "tgt", "tq"))
    m = c.model
    n_ok = n_fail = 0
    for tol in (1e-2, 1e-6):
        for quat in (None, tq):
            qd = torch.tensor(q, device="cuda")
            res = ik.solve(qd, torch.tensor(tgt, device="cuda"), torch.tensor(quat, device="cuda") if quat is not None else None, max_steps=100, tol=tol)
            gq, ge, gs, gok = res.qpos.cpu().numpy(), res.err_norm.cpu().numpy(), res.steps.cpu().numpy(), res.success.cpu().numpy()
            for e in range(E):
                oq, oe, os_, ook = orc.ik_solve(q[e], tgt[e], ik.joint_ids, ik.site_body, ik.site_off, max_steps=100, tol=tol,
                                                target_quat=quat[e] if quat is not None else None, site_quat=m.site_quat[0])
                what = (name, tol, quat is not None, e)
                assert np.array_equal(_bits(gq[e]), _bits(oq)), (what, np.abs(gq[e] - oq).max())
                assert _bits(ge[e]) == _bits(oe) and gs[e] == os_ and bool(gok[e]) == ook, (what, ge[e], oe, gs[e], os_)
                n_ok += int(ook)
                n_fail += int(not ook)
                if name == "none_on_chain":
                    assert os_ == 0 and np.array_equal(_bits(gq[e]), _bits(q[e])), what
    if name == "none_on_chain":
        assert n_ok > 0          # (an unmoved target is met at once; nothing can move the site)
    else:
        assert n_ok > 0 and n_fail > 0, (n_ok, n_fail)


@pytest.mark.parametrize("name", list(RI.CHAINS))
def test_site_pose_is_the_fma_exact_restatement(setups, name):
    import torch
    S = setups(name)
    c, ik, orc, q = S["c"], S["ik"], S["orc"], S["q"]
    pos, mat = ik.site_pose(torch.tensor(q, device="cuda"))
    pos, mat = pos.cpu().numpy(), mat.cpu().numpy().reshape(E, 9)
    sl = _quat2mat(c.model.site_quat[0])
    off = [float(v) for v in ik.site_off]
    for e in range(E):
        xpos, xquat = orc.fk_bodies(q[e])
        M = _quat2mat(xquat[ik.site_body])
        want_pos = [float(xpos[ik.site_body][r]) + _fma(M[3 * r + 2], off[2], _fma(M[3 * r + 1], off[1], M[3 * r] * off[0])) for r in range(3)]
        want_mat = [_fma(M[3 * r + 2], sl[6 + k], _fma(M[3 * r + 1], sl[3 + k], M[3 * r] * sl[k])) for r in range(3) for k in range(3)]
        assert np.array_equal(_bits(pos[e]), _bits(want_pos)), (name, e)
        assert np.array_equal(_bits(mat[e]), _bits(want_mat)), (name, e)


@pytest.mark.parametrize("name", list(RI.CHAINS))
def test_fused_pre_step_is_the_composition_of_the_separate_launches(setups, name):
    """mopa_ik_displacement_pos_batch (n_cart = 3) against site_pose -> targets_pos -> solve -> clip -> subtract"""
    import torch
    S = setups(name)
    c, ik, q = S["c"], S["ik"], S["q"]
    m = c.model
    ids = RI.joint_ids(c)
    adr = torch.tensor([int(m.jnt_qposadr[j]) for j in ids], device="cuda")
    lim = np.asarray(m.jnt_limited)[ids] == 1
    lo = torch.tensor(np.where(lim, np.asarray(m.jnt_range)[ids, 0], -3.14), device="cuda")
    hi = torch.tensor(np.where(lim, np.asarray(m.jnt_range)[ids, 1], 3.14), device="cuda")
    rng = np.random.default_rng(52)
    ac = torch.tensor(rng.uniform(-1, 1, (E, 3)) * np.array([0.004, 0.06, 1.0])[np.arange(E) % 3][:, None], device="cuda")
    wlo, whi = (-0.6, -0.6, -0.6), (0.6, 0.6, 0.6)
    qd = torch.tensor(q, device="cuda")
    keep = qd.clone()
    site_pos, _ = ik.site_pose(qd)
    tgt = ik.targets_pos(site_pos, ac, 3, 1.0, wlo, whi)
    q2 = qd.clone()
    res = ik.solve(q2, tgt, None, max_steps=100, tol=1e-2)
    arm = torch.minimum(torch.maximum(q2[:, adr], lo), hi)
    want = arm - qd[:, adr]
    got, r = ik.displacement_pos(qd, ac, 3, 1.0, wlo, whi, lo, hi, want_result=True)
    torch.cuda.synchronize()
    assert torch.equal(qd, keep), "displacement_pos wrote its input"
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy())), name
    assert torch.equal(r.steps, res.steps) and torch.equal(r.success, res.success)
    assert np.array_equal(_bits(r.err_norm.cpu().numpy()), _bits(res.err_norm.cpu().numpy()))
    if name != "none_on_chain":
        assert bool((want != 0).any())
