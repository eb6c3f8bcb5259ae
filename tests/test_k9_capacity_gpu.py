"""The capacities of the three K9 entry points (csrc/mopa_k9.inc: one LDS layout as a function of the level) against the values
the three separate kernels of commit 0cd73e6 ("Pin run_episode under IK and discrete actions; fix NaN sit-out envs") returned
for the same scenes, read off that commit's library on an MI355X.  They guard the per-wave layouts -- 16 na + 6 max_path bytes for the vertex passes
alone, without the lists of the higher levels.  A launch at exactly the capacity succeeds, one row more is refused by the
argument check.  Scene construction only, no planner run."""
import numpy as np
import pytest

import simplify_ref as R

pytestmark = pytest.mark.gpu

# env -> (mopa_simplify_paths_max_path, mopa_shortcut_paths_max_path, mopa_smooth_paths_max_path) at commit 0cd73e6
PARENT_CAPS = {"SawyerPushObstacle-v0": (5770, 2136, 1222), "PusherObstacle-v0": (6197, 2309, 1663)}
UNSUPPORTED = 2         # MOPA_ERR_UNSUPPORTED


@pytest.mark.parametrize("env", sorted(PARENT_CAPS))
def test_capacities_are_the_parents_and_a_launch_at_capacity_succeeds(env):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    from mopa_rl_amd.scene import default_qpos, planner_inputs
    pi = planner_inputs(env)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    L = _lib.lib()
    caps = (L.mopa_simplify_paths_max_path(scene.handle), L.mopa_shortcut_paths_max_path(scene.handle),
            L.mopa_smooth_paths_max_path(scene.handle))
    print(env, "capacities", caps)
    assert caps == PARENT_CAPS[env]
    # E = 2 out-and-back paths of 5 rows around the initial pose
    row = default_qpos(env, pi.model)
    act = np.asarray(scene.active_idx)
    rows = R.out_and_back(row[act], row[act] + 0.05, 3, act, row)[:5]
    plen = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    entries = ((L.mopa_simplify_paths_batch, ()), (L.mopa_shortcut_paths_batch, (16,)), (L.mopa_smooth_paths_batch, (16,)))
    for level, (cap, (entry, max_rounds)) in enumerate(zip(caps, entries)):
        def call(mp):
            path = torch.zeros(2, mp, scene.nq, dtype=torch.float64, device="cuda")
            path[:, :5] = torch.from_numpy(rows).cuda()
            n = plen.clone()
            rc = entry(scene.handle, 2, mp, _ptr(path), _ptr(n), None, 5, 0, None, None, (4 << level) - 1, *max_rounds, None, None)
            torch.cuda.synchronize()
            return rc, n.cpu().numpy()
        rc, n = call(cap)
        assert rc == 0, f"level {level}: a launch at max_path = {cap} was refused: {L.mopa_last_error()}"
        assert ((2 <= n) & (n <= cap)).all()
        rc, n = call(cap + 1)
        assert rc == UNSUPPORTED and b"max_path" in L.mopa_last_error(), f"level {level}: max_path = {cap + 1}"
        assert (n == 5).all(), "a refused call launched something"
