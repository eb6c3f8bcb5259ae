"""Baked K1 forward kinematics, host side (no GPU): the walk compiled into the baked instantiation, run on the host, against
the CPU oracle bit for bit; the generator's refusals; the header layout it reads the export with; and the fingerprint
guarding the constants of the walk."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENV = "SawyerPushObstacle-v0"


def _args(env=ENV):
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(env)
    return pi, (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        monkeypatch.delenv(k)


def _export():
    from mopa_rl_amd import _lib
    _, args = _args()
    return _lib.k1_export(*args)


def test_header_layout_comes_from_the_library():
    import bake_k1_scenes as B
    from mopa_rl_amd import _lib
    L = _lib.lib()
    ex = _export()
    size = len(ex["hdr"])
    assert L.mopa_scene_hdr_offset(b"na") == 0
    assert L.mopa_scene_hdr_offset(b"no_such_field") == -1
    fields = ["na", "nq", "n_pq", "nmb", "nmg", "nsf", "n_save", "n_pas_b", "n_dbl", "n_int", "o_mbr", "o_mbd", "o_mgd", "o_sf_pos",
              "o_sf_quat", "o_sf_mat", "o_act_ref", "o_pq_adr"]
    offs = [L.mopa_scene_hdr_offset(f.encode()) for f in fields]
    assert all(0 <= o <= size - 4 and o % 4 == 0 for o in offs) and len(set(offs)) == len(offs)
    # what the offsets read agrees with what the export says on its own
    assert B.hdr_int(ex, "n_dbl") == len(ex["dbl"]) and B.hdr_int(ex, "n_int") == len(ex["ints"])
    assert B.hdr_int(ex, "nmg") == ex["nmg"]
    pi, _ = _args()
    assert B.hdr_int(ex, "na") == len(pi.ref_joint_pos_indexes) and B.hdr_int(ex, "nq") == pi.model.nq
    assert B.hdr_double(ex, "thr") == pi.spec.contact_threshold
    o = B.hdr_int(ex, "o_mbr")
    assert 0 <= o and o + 8 * B.hdr_int(ex, "nmb") <= len(ex["ints"])
    with pytest.raises(KeyError):
        B.hdr_int(ex, "no_such_field")


def test_fk_program_of_the_bench_scene():
    import bake_k1_scenes as B
    fk = B.fk_program(_export())
    assert fk["nmb"] == 14 and fk["na"] == 7 and fk["n_save"] == 2
    jt = [b[6] for b in fk["bodies"] if b[5] == 1]
    assert jt.count(B.J_HINGE) == 7 and jt.count(B.J_SLIDE) == 2 and jt.count(B.J_FREE) == 1


def _set_hdr_int(ex, field, value):
    import bake_k1_scenes as B
    from mopa_rl_amd import _lib
    off = _lib.lib().mopa_scene_hdr_offset(field.encode())
    hdr = ex["hdr"].copy()
    hdr[off: off + 4] = np.array([value], dtype="<i4").view(np.uint8)
    out = dict(ex, hdr=hdr)
    assert B.hdr_int(out, field) == value
    return out


def test_generator_refuses_scenes_outside_the_baked_walk():
    import bake_k1_scenes as B
    ex = _export()
    B.fk_program(ex)
    with pytest.raises(B.Unsupported, match="tile-posed"):
        B.fk_program(_set_hdr_int(ex, "n_pas_b", 4))
    with pytest.raises(B.Unsupported, match="active values"):
        B.fk_program(_set_hdr_int(ex, "na", 9))
    with pytest.raises(B.Unsupported, match="mesh pairs"):
        B.fk_program(dict(ex, n_mesh_pairs=2))
    with pytest.raises(B.Unsupported, match="centres in LDS"):
        B.fk_program(dict(ex, cen_lds=False))
    # a moving body with two joints
    o = B.hdr_int(ex, "o_mbr")
    ints = ex["ints"].copy()
    ints[o + 8 * 3] = 2
    with pytest.raises(B.Unsupported, match="2 joints"):
        B.fk_program(dict(ex, ints=ints))


def test_one_ulp_in_the_body_chain_changes_the_fingerprint():
    """A moving body's position or a joint axis one ULP off: another fingerprint, so the scene gets the generic kernel."""
    from mopa_rl_amd import _lib
    import bake_k1_scenes as B
    import re
    pi, args = _args()
    fp = _lib.k1_export(*args)["fingerprint"]
    baked = [int(x, 16) for x in re.findall(r"kFingerprint = 0x([0-9a-f]{16})ull", open(B.OUT).read())]
    assert fp in baked
    m = pi.model
    j = m.joint_name2id(pi.spec.robot_joints[3])
    b = int(m.jnt_body[j])
    for arr, idx in ((m.body_pos, (b, 1)), (m.jnt_axis, (j, 2))):
        old = arr[idx]
        try:
            arr[idx] = np.nextafter(old, np.inf)
            fp2 = _lib.k1_export(*args)["fingerprint"]
            assert fp2 != fp and fp2 not in baked
        finally:
            arr[idx] = old
    assert _lib.k1_export(*args)["fingerprint"] == fp


def _states(pi, n, seed):
    """full qpos rows: active joints uniform in their box, at and one ULP past the limits, zero, the default pose; gripper slides
    across (and past) their range; the cube at varied, not always unit-norm poses"""
    from mopa_rl_amd.scene import default_qpos
    m = pi.model
    rng = np.random.default_rng(seed)
    row = default_qpos(ENV, m)
    act = np.asarray(pi.ref_joint_pos_indexes)
    lo, hi = pi.jnt_minimum, pi.jnt_maximum
    q = np.repeat(row[None], n, axis=0)
    qa = rng.uniform(lo, hi, size=(n, len(act)))
    k = n // 8
    qa[:k] = np.where(rng.random((k, len(act))) < 0.5, lo, hi)
    qa[k:2 * k] = np.where(rng.random((k, len(act))) < 0.5, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf))
    qa[2 * k] = 0.0
    qa[2 * k + 1] = row[act]
    q[:, act] = qa
    for name in ("rc_close", "lc_close"):
        jj = m.joint_name2id(name)
        a, (r0, r1) = int(m.jnt_qposadr[jj]), m.jnt_range[jj]
        q[2 * k + 2:, a] = rng.uniform(r0 - 0.01, r1 + 0.01, size=n - 2 * k - 2)
    cube = int(m.jnt_qposadr[[j for j in range(len(m.jnt_names)) if int(m.jnt_type[j]) == 0][0]])
    q[3 * k:, cube: cube + 3] += rng.uniform(-0.2, 0.2, size=(n - 3 * k, 3))
    qq = rng.normal(size=(n - 3 * k, 4))
    qq /= np.linalg.norm(qq, axis=1, keepdims=True)
    qq[::3] *= rng.uniform(0.9, 1.1, size=(len(qq[::3]), 1))     # quat_normalize's slow branch
    q[3 * k:, cube + 3: cube + 7] = qq
    return q


def test_baked_walk_equals_the_oracle_bitwise():
    import ctypes as C
    from mopa_rl_amd import _lib
    from oracle import oracle as O
    pi, args = _args()
    ex = _lib.k1_export(*args)
    L = _lib.lib()
    import bake_k1_scenes as B
    nmg = ex["nmg"]
    o = B.hdr_int(ex, "o_mg_geom")                      # moving geom slot -> model geom id
    mg = [int(g) for g in ex["ints"][o: o + nmg]]
    n = 100_000
    q = _states(pi, n, 7)
    qa = np.ascontiguousarray(q[:, np.asarray(pi.ref_joint_pos_indexes)])
    out = np.zeros((n, nmg, 12))
    assert L.mopa_k1_baked_fk_host(1, n, qa.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    assert L.mopa_k1_baked_fk_host(99, 0, None, None, None) != 0
    orc = O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    bad = 0
    for s in range(n):
        gp, gm = orc.fk(q[s])
        got = out[s]
        if not (np.array_equal(gp[mg].view(np.uint64), got[:, :3].view(np.uint64))
                and np.array_equal(gm[mg].reshape(nmg, 9).view(np.uint64), got[:, 3:].view(np.uint64))):
            bad += 1
    assert bad == 0, f"{bad} of {n} states differ"
