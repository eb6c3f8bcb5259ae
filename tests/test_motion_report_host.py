"""The sequential form of the motion report (motion_report_ref.py) on the CPU oracle alone: its verdicts are the oracle's
check_motion, its rows are what was validated, the shared inputs hold all four classes of segment on every scene, and a blocked
segment always has a blocker at or below the threshold.  No device."""
import numpy as np
import pytest

from conftest import SUPPORTED_ENVS
import motion_report_ref as R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _verdicts(pi, orc, q, row):
    return orc.is_valid_batch(np.ascontiguousarray(q), row, samples_per_env=len(q), nthreads=0, want_min_dist=False)[0]


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_shared_inputs_hold_every_class_and_agree_with_check_motion(env, oracle_mod):
    pi, orc, qa, qb, row = R.shared_segments(env)
    rep = R.shared_report(env)
    assert np.array_equal(rep["valid"], orc.check_motion_batch(qa, qb, row, samples_per_env=len(qa), nthreads=0))
    cls = R.classes(rep)
    print(env, {k: int(v.sum()) for k, v in cls.items()}, "longest segment", int(rep["n_states"].max()), "states")
    for name, m in cls.items():
        assert m.sum() >= 1, f"{env}: no segment of class '{name}'"
    assert sum(int(m.sum()) for m in cls.values()) == len(qa)        # the classes partition the shared inputs
    assert (rep["n_states"][:64] == 1).all() and (rep["valid"][:64] == 1).all()


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_parameters_and_rows(env, oracle_mod):
    pi, orc, qa, qb, row = R.shared_segments(env)
    rep = R.shared_report(env)
    fb, c, t = rep["first_bad"], rep["n_states"], rep["last_valid_t"]
    ok = fb == 0
    assert np.array_equal(ok, rep["valid"] == 1)
    assert (t[ok] == 1.0).all() and np.array_equal(_bits(t[~ok]), _bits((fb[~ok] - 1).astype(np.float64) / c[~ok].astype(np.float64)))
    assert (t[fb == 1] == 0.0).all() and ((t >= 0.0) & (t <= 1.0)).all() and (t[~ok] < 1.0).all()
    assert ((fb >= 0) & (fb <= c)).all() and (c >= 1).all()
    # valid: both rows are qb; blocked at k = 1: last_valid_q is qa; blocked at the end: first_bad_q is qb
    assert np.array_equal(_bits(rep["last_valid_q"][ok]), _bits(qb[ok])) and np.array_equal(_bits(rep["first_bad_q"][ok]), _bits(qb[ok]))
    assert np.array_equal(_bits(rep["last_valid_q"][fb == 1]), _bits(qa[fb == 1]))
    assert np.array_equal(_bits(rep["first_bad_q"][fb == c]), _bits(qb[fb == c]))
    # the row before first_bad is valid (where it is a tested state), the row at first_bad is not
    assert (_verdicts(pi, orc, rep["first_bad_q"][~ok], row) == 0).all()
    assert (_verdicts(pi, orc, rep["last_valid_q"][fb > 1], row) == 1).all()
    # the rows are the states of the segment at those indices
    so2 = R.so2_flags(pi.model, pi.ref_joint_pos_indexes)
    ext = R.extents(pi.model, pi.ref_joint_pos_indexes, so2)
    for i in np.nonzero(fb > 1)[0][:40]:
        s = R.segment_states(qa[i], qb[i], so2, ext)
        assert len(s) == c[i]
        assert np.array_equal(_bits(s[fb[i] - 1]), _bits(rep["first_bad_q"][i])) and np.array_equal(_bits(s[fb[i] - 2]), _bits(rep["last_valid_q"][i]))
        assert (_verdicts(pi, orc, s[:fb[i] - 1], row) == 1).all()       # nothing before first_bad is blocked


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_degenerate_segments_and_the_seam(env, oracle_mod):
    pi, orc, qa, qb, row = R.shared_segments(env)
    A, B, labels = R.edge_segments(env)
    rep = R.motion_report(pi, orc, A, B, row, len(A))
    lab = {k: labels.index(k) for k in ("equal-valid", "equal-invalid", "nd1-valid", "nd1-invalid")}
    assert (rep["n_states"][:4] == 1).all()
    i = lab["equal-valid"]
    assert rep["valid"][i] == 1 and rep["first_bad"][i] == 0 and rep["last_valid_t"][i] == 1.0
    assert np.array_equal(_bits(rep["last_valid_q"][i]), _bits(B[i])) and np.array_equal(_bits(rep["first_bad_q"][i]), _bits(B[i]))
    # nd == 0 with an invalid qb: c = 1, first_bad = 1, t = 0.0, last_valid_q = qa (the documented deviation from OMPL)
    i = lab["equal-invalid"]
    assert rep["valid"][i] == 0 and rep["first_bad"][i] == 1 and rep["last_valid_t"][i] == 0.0
    assert np.array_equal(_bits(rep["last_valid_q"][i]), _bits(A[i])) and np.array_equal(_bits(rep["first_bad_q"][i]), _bits(B[i]))
    so2 = R.so2_flags(pi.model, pi.ref_joint_pos_indexes)
    ext = R.extents(pi.model, pi.ref_joint_pos_indexes, so2)
    for k in ("nd1-valid", "nd1-invalid"):
        i = lab[k]
        assert R.segment_count(A[i], B[i], so2, ext) == 1
        assert rep["valid"][i] == (1 if k == "nd1-valid" else 0) and rep["first_bad"][i] == (0 if k == "nd1-valid" else 1)
        assert np.array_equal(_bits(rep["first_bad_q"][i]), _bits(B[i]))
        assert np.array_equal(_bits(rep["last_valid_q"][i]), _bits(B[i] if k == "nd1-valid" else A[i]))
    assert np.array_equal(rep["valid"], orc.check_motion_batch(A, B, row, samples_per_env=len(A), nthreads=0))
    if env == "PusherObstacle-v0":
        assert so2[0]
        seam = [i for i, k in enumerate(labels) if k == "seam"]
        assert len(seam) == 8
        for i in seam:
            s = R.segment_states(A[i], B[i], so2, ext)
            # the short way round: 2 pi - 6 rad in all, every state beyond +-3.0, and the sign changes once
            assert len(s) == rep["n_states"][i] == int(np.ceil((2 * np.pi - 6.0) / (0.005 * np.pi)))
            assert (np.abs(s[:, 0]) >= 3.0).all() and (np.abs(s[:, 0]) <= np.pi).all()
            assert s[0, 0] > 3.0 and s[-1, 0] == -3.0 and (np.diff(np.sign(s[:, 0])) != 0).sum() == 1
            if rep["first_bad"][i] > 1:
                assert np.array_equal(_bits(rep["last_valid_q"][i]), _bits(s[rep["first_bad"][i] - 2]))


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_every_blocked_segment_has_a_blocker(env, oracle_mod):
    pi, orc, qa, qb, row = R.shared_segments(env)
    rep = R.shared_report(env)
    thr = pi.spec.contact_threshold
    for K in (4, 1):
        cnt, pair, dist = R.blockers(pi, orc, rep, row, K, len(qa))
        blocked = rep["first_bad"] > 0
        assert (cnt[blocked] >= 1).all() and (pair[blocked, 0] >= 0).all() and (dist[blocked].min(axis=1) <= thr).all()
        assert (cnt[~blocked] == 0).all() and (pair[~blocked] == -1).all() and (dist[~blocked] == R.FAR).all()
