"""The host side of the reports on the Push scene: the argument rule every batch method shares (refusals raised in Python, before
anything reaches the library), the walk behind the contact report (k_contact_frames / k_contact_manifolds) at
its edges -- a state without a record, a truncated row, a row longer than a wave -- and the six single-state forms against their
batch forms at N = 1, every returned field by bytes."""
import numpy as np
import pytest

from conftest import sample_states
from contacts_ref import FAR, full_state, oracle_pair_dists, report_from_dists

pytestmark = pytest.mark.gpu
ENV = "SawyerPushObstacle-v0"
K16 = 16


def _bytes(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


@pytest.fixture(scope="module")
def push(oracle_mod):
    """scene, planner, oracle and five states near the initial pose; by the oracle's counts two of them have no record at the
    contact threshold (1, 4: the segment between them is free) and two have several (0, 2)"""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(ENV)
    sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
    orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    qa, rows = sample_states(pi, 5, 4, "near")
    count = report_from_dists(oracle_pair_dists(pi, orc, qa, rows, len(qa)), pi.spec.contact_threshold, K16)[0]
    yield pi, sc, BatchPlanner(sc), orc, qa, rows, count, torch.from_numpy(qa).cuda(), torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    sc.close()


def _batch_methods(bp, seg_only=False):
    """the six batch methods as f(qa, qb, rows, samples_per_env); the first three take states and ignore qb"""
    states = [("is_valid", lambda a, b, r, spe: bp.is_valid(a, r, samples_per_env=spe)),
              ("contacts", lambda a, b, r, spe: bp.contacts(a, r, samples_per_env=spe)),
              ("proximity", lambda a, b, r, spe: bp.proximity(a, r, samples_per_env=spe))]
    segments = [("check_motion", lambda a, b, r, spe: bp.check_motion(a, b, r, samples_per_env=spe)),
                ("motion_report", lambda a, b, r, spe: bp.motion_report(a, b, r, samples_per_env=spe)),
                ("motion_clearance", lambda a, b, r, spe: bp.motion_clearance(a, b, r, samples_per_env=spe))]
    return segments if seg_only else states + segments


def test_batch_methods_refuse_in_python_before_any_launch(push, monkeypatch):
    from mopa_rl_amd import _lib
    pi, sc, bp, orc, qa, rows, count, tq, tr = push
    sc.contact_scene()       # (created now: the refusals below must not need the library at all)
    a, b = tq[:3].contiguous(), tq[1:4].contiguous()
    rows3 = tr.repeat(3, 1).contiguous()

    def no_library():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    for name, f in _batch_methods(bp):
        with pytest.raises(_lib.MopaError):      # N = 3, two samples per env: two env rows are needed, one is there
            f(a, b, tr, 2)
        with pytest.raises(_lib.MopaError):
            f(a, b, tr, 0)
        with pytest.raises(_lib.MopaError):
            f(a, b, rows3, 0)
    for name, f in _batch_methods(bp, seg_only=True):
        with pytest.raises(_lib.MopaError):      # qb one row shorter than qa, enough env rows
            f(a, b[:2].contiguous(), rows3, 1)


def _contacts(bp, tq, tr, K, frames, manifold):
    import torch
    rep = bp.contacts(tq, tr, samples_per_env=tq.shape[0], max_contacts=K, frames=frames, manifold=manifold)
    torch.cuda.synchronize()
    return {k: getattr(rep, k).cpu().numpy() for k in ("count", "pair", "dist", "normal", "pos", "npoint", "point_dist", "point_pos")
            if getattr(rep, k) is not None}


def test_record_walk_at_its_edges(push):
    pi, sc, bp, orc, qa, rows, count, tq, tr = push
    assert (count == 0).any() and (count >= 2).any(), count       # the oracle's counts: a state without a record, a state with several
    ref = _contacts(bp, tq, tr, K16, True, True)
    assert np.array_equal(ref["count"], count)
    unused = {"pair": -1, "dist": FAR, "normal": 0.0, "pos": 0.0, "npoint": 0, "point_dist": FAR, "point_pos": 0.0}
    for K in (1, K16, 65):       # 1 truncates the rows of the states with several records, 65 crosses the walk's stride of 64 slots
        got = _contacts(bp, tq, tr, K, True, True)
        assert np.array_equal(got["count"], ref["count"])
        k = min(K, K16)
        for name, fill in unused.items():
            assert got[name].shape[:2] == (len(qa), K), name
            assert got[name][:, :k].tobytes() == ref[name][:, :k].tobytes(), f"K = {K}: {name} differs from the K = {K16} call"
            for s in range(len(qa)):
                tail = got[name][s, min(int(count[s]), K):]
                assert tail.tobytes() == np.full_like(tail, fill).tobytes(), f"K = {K}: {name} of state {s} past its records"
        only_f = _contacts(bp, tq, tr, K, True, False)
        only_m = _contacts(bp, tq, tr, K, False, True)
        assert only_f["normal"].tobytes() == only_m["normal"].tobytes() == got["normal"].tobytes()
        assert "npoint" not in only_f and "pos" not in only_m


def test_single_state_forms_have_the_bytes_of_their_batch_forms(push):
    import torch
    pi, sc, bp, orc, qa, rows, count, tq, tr = push
    thr, na = pi.spec.contact_threshold, len(qa[0])
    K = 4
    for s in range(len(qa)):       # the four state forms, on states with and without records
        q = full_state(pi, qa[s], rows[0])
        one = tq[s:s + 1].contiguous()
        n, pair, dist = sc.contacts_state_raw(q, None, K)
        rep = bp.contacts(one, tr, max_contacts=K)
        assert n == int(rep.count[0]) == count[s]
        assert pair.tobytes() == _bytes(rep.pair) and dist.tobytes() == _bytes(rep.dist)
        n, pair, dist, normal, pos = sc.contact_frames_state_raw(q, None, K)
        rep = bp.contacts(one, tr, max_contacts=K, frames=True)
        assert n == int(rep.count[0]) and [x.tobytes() for x in (pair, dist, normal, pos)] == [_bytes(x) for x in (rep.pair, rep.dist, rep.normal, rep.pos)]
        n, pair, dist, normal, npoint, pdist, ppos = sc.contact_manifolds_state_raw(q, None, K, 3, 0.0)
        rep = bp.contacts(one, tr, max_contacts=K, manifold=True, max_points=3)
        assert n == int(rep.count[0])
        assert [x.tobytes() for x in (pair, dist, normal, npoint, pdist, ppos)] == [_bytes(x) for x in (rep.pair, rep.dist, rep.normal, rep.npoint, rep.point_dist,
                                                                                                          rep.point_pos)]
        cl, n, pair, dist = sc.proximity_state_raw(q, 0.05, K)
        rep = bp.proximity(one, tr, band=0.05, max_pairs=K)
        assert n == int(rep.count[0]) and np.float64(cl).tobytes() == _bytes(rep.clearance)
        assert pair.tobytes() == _bytes(rep.pair) and dist.tobytes() == _bytes(rep.dist)
    verdicts = []
    for a, b in ((1, 4), (1, 0)):       # the two segment forms: a free segment and a blocked one (the oracle's verdicts)
        want, _ = orc.check_motion(rows[0], qa[a], qa[b])
        verdicts.append(want)
        q_a, q_b = full_state(pi, qa[a], rows[0]), full_state(pi, qa[b], rows[0])
        ta, tb = tq[a:a + 1].contiguous(), tq[b:b + 1].contiguous()
        for Kb in (0, K):
            valid, n, fb, t, lvq, fbq, blk = sc.motion_report_raw(q_a, q_b, Kb)
            rep = bp.motion_report(ta, tb, tr, max_contacts=Kb)
            assert valid == bool(rep.valid[0]) == want and n == int(rep.n_states[0]) and fb == int(rep.first_bad[0])
            assert np.float64(t).tobytes() == _bytes(rep.last_valid_t) and lvq.tobytes() == _bytes(rep.last_valid_q) and fbq.tobytes() == _bytes(rep.first_bad_q)
            assert (blk is None) == (Kb == 0) == (rep.blockers is None)
            if Kb:
                assert blk[0] == int(rep.blockers.count[0]) and blk[1].tobytes() == _bytes(rep.blockers.pair) and blk[2].tobytes() == _bytes(rep.blockers.dist)
                assert (blk[0] > 0) == (not want)
        cl, n, near, k, t, pair, ec, q_min = sc.motion_clearance_raw(q_a, q_b, 0.05)
        rep = bp.motion_clearance(ta, tb, tr, band=0.05, states=True)
        assert [n, near, k, pair] == [int(x[0]) for x in (rep.n_states, rep.n_near, rep.k_min, rep.pair_min)]
        assert [np.float64(x).tobytes() for x in (cl, t, ec)] == [_bytes(x) for x in (rep.clearance, rep.t_min, rep.end_clearance)]
        assert q_min.tobytes() == _bytes(rep.q_min) and q_min.shape == (na,)
    assert verdicts == [True, False]
    torch.cuda.synchronize()
