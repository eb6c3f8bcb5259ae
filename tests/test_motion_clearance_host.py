"""The sequential form of the clearance report (motion_clearance_ref.py) on the CPU oracle alone: it agrees with the motion report's
verdicts, its inputs hold every class of segment on every scene (the GPU test runs on the same ones), ties go to the smallest k, and
the path form handles a single vertex, an unsolved query and a minimum at vertex 0.  No device."""
import numpy as np
import pytest

from conftest import SUPPORTED_ENVS
import motion_clearance_ref as M
import motion_report_ref as R
import proximity_ref as P

MIX_BAND = 0.01
MIX_MIN = 8
GPU_PREFIX = 300          # the largest batch of test_motion_clearance_gpu.py: the mix condition holds on it too


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_consistent_with_the_motion_report(env, oracle_mod):
    pi, orc, A, B, rows, base = M.mix_segments(env)
    shared = R.shared_report(env)
    thr = pi.spec.contact_threshold
    own = np.nonzero(base >= 0)[0]
    assert len(own) == len(M.BASE) and len(A) >= GPU_PREFIX
    for band in P.BANDS:
        rep = M.mix_report(env, band)
        c, k = rep["n_states"], rep["k_min"]
        assert (rep["clearance"] <= rep["end_clearance"]).all() and (rep["clearance"] <= band).all() and (rep["end_clearance"] <= band).all()
        assert ((k >= 0) & (k <= c)).all() and (c >= 1).all() and ((rep["n_near"] >= 0) & (rep["n_near"] <= c)).all()
        assert np.array_equal(k == 0, rep["n_near"] == 0) and np.array_equal(k == 0, rep["pair_min"] < 0)
        assert (rep["clearance"][k == 0] == band).all() and (rep["t_min"][k == 0] == 0.0).all() and (rep["t_min"][k == c] == 1.0).all()
        assert np.array_equal(_bits(rep["t_min"][k > 0]), _bits(k[k > 0].astype(np.float64) / c[k > 0].astype(np.float64)))
        assert np.array_equal(_bits(rep["q_min"][k == 0]), _bits(B[k == 0])) and np.array_equal(_bits(rep["q_min"][k == c]), _bits(B[k == c]))
        # the shared segments: the verdict of the motion report is "the clearance lies above the threshold"
        assert np.array_equal(rep["n_states"][own], shared["n_states"][base[own]])
        assert np.array_equal(rep["clearance"][own] > thr, shared["valid"][base[own]] == 1), (env, band)
        n_bad = 0
        for i in own:
            fb = int(shared["first_bad"][base[i]])
            if fb:          # k_min <= first_bad is NOT claimed: the deepest state may come later
                assert rep["d"][i][fb - 1] <= thr and (rep["d"][i][:fb - 1] > thr).all()
                n_bad += 1
        assert n_bad >= 8


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_inputs_hold_every_class(env, oracle_mod):
    rep = M.mix_report(env, MIX_BAND)
    for n in (len(rep["k_min"]), GPU_PREFIX):
        cls = {name: int(m[:n].sum()) for name, m in M.classes(rep).items()}
        print(env, "first", n, "segments:", cls, "longest", int(rep["n_states"][:n].max()), "states")
        for name, count in cls.items():
            assert count >= MIX_MIN, f"{env}: {count} segments of class '{name}' among the first {n}"


@pytest.mark.parametrize("env", [e for e in SUPPORTED_ENVS if e.startswith("Sawyer")])
def test_a_tie_goes_to_the_smallest_k(env, oracle_mod):
    rep = M.mix_report(env, MIX_BAND)
    ties = []
    for i, (d, p) in enumerate(zip(rep["d"], rep["p"])):
        at = np.nonzero((_bits(d) == _bits(rep["clearance"][i])) & (p >= 0))[0]
        if len(at) > 1:
            ties.append(i)
            assert rep["k_min"][i] == at[0] + 1 and rep["pair_min"][i] == p[at[0]]
    in_prefix = [i for i in ties if i < GPU_PREFIX]
    print(env, "segments whose minimum is attained more than once with identical bits:", len(ties), "of them among the first", GPU_PREFIX, ":", len(in_prefix))
    assert len(in_prefix) >= 1          # the GPU test's batch holds a tie


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_degenerate_segments_and_the_seam(env, oracle_mod):
    pi, orc, qa, qb, row = R.shared_segments(env)
    A, B, labels = R.edge_segments(env)
    thr = pi.spec.contact_threshold
    rep = M.motion_clearance(pi, orc, A, B, row, MIX_BAND, len(A))
    lab = {k: labels.index(k) for k in ("equal-valid", "equal-invalid", "nd1-valid", "nd1-invalid")}
    for name, i in lab.items():
        assert rep["n_states"][i] == 1 and rep["k_min"][i] in (0, 1) and rep["t_min"][i] in (0.0, 1.0)
        assert _bits(rep["clearance"][i]) == _bits(rep["end_clearance"][i]) and np.array_equal(_bits(rep["q_min"][i]), _bits(B[i]))
        assert (rep["clearance"][i] > thr) == name.endswith("-valid")
    for name in ("equal-invalid", "nd1-invalid"):
        assert rep["k_min"][lab[name]] == 1 and rep["pair_min"][lab[name]] >= 0 and rep["n_near"][lab[name]] == 1
    if env == "PusherObstacle-v0":
        so2 = R.so2_flags(pi.model, pi.ref_joint_pos_indexes)
        ext = R.extents(pi.model, pi.ref_joint_pos_indexes, so2)
        seam = [i for i, k in enumerate(labels) if k == "seam"]
        assert len(seam) == 8
        for i in seam:
            s = R.segment_states(A[i], B[i], so2, ext)
            assert len(s) == rep["n_states"][i] and (np.abs(s[:, 0]) >= 3.0).all()
            k = rep["k_min"][i]
            assert k >= 1 and np.array_equal(_bits(rep["q_min"][i]), _bits(s[k - 1]))


def test_path_form(oracle_mod):
    env = "SawyerPushObstacle-v0"
    pi, orc, A, B, rows, base = M.mix_segments(env)
    rep = M.mix_report(env, MIX_BAND)
    act = np.asarray(pi.ref_joint_pos_indexes)
    cls = M.classes(rep)
    # a path walked from its nearest state away: the reversed "minimum at the end state" segments; at least one keeps its minimum at vertex 0
    cand = np.nonzero(cls["end"])[0][:12]
    far = np.nonzero(cls["far"] & (rep["n_states"] > 1))[0][:16]
    far = far[M.state_clearances(pi, orc, A[far], rows[far], MIX_BAND)[1] < 0][:2]       # ... whose start state is out of band too
    assert len(far) == 2
    E, Pmax = len(cand) + len(far) + 2, 3
    path = np.zeros((E, Pmax, rows.shape[1]))
    plen = np.zeros(E, dtype=np.int32)
    for e, i in enumerate(cand):
        path[e, :2] = rows[i]
        path[e, 0, act], path[e, 1, act] = B[i], A[i]
        plen[e] = 2
    for n, i in enumerate(far):
        e = len(cand) + n
        path[e] = rows[i]
        path[e, 0, act], path[e, 1, act] = A[i], B[i]
        plen[e] = 2
    e1, e0 = E - 2, E - 1
    path[e1, 0] = rows[cand[0]]
    path[e1, 0, act] = B[cand[0]]
    plen[e1], plen[e0] = 1, 0
    out = M.path_clearance(pi, orc, path, plen, MIX_BAND)
    seg = out["segments"]
    assert len(seg["clearance"]) == int(np.maximum(plen - 1, 0).sum()) and np.array_equal(seg["path_index"][:len(cand)], np.arange(len(cand)))
    at_v0 = [e for e in range(len(cand)) if out["seg_min"][e] == -1]
    assert len(at_v0) >= 1
    for e, i in enumerate(cand):
        v0 = rep["end_clearance"][i]                   # vertex 0 is the segment's end state
        assert _bits(out["clearance"][e]) == _bits(min(v0, seg["clearance"][e]))
        if e in at_v0:
            assert out["k_min"][e] == 0 and out["pair_min"][e] == rep["pair_min"][i] and v0 <= seg["clearance"][e]
        else:
            assert out["seg_min"][e] == 0 and out["k_min"][e] == seg["k_min"][e] and out["pair_min"][e] == seg["pair_min"][e]
        assert _bits(out["mean_vertex_clearance"][e]) == _bits((v0 + seg["end_clearance"][e]) / 2.0)
    for n in range(len(far)):              # nothing within the band anywhere on the path
        e = len(cand) + n
        assert out["clearance"][e] == MIX_BAND and out["seg_min"][e] == -1 and out["k_min"][e] == 0 and out["pair_min"][e] == -1
        assert _bits(out["mean_vertex_clearance"][e]) == _bits((MIX_BAND + MIX_BAND) / 2.0)
    # a single vertex: its own state clearance; an unsolved query: NaN
    i = cand[0]
    assert _bits(out["clearance"][e1]) == _bits(rep["end_clearance"][i]) == _bits(out["mean_vertex_clearance"][e1])
    assert out["seg_min"][e1] == -1 and out["k_min"][e1] == 0 and out["pair_min"][e1] == rep["pair_min"][i]
    assert np.isnan(out["clearance"][e0]) and np.isnan(out["mean_vertex_clearance"][e0])
    assert out["seg_min"][e0] == -1 and out["k_min"][e0] == 0 and out["pair_min"][e0] == -1
