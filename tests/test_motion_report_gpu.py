"""Motion report on the GPU (mopa_motion_report_batch / BatchPlanner.motion_report) against motion_report_ref.py, the sequential
form over the CPU oracle: every output word is compared on integer / uint64 views, on the wave-per-segment path (k_motion_report)
and on the expanded path (k_motion_expand -> k_motion_report_reduce), with per-env rows, degenerate segments, the +-pi seam,
the blockers, streams, the single-segment host form and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import SUPPORTED_ENVS
from contacts_ref import FAR, full_state
import motion_report_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("valid", "n_states", "first_bad", "last_valid_t", "last_valid_q", "first_bad_q")
_SCENES = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _mk(env):
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    if env not in _SCENES:
        pi = R.shared_segments(env)[0]
        sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
        _SCENES[env] = (sc, BatchPlanner(sc))
    return _SCENES[env]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for sc, _ in _SCENES.values():
        sc.close()
    _SCENES.clear()


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()      # (a copy: the shared inputs are read-only)


def _np(rep):
    """MotionReport -> dict of numpy arrays (blockers: count / pair / dist)"""
    import torch
    torch.cuda.synchronize()
    out = {k: getattr(rep, k).cpu().numpy() for k in FIELDS if getattr(rep, k) is not None}
    if rep.blockers is not None:
        out["blockers"] = tuple(x.cpu().numpy() for x in rep.blockers)
    return out


def _run(bp, qa, qb, rows, spe, **kw):
    return _np(bp.motion_report(_cuda(qa), _cuda(qb), _cuda(rows), samples_per_env=spe, **kw))


def _assert_report(got, want, idx=None, what=""):
    for k in FIELDS:
        w = want[k] if idx is None else want[k][idx]
        assert got[k].dtype == want[k].dtype and got[k].shape == w.shape, (what, k)
        diff = _bits(got[k]) != _bits(w)
        assert not diff.any(), f"{what}: {k} differs in {int(diff.reshape(len(w), -1).any(axis=1).sum())} of {len(w)} segments"


def _assert_blockers(got, want, idx=None, what=""):
    for g, w, name in zip(got, want, ("count", "pair", "dist")):
        w = w if idx is None else w[idx]
        assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), f"{what}: blocker {name} differs"


def _expand_size(sc):
    """the first multiple of 512 at which check_motion / the motion report take the expanded path on this scene, None if never"""
    for n in range(512, 64 * 512 + 1, 512):
        if sc.motion_kernel(n) == "k_motion_expand":
            return n
    return None


def _large_index(n):
    return np.resize(np.random.default_rng(3).permutation(512), n)


@functools.lru_cache(maxsize=None)
def _small(env):
    pi, orc, qa, qb, row = R.shared_segments(env)
    sc, bp = _mk(env)
    assert sc.motion_kernel(len(qa)) == "k_check_motion"
    return _run(bp, qa, qb, row, len(qa))


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_small_path_equals_the_reference(env, oracle_mod):
    import torch
    pi, orc, qa, qb, row = R.shared_segments(env)
    want = R.shared_report(env)
    for name, m in R.classes(want).items():
        assert m.sum() >= 1, f"{env}: no segment of class '{name}'"
    got = _small(env)
    _assert_report(got, want, what=f"{env} small path")
    sc, bp = _mk(env)
    v = bp.check_motion(_cuda(qa), _cuda(qb), _cuda(row), samples_per_env=len(qa))
    torch.cuda.synchronize()
    assert v.cpu().numpy().tobytes() == got["valid"].tobytes()
    # states=False: the four per-segment words alone, the same bytes
    lean = _run(bp, qa, qb, row, len(qa), states=False)
    assert "last_valid_q" not in lean and "first_bad_q" not in lean
    for k in FIELDS[:4]:
        assert lean[k].tobytes() == got[k].tobytes()


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_large_path_equals_the_reference_and_the_small_path(env, oracle_mod):
    import torch
    pi, orc, qa, qb, row = R.shared_segments(env)
    sc, bp = _mk(env)
    n = _expand_size(sc)
    if n is None:
        assert env not in ("SawyerPushObstacle-v0", "PusherObstacle-v0"), "the expanded path must be reachable on Push and Pusher"
        print(f"{env}: this scene never takes the expanded path (no lane-per-state kernel): nothing to compare")
        return
    assert sc.motion_kernel(n - 512) == "k_check_motion" or n == 512
    idx = _large_index(n + 37)          # the last block of 256 is not full, segments straddle blocks
    assert sc.motion_kernel(len(idx)) == "k_motion_expand" and len(idx) % 256 != 0
    got = _run(bp, qa[idx], qb[idx], row, len(idx))
    _assert_report(got, R.shared_report(env), idx, f"{env} expanded path, N = {len(idx)}")
    small = _small(env)
    for k in FIELDS:
        assert got[k].tobytes() == small[k][idx].tobytes(), k
    v = bp.check_motion(_cuda(qa[idx]), _cuda(qb[idx]), _cuda(row), samples_per_env=len(idx))
    torch.cuda.synchronize()
    assert v.cpu().numpy().tobytes() == got["valid"].tobytes()
    lean = _run(bp, qa[idx], qb[idx], row, len(idx), states=False)
    for k in FIELDS[:4]:
        assert lean[k].tobytes() == got[k].tobytes()


def test_per_env_rows_on_both_paths(oracle_mod):
    """four env rows, the cube of Push displaced per env as test_contacts_gpu.py::test_per_env_passive_rows_and_samples_per_env does:
    segment i takes env row i // samples_per_env"""
    env = "SawyerPushObstacle-v0"
    pi, orc, qa, qb, row = R.shared_segments(env)
    sc, bp = _mk(env)
    rows = np.repeat(row, 4, axis=0)
    cube = pi.model.get_joint_qpos_addr("cube")
    rng = np.random.default_rng(5)
    rows[1, cube:cube + 3] = [1.6, 0.9, 0.02]                    # parked, 1 cm into the floor: every state of this env is invalid
    rows[2, cube:cube + 3] = [0.6, 0.1, 1.25] + rng.normal(0, 0.05, 3)
    q = rng.normal(size=4)
    rows[2, cube + 3:cube + 7] = q / np.linalg.norm(q)
    rows[3, cube:cube + 2] += [0.015, -0.008]
    per_env = [R.motion_report(pi, orc, qa, qb, rows[e:e + 1], len(qa)) for e in range(4)]
    assert (per_env[1]["first_bad"] == 1).all()
    assert any(not np.array_equal(per_env[0]["first_bad"], per_env[e]["first_bad"]) for e in (2, 3))
    pick = lambda env_of, seg: {k: np.stack([per_env[e][k][s] for e, s in zip(env_of, seg)]) for k in FIELDS}
    # small path: 512 segments, 128 per env
    seg = np.arange(512)
    got = _run(bp, qa, qb, rows, 128)
    _assert_report(got, pick(seg // 128, seg), what="per-env rows, small path")
    # expanded path: the first size a multiple of 4 that expands
    n = _expand_size(sc)
    assert n is not None and n % 4 == 0
    seg = _large_index(n)
    got = _run(bp, qa[seg], qb[seg], rows, n // 4)
    _assert_report(got, pick(np.arange(n) // (n // 4), seg), what="per-env rows, expanded path")
    v = bp.check_motion(_cuda(qa[seg]), _cuda(qb[seg]), _cuda(rows), samples_per_env=n // 4)
    assert v.cpu().numpy().tobytes() == got["valid"].tobytes()


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_degenerate_segments_and_the_seam(env, oracle_mod):
    pi, orc, qa, qb, row = R.shared_segments(env)
    A, B, labels = R.edge_segments(env)
    sc, bp = _mk(env)
    want = R.motion_report(pi, orc, A, B, row, len(A))
    i = labels.index("equal-invalid")
    assert want["first_bad"][i] == 1 and want["n_states"][i] == 1 and want["last_valid_t"][i] == 0.0
    if "seam" in labels:
        assert want["n_states"][labels.index("seam")] == 19
    _assert_report(_run(bp, A, B, row, len(A)), want, what=f"{env} edge segments, small path")
    n = _expand_size(sc)
    if n is not None:
        idx = np.resize(np.arange(len(A)), n + 5)
        _assert_report(_run(bp, A[idx], B[idx], row, len(idx)), want, idx, f"{env} edge segments, expanded path")


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_blockers(env, oracle_mod):
    from mopa_rl_amd.batch import BatchPlanner
    pi, orc, qa, qb, row = R.shared_segments(env)
    sc, bp = _mk(env)
    thr = pi.spec.contact_threshold
    want = R.shared_report(env)
    blocked = want["first_bad"] > 0
    full = BatchPlanner(sc.contact_scene())      # the scene with the whole pair list: the call chains mopa_contacts_batch itself
    for K in (4, 1):
        ref = R.blockers(pi, orc, want, row, K, len(qa))
        got = _run(bp, qa, qb, row, len(qa), max_contacts=K)
        _assert_report(got, want, what=f"{env} K = {K}")
        _assert_blockers(got["blockers"], ref, what=f"{env} K = {K}")
        cnt, pair, dist = got["blockers"]
        assert (cnt[blocked] >= 1).all() and (dist[blocked].min(axis=1) <= thr).all()
        assert (cnt[~blocked] == 0).all() and (pair[~blocked] == -1).all() and np.array_equal(_bits(dist[~blocked]), _bits(np.full_like(dist[~blocked], FAR)))
        sep = bp.contacts(_cuda(got["first_bad_q"]), _cuda(row), samples_per_env=len(qa), cutoff=thr, max_contacts=K)
        _assert_blockers(got["blockers"], tuple(x.cpu().numpy() for x in sep), what=f"{env} K = {K} against contacts()")
        lean = _run(bp, qa, qb, row, len(qa), states=False, max_contacts=K)
        assert "first_bad_q" not in lean
        _assert_blockers(lean["blockers"], ref, what=f"{env} K = {K}, states=False")
        for states in (True, False):     # first_bad_q in library scratch when the caller keeps no rows
            chained = _run(full, qa, qb, row, len(qa), states=states, max_contacts=K)
            _assert_blockers(chained["blockers"], ref, what=f"{env} K = {K}, full scene, states={states}")
            assert chained["first_bad"].tobytes() == want["first_bad"].tobytes()
    n = _expand_size(sc)
    if n is not None and env == "SawyerPushObstacle-v0":
        idx = _large_index(n + 37)
        ref = R.blockers(pi, orc, want, row, 4, len(qa))
        for planner, states in ((bp, True), (full, False)):
            got = _run(planner, qa[idx], qb[idx], row, len(idx), states=states, max_contacts=4)
            _assert_blockers(got["blockers"], ref, idx, f"{env} expanded path")


def test_two_runs_two_streams_and_the_host_form(oracle_mod):
    import torch
    from mopa_rl_amd.planner import PyKinematicPlanner
    env = "SawyerPushObstacle-v0"
    pi, orc, qa, qb, row = R.shared_segments(env)
    sc, bp = _mk(env)
    want = R.shared_report(env)
    n = _expand_size(sc)
    for idx in (np.arange(512), _large_index(n + 37)):
        ta, tb, tr = _cuda(qa[idx]), _cuda(qb[idx]), _cuda(row)
        torch.cuda.synchronize()
        reps = []
        for st in (None, None, torch.cuda.Stream(), torch.cuda.Stream()):
            if st is None:
                reps.append(bp.motion_report(ta, tb, tr, samples_per_env=len(idx), max_contacts=4))
            else:
                with torch.cuda.stream(st):
                    reps.append(bp.motion_report(ta, tb, tr, samples_per_env=len(idx), max_contacts=4, stream=st))
        outs = [_np(r) for r in reps]
        for o in outs[1:]:
            assert all(o[k].tobytes() == outs[0][k].tobytes() for k in FIELDS)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(o["blockers"], outs[0]["blockers"]))
    # the single-segment host form: two segments of every class
    batch = _run(bp, qa, qb, row, len(qa), max_contacts=4)
    m = pi.model
    g = np.asarray(m.pair_geom).reshape(-1, 2)
    name = lambda k: m.all_geom_names[int(m.geom_mjid[int(k)])]
    pl = PyKinematicPlanner(pi.spec.scene, "rrt_connect", 7, "", 0.0, pi.spec.range, pi.passive_joint_idx, [], pi.ignored_contacts,
                            pi.spec.contact_threshold, 0.05, False, 0.0, 1)
    for cls in R.classes(want).values():
        for i in np.nonzero(cls)[0][:2]:
            a, b = full_state(pi, qa[i], row[0]), full_state(pi, qb[i], row[0])
            b[pi.passive_joint_idx] += 0.25          # the passive entries come from a
            valid, c, fb, t, lvq, fbq, blk = sc.motion_report_raw(a, b, 4)
            assert (int(valid), c, fb) == (batch["valid"][i], batch["n_states"][i], batch["first_bad"][i])
            assert np.array_equal(_bits(np.float64(t)), _bits(batch["last_valid_t"][i]))
            assert np.array_equal(_bits(lvq), _bits(batch["last_valid_q"][i])) and np.array_equal(_bits(fbq), _bits(batch["first_bad_q"][i]))
            assert blk[0] == batch["blockers"][0][i] and np.array_equal(blk[1], batch["blockers"][1][i])
            assert np.array_equal(_bits(blk[2]), _bits(batch["blockers"][2][i]))
            d = sc.motion_report_state(a, b, max_contacts=4)
            k = min(blk[0], 4)
            assert d["valid"] == valid and d["first_bad"] == fb and d["n_states"] == c and d["n_blockers"] == blk[0]
            assert d["blockers"] == [(name(g[p, 0]), name(g[p, 1]), float(x)) for p, x in zip(blk[1][:k], blk[2][:k])]
            assert bool(d["blockers"]) == (fb > 0)
            assert sc.motion_report_state(a, b)["blockers"] is None
            pd = pl.motion_report(a, b, max_contacts=4)
            assert pd["blockers"] == d["blockers"] and pd["first_bad"] == fb and np.array_equal(_bits(pd["first_bad_q"]), _bits(fbq))
    # the chained host form on the scene with the whole pair list
    full = sc.contact_scene()
    i = int(np.nonzero(want["first_bad"] > 1)[0][0])
    a, b = full_state(pi, qa[i], row[0]), full_state(pi, qb[i], row[0])
    r = full.motion_report_raw(a, b, 4)
    assert r[2] == batch["first_bad"][i] and r[6][0] == batch["blockers"][0][i] and np.array_equal(_bits(r[6][2]), _bits(batch["blockers"][2][i]))
    pl.close()


def test_refusals(oracle_mod):
    import torch
    import glue_ref as G
    from mopa_rl_amd import _lib
    env = "SawyerPushObstacle-v0"
    pi, orc, qa, qb, row = R.shared_segments(env)
    sc, bp = _mk(env)
    L = _lib.lib()
    N, K = 64, 4
    ta, tb, tr = _cuda(qa[:N]), _cuda(qb[:N]), _cuda(row)
    u8 = torch.zeros(N, dtype=torch.uint8, device="cuda")
    i32 = [torch.zeros(N * K, dtype=torch.int32, device="cuda") for _ in range(4)]
    f64 = [torch.zeros(N * max(K, sc.na), dtype=torch.float64, device="cuda") for _ in range(4)]
    vp = lambda t: C.c_void_p(t.data_ptr())
    h = sc.handle
    base = [h, vp(ta), vp(tb), vp(tr), N, N, vp(u8), vp(i32[0]), vp(i32[1]), vp(f64[0]), vp(f64[1]), vp(f64[2]), 0, None, None, None, None]
    call = lambda **kw: L.mopa_motion_report_batch(*[kw.get(k, v) for k, v in zip(
        ("scene", "qa", "qb", "env", "N", "spe", "valid", "n_states", "first_bad", "t", "lvq", "fbq", "K", "cnt", "pair", "dist", "stream"), base)])
    assert call() == 0
    assert call(lvq=None, fbq=None) == 0                       # the two rows are optional
    for k in ("scene", "qa", "qb", "env", "valid", "n_states", "first_bad", "t"):
        assert call(**{k: None}) == 1, k                       # MOPA_ERR_INVALID_ARG
        assert b"null" in L.mopa_last_error()
    assert call(N=-1) == 1 and call(spe=0) == 1 and call(spe=-2) == 1
    blk = dict(cnt=vp(i32[2]), pair=vp(i32[3]), dist=vp(f64[3]))
    assert call(K=K, **blk) == 0
    assert call(K=-1, **blk) == 1 and call(K=-1) == 1 and call(K=0, **blk) == 1
    for k in blk:
        assert call(K=K, **dict(blk, **{k: None})) == 1, k
    assert call(N=0) == 0 and call(N=0, K=K, **blk) == 0
    # a scene whose threshold is not negative: the blockers are refused as mopa_contacts_batch refuses the cutoff, the report runs
    zero = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, 0.0, range_=pi.spec.range, seed=7, prune_pairs=False)
    assert call(scene=zero.handle) == 0 and call(scene=zero.handle, K=K, **blk) == 1
    assert b"cutoff" in L.mopa_last_error()
    # a glued scene
    c = G.glue_case(oracle_mod, env)
    plain = _lib.Scene(*c.scene_args(), range_=c.pi.spec.range, seed=7)
    gl = plain.glued(c.a, c.b)
    assert call(scene=gl.handle) == 2 and call(scene=gl.handle, K=K, **blk) == 2      # MOPA_ERR_UNSUPPORTED
    assert "glued scene" in L.mopa_last_error().decode()
    a = full_state(pi, qa[0], row[0])
    with pytest.raises(_lib.MopaError, match="error 2"):
        gl.motion_report_raw(a, a)
    with pytest.raises(_lib.MopaError):
        bp.motion_report(ta, tb, tr, max_contacts=-1)
    with pytest.raises(_lib.MopaError):
        bp.motion_report(ta, tb[:32].contiguous(), tr)
    torch.cuda.synchronize()
    for s in (zero, plain):
        s.close()


def test_planner_refuses_glue_bodies(oracle_mod):
    import glue_ref as G
    from mopa_rl_amd.planner import PyKinematicPlanner
    c = G.glue_case(oracle_mod, "SawyerPushObstacle-v0")
    pk = PyKinematicPlanner(b"sawyer_push_obstacle.xml", b"rrt_connect", 7, b"", 0.0, c.pi.spec.range, c.passive, [b"clawGripper", b"cube"], c.ignored,
                            c.thr, 0.05, False, 0.1, 11)
    q = np.zeros(c.pi.model.nq)
    with pytest.raises(NotImplementedError, match="motion_report"):
        pk.motion_report(q, q)
    pk.close()
