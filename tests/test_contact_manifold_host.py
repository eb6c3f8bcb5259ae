"""Contact manifolds, host form (mopa_geom_manifolds_host: the host compile of the kernels' geom_manifold): agreement with the
numpy restatement of the candidate table (manifold_ref.manifold), the link to the contact frames (mopa_geom_frames_host),
invariants of the witnesses by signed-distance functions, known answers in closed form, the ABI's refusals.  No GPU.

The candidate table is restated from MuJoCo's documented behaviour ([3P], PARITY UNPINNED): nothing here compares with MuJoCo."""
import ctypes as C
import math

import numpy as np
import pytest

import frames_ref as F
import manifold_ref as M
from geom_ref import BOX, CAPSULE, CYLINDER, PLANE, SPHERE, rand_rot

CUTS = (0.0, 0.05, -0.01)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def can():
    from mopa_rl_amd.scene import load_scene
    m = load_scene("sawyer_lift_obstacle")
    return m.mesh_vert[m.mesh_vertadr[0]:m.mesh_vertadr[0] + m.mesh_vertnum[0]].copy()


@pytest.fixture(scope="module")
def solved(can):
    """cases (both orders of the two geoms), their frames, and the host form at P = 8 for every cutoff of CUTS"""
    cs = M.cases()
    cs = cs + [c.swapped() for c in cs if c.t1 != c.t2 and c.t2 != F.MESH]
    return cs, F.host_frames(cs, can), {cut: M.host(cs, can, cut, 8) for cut in CUTS}


def _canon(c):
    return (min(c.t1, c.t2), max(c.t1, c.t2))


def test_agreement_with_the_independent_form(solved):
    cs, fr, out = solved
    seen = {}
    for cut in CUTS:
        nd, npt, pts = out[cut]
        for i, c in enumerate(cs):
            k, want = M.manifold(c, fr[i], cut)
            assert k == npt[i], (c.cls, c.what, cut, k, npt[i])
            M.assert_same_points(pts[i], want, (c.cls, c.what, cut))
            seen.setdefault(_canon(c), set()).add(int(npt[i]))
    # the multi-point paths ran: every count each class can give
    assert seen[(PLANE, CAPSULE)] >= {0, 1, 2} and seen[(PLANE, BOX)] >= {0, 1, 2, 4} and seen[(PLANE, CYLINDER)] >= {0, 1, 2, 3, 4}
    assert seen[(CAPSULE, BOX)] >= {0, 1, 2} and seen[(BOX, BOX)] >= {0, 1, 4, 8}, seen
    assert all(v <= {0, 1} for k, v in seen.items() if k not in M.MULTI)


def test_link_to_the_frames(solved, can):
    cs, fr, out = solved
    n_single = n_fallback = 0
    for cut in CUTS:
        nd, npt, pts = out[cut]
        assert np.array_equal(_bits(nd[:, :3]), _bits(fr[:, 1:4])) and np.array_equal(_bits(nd[:, 3]), _bits(fr[:, 0]))
        for i, c in enumerate(cs):
            d = fr[i, 0]
            if d == F.FAR:
                assert npt[i] == 0 and not nd[i, :3].any() and (pts[i, :, 3] == F.FAR).all() and not pts[i, :, :3].any()
                continue
            frame_pt = np.concatenate([fr[i, 4:7], [d]])
            if _canon(c) not in M.MULTI:
                assert npt[i] == (1 if d <= cut else 0), (c.cls, c.what)
                n_single += 1
            if npt[i] == 1 and (_canon(c) not in M.MULTI or not _rule_points(c, fr[i], cut)):
                assert np.array_equal(_bits(pts[i, 0]), _bits(frame_pt)), (c.cls, c.what)     # the frame's pos and dist, bit for bit
                n_fallback += _canon(c) in M.MULTI
        # P = 1 and P = 2 hold the prefix of P = 8, npoint unchanged
        for P in (1, 2):
            nd2, npt2, pts2 = M.host(cs, can, cut, P)
            assert np.array_equal(npt2, npt) and np.array_equal(_bits(nd2), _bits(nd)) and np.array_equal(_bits(pts2), _bits(pts[:, :P]))
    assert n_single > 300 and n_fallback >= 10, (n_single, n_fallback)


def _rule_points(c, frame, cut):
    """the class rule's own points under the cutoff (independent form); empty: the fallback applies"""
    n = frame[1:4]
    if c.t1 > c.t2:
        c, n = c.swapped(), -n
    return [x for _, x in M.candidates(c, n) if x <= cut]


def test_invariants_of_the_witnesses(solved):
    """Every point that a class rule generated has its two witnesses ON the two surfaces.  A point that is the frame's, bit for
    bit (single-point classes, fallbacks), is checked where the frame's witnesses lie on the surfaces by construction -- plane-X,
    sphere-X, capsule-capsule; the frame of a SAT class names a feature centre or a clamped edge point, whose own invariants
    test_contact_frames_host checks through support functions."""
    cs, fr, out = solved
    exact_frame = {(PLANE, SPHERE), (PLANE, CAPSULE), (PLANE, CYLINDER), (PLANE, BOX), (SPHERE, SPHERE), (SPHERE, CAPSULE), (SPHERE, CYLINDER),
                   (SPHERE, BOX), (CAPSULE, CAPSULE)}
    n_rule = n_frame = 0
    for cut in CUTS:
        nd, npt, pts = out[cut]
        for i, c in enumerate(cs):
            if c.t1 not in M.SDF_TYPES or c.t2 not in M.SDF_TYPES:
                continue
            n, dpair = nd[i, :3], nd[i, 3]
            for j in range(int(npt[i])):
                pos, d = pts[i, j, :3], pts[i, j, 3]
                is_frame = np.array_equal(_bits(pts[i, j]), _bits(np.concatenate([fr[i, 4:7], [fr[i, 0]]])))
                assert d <= cut and d >= dpair - 1e-9, (c.cls, c.what, d, dpair)       # under the cutoff, and no deeper than the pair
                if j:
                    assert pts[i, j - 1, 3] <= d
                if is_frame and _canon(c) not in exact_frame:
                    continue
                w1, w2 = pos - 0.5 * d * n, pos + 0.5 * d * n
                assert np.abs((w2 - w1) - d * n).max() <= 1e-12
                e1, e2 = M.sdf(c.t1, c.s1, c.p1, c.m1, w1), M.sdf(c.t2, c.s2, c.p2, c.m2, w2)
                assert abs(e1) <= 1e-9 and abs(e2) <= 1e-9, (c.cls, c.what, cut, j, e1, e2)
                n_rule += not is_frame
                n_frame += is_frame
    assert n_rule > 500 and n_frame > 200, (n_rule, n_frame)


def test_rigid_motion_and_order_of_the_geoms(solved, can):
    cs, fr, out = solved
    nd, npt, pts = out[0.0]
    half = len(M.cases())
    rng = np.random.default_rng(17)
    pick = [i for i in range(half) if not cs[i].mpr and cs[i].what == "random" and cs[i].t2 != F.MESH and npt[i] > 0][::2]
    assert len(pick) >= 40 and sum(npt[i] > 1 for i in pick) >= 15
    moved = []
    for i in pick:
        R, t = rand_rot(rng), rng.uniform(-1, 1, 3)
        moved.append((R, t, cs[i].moved(R, t)))
    nd2, npt2, pts2 = M.host([m[2] for m in moved], can, 0.0, 8)
    for k, (i, (R, t, _)) in enumerate(zip(pick, moved)):
        assert npt2[k] == npt[i], cs[i].cls
        assert np.abs(nd2[k, :3] - R @ nd[i, :3]).max() <= 1e-9 and abs(nd2[k, 3] - nd[i, 3]) <= 1e-12
        # (two points of equal depth -- the cylinder's +-120 degree pair always is one -- are ordered by the last bit: sorted distances
        #  agree in order, the points as a set)
        assert np.abs(pts2[k, :, 3] - pts[i, :, 3]).max() <= 1e-9, cs[i].cls
        left = list(range(int(npt[i])))
        for j in range(int(npt[i])):
            m = [b for b in left if abs(pts2[k, b, 3] - pts[i, j, 3]) <= 1e-9 and np.abs(pts2[k, b, :3] - (R @ pts[i, j, :3] + t)).max() <= 1e-9]
            assert m, (cs[i].cls, j)
            left.remove(m[0])
    # the geoms given the other way round: the normal negated, the points unchanged
    n_sw = 0
    given = [k for k in range(half) if cs[k].t1 != cs[k].t2 and cs[k].t2 != F.MESH]       # (the fixture appended their reverses in this order)
    assert len(given) == len(cs) - half
    for cut in CUTS:
        nd, npt, pts = out[cut]
        for i, j in zip(range(half, len(cs)), given):
            assert npt[i] == npt[j] and np.array_equal(_bits(pts[i]), _bits(pts[j])) and _bits(nd[i, 3]) == _bits(nd[j, 3])
            assert np.array_equal(_bits(nd[i, :3]), _bits(-nd[j, :3]) if nd[j, 3] != F.FAR else _bits(nd[j, :3]))
            n_sw += npt[i] > 1
    assert n_sw >= 60


def _one(what, cut=0.0, P=8):
    c = next(c for c in M.flat_cases() if c.what == what)
    nd, npt, pts = M.host([c], None, cut, P)
    return c, nd[0], int(npt[0]), pts[0]


def _same_set(got, want):
    got, want = np.asarray(got), np.asarray(want, dtype=float)
    assert len(got) == len(want)
    for w in want:
        assert (np.abs(got - w).max(axis=1) <= 1e-12).sum() == 1, (got, w)


def test_known_answers():
    # plane - box: flat 4, an edge 2, a vertex 1
    c, nd, k, p = _one("box sunk flat")
    assert k == 4 and np.allclose(p[:4, 3], -0.02, atol=1e-12) and np.array_equal(nd[:3], [0, 0, 1])
    _same_set(p[:4, :3], [[0.3 + a, -0.2 + b, -0.01] for a in (-0.1, 0.1) for b in (-0.2, 0.2)])
    assert (p[4:, 3] == F.FAR).all() and not p[4:, :3].any()
    c, nd, k, p = _one("box on a vertex")
    assert k == 1 and np.allclose(p[0], [0.1, 0.2, -0.005, -0.01], atol=1e-12)
    c, nd, k, p = _one("box on an edge")
    assert k == 2 and np.allclose(p[:2, 3], -0.01, atol=1e-12)
    _same_set(p[:2, :3], [[0.1, 0.0, -0.005], [0.1, 0.4, -0.005]])
    # plane - capsule: lying 2, standing 1
    c, nd, k, p = _one("capsule lying")
    assert k == 2 and np.allclose(p[:2, 3], -0.01, atol=1e-12)
    _same_set(p[:2, :3], [[0.1, 0.2, -0.005], [0.1, -0.2, -0.005]])
    c, nd, k, p = _one("capsule standing")
    assert k == 1 and np.allclose(p[0], [0.1, 0.0, -0.005, -0.01], atol=1e-12)
    # plane - cylinder, standing: the deepest rim point along the cylinder's own x axis and its two companions at 120 degrees; the
    # top rim's point (b) at 0.59 only under a point_cutoff that admits it
    rim = lambda ang, z: [0.2 + 0.1 * math.cos(0.3 + ang), 0.1 + 0.1 * math.sin(0.3 + ang), z]
    c, nd, k, p = _one("cylinder standing")
    assert k == 3 and np.allclose(p[:3, 3], -0.01, atol=1e-12)
    assert np.allclose(p[0, :3], rim(0, -0.005), atol=1e-12)                                  # (a) first: ties keep generation order
    _same_set(p[:3, :3], [rim(0, -0.005), rim(2 * math.pi / 3, -0.005), rim(-2 * math.pi / 3, -0.005)])
    c, nd, k, p = _one("cylinder standing", cut=0.6)
    assert k == 4 and np.allclose(p[3], rim(0, 0.59 - 0.295) + [0.59], atol=1e-12)
    assert _one("cylinder standing", cut=0.58)[2] == 3
    c, nd, k, p = _one("cylinder lying")
    assert k == 2 and np.allclose(p[:2, 3], -0.01, atol=1e-12)
    _same_set(p[:2, :3], [[0.2, 0.4, -0.005], [0.2, -0.2, -0.005]])
    # box - box
    c, nd, k, p = _one("small box flat on a large box")
    cs_, sn = math.cos(0.3), math.sin(0.3)
    assert k == 4 and np.allclose(p[:4, 3], -0.01, atol=1e-12) and np.allclose(nd[:3], [0, 0, 1])
    _same_set(p[:4, :3], [[0.1 + cs_ * a - sn * b, -0.1 + sn * a + cs_ * b, 0.095] for a in (-0.05, 0.05) for b in (-0.06, 0.06)])
    c2, nd2, k2, p2 = _one("large box under a small box (mirror)")
    assert k2 == 4 and np.allclose(nd2[:3], [0, 0, -1])
    _same_set(p2[:4, :3], p[:4, :3])
    c, nd, k, p = _one("equal boxes at 45 degrees")
    rad = 0.1 / math.cos(math.pi / 8)
    assert k == 8 and np.allclose(p[:, 3], -0.01, atol=1e-12)
    _same_set(p[:, :3], [[rad * math.cos(math.pi / 8 + j * math.pi / 4), rad * math.sin(math.pi / 8 + j * math.pi / 4), 0.095] for j in range(8)])
    c, nd, k, p = _one("box overhanging an edge")
    assert k == 4 and np.allclose(p[:4, 3], -0.01, atol=1e-12)
    _same_set(p[:4, :3], [[x, y, 0.095] for x in (0.35, 0.5) for y in (0.25, 0.4)])
    c, nd, k, p = _one("edge crossing edge")
    fr = F.host_frames([c], None)[0]
    assert k == 1 and fr[0] == pytest.approx(0.13 - 0.1 * math.sqrt(2)) and np.array_equal(_bits(p[0]), _bits(np.concatenate([fr[4:7], [fr[0]]])))
    # capsule - box
    c, nd, k, p = _one("capsule flat on a box face")
    assert k == 2 and np.allclose(p[:2, 3], -0.01, atol=1e-12)
    _same_set(p[:2, :3], [[-0.15, 0, 0.095], [0.25, 0, 0.095]])
    c, nd, k, p = _one("capsule flat, one end beyond the face")
    assert k == 1 and np.allclose(p[0], [0.2, 0, 0.095, -0.01], atol=1e-12)
    c, nd, k, p = _one("capsule across a box edge")
    fr = F.host_frames([c], None)[0]
    assert k == 1 and np.array_equal(_bits(p[0]), _bits(np.concatenate([fr[4:7], [fr[0]]])))     # the fallback: the frame's point
    assert not M.candidates(c, fr[1:4])


def test_abi_symbols_and_refusals():
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import ContactReport
    from mopa_rl_amd.planner import PyKinematicPlanner
    L = _lib.lib()
    for sym in ("mopa_contact_manifolds_batch", "mopa_contact_manifolds_state", "mopa_geom_manifolds_batch", "mopa_geom_manifolds_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and getattr(L, sym) is not None
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    t = np.zeros((1, 2), dtype=np.int32)
    r = np.zeros((1, 30))
    nd, k, pts = np.zeros((1, 4)), np.zeros(1, dtype=np.int32), np.zeros((1, 8, 4))
    tp, rp, ndp, kp, pp = t.ctypes.data_as(ip), r.ctypes.data_as(dp), nd.ctypes.data_as(dp), k.ctypes.data_as(ip), pts.ctypes.data_as(dp)
    host = L.mopa_geom_manifolds_host
    assert host(0, None, None, None, 0, 0.0, 4, None, None, None) == 0
    assert host(1, tp, rp, None, 0, 0.0, 8, ndp, kp, pp) == 0 and nd[0, 3] == F.FAR and k[0] == 0 and (pts[0, :, 3] == F.FAR).all()   # (plane, plane)
    for P in (0, 9, -1):
        assert host(1, tp, rp, None, 0, 0.0, P, ndp, kp, pp) == 1 and b"max_points" in L.mopa_last_error()       # MOPA_ERR_INVALID_ARG
    for cut in (float("nan"), float("inf")):
        assert host(1, tp, rp, None, 0, cut, 4, ndp, kp, pp) == 1 and b"point_cutoff" in L.mopa_last_error()
    assert host(-1, tp, rp, None, 0, 0.0, 4, ndp, kp, pp) == 1
    assert host(1, None, rp, None, 0, 0.0, 4, ndp, kp, pp) == 1 and host(1, tp, rp, None, 0, 0.0, 4, None, kp, pp) == 1
    assert host(1, tp, rp, None, 0, 0.0, 4, ndp, None, pp) == 1 and host(1, tp, rp, None, 0, 0.0, 4, ndp, kp, None) == 1
    assert host(1, tp, rp, None, 3, 0.0, 4, ndp, kp, pp) == 1
    assert L.mopa_geom_manifolds_batch(0, -1, None, None, 0.0, 4, None, None, None, None) == 1
    assert L.mopa_geom_manifolds_batch(0, 1, None, None, 0.0, 4, None, None, None, None) == 1
    assert L.mopa_contact_manifolds_batch(None, None, None, 1, 1, -0.001, 0.0, 4, 4, None, None, None, None, None, None, None, None) == 1
    assert L.mopa_contact_manifolds_state(None, None, -0.001, 0.0, 4, 4, None, None, None, None, None, None, None) == 1
    with pytest.raises(_lib.MopaError):
        _lib.geom_manifolds_host(np.zeros((2, 2)), np.zeros((1, 2, 15)))
    with pytest.raises(_lib.MopaError, match="max_points"):
        _lib.geom_manifolds_host(t, r, max_points=9)
    # without manifolds a report carries none, and iterates as before
    rep = ContactReport(1, 2, 3, None)
    assert rep.npoint is None and rep.point_dist is None and rep.point_pos is None and rep.normal is None and tuple(rep) == (1, 2, 3)
    rep = ContactReport(1, 2, 3, None, 4, None, 5, 6, 7)
    assert (rep.normal, rep.pos, rep.npoint, rep.point_dist, rep.point_pos) == (4, None, 5, 6, 7) and tuple(rep) == (1, 2, 3)
    # glue_bodies keeps raising (decided before the scene is touched)
    pl = PyKinematicPlanner.__new__(PyKinematicPlanner)
    pl.glue_bodies = ["a", "b"]
    with pytest.raises(NotImplementedError):
        pl.contacts(np.zeros(3), manifold=True)
