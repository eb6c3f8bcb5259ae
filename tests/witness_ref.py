"""Independent checks and the sequential form of the proximity report's witness points (helpers of test_proximity_witness_host /
test_proximity_witness_gpu).

What a witness (d, n, p1, p2) of a posed pair has to satisfy does not depend on how it was found, and nothing here shares code with
mopa_gjk.hpp / mopa_witness.hpp: a point's membership in a primitive is its local-frame inequalities, in a hull the facet
equations of scipy's ConvexHull of the hull vertices.

    membership   p1 inside or on shape 1, p2 inside or on shape 2, to E_m
    attainment   true - 2 E_m <= |p2 - p1| <= d + kGjkTol.  The lower bound is a theorem given membership: two points within E_m of
                 the shapes are at least true - 2 E_m apart.  The upper bound is the project's tolerance for d itself, granted once
                 more for the barycentric reconstruction of the two points.
    normal       | |n| - 1 | <= 1e-12 and | n . (p2 - p1) - |p2 - p1| | <= 1e-12 (1 + scale)

E_m = 1e-11 (1 + scale): ten times the pose-rounding slack test_gjk_truth_host derives (a case's coordinates stay below 3 m, one
rounding is at most 3.3e-16 m, a pose is a few dozen of them); the witness adds a convex combination of up to three support points
and the rigid motions in and out of the shapes' frames, a few dozen roundings more.

Sequential form of the scene-level report: the oracle's geom poses, geom_witness_host on every candidate pair with no broad phase in
front, proximity_ref's selection."""
import numpy as np

import frames_ref as F
import gjk_cases as G
import proximity_ref as P
from contacts_ref import ignored_mask
from geom_ref import BOX, CAPSULE, CYLINDER, MESH, PLANE, SPHERE

K_GJK_TOL = 1e-6          # kGjkTol (mopa_gjk.hpp)
FAR = F.FAR
OUTPUTS = ("clearance", "count", "pair", "dist", "normal", "p1", "p2")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def e_m(scale):
    return 1e-11 * (1.0 + np.asarray(scale, dtype=np.float64))


def host_witness(cs, can, band, iters=False):
    """mopa_geom_witness_host on a case list: [M, 10] = d, n, p1, p2; with iters=True also the [M] support-evaluation counts"""
    from mopa_rl_amd import _lib
    types, recs = F.recs_of(cs)
    return _lib.geom_witness_host(types, recs, band, mesh_verts=can, return_iters=iters)


# ---------------- membership: local-frame inequalities ----------------
def outside_by(t, size, pos, mat, x, can):
    """how far the point x lies outside the shape: <= 0 inside or on it.  (For a box, a cylinder and a hull the largest violated
    inequality: the distance where one inequality is violated, within a factor sqrt(3) of it near an edge or a vertex.)"""
    l = mat.T @ (x - pos)
    if t == PLANE:                   # the half space below the plane
        return float(l[2])
    if t == SPHERE:
        return float(np.linalg.norm(l) - size[0])
    if t == CAPSULE:
        return float(np.linalg.norm(l - np.array([0.0, 0.0, np.clip(l[2], -size[1], size[1])])) - size[0])
    if t == CYLINDER:
        return float(max(np.hypot(l[0], l[1]) - size[0], abs(l[2]) - size[1]))
    if t == BOX:
        return float((np.abs(l) - size[:3]).max())
    if t == MESH:                    # scipy's facets: unit outward normals a, offsets b, a . x + b <= 0 inside
        eq = G._hull(can).equations
        return float((eq[:, :3] @ l + eq[:, 3]).max())
    raise ValueError(t)


def check_membership(cs, W, scale, can, rows=None):
    """-> the largest excess seen; AssertionError where a reported witness point lies more than E_m outside its shape"""
    e = np.broadcast_to(e_m(scale), (len(cs),))
    worst = -np.inf
    for i in (range(len(cs)) if rows is None else rows):
        if W[i, 0] == FAR:
            continue
        c = cs[i]
        o1 = outside_by(c.t1, c.s1, c.p1, c.m1, W[i, 4:7], can)
        o2 = outside_by(c.t2, c.s2, c.p2, c.m2, W[i, 7:10], can)
        worst = max(worst, o1, o2)
        assert o1 <= e[i] and o2 <= e[i], (c.cls, c.what, i, o1, o2, e[i])
    return worst


def check_attainment(cs, W, true, scale, rows=None):
    """separated pairs (d > 0): true - 2 E_m <= |p2 - p1| <= d + kGjkTol; -> [M] |p2 - p1| - d (NaN where not checked)"""
    e = np.broadcast_to(e_m(scale), (len(cs),))
    true = np.broadcast_to(np.asarray(true, dtype=np.float64), (len(cs),))
    gap = np.full(len(cs), np.nan)
    for i in (range(len(cs)) if rows is None else rows):
        d = W[i, 0]
        if d == FAR or not d > 0.0:
            continue
        ln = float(np.linalg.norm(W[i, 7:10] - W[i, 4:7]))
        gap[i] = ln - d
        assert true[i] - 2.0 * e[i] <= ln <= d + K_GJK_TOL, (cs[i].cls, cs[i].what, i, ln, d, true[i])
    return gap


def check_normal(cs, W, scale, rows=None):
    """reported separated pairs: n is a unit vector, and it is the direction from p1 to p2"""
    e = np.broadcast_to(1e-12 * (1.0 + np.asarray(scale, dtype=np.float64)), (len(cs),))
    for i in (range(len(cs)) if rows is None else rows):
        d = W[i, 0]
        if d == FAR:
            continue
        n, u = W[i, 1:4], W[i, 7:10] - W[i, 4:7]
        assert abs(float(np.linalg.norm(n)) - 1.0) <= 1e-12, (cs[i].cls, cs[i].what, i, n)
        if d > 0.0:
            assert abs(float(n @ u) - float(np.linalg.norm(u))) <= e[i], (cs[i].cls, cs[i].what, i, n, u)


def check_all(cs, W, true, scale, can, rows=None):
    worst = check_membership(cs, W, scale, can, rows)
    gap = check_attainment(cs, W, true, scale, rows)
    check_normal(cs, W, scale, rows)
    return worst, gap


def exchanged(W):
    """what the other order of the pairs has to return: p1 / p2 exchanged, n negated, the same d; FAR rows unchanged (all zero)"""
    out = W.copy()
    rep = W[:, 0] != FAR
    out[rep, 1:4] = -W[rep, 1:4]
    out[rep, 4:7], out[rep, 7:10] = W[rep, 7:10], W[rep, 4:7]
    return out


# ---------------- closed-form classes: random separated pairs ----------------
CLOSED_CLASSES = [(PLANE, SPHERE), (PLANE, CAPSULE), (PLANE, CYLINDER), (PLANE, BOX), (PLANE, MESH), (SPHERE, SPHERE), (SPHERE, CAPSULE),
                  (SPHERE, CYLINDER), (SPHERE, BOX), (CAPSULE, CAPSULE), (CAPSULE, BOX)]
N_CLOSED = 25             # base pairs per class; each at every gap of gjk_cases.GAPS: 200 per class
RANDOM_SCALE = 1.0        # geom_ref.rand_size: sizes up to 0.3 m, centres within 1 m -- the magnitudes of gjk_cases at scale 1
_CACHE = {}


def closed_cases(can):
    """N_CLOSED random pairs of every closed-form class (frames_ref.random_cases: geom_ref.rand_rot / rand_size), the second shape
    moved along the centre line to every gap of gjk_cases.GAPS (proximity_ref.place: WHERE a case lands, not what its distance is)"""
    if "closed" not in _CACHE:
        _CACHE["closed"] = P.place(F.random_cases(classes=CLOSED_CLASSES, n=N_CLOSED), can, gaps=G.GAPS)
    return _CACHE["closed"]


# ---------------- scene level: the sequential form ----------------
def pair_witness(pi, gpos, gmat, band):
    """[N, npair, 10]: geom_witness_host of every candidate pair on the poses given, no broad phase in front; ignored pairs FAR / 0"""
    from mopa_rl_amd import _lib
    m = pi.model
    pg = np.asarray(m.pair_geom).reshape(-1, 2)
    N, npair = len(gpos), len(pg)
    size = np.asarray(m.geom_size, dtype=np.float64)
    gt = np.asarray(m.geom_type)
    size = np.where((gt == MESH)[:, None], 0.0, size)
    rec = np.concatenate([gpos, gmat, np.broadcast_to(size, (N,) + size.shape)], axis=2)
    types = np.broadcast_to(gt[pg].astype(np.int32), (N, npair, 2))
    W = _lib.geom_witness_host(types.reshape(-1, 2), rec[:, pg].reshape(-1, 30), band, mesh_verts=P.can_of(m)).reshape(N, npair, 10)
    ign = ignored_mask(pi)
    W[:, ign, 0] = FAR
    W[:, ign, 1:] = 0.0
    return W


def proximity_witness(pi, poses, band, K, table=None):
    """the contract of mopa_proximity_witness_batch on the poses (gpos, gmat) of N states: dict of OUTPUTS -- proximity_ref.select on
    the witness table's distances, then n / p1 / p2 of the selected pairs, 0.0 in unused slots.  table: `pair_witness` of the same
    poses and band, where several K share it"""
    W = pair_witness(pi, *poses, band) if table is None else table
    clearance, count, pair, dist = P.select(W[:, :, 0].copy(), band, K)
    N = len(W)
    out = {k: np.zeros((N, K, 3)) for k in ("normal", "p1", "p2")}
    for i in range(N):
        for k in range(min(int(count[i]), K)):
            w = W[i, pair[i, k]]
            out["normal"][i, k], out["p1"][i, k], out["p2"][i, k] = w[1:4], w[4:7], w[7:10]
    out.update(clearance=clearance, count=count, pair=pair, dist=dist)
    return out


# the GPU tests' batch: 3 env rows x 43 states -- more states than one workgroup has waves, no multiple of 64 or of the waves per block
N_ENVS, PER_ENV = 3, 43
STATE_SEED = 11           # chosen on the CPU with the sequential form: on all four scenes some states have no pair in band, some hold
                          # overlaps and some separated pairs in band (test_proximity_witness_gpu asserts it)


def mixed_states(pi, env, seed=STATE_SEED):
    """(qa [129, na], rows [3, nq]): half of the states uniform in the joint box, half near the env's initial pose, shuffled; the rows
    differ in where their free bodies stand"""
    from conftest import sample_states
    m = pi.model
    n = N_ENVS * PER_ENV
    rng = np.random.default_rng(seed)
    qa = np.concatenate([sample_states(pi, (n + 1) // 2, seed)[0], sample_states(pi, n // 2, seed + 1, "near")[0]])[rng.permutation(n)]
    rows = np.repeat(sample_states(pi, 1, 3)[1], N_ENVS, axis=0)
    for j in np.nonzero(np.asarray(m.jnt_type) == 0)[0]:
        a = int(m.jnt_qposadr[j])
        rows[:, a:a + 2] += rng.normal(0.0, 0.03, (N_ENVS, 2))
    if env == "PusherObstacle-v0":          # box and target rest 4 mm above each other amid the obstacles in the default row: moved out
        rows[:, 12:16] = rng.uniform(0.3, 0.5, (N_ENVS, 4))
    return np.ascontiguousarray(qa), rows
