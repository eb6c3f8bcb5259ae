"""Separated pairs whose distance is a formula (helpers of test_gjk_truth_host / test_gjk_truth_gpu): the configurations GJK finds
hardest -- parallel faces and edges, curved on curved, thin plates and needles, many coplanar hull vertices -- each with its true
distance as a float64 expression of the inputs.

Every family is built in a base frame with exact alignment (I3 or exact 90-degree permutation matrices; a 45-degree turn has both of
its entries equal to sqrt(0.5), bit for bit) and comes with a direction n and two numbers: shape A lies in n.x <= alpha, shape B in
n.x >= beta, and one point of each support set lies on a common line along n (asserted where it constrains the placement), so the
distance is beta - alpha.  Rim to rim, vertex to vertex and the barrel against an edge are the distance of two points or of a point and a
line, by the same argument along the line that joins them.  The truth of the sphere-mesh and capsule-mesh families is the distance of a
point from the hull, by enumeration of the faces, edges and vertices of scipy's ConvexHull, minimised along the capsule's axis by a
golden-section search (the function is convex there).  No search over directions, no library distance code: nothing here shares code
with geom_ref.signed_dist, oracle/ or mopa_gjk.hpp; geom_ref.support is the closed-form support function h_B of the "large face" family.

Each base case is emitted as built, under two random rigid motions (geom_ref.rand_rot, a translation of up to 1 m) -- parallelism that
is exact and parallelism that is off by rounding are different inputs to the simplex code -- and with the two shapes swapped where the
class allows it (a mesh is the second shape).  The sweep: GAPS x SCALES (every size but not the gap; the mesh stays at scale 1) x
VARIANTS of the boxes and cylinders (plain, a plate with one half-extent 1/100 of the others, a needle with two)."""
import functools
import math
from collections import namedtuple

import numpy as np
from scipy.spatial import ConvexHull

import frames_ref as F
from geom_ref import BOX, CAPSULE, CYLINDER, MESH, SPHERE, rand_rot, support

# the smallest gap is ten times kGjkTol; the pairs around 0.01 and 0.05 straddle the two bands of proximity_exact_ref.BANDS
GAPS = (1e-5, 1e-3, 0.0099, 0.0101, 0.03, 0.0499, 0.0501, 0.3)
SCALES = (0.05, 1.0, 4.0)
VARIANTS = ("plain", "plate", "needle")
ORIENTS = ("end-on", "lying", "tilted")         # the capsule-mesh families' variants

R2 = math.sqrt(0.5)
I3 = np.eye(3)
RZ45 = np.array([[R2, -R2, 0.0], [R2, R2, 0.0], [0.0, 0.0, 1.0]])
RY45 = np.array([[R2, 0.0, R2], [0.0, 1.0, 0.0], [-R2, 0.0, R2]])
Z_TO_X = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])        # the local z axis (a cylinder's, a capsule's) along world x
Z_TO_Y = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])        # ... along world y
O3 = np.zeros(3)

Item = namedtuple("Item", "case true family scale gap variant form")


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def box_half(s, variant, base, thin=0, long=2):
    """half extents: `base` x s; a plate: the largest of them, 1/100 of it along `thin`; a needle: 1/100 of it but along `long`"""
    m = max(base) * s
    if variant == "plate":
        h = [m, m, m]
        h[thin] = m / 100.0
    elif variant == "needle":
        h = [m / 100.0] * 3
        h[long] = m
    else:
        h = [b * s for b in base]
    return np.array(h)


def cyl_size(s, variant, base):
    """(radius, half height): a plate is a disc, a needle a rod"""
    m = max(base) * s
    r, h = {"plate": (m, m / 100.0), "needle": (m / 100.0, m)}.get(variant, (base[0] * s, base[1] * s))
    return np.array([r, h, 0.0])


def _case(t1, s1, p1, m1, t2, s2, p2, m2, what):
    f = lambda x: np.array(x, dtype=np.float64)
    return F.Case(t1, f(s1), f(p1), f(m1), t2, O3.copy() if t2 == MESH else f(s2), f(p2), f(m2), what)


BOX_A, BOX_B = (0.10, 0.07, 0.05), (0.06, 0.08, 0.04)
CYL_A, CYL_B = (0.05, 0.08), (0.04, 0.06)
CAP = (0.03, 0.06)


# ---------------- box - box ----------------
def bb_face(g, s, v, can):
    a, b = box_half(s, v, BOX_A, 0, 1), box_half(s, v, BOX_B, 0, 1)
    p = np.array([a[0] + g + b[0], 0.5 * (a[1] + b[1]), -0.3 * (a[2] + b[2])])
    assert abs(p[1]) < a[1] + b[1] and abs(p[2]) < a[2] + b[2]                  # the faces overlap, partly
    return _case(BOX, a, O3, I3, BOX, b, p, I3, "box-box face to face"), p[0] - a[0] - b[0]


def bb_edges(g, s, v, can):
    a, b = box_half(s, v, BOX_A, 0, 2), box_half(s, v, BOX_B, 0, 2)
    p = np.array([a[0] + 0.6 * g + b[0], a[1] + 0.8 * g + b[1], 0.4 * (a[2] + b[2])])
    assert abs(p[2]) < a[2] + b[2]
    return _case(BOX, a, O3, I3, BOX, b, p, I3, "box-box parallel edges"), math.hypot(p[0] - a[0] - b[0], p[1] - a[1] - b[1])


def bb_vertex(g, s, v, can):
    a, b = box_half(s, v, BOX_A, 0, 2), box_half(s, v, BOX_B, 1, 0)
    p = a + b + g * np.array([2.0, 3.0, 6.0]) / 7.0
    q = p - a - b
    return _case(BOX, a, O3, I3, BOX, b, p, I3, "box-box vertex to vertex"), math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])


def bb_edge_face(g, s, v, can):
    a, b = box_half(s, v, BOX_A, 0, 2), box_half(s, v, BOX_B, 0, 2)
    hx = R2 * b[0] + R2 * b[1]                      # h_B(-x) of B turned 45 degrees about z: its edge (-bx, +by, .), along z
    ey = 0.3 * a[1]
    p = np.array([a[0] + g + hx, ey - (R2 * b[1] - R2 * b[0]), 0.4 * (a[2] + b[2])])
    assert abs(p[1] + R2 * b[1] - R2 * b[0]) < a[1] and abs(p[2]) < a[2] + b[2]
    return _case(BOX, a, O3, I3, BOX, b, p, RZ45, "box-box edge to face"), p[0] - a[0] - hx


def bb_crossed(g, s, v, can):
    a, b = box_half(s, v, BOX_A, 0, 2), box_half(s, v, BOX_B, 0, 1)
    ha, hb = R2 * a[0] + R2 * a[1], R2 * b[0] + R2 * b[2]
    ya = R2 * a[0] - R2 * a[1]                      # A's edge (ax, -ay, .): the line x = ha, y = ya, |z| <= az
    p = np.array([ha + g + hb, ya + 0.3 * b[1], 0.3 * a[2] - (R2 * b[0] - R2 * b[2])])
    zb = p[2] + (R2 * b[0] - R2 * b[2])             # B's edge (-bx, ., -bz): the line x = px - hb, z = zb, |y - py| <= by
    assert abs(ya - p[1]) < b[1] and abs(zb) < a[2]                             # the edges cross in projection
    return _case(BOX, a, O3, RZ45, BOX, b, p, RY45, "box-box crossed edges"), p[0] - ha - hb


# ---------------- the large face / large cap family ----------------
def _large(name, a_type, b_type, b_rot):
    """A: a box whose +x face, or a cylinder (axis along x) whose cap, is large; B: any shape, b_rot(rng) its orientation.
    d = px - a_x - h_B(-x)"""
    def make(g, s, v, can):
        rng = np.random.default_rng([sum(map(ord, name)), int(round(g * 1e6)), int(round(s * 100)), VARIANTS.index(v)])
        if b_type == BOX:
            sb = box_half(s, v, BOX_B, 0, 2)
            rb = float(np.linalg.norm(sb))
        elif b_type == CYLINDER:
            sb = cyl_size(s, v, CYL_B)
            rb = math.hypot(sb[0], sb[1])
        else:
            sb = can
            rb = float(np.linalg.norm(can, axis=1).max())
        mb = b_rot(rng, can)
        W = max(0.2 * s, 2.5 * rb)
        ax = W / 100.0 if v == "plate" else 0.05 * s
        hb = float(support(b_type, sb, mb, np.array([[-1.0, 0.0, 0.0]]))[0])
        p = np.array([ax + g + hb, 0.3 * rb, -0.2 * rb])
        # B's bounding sphere, and with it its support set, projects inside the face / the disc
        assert math.hypot(p[1], p[2]) + rb <= W
        A = (BOX, [ax, W, W], O3, I3) if a_type == BOX else (CYLINDER, [W, ax, 0.0], O3, Z_TO_X)
        return _case(*A, b_type, sb, p, mb, name), p[0] - ax - hb
    return make


def _end_normal(can):
    """the outward normal of the can's flat end: the hull plane with the most vertices on it"""
    hull = _hull(can)
    best, best_n = None, 0
    for eq in hull.equations:
        n = int((np.abs(can @ eq[:3] + eq[3]) < 1e-9).sum())
        if n > best_n:
            best, best_n = eq[:3].copy(), n
    assert best_n >= 8, best_n
    return best / np.linalg.norm(best), best_n


def _rot_taking(a, b):
    """a rotation matrix R with R a = b (unit vectors), by Rodrigues' formula; a permutation-like matrix where a = +-b"""
    v, c = np.cross(a, b), float(a @ b)
    if c > 1.0 - 1e-15:
        return I3.copy()
    if c < -1.0 + 1e-15:                            # half a turn about an axis normal to a
        u = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        return 2.0 * np.outer(u, u) - I3
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return I3 + K + K @ K / (1.0 + c)


_rand = lambda rng, can: rand_rot(rng)
_end_down = lambda rng, can: _rot_taking(_end_normal(can)[0], np.array([-1.0, 0.0, 0.0]))        # the flat end faces A

LARGE = {
    "large face: box vertex": _large("large face: box vertex", BOX, BOX, _rand),
    "large face: cylinder cap flat": _large("large face: cylinder cap flat", BOX, CYLINDER, lambda rng, can: Z_TO_X),
    "large face: cylinder rim tilted": _large("large face: cylinder rim tilted", BOX, CYLINDER, lambda rng, can: rot_y(0.3) @ Z_TO_X),
    "large face: cylinder barrel on its side": _large("large face: cylinder barrel on its side", BOX, CYLINDER, lambda rng, can: Z_TO_Y),
    "large face: mesh": _large("large face: mesh", BOX, MESH, _rand),
    "large face: mesh flat end": _large("large face: mesh flat end", BOX, MESH, _end_down),
    "large cap: box vertex": _large("large cap: box vertex", CYLINDER, BOX, _rand),
    "large cap: cylinder rim tilted": _large("large cap: cylinder rim tilted", CYLINDER, CYLINDER, lambda rng, can: rot_y(0.3) @ Z_TO_X),
    "large cap: mesh": _large("large cap: mesh", CYLINDER, MESH, _rand),
    "large cap: mesh flat end": _large("large cap: mesh flat end", CYLINDER, MESH, _end_down),
}


# ---------------- cylinder - cylinder (A at the origin, its axis along z) ----------------
def cc_coaxial(g, s, v, can):
    a, b = cyl_size(s, v, CYL_A), cyl_size(s, v, CYL_B)
    p = np.array([0.0, 0.0, a[1] + g + b[1]])
    return _case(CYLINDER, a, O3, I3, CYLINDER, b, p, I3, "cylinders coaxial, stacked"), p[2] - a[1] - b[1]


def cc_caps(g, s, v, can):
    a, b = cyl_size(s, v, CYL_A), cyl_size(s, v, CYL_B)
    p = np.array([0.6 * (a[0] + b[0]), 0.0, a[1] + g + b[1]])
    assert p[0] < a[0] + b[0]
    return _case(CYLINDER, a, O3, I3, CYLINDER, b, p, I3, "cylinders parallel, caps facing"), p[2] - a[1] - b[1]


def cc_rims(g, s, v, can):
    a, b = cyl_size(s, v, CYL_A), cyl_size(s, v, CYL_B)
    p = np.array([a[0] + b[0] + 0.6 * g, 0.0, a[1] + b[1] + 0.8 * g])
    assert p[0] > a[0] + b[0]
    return _case(CYLINDER, a, O3, I3, CYLINDER, b, p, I3, "cylinders parallel, rim to rim"), math.hypot(p[0] - a[0] - b[0], p[2] - a[1] - b[1])


def cc_side(g, s, v, can):
    a, b = cyl_size(s, v, CYL_A), cyl_size(s, v, CYL_B)
    p = np.array([a[0] + b[0] + g, 0.0, 0.5 * (a[1] + b[1])])
    assert abs(p[2]) < a[1] + b[1]
    return _case(CYLINDER, a, O3, I3, CYLINDER, b, p, I3, "cylinders parallel, side by side"), p[0] - a[0] - b[0]


def cc_crossed(g, s, v, can):
    a, b = cyl_size(s, v, CYL_A), cyl_size(s, v, CYL_B)
    p = np.array([a[0] + b[0] + g, 0.3 * b[1], 0.3 * a[1]])
    assert abs(p[1]) < b[1] and abs(p[2]) < a[1]                                # the two nearest rulings cross in projection
    return _case(CYLINDER, a, O3, I3, CYLINDER, b, p, Z_TO_Y, "cylinders perpendicular, crossed barrels"), p[0] - a[0] - b[0]


def cc_across_cap(g, s, v, can):
    a, b = cyl_size(s, v, CYL_A), cyl_size(s, v, CYL_B)
    p = np.array([0.2 * a[0], 0.3 * a[0], a[1] + g + b[0]])
    assert math.hypot(p[0], p[1]) < a[0]                                        # B's lowest ruling passes over the disc
    return _case(CYLINDER, a, O3, I3, CYLINDER, b, p, Z_TO_X, "cylinder barrel lying across a cap"), p[2] - a[1] - b[0]


# ---------------- capsule - cylinder (the cylinder at the origin, its axis along z) ----------------
def kc_side(g, s, v, can):
    c, k = cyl_size(s, v, CYL_A), np.array([CAP[0] * s, CAP[1] * s, 0.0])
    p = np.array([c[0] + k[0] + g, 0.0, 0.5 * c[1]])
    assert abs(p[2]) - k[1] < c[1]
    return _case(CAPSULE, k, p, I3, CYLINDER, c, O3, I3, "capsule-cylinder parallel, side by side"), p[0] - c[0] - k[0]


def kc_end_on(g, s, v, can):
    c, k = cyl_size(s, v, CYL_A), np.array([CAP[0] * s, CAP[1] * s, 0.0])
    p = np.array([0.3 * c[0], 0.2 * c[0], c[1] + g + k[0] + k[1]])
    assert math.hypot(p[0], p[1]) < c[0]
    return _case(CAPSULE, k, p, I3, CYLINDER, c, O3, I3, "capsule end-on over the cap"), p[2] - c[1] - k[1] - k[0]


def kc_across(g, s, v, can):
    c, k = cyl_size(s, v, CYL_A), np.array([CAP[0] * s, CAP[1] * s, 0.0])
    p = np.array([0.2 * c[0], 0.3 * c[0], c[1] + g + k[0]])
    assert math.hypot(p[0], p[1]) < c[0]
    return _case(CAPSULE, k, p, Z_TO_X, CYLINDER, c, O3, I3, "capsule lying across the cap"), p[2] - c[1] - k[0]


def kc_radial(g, s, v, can):
    c, k = cyl_size(s, v, CYL_A), np.array([CAP[0] * s, CAP[1] * s, 0.0])
    p = np.array([c[0] + g + k[0] + k[1], 0.0, 0.4 * c[1]])
    assert abs(p[2]) < c[1]
    return _case(CAPSULE, k, p, Z_TO_X, CYLINDER, c, O3, I3, "capsule pointing radially at the barrel"), p[0] - k[1] - k[0] - c[0]


# ---------------- cylinder - box ----------------
def cb_edge(g, s, v, can):
    """the box turned 45 degrees about the cylinder's axis: its edge (-bx, +by, .) faces the barrel, the direction to the axis in the
    middle of the edge's normal cone"""
    c, b = cyl_size(s, v, CYL_A), box_half(s, v, BOX_B, 0, 2)
    hx = R2 * b[0] + R2 * b[1]
    p = np.array([c[0] + g + hx, -(R2 * b[1] - R2 * b[0]), 0.4 * (c[1] + b[2])])
    ex, ey = p[0] - hx, p[1] + (R2 * b[1] - R2 * b[0])
    assert abs(p[2]) < c[1] + b[2] and abs(ey) < 1e-3 * ex
    return _case(CYLINDER, c, O3, I3, BOX, b, p, RZ45, "cylinder barrel against a box edge"), math.hypot(ex, ey) - c[0]


# ---------------- sphere - mesh, capsule - mesh ----------------
@functools.lru_cache(maxsize=None)
def _hull_of(key):
    return ConvexHull(np.frombuffer(key, dtype=np.float64).reshape(-1, 3))


def _hull(can):
    return _hull_of(np.ascontiguousarray(can, dtype=np.float64).tobytes())


def point_hull_dist(x, can):
    """the distance of a point outside the hull from it: the smallest over the hull's triangles of the distance to the face's interior
    (where the foot on its plane lies inside), to its three edges and, by clamping, to its vertices"""
    a, n, nn, side, eu, e, ee = _tables_of(np.ascontiguousarray(can, dtype=np.float64).tobytes())
    best = np.inf
    xa = x - a
    t = np.einsum("ij,ij->i", xa, n) / nn
    q = xa - t[:, None] * n                             # the foot on the face's plane, from the face's first vertex
    # inside: on the inner side of the three edge planes (side[k] = n x edge k, through the edge's first vertex u_k = a + off_k)
    inside = np.ones(len(a), dtype=bool)
    for m, off in side:
        inside &= np.einsum("ij,ij->i", q - off, m) >= 0.0
    if inside.any():
        best = float((np.abs(t) * np.sqrt(nn))[inside].min())
    xu = x - eu
    lam = np.clip(np.einsum("ij,ij->i", xu, e) / ee, 0.0, 1.0)
    r = xu - lam[:, None] * e
    return min(best, math.sqrt(float(np.einsum("ij,ij->i", r, r).min())))


@functools.lru_cache(maxsize=None)
def _tables_of(key):
    """what point_hull_dist reads of the hull: per triangle of positive area its first vertex, normal, squared normal and the three
    edge planes; the edges (every one of every triangle) as first vertex, vector, squared length"""
    can = np.frombuffer(key, dtype=np.float64).reshape(-1, 3)
    tri = _hull_of(key).simplices
    a, b, c = can[tri[:, 0]], can[tri[:, 1]], can[tri[:, 2]]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    ok = nn > 0.0
    a, b, c, n, nn = a[ok], b[ok], c[ok], n[ok], nn[ok]
    side = [(np.cross(n, w - u), u - a) for u, w in ((a, b), (b, c), (c, a))]
    eu, e = np.concatenate([a, b, c]), np.concatenate([b - a, c - b, a - c])
    ee = (e * e).sum(axis=1)
    return a, n, nn, side, eu[ee > 0.0], e[ee > 0.0], ee[ee > 0.0]


def segment_hull_dist(c, axis, half, can):
    """min over |t| <= half of point_hull_dist(c + t axis): golden-section search on the convex function, to 1e-13 of the segment"""
    f = lambda t: point_hull_dist(c + t * axis, can)
    lo, hi = -half, half
    k = (math.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = hi - k * (hi - lo), lo + k * (hi - lo)
    f1, f2 = f(x1), f(x2)
    while hi - lo > 1e-13 * max(half, 1e-3):
        if f1 <= f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - k * (hi - lo)
            f1 = f(x1)
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + k * (hi - lo)
            f2 = f(x2)
    return min(f1, f2, f(lo), f(hi), f(-half), f(half))


@functools.lru_cache(maxsize=None)
def _aims_of(key):
    """name -> (point on the hull, outward unit direction inside the normal cone there): a side face's interior, an edge between two
    faces at an angle, a vertex, the flat end off its centre"""
    can = np.frombuffer(key, dtype=np.float64).reshape(-1, 3)
    hull = _hull(can)
    nrm = hull.equations[:, :3]
    end, _ = _end_normal(can)
    tri = hull.simplices
    area = 0.5 * np.linalg.norm(np.cross(can[tri[:, 1]] - can[tri[:, 0]], can[tri[:, 2]] - can[tri[:, 0]]), axis=1)
    side = np.abs(nrm @ end) < 0.5
    f = int(np.argmax(np.where(side, area, 0.0)))
    aims = {"face": (can[tri[f]].mean(axis=0), nrm[f])}
    # an edge of that face whose other face is at more than 10 degrees; a vertex of it
    for g in hull.neighbors[f]:
        if nrm[f] @ nrm[g] < math.cos(math.radians(10.0)):
            shared = sorted(set(tri[f]) & set(tri[g]))
            d = nrm[f] + nrm[g]
            aims["edge"] = (can[shared].mean(axis=0), d / np.linalg.norm(d))
            break
    vtx = int(tri[f][0])
    d = np.unique(np.round(nrm[(tri == vtx).any(axis=1)], 9), axis=0).sum(axis=0)
    aims["vertex"] = (can[vtx], d / np.linalg.norm(d))
    on_end = np.abs(can @ end - (can @ end).max()) < 1e-9
    centre = can[on_end].mean(axis=0)
    aims["flat end"] = (centre + 0.3 * (can[on_end][0] - centre), end)
    assert set(aims) == {"face", "edge", "vertex", "flat end"}
    return aims


def _aims(can):
    return _aims_of(np.ascontiguousarray(can, dtype=np.float64).tobytes())


def _tangent(d):
    u = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    return u / np.linalg.norm(u)


def _sphere_mesh(aim):
    name = f"sphere-mesh {aim}"

    def make(g, s, v, can):
        at, d = _aims(can)[aim]
        r = 0.04 * s
        x = at + (g + r) * d
        return _case(SPHERE, [r, 0.0, 0.0], x, I3, MESH, None, O3, I3, name), point_hull_dist(x, can) - r
    return make


def _capsule_mesh(aim):
    name = f"capsule-mesh {aim}"

    def make(g, s, orient, can):
        at, d = _aims(can)[aim]
        r, half = CAP[0] * s, CAP[1] * s
        u = _tangent(d)
        axis = {"end-on": d, "lying": u, "tilted": math.cos(0.5) * d + math.sin(0.5) * u}[orient]
        m = _rot_taking(np.array([0.0, 0.0, 1.0]), axis)
        axis = m[:, 2]                                 # the axis the pose actually has
        # lying: the segment's middle over the aim; otherwise its lower end, the segment leading away from the hull
        x = at + (g + r) * d + (0.0 if orient == "lying" else half) * axis
        return _case(CAPSULE, [r, half, 0.0], x, m, MESH, None, O3, I3, name), segment_hull_dist(x, axis, half, can) - r
    return make


PRIMITIVE = {f.__name__: f for f in (bb_face, bb_edges, bb_vertex, bb_edge_face, bb_crossed, cc_coaxial, cc_caps, cc_rims, cc_side, cc_crossed,
                                     cc_across_cap, kc_side, kc_end_on, kc_across, kc_radial, cb_edge)}
AIMS = ("face", "edge", "vertex", "flat end")


def base_cases(can):
    """[(case, true, scale, gap, variant)]: every family at every gap, scale and variant, as built"""
    can = np.ascontiguousarray(can, dtype=np.float64)
    out = []
    for g in GAPS:
        for s in SCALES:
            for make in list(PRIMITIVE.values()) + list(LARGE.values()):
                for v in VARIANTS:
                    out.append(make(g, s, v, can) + (s, g, v))
            for aim in AIMS:
                out.append(_sphere_mesh(aim)(g, s, "plain", can) + (s, g, "plain"))
                for o in ORIENTS:
                    out.append(_capsule_mesh(aim)(g, s, o, can) + (s, g, o))
    return out


_CACHE = {}


def items(can):
    """the whole list of Item(case, true, family, scale, gap, variant, form), form in built / moved1 / moved2 / swapped; built once per
    process, read-only.  A rigid motion and a swap leave the distance as it is: `true` is the base frame's"""
    if "items" not in _CACHE:
        rng = np.random.default_rng(2024)
        out = []
        for c, true, s, g, v in base_cases(can):
            assert true > 0.0 and abs(true - g) <= 0.35 * g + 1e-12, (c.what, s, g, v, true)       # every family lands near its gap
            forms = [("built", c)] + [(f"moved{k}", c.moved(rand_rot(rng), rng.uniform(-1.0, 1.0, 3))) for k in (1, 2)]
            if c.t2 != MESH:
                forms.append(("swapped", c.swapped()))
            out += [Item(cc, float(true), c.what, s, g, v, form) for form, cc in forms]
        _CACHE["items"] = out
    return _CACHE["items"]


def families(its):
    return sorted({it.family for it in its})
