"""Inputs and independent checks for the contact-frame tests (helpers of test_contact_frames_host / test_contact_frames_gpu).

A case is one posed pair; `cases()` builds the list both test files use: 16 random pairs per narrow-phase class by the recipe
of tests/test_oracle_primitives.py::_rand_pair, the plane classes, a mesh (Lift's can hull) and the degenerate configurations.
The invariants go through geom_ref.support only: nothing here shares code with oracle/ or the kernels."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from geom_ref import BOX, CAPSULE, CYLINDER, MESH, PLANE, SPHERE, _DIRS, rand_rot, rand_size, support

FAR = 1.0e10
I3 = np.eye(3)
NAMES = {PLANE: "plane", SPHERE: "sphere", CAPSULE: "capsule", CYLINDER: "cylinder", BOX: "box", MESH: "mesh"}
# the classes that go through mpr_penetration
MPR = {(CAPSULE, CYLINDER), (CYLINDER, CYLINDER), (CYLINDER, BOX), (SPHERE, MESH), (CAPSULE, MESH), (CYLINDER, MESH), (BOX, MESH)}
PRIMITIVE_CLASSES = [(PLANE, SPHERE), (PLANE, CAPSULE), (PLANE, CYLINDER), (PLANE, BOX), (SPHERE, SPHERE), (SPHERE, CAPSULE),
                     (SPHERE, CYLINDER), (SPHERE, BOX), (CAPSULE, CAPSULE), (CAPSULE, CYLINDER), (CAPSULE, BOX), (CYLINDER, CYLINDER),
                     (CYLINDER, BOX), (BOX, BOX)]
MESH_CLASSES = [(PLANE, MESH), (SPHERE, MESH), (CAPSULE, MESH), (CYLINDER, MESH), (BOX, MESH)]


@dataclass
class Case:
    t1: int
    s1: np.ndarray
    p1: np.ndarray
    m1: np.ndarray
    t2: int
    s2: np.ndarray
    p2: np.ndarray
    m2: np.ndarray
    what: str = "random"

    @property
    def cls(self):
        return f"{NAMES[self.t1]}-{NAMES[self.t2]}"

    @property
    def mpr(self):
        return (self.t1, self.t2) in MPR

    def moved(self, R, t):
        return Case(self.t1, self.s1, R @ self.p1 + t, R @ self.m1, self.t2, self.s2, R @ self.p2 + t, R @ self.m2, self.what)

    def swapped(self):
        return Case(self.t2, self.s2, self.p2, self.m2, self.t1, self.s1, self.p1, self.m1, self.what)


def _rand_pair(rng, t1, t2, dist_hi=0.5):
    """tests/test_oracle_primitives.py::_rand_pair"""
    s1, s2 = rand_size(rng, t1), rand_size(rng, t2)
    m1, m2 = rand_rot(rng), rand_rot(rng)
    p1 = rng.uniform(-0.1, 0.1, 3)
    dirn = rng.normal(size=3)
    dirn /= np.linalg.norm(dirn)
    return s1, p1, m1, s2, p1 + dirn * rng.uniform(0.0, dist_hi), m2


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=float)


def _c(t1, s1, p1, m1, t2, s2, p2, m2, what):
    f = lambda x: np.asarray(x, dtype=np.float64)
    return Case(t1, f(s1), f(p1), f(m1), t2, f(s2), f(p2), f(m2), what)


def random_cases(classes=PRIMITIVE_CLASSES + MESH_CLASSES, n=16):
    out = []
    for t1, t2 in classes:
        rng = np.random.default_rng(1000 * t1 + t2)
        for _ in range(n):
            # (the can is 25 mm x 80 mm: its partners start closer, so that about half of the pairs overlap)
            s1, p1, m1, s2, p2, m2 = _rand_pair(rng, t1, t2, dist_hi=0.25 if t2 == MESH else 0.5)
            out.append(_c(t1, s1, p1, m1, t2, s2, p2, m2, "random"))
    return out


def degenerate_cases():
    B = (BOX, [0.1, 0.2, 0.3], [0.0, 0.0, 0.0], I3)
    CY = (CYLINDER, [0.1, 0.3, 0.0], [0.0, 0.0, 0.0], I3)
    P = (PLANE, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], I3)
    S = lambda p, r=0.05: (SPHERE, [r, 0.0, 0.0], p, I3)
    return [
        _c(*S([0.1, 0.2, 0.3], 0.1), *S([0.1, 0.2, 0.3], 0.2), what="coincident sphere centres"),
        _c(CAPSULE, [0.05, 0.2, 0], [0, 0, 0], I3, CAPSULE, [0.03, 0.1, 0], [0.06, 0, 0.05], I3, what="parallel capsules, overlapping"),
        _c(CAPSULE, [0.05, 0.2, 0], [0, 0, 0], I3, CAPSULE, [0.03, 0.1, 0], [0.3, 0, 0.05], I3, what="parallel capsules, apart"),
        _c(*S([0.08, 0.0, 0.0]), *B, what="sphere centre inside a box"),
        _c(*S([0.0, 0.0, 0.0]), *B, what="sphere centre at the box centre"),
        _c(*S([0.05, 0.1, 0.25]), *B, what="sphere centre inside a box, z face"),
        _c(*S([0.05, 0.0, 0.0]), *CY, what="sphere centre inside a cylinder, barrel"),
        _c(*S([0.0, 0.0, 0.28]), *CY, what="sphere centre inside a cylinder, cap, on the axis"),
        _c(*S([0.0, 0.0, 0.0]), CYLINDER, [0.05, 0.3, 0.0], [0, 0, 0], I3, what="sphere centre on a long cylinder's axis"),
        _c(CAPSULE, [0.02, 0.15, 0], [0, 0, 0], I3, *B, what="capsule axis piercing a box, centred"),
        _c(CAPSULE, [0.02, 0.5, 0], [0.03, -0.05, 0.1], rot_x(0.4), *B, what="capsule axis piercing a box, tilted"),
        _c(CAPSULE, [0.02, 0.5, 0], [0.085, 0.19, 0.0], rot_x(0.7) @ np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0.0]]), *B,
           what="capsule axis piercing a box near an edge"),
        _c(*B, BOX, [0.1, 0.1, 0.1], [0.19, 0.0, 0.0], I3, what="two face-aligned boxes, overlapping"),
        _c(*B, BOX, [0.1, 0.1, 0.1], [0.25, 0.0, 0.0], I3, what="two face-aligned boxes, apart"),
        _c(*B, BOX, [0.1, 0.1, 0.1], [0.0, 0.0, 0.0], I3, what="two concentric face-aligned boxes"),
        _c(*P, CYLINDER, [0.1, 0.3, 0], [0.2, 0.1, 0.25], I3, what="cylinder axis normal to a plane"),
        _c(*P, CYLINDER, [0.1, 0.3, 0], [0.2, 0.1, 0.05], rot_x(math.pi / 2), what="cylinder axis parallel to a plane"),
        _c(*P, BOX, [0.1, 0.2, 0.3], [0.0, 0.0, 0.25], I3, what="box flat on a plane"),
        _c(*P, CAPSULE, [0.05, 0.2, 0], [0.0, 0.0, 0.03], rot_x(math.pi / 2), what="capsule lying on a plane"),
    ]


def cases():
    return random_cases() + degenerate_cases()


def recs_of(cs):
    """-> types [M, 2] int32, recs [M, 2, 15]: pos[3] mat[9] size[3] per geom (a mesh's size slots are not read)"""
    types = np.array([[c.t1, c.t2] for c in cs], dtype=np.int32)
    recs = np.zeros((len(cs), 2, 15))
    for i, c in enumerate(cs):
        recs[i, 0] = np.concatenate([c.p1, c.m1.ravel(), c.s1])
        recs[i, 1] = np.concatenate([c.p2, c.m2.ravel(), np.zeros(3) if c.t2 == MESH else c.s2])
    return types, recs


def host_frames(cs, can):
    from mopa_rl_amd import _lib
    types, recs = recs_of(cs)
    return _lib.geom_frames_host(types, recs, mesh_verts=can)


def oracle_dist(O, c, can):
    a, b = (c, False) if (c.t1 <= c.t2) else (c.swapped(), True)
    if a.t2 == MESH:
        return O.geom_dist_mesh(a.t1, a.s1, a.p1, a.m1, can, a.p2, a.m2)
    return O.geom_dist(a.t1, a.s1, a.p1, a.m1, a.t2, a.s2, a.p2, a.m2)


# ---------------- independent invariants (geom_ref.support) ----------------
def h(t, size, mat, n, can):
    """support about the centre along unit directions n [k, 3]; a plane: 0 along its own normal (its surface passes through its centre)"""
    n = np.atleast_2d(n)
    if t == PLANE:
        return np.zeros(len(n))
    return support(t, can if t == MESH else size, mat, n)


def overlap_along(c, n, can):
    """o(n) = h1(n) + h2(-n) - n.(c2 - c1): the overlap of the two shapes' extents along n"""
    return float(h(c.t1, c.s1, c.m1, n, can)[0] + h(c.t2, c.s2, c.m2, -n, can)[0] - n @ (c.p2 - c.p1))


def mid_plane(c, n, can):
    """the midpoint, along n, of the two supporting planes"""
    return 0.5 * float((n @ c.p1 + h(c.t1, c.s1, c.m1, n, can)[0]) + (n @ c.p2 - h(c.t2, c.s2, c.m2, -n, can)[0]))


def dist_to_shape(t, size, pos, mat, x, can):
    """signed distance of the point x from the shape (positive outside), over geom_ref's direction set"""
    if t == PLANE:
        return float(mat[:, 2] @ (x - pos))
    return float((_DIRS @ (x - pos) - h(t, size, mat, _DIRS, can)).max())
