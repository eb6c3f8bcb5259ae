"""Sequential form, inputs and restated broad phase of the proximity report (helpers of test_proximity_host / test_proximity_gpu).

Sequential form: the CPU oracle's FK poses of a state, per candidate pair `mopa_geom_sep_host` (the host compile of the kernels'
geom_sep) with NO broad phase in front, and the selection rule in numpy.  Pair cases: frames_ref's random and degenerate pairs,
their second shape moved along the centre line (a plane's partner along the plane's normal) so that every class has cases in
overlap, inside the band, just outside it and far from it."""
import numpy as np

import frames_ref as F
from contacts_ref import full_state, ignored_mask
from geom_ref import BOX, CAPSULE, CYLINDER, MESH, PLANE, SPHERE, _DIRS, signed_dist, support

FAR = F.FAR
BANDS = (0.0, 0.01, 0.05)
# classes whose pair function is the separation distance of disjoint shapes; every other class takes the inflated route
CLOSED = {(PLANE, SPHERE), (PLANE, CAPSULE), (PLANE, CYLINDER), (PLANE, BOX), (PLANE, MESH), (SPHERE, SPHERE), (SPHERE, CAPSULE),
          (SPHERE, CYLINDER), (SPHERE, BOX), (CAPSULE, CAPSULE), (CAPSULE, BOX)}
# sampled gaps a case is moved to (its distance lies up to a few millimetres above): two inside the 1 cm band, one just outside it, one
# more inside the 5 cm band, one just outside that one, one far
GAPS = (0.002, 0.005, 0.0102, 0.03, 0.0502, 0.3)
N_BASE = 4


def closed(c):
    return (min(c.t1, c.t2), max(c.t1, c.t2)) in CLOSED


def host_sep(cs, can, band):
    from mopa_rl_amd import _lib
    types, recs = F.recs_of(cs)
    return _lib.geom_sep_host(types, recs, band, mesh_verts=can)


def _line(c):
    """unit direction the second shape is moved along"""
    if c.t1 == PLANE:
        return c.m1[:, 2]
    d = c.p2 - c.p1
    n = np.linalg.norm(d)
    return d / n if n > 0 else np.array([1.0, 0.0, 0.0])


def _at(c, u, s):
    return F.Case(c.t1, c.s1, c.p1, c.m1, c.t2, c.s2, c.p1 + s * u, c.m2, c.what)


def _support_gap(c, n, can):
    """n . (c2 - c1) - h1(n) - h2(-n) for unit directions n [k, 3]: each value is a lower bound of the signed distance"""
    return n @ (c.p2 - c.p1) - F.h(c.t1, c.s1, c.m1, n, can) - F.h(c.t2, c.s2, c.m2, -n, can)


def place(base, can, gaps=GAPS):
    """the base cases with their second shape moved along the centre line to where the SAMPLED signed distance (the largest support
    gap over geom_ref's direction set, a lower bound that is short of the distance by up to a few millimetres for polytopes, exact for a plane)
    equals each gap: the support gap of a direction is linear in the offset, so the sampled distance is a maximum of lines.  Only
    WHERE a case lands comes from here; what its distance is comes from `ref_dist`."""
    out = []
    for c in base:
        u = _line(c)
        n = c.m1[:, 2][None] if c.t1 == PLANE else _DIRS
        slope, at0 = n @ u, _support_gap(_at(c, u, 0.0), n, can)
        for g in gaps:
            lo, hi = 0.0, 4.0
            for _ in range(50):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if (mid * slope + at0).max() < g else (lo, mid)
            out.append(_at(c, u, hi))
    return out


def ref_dist(c, can):
    """the independent signed distance (geom_ref.signed_dist, accurate to about 1e-7); far cases stop at the sampled lower bound"""
    if c.t1 != PLANE:
        lb = float(_support_gap(c, _DIRS, can).max())
        if lb > 0.1:
            return lb
    return signed_dist(c.t1, c.s1, c.p1, c.m1, c.t2, can if c.t2 == MESH else c.s2, c.p2, c.m2)


_CACHE = {}


def sep_case_list(can):
    """per class 8 random pairs as frames_ref poses them (about half in overlap) and the degenerate pairs, then N_BASE of the random
    pairs at every gap of GAPS (the last N_BASE * len(GAPS) * 19 cases); built once per process"""
    if "cases" not in _CACHE:
        base = [c for k, c in enumerate(F.random_cases()) if k % 16 < N_BASE]
        moved = place(base, can)
        _CACHE["cases"] = (F.random_cases(n=8) + F.degenerate_cases() + moved, len(moved))
    return _CACHE["cases"][0]


def sep_cases(can):
    """-> (cases, ref [M]): `sep_case_list` and the independent signed distance of the moved cases, NaN for the others (about two
    minutes of direction searches, once per process)"""
    cs = sep_case_list(can)
    if "ref" not in _CACHE:
        n = _CACHE["cases"][1]
        ref = np.full(len(cs), np.nan)
        ref[len(cs) - n:] = [ref_dist(c, can) for c in cs[len(cs) - n:]]
        _CACHE["ref"] = ref
    return cs, _CACHE["ref"]


# ---------------- scene level ----------------
def can_of(m):
    if getattr(m, "mesh_vert", None) is None or len(m.mesh_vert) == 0:
        return None
    return m.mesh_vert[m.mesh_vertadr[0]:m.mesh_vertadr[0] + m.mesh_vertnum[0]].copy()


def poses(pi, orc, qa, rows, spe):
    """the oracle's FK of every state: (gpos [N, ng, 3], gmat [N, ng, 9])"""
    out = [orc.fk(full_state(pi, qa[i], rows[i // spe])) for i in range(len(qa))]
    return np.array([p[0] for p in out]), np.array([np.asarray(p[1]).reshape(-1, 9) for p in out])


def pair_dists(pi, gpos, gmat, band):
    """[N, npair] band-limited distances of the sequential form on the poses given -- mopa_geom_sep_host on every candidate pair,
    no broad phase in front -- ignored pairs at FAR; one host call for the whole batch"""
    from mopa_rl_amd import _lib
    m = pi.model
    pg = np.asarray(m.pair_geom).reshape(-1, 2)
    N, npair = len(gpos), len(pg)
    size = np.asarray(m.geom_size, dtype=np.float64)
    gt = np.asarray(m.geom_type)
    size = np.where((gt == MESH)[:, None], 0.0, size)                     # (a mesh's size slots are not read)
    rec = np.concatenate([gpos, gmat, np.broadcast_to(size, (N,) + size.shape)], axis=2)       # [N, ng, 15]
    recs = rec[:, pg]                                                      # [N, npair, 2, 15]
    types = np.broadcast_to(gt[pg].astype(np.int32), (N, npair, 2))
    D = _lib.geom_sep_host(types.reshape(-1, 2), recs.reshape(-1, 30), band, mesh_verts=can_of(m)).reshape(N, npair)
    D[:, ignored_mask(pi)] = FAR
    return D


def select(D, band, K):
    """the contract of mopa_proximity_batch on a table of band-limited distances: clearance [N], count [N] int32, pair [N, K] int32, dist [N, K]"""
    N = len(D)
    clearance = np.full(N, float(band))
    count = np.zeros(N, dtype=np.int32)
    pair = np.full((N, K), -1, dtype=np.int32)
    dist = np.full((N, K), FAR)
    for i in range(N):
        hit = np.nonzero(D[i] <= band)[0]
        count[i] = len(hit)
        order = hit[np.lexsort((hit, D[i, hit]))][:K]          # ascending by (distance, pair index)
        pair[i, :len(order)] = order
        dist[i, :len(order)] = D[i, order]
        if len(hit):
            clearance[i] = min(float(band), D[i, hit].min())
    return clearance, count, pair, dist


# ---------------- the margin broad phase, restated from the scene's bounds ----------------
def rbound(m):
    """bounding radius of every collidable geom about its origin"""
    out = np.zeros(len(m.geom_type))
    for g, (t, s) in enumerate(zip(m.geom_type, m.geom_size)):
        if t == SPHERE:
            out[g] = s[0]
        elif t == CAPSULE:
            out[g] = s[0] + s[1]
        elif t == CYLINDER:
            out[g] = np.hypot(s[0], s[1])
        elif t == BOX:
            out[g] = np.linalg.norm(s)
        elif t == MESH:
            out[g] = np.linalg.norm(can_of(m), axis=1).max()
    return out


def aabb_half(t, size, mat, rb):
    """world-AABB half extents of a posed primitive (+ 1e-9), a mesh by its bounding sphere"""
    a = np.abs(mat)
    if t == BOX:
        h = a @ size
    elif t == SPHERE:
        h = np.full(3, size[0])
    elif t == CAPSULE:
        h = a[:, 2] * size[1] + size[0]
    elif t == CYLINDER:
        h = a[:, 2] * size[1] + size[0] * np.sqrt(np.maximum(0.0, 1.0 - a[:, 2] ** 2))
    else:
        h = np.full(3, rb)
    return h + 1e-9


def culled_band(m, rb, static, gpos, gmat, band):
    """bool [npair]: pair_culled_band of every candidate pair -- bounding spheres at rba + rbb + band, a plane at rbb + band, a static
    geom's world AABB against the moving geom's sphere at H + rM + band.  `static` [ngeom]: the geom's pose does not depend on the state."""
    out = np.zeros(len(m.pair_geom), dtype=bool)
    for p, (a, b) in enumerate(np.asarray(m.pair_geom).reshape(-1, 2)):
        diff = gpos[b] - gpos[a]
        if m.geom_type[a] == PLANE:
            out[p] = diff @ np.asarray(gmat[a]).reshape(3, 3)[:, 2] > rb[b] + band
            continue
        rs = rb[a] + rb[b] + band
        if diff @ diff > rs * rs:
            out[p] = True
        elif static[a] != static[b]:
            s, mv = (a, b) if static[a] else (b, a)
            H = aabb_half(int(m.geom_type[s]), np.asarray(m.geom_size[s], dtype=float), np.asarray(gmat[s]).reshape(3, 3), rb[s])
            out[p] = bool((np.abs(gpos[mv] - gpos[s]) > H + (rb[mv] + band)).any())
    return out
