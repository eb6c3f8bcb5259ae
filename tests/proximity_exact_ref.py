"""Helpers of test_proximity_exact_host / test_proximity_exact_gpu: the sequential forms of proximity_ref and motion_clearance_ref
with the exact route's host pair function (mopa_geom_sep_exact_host) in place of mopa_geom_sep_host.  Those helpers look
`_lib.geom_sep_host` up at every call, so the exact function is swapped in around the call; nothing of theirs is cached inside."""
import contextlib
import functools

import numpy as np

import frames_ref as F
import proximity_ref as P

K_GJK_TOL = 1e-6          # kGjkTol (mopa_gjk.hpp)
BANDS = (0.01, 0.05)


@contextlib.contextmanager
def exact_host():
    from mopa_rl_amd import _lib
    orig = _lib.geom_sep_host
    _lib.geom_sep_host = functools.partial(orig, exact=True)
    try:
        yield
    finally:
        _lib.geom_sep_host = orig


def host_sep(cs, can, band, iters=False):
    """mopa_geom_sep_exact_host on a case list: [M] distances, with iters=True also the [M] support-evaluation counts"""
    from mopa_rl_amd import _lib
    types, recs = F.recs_of(cs)
    return _lib.geom_sep_host(types, recs, band, mesh_verts=can, exact=True, return_iters=iters)


def pair_dists(pi, gpos, gmat, band):
    with exact_host():
        return P.pair_dists(pi, gpos, gmat, band)


def inflated_pairs(m):
    """bool [npair]: the candidate pair belongs to a class that takes the inflated / exact route when its shapes are disjoint"""
    gt = np.asarray(m.geom_type)
    pg = np.asarray(m.pair_geom).reshape(-1, 2)
    return np.array([(min(gt[a], gt[b]), max(gt[a], gt[b])) not in P.CLOSED for a, b in pg])
