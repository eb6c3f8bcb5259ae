"""The scene-level kernels off the four shipped scenes: on random body trees and on one directed scene per decision of the scene
compiler (random_scenes.py) the FK, the per-pair distances, the verdicts of all three K1 generations, K2, the four reports and
RRT-Connect are bit-identical to the CPU oracle or to the existing sequential forms, as on the shipped scenes: every comparison is on
bits, no tolerance is involved.  The proximity and clearance reports also run with exact=True (the GJK route) against the sequential
forms under the exact host pair table, on random_scenes.EXACT_KEYS.  229 states = three full tiles and a tail of 37, 50 per env row: five rows with different passive
values and free-body poses, tiles that span two rows.  No test here provokes a fault."""
import functools

import numpy as np
import pytest

import motion_clearance_ref as MC
import motion_report_ref as MR
import proximity_exact_ref as X
import proximity_ref as P
import random_scenes as RS
from contacts_ref import FAR, ignored_mask, oracle_pair_dists, report_from_dists
from test_gpu_parity import KERNELS, _scene_with_kernel

pytestmark = pytest.mark.gpu

KEYS = list(RS.DIRECTED) + list(RS.GPU_SEEDS)
REPORT_KEYS = [0, 3, 7, 15, "tile_posed", "mesh", "deep_branches", "wide"]
PLAN_KEYS = ["long_chain", "wide", "deep_branches", "tile_posed", 3, 7]
N, SPE = 229, 50
N_SEG, SEG_SPE = 96, 20
N_REP, REP_SPE = 64, 13


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class World:
    """one scene's inputs and what the oracle says about them, computed once per process and never written to"""

    def __init__(self, key, oracle_mod):
        self.key = key
        self.m, self.pi = RS.scene(key)
        pi = self.pi
        self.args = (self.m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
        self.orc = oracle_mod.OracleScene(*self.args)
        self.rows = RS.env_rows(pi, (N + SPE - 1) // SPE, 7)
        self.qa = RS.sample(pi, N, 7)
        self.valid, self.min_dist = self.orc.is_valid_batch(self.qa, self.rows, samples_per_env=SPE, nthreads=0)
        self.sa, self.sb = RS.segments(pi, N_SEG, 7)
        self.motion = self.orc.check_motion_batch(self.sa, self.sb, self.rows, samples_per_env=SEG_SPE, nthreads=0)
        self.ign = ignored_mask(pi) if len(self.m.pair_geom) else np.zeros(0, dtype=bool)

    def scene(self, kernel=None):
        return _scene_with_kernel(kernel, *self.args, range_=self.pi.spec.range, seed=7)

    def use_v5(self, kernel):
        """does the scene's K1 policy take the third generation under these pins (the host export, no device involved)"""
        import os
        from mopa_rl_amd import _lib
        gen, _, cen = kernel.partition("-")
        pins = {"MOPA_VALID_KERNEL": gen, **({"MOPA_V5_CENTRES": cen} if cen else {})}
        old = {k: os.environ.get(k) for k in pins}
        os.environ.update(pins)
        try:
            return _lib.k1_export(*self.args)["use_v5"]
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def state(self, i):
        return RS.full_state(self.pi, self.qa[i], self.rows[i // SPE])


_WORLDS = {}


@pytest.fixture
def world(request, oracle_mod):
    key = request.param
    if key not in _WORLDS:
        _WORLDS[key] = World(key, oracle_mod)
    return _WORLDS[key]


def _ids(keys):
    return [str(k) for k in keys]


@pytest.mark.parametrize("world", KEYS, indirect=True, ids=_ids(KEYS))
def test_fk_pair_distances_and_single_states(world):
    from mopa_rl_amd import _lib
    w = world
    sc = w.scene()
    try:
        assert _lib.lib().mopa_scene_k1_baked(sc.handle) == 0         # a baked kernel is fingerprint-gated: none of these scenes has one
        assert list(sc.active_idx) == list(w.pi.ref_joint_pos_indexes)
        for i in range(0, N, 29)[:8]:
            q = w.state(i)
            gp, gm = sc.debug_fk(q)
            op, om = w.orc.fk(q)
            assert np.array_equal(_bits(gp), _bits(op)), f"{w.key}: geom positions differ, state {i}"
            assert np.array_equal(_bits(gm), _bits(om)), f"{w.key}: geom matrices differ, state {i}"
            do = w.orc.pair_dist(q)
            do[w.ign] = FAR
            dg = sc.debug_pair_dist(q)
            bad = np.nonzero(_bits(dg) != _bits(do))[0]
            assert not len(bad), (w.key, i, bad[:4], w.m.pair_geom[bad[:4]].tolist(), dg[bad[:4]], do[bad[:4]])
        for i in (0, SPE + 1, N - 1):
            q = w.state(i)
            v, md = sc.is_valid_state(q, want_min_dist=True)
            assert (v, _bits(md)) == (bool(w.valid[i]), _bits(w.min_dist[i])), (w.key, i)
            assert sc.is_valid_state(q) == bool(w.valid[i])
    finally:
        sc.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("world", KEYS, indirect=True, ids=_ids(KEYS))
def test_is_valid_matches_the_oracle(world, kernel):
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    sc = w.scene(kernel)
    try:
        bp = BatchPlanner(sc)
        tq, tr = _cuda(w.qa), _cuda(w.rows)
        v, md = bp.is_valid(tq, tr, samples_per_env=SPE, want_min_dist=True)
        v2 = bp.is_valid(tq, tr, samples_per_env=SPE)
        torch.cuda.synchronize()
        v, md, v2 = v.cpu().numpy(), md.cpu().numpy(), v2.cpu().numpy()
        assert np.array_equal(v, w.valid), f"{w.key} {kernel}: {(v != w.valid).sum()} verdicts differ (min-dist kernel) at {np.nonzero(v != w.valid)[0][:8]}"
        assert np.array_equal(v2, w.valid), f"{w.key} {kernel}: {(v2 != w.valid).sum()} verdicts differ (early-out kernel) at {np.nonzero(v2 != w.valid)[0][:8]}"
        bad = np.nonzero(_bits(md) != _bits(w.min_dist))[0]
        assert not len(bad), f"{w.key} {kernel}: {len(bad)} min distances differ at {bad[:8]}: {md[bad[:4]]} vs {w.min_dist[bad[:4]]}"
        # the generation that ran is the pinned one, wherever the scene's policy serves it (the host export of the same pins says so:
        # not for the crowded owner and the far geom, and not with the centres pinned to an LDS that cannot hold them)
        v5 = w.use_v5(kernel)
        assert v5 or kernel != "v5" or w.key in ("crowded_owner", "far")
        want = "k_is_valid" if kernel == "v1" else "k_is_valid_v5" if v5 else "k_is_valid_v2"
        assert sc.valid_kernel(N) == want, (w.key, kernel, sc.valid_kernel(N))
    finally:
        sc.close()


@pytest.mark.parametrize("kernel", ["v1", "v5"])        # wave per segment / segments expanded into states
@pytest.mark.parametrize("world", KEYS, indirect=True, ids=_ids(KEYS))
def test_check_motion_matches_the_oracle(world, kernel):
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    sc = w.scene(kernel)
    try:
        assert sc.motion_kernel(N_SEG) == ("k_check_motion" if kernel == "v1" else "k_motion_expand")
        v = BatchPlanner(sc).check_motion(_cuda(w.sa), _cuda(w.sb), _cuda(w.rows), samples_per_env=SEG_SPE)
        torch.cuda.synchronize()
        v = v.cpu().numpy()
        assert np.array_equal(v, w.motion), f"{w.key} {kernel}: {(v != w.motion).sum()} motion verdicts differ at {np.nonzero(v != w.motion)[0][:8]}"
    finally:
        sc.close()


def test_the_segments_cross_the_seam_and_are_mixed(oracle_mod):
    seam = n_valid = n = 0
    for key in KEYS:
        w = _WORLDS.get(key) or _WORLDS.setdefault(key, World(key, oracle_mod))
        for c in w.pi.non_limited_idx:
            seam += int((np.abs(w.sa[:, c] - w.sb[:, c]) > np.pi).sum())
        n_valid, n = n_valid + int(w.motion.sum()), n + len(w.motion)
    assert seam >= 20 and 0.10 * n <= n_valid <= 0.90 * n, (seam, n_valid, n)


# ---------------- the reports ----------------
@functools.lru_cache(maxsize=None)
def _report_inputs(key):
    w = _WORLDS[key]
    pi = w.pi
    qa, qb = RS.segments(pi, N_REP, 11, span=0.05)
    rows = RS.env_rows(pi, (N_REP + REP_SPE - 1) // REP_SPE, 11)
    return qa, qb, rows


@pytest.mark.parametrize("world", REPORT_KEYS, indirect=True, ids=_ids(REPORT_KEYS))
def test_contact_and_proximity_reports(world):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    pi = w.pi
    sc = w.scene()
    try:
        bp = BatchPlanner(sc)
        tq, tr = _cuda(w.qa), _cuda(w.rows)
        D = oracle_pair_dists(pi, w.orc, w.qa, w.rows, SPE)
        # cutoff = 0 is refused (the broad phase culls at zero margin): the largest cutoff below it is "every pair in overlap"
        with pytest.raises(_lib.MopaError, match="cutoff must be finite and < 0"):
            bp.contacts(tq, tr, samples_per_env=SPE, cutoff=0.0, max_contacts=8)
        n_rec = 0
        for cutoff in (-5e-324, None):
            rep = bp.contacts(tq, tr, samples_per_env=SPE, cutoff=cutoff, max_contacts=8)
            torch.cuda.synchronize()
            c, p, d = rep.count.cpu().numpy(), rep.pair.cpu().numpy(), rep.dist.cpu().numpy()
            oc, op, od = report_from_dists(D, pi.spec.contact_threshold if cutoff is None else cutoff, 8)
            assert np.array_equal(c, oc), f"{w.key} cutoff {cutoff}: {(c != oc).sum()} counts differ"
            assert np.array_equal(p, op), f"{w.key} cutoff {cutoff}: pair lists differ in {(p != op).any(axis=1).sum()} states"
            assert np.array_equal(_bits(d), _bits(od)), f"{w.key} cutoff {cutoff}: {(_bits(d) != _bits(od)).sum()} distances differ"
            n_rec += int(oc.sum())
        assert n_rec > 0
        gpos, gmat = P.poses(pi, w.orc, w.qa, w.rows, SPE)
        want = P.select(P.pair_dists(pi, gpos, gmat, 0.01), 0.01, 4)
        rep = bp.proximity(tq, tr, samples_per_env=SPE, band=0.01, max_pairs=4)
        torch.cuda.synchronize()
        for name, g, o in zip(("clearance", "count", "pair", "dist"), (rep.clearance, rep.count, rep.pair, rep.dist), want):
            g = g.cpu().numpy()
            assert g.dtype == o.dtype and g.shape == o.shape and g.tobytes() == o.tobytes(), f"{w.key}: proximity {name} differs in {(g != o).sum()} words"
        assert (want[1] > 0).any() and (want[1] == 0).any()
    finally:
        sc.close()


@pytest.mark.parametrize("kernel", [None, "v5"])        # None: 64 segments take the wave-per-segment form; v5 pinned: the expanded one
@pytest.mark.parametrize("world", REPORT_KEYS, indirect=True, ids=_ids(REPORT_KEYS))
def test_motion_report_and_clearance(world, kernel):
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    pi = w.pi
    qa, qb, rows = _report_inputs(w.key)
    want = _motion_refs(w.key)
    sc = w.scene(kernel)
    try:
        assert sc.motion_kernel(N_REP) == ("k_motion_expand" if kernel else "k_check_motion")
        bp = BatchPlanner(sc)
        ta, tb, tr = _cuda(qa), _cuda(qb), _cuda(rows)
        rep = bp.motion_report(ta, tb, tr, samples_per_env=REP_SPE, max_contacts=2)
        torch.cuda.synchronize()
        for k in ("valid", "n_states", "first_bad", "last_valid_t", "last_valid_q", "first_bad_q"):
            g, o = getattr(rep, k).cpu().numpy(), want["report"][k]
            assert g.dtype == o.dtype and g.shape == o.shape and g.tobytes() == o.tobytes(), f"{w.key} {kernel}: motion report {k} differs at {np.nonzero(np.atleast_2d((g != o).T).any(axis=0))[0][:8]}"
        for g, o, name in zip(rep.blockers, want["blockers"], ("count", "pair", "dist")):
            g = g.cpu().numpy()
            assert g.dtype == o.dtype and g.tobytes() == o.tobytes(), f"{w.key} {kernel}: blocker {name} differs"
        cl = bp.motion_clearance(ta, tb, tr, samples_per_env=REP_SPE, band=0.01, states=True)
        torch.cuda.synchronize()
        for k in MC.OUTPUTS:
            g, o = getattr(cl, k).cpu().numpy(), want["clearance"][k]
            assert g.dtype == o.dtype and g.shape == o.shape and g.tobytes() == o.tobytes(), f"{w.key} {kernel}: clearance {k} differs at {np.nonzero(np.atleast_2d((g != o).T).any(axis=0))[0][:8]}"
    finally:
        sc.close()


@functools.lru_cache(maxsize=None)
def _motion_refs(key):
    w = _WORLDS[key]
    qa, qb, rows = _report_inputs(key)
    rep = MR.motion_report(w.pi, w.orc, qa, qb, rows, REP_SPE)
    assert 0 < rep["valid"].sum() < N_REP, (key, int(rep["valid"].sum()))        # blocked and free segments
    return {"report": rep, "blockers": MR.blockers(w.pi, w.orc, rep, rows, 2, REP_SPE),
            "clearance": MC.motion_clearance(w.pi, w.orc, qa, qb, rows, 0.01, REP_SPE)}


# ---------------- the exact route of the proximity and clearance reports ----------------
# (test_random_scenes_host::test_the_exact_route_is_reached: on every one of these scenes the states below hold separated pairs that
# gjk_distance answers for)
@functools.lru_cache(maxsize=None)
def _exact_refs(key):
    """the sequential forms under the exact host pair table: proximity tables per band on RS.exact_states, the clearance report of the
    64 report segments per band, and paths of 0 .. 3 vertices made of those segments with their path report"""
    w = _WORLDS[key]
    pi = w.pi
    qs, srows, spe = RS.exact_states(pi)
    gpos, gmat = P.poses(pi, w.orc, qs, srows, spe)
    qa, qb, rows = _report_inputs(key)
    E = 24
    hp = np.zeros((E, 3, w.m.nq))
    for e in range(E):
        for j, q in enumerate((qa[e], qb[e], qa[e + 1])):
            hp[e, j] = RS.full_state(pi, q, rows[e // REP_SPE])
    hl = (np.arange(E) % 4).astype(np.int32)
    out = {"states": (qs, srows, spe), "paths": (hp, hl), "D": {}, "clearance": {}, "path": {}}
    for band in X.BANDS:
        out["D"][band] = X.pair_dists(pi, gpos, gmat, band)
        with X.exact_host():
            out["clearance"][band] = MC.motion_clearance(pi, w.orc, qa, qb, rows, band, REP_SPE)
            out["path"][band] = MC.path_clearance(pi, w.orc, hp, hl, band)
    # the exact table matters on these inputs
    assert (_bits(out["D"][0.05]) != _bits(P.pair_dists(pi, gpos, gmat, 0.05))).any(), key
    return out


@pytest.mark.parametrize("world", RS.EXACT_KEYS, indirect=True, ids=_ids(RS.EXACT_KEYS))
def test_exact_proximity_and_path_clearance(world):
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    ref = _exact_refs(w.key)
    qs, srows, spe = ref["states"]
    hp, hl = ref["paths"]
    sc = w.scene()
    try:
        bp = BatchPlanner(sc)
        tq, tr, tp, tl = _cuda(qs), _cuda(srows), _cuda(hp), _cuda(hl)
        for band in X.BANDS:
            for K in (1, 4):
                want = P.select(ref["D"][band], band, K)
                rep = bp.proximity(tq, tr, samples_per_env=spe, band=band, max_pairs=K, exact=True)
                torch.cuda.synchronize()
                for name, g, o in zip(("clearance", "count", "pair", "dist"), (rep.clearance, rep.count, rep.pair, rep.dist), want):
                    g = g.cpu().numpy()
                    assert g.dtype == o.dtype and g.shape == o.shape and g.tobytes() == o.tobytes(), f"{w.key} band {band} K {K}: exact proximity {name} differs in {(g != o).sum()} words"
            got = bp.path_clearance(tp, tl, band=band, exact=True)
            torch.cuda.synchronize()
            for k in ("clearance", "seg_min", "k_min", "pair_min", "mean_vertex_clearance"):
                g, o = getattr(got, k).cpu().numpy(), ref["path"][band][k]
                assert g.dtype == o.dtype and g.tobytes() == o.tobytes(), (w.key, band, k, g, o)
    finally:
        sc.close()


@pytest.mark.parametrize("kernel", [None, "v5"])        # the wave-per-segment form / the expanded one, as in test_motion_report_and_clearance
@pytest.mark.parametrize("world", RS.EXACT_KEYS, indirect=True, ids=_ids(RS.EXACT_KEYS))
def test_exact_motion_clearance(world, kernel):
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    qa, qb, rows = _report_inputs(w.key)
    ref = _exact_refs(w.key)
    sc = w.scene(kernel)
    try:
        assert sc.motion_kernel(N_REP) == ("k_motion_expand" if kernel else "k_check_motion")
        bp = BatchPlanner(sc)
        ta, tb, tr = _cuda(qa), _cuda(qb), _cuda(rows)
        for band in X.BANDS:
            cl = bp.motion_clearance(ta, tb, tr, samples_per_env=REP_SPE, band=band, states=True, exact=True)
            torch.cuda.synchronize()
            for k in MC.OUTPUTS:
                g, o = getattr(cl, k).cpu().numpy(), ref["clearance"][band][k]
                assert g.dtype == o.dtype and g.shape == o.shape and g.tobytes() == o.tobytes(), f"{w.key} {kernel} band {band}: exact clearance {k} differs at {np.nonzero(np.atleast_2d((g != o).T).any(axis=0))[0][:8]}"
    finally:
        sc.close()


# ---------------- RRT-Connect ----------------
@pytest.mark.parametrize("world", PLAN_KEYS, indirect=True, ids=_ids(PLAN_KEYS))
def test_plan_matches_the_oracle(world):
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w = world
    pi = w.pi
    E = 6
    # starts and goals on one env row, the one on which the oracle calls most of the shared samples valid
    r = int(np.argmax([w.valid[e * SPE:(e + 1) * SPE].mean() for e in range(len(w.rows))]))
    row = w.rows[r:r + 1]
    qa = RS.sample(pi, 400, 13)
    ov, _ = w.orc.is_valid_batch(qa, row, samples_per_env=len(qa), nthreads=0)
    good, bad = qa[ov == 1], qa[ov == 0]
    assert len(good) >= 2 * E, (w.key, len(good))
    starts, goals = np.repeat(row, E, axis=0), np.repeat(row, E, axis=0)
    starts[:, pi.ref_joint_pos_indexes] = good[:E]
    goals[:, pi.ref_joint_pos_indexes] = good[E:2 * E]
    if len(bad):
        goals[0, pi.ref_joint_pos_indexes] = bad[0]          # one query with an invalid goal
    max_iters, max_nodes, max_path = 60, 256, 128
    sc = w.scene()
    try:
        path, plen, status, nchk = BatchPlanner(sc).plan(_cuda(starts), _cuda(goals), max_iters=max_iters, max_nodes=max_nodes, max_path=max_path,
                                                         seed=123, env_id_base=5)
        torch.cuda.synchronize()
        path, plen, status, nchk = path.cpu().numpy(), plen.cpu().numpy(), status.cpu().numpy(), nchk.cpu().numpy()
        for e in range(E):
            st, opath, ochk, _ = w.orc.plan(starts[e], goals[e], pi.spec.range, 0.005, max_iters, max_nodes, seed=123, env_id=5 + e, max_path=max_path)
            assert (status[e], plen[e], nchk[e]) == (st, len(opath), ochk), (w.key, e, status[e], st, plen[e], len(opath), nchk[e], ochk)
            assert np.array_equal(_bits(path[e, :plen[e]]), _bits(opath)), f"{w.key} query {e}: path differs"
        if len(bad):
            assert status[0] == -5
        assert nchk.max() > 0
    finally:
        sc.close()


# ---------------- the comparison can fail ----------------
def test_a_joint_anchor_moved_by_1e_12_shows_in_the_bits(oracle_mod):
    """the scene compiled from a model in which one jnt_pos component of a branch body differs by 1e-12, the oracle on the unchanged
    model: the FK bits differ on exactly the geoms of that body and of its descendants"""
    import copy
    from mopa_rl_amd import _lib
    m, pi = RS.scene("deep_branches")
    orc = oracle_mod.OracleScene(m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    b = int(np.nonzero(m.body_jntnum)[0][2])                 # the tree's third body: a hinge, with two subtrees below it
    j = int(m.body_jntadr[b])
    assert m.jnt_type[j] == 3 and (m.body_parent == b).sum() >= 2
    below = np.zeros(len(m.body_parent), dtype=bool)
    below[b] = True
    for c in range(b + 1, len(below)):
        below[c] = below[m.body_parent[c]]
    m2 = copy.copy(m)
    m2.jnt_pos = m.jnt_pos.copy()
    m2.jnt_pos[j, 0] += 1e-12
    sc = _lib.Scene(m2, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
    try:
        rows, qa = RS.env_rows(pi, 1, 7), RS.sample(pi, 4, 7)
        for i in range(4):
            q = RS.full_state(pi, qa[i], rows[0])
            q[m.jnt_qposadr[j]] = m.jnt_ref[j] + 1.0 + 0.1 * i       # a rotation that moves the anchor's offset well above an ulp
            gp, gm = sc.debug_fk(q)
            op, om = orc.fk(q)
            differs = (_bits(gp) != _bits(op)).any(axis=1) | (_bits(gm) != _bits(om)).reshape(len(gp), -1).any(axis=1)
            assert np.array_equal(differs, below[m.geom_body]), (i, np.nonzero(differs)[0], np.nonzero(below[m.geom_body])[0])
            assert differs.any() and not differs.all()
    finally:
        sc.close()
