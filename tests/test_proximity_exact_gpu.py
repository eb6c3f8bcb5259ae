"""Exact route of the proximity and clearance reports on the GPU (exact=True: mopa_proximity_exact_batch,
mopa_motion_clearance_exact_batch, mopa_geom_sep_exact_batch) against the sequential forms of proximity_ref / motion_clearance_ref
evaluated with the exact host pair table (mopa_geom_sep_exact_host, no broad phase): every comparison is on bytes."""
import numpy as np
import pytest

import frames_ref as F
import motion_clearance_ref as M
import proximity_exact_ref as X
import proximity_ref as P
from conftest import SUPPORTED_ENVS, sample_states

pytestmark = pytest.mark.gpu
N_MAX = 4 * 64 + 1
SIZES = (1, 65, N_MAX)          # one wave, one block, more blocks than a wave's pull
SPES = (1, 5)
N_SEG = 300                     # test_motion_clearance_gpu's segment count


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class World:
    """one scene, N_MAX states near the env's initial pose on per-env rows that all differ, and the sequential form's EXACT pair table
    per (samples_per_env, band); a batch of N < N_MAX states is a prefix"""

    def __init__(self, env, oracle_mod):
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        from mopa_rl_amd.scene import planner_inputs
        self.env = env
        self.pi = pi = planner_inputs(env)
        m = pi.model
        self.sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
        self.bp = BatchPlanner(self.sc)
        self.orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
        self.npair = len(m.pair_geom)
        rng = np.random.default_rng(47)
        self.qa = sample_states(pi, N_MAX, 5, "near")[0]
        rows = np.repeat(sample_states(pi, 1, 3)[1], N_MAX, axis=0)
        for j in np.nonzero(np.asarray(m.jnt_type) == 0)[0]:          # a free body: moved in the plane, row by row
            a = int(m.jnt_qposadr[j])
            rows[:, a:a + 2] += rng.normal(0.0, 0.03, (N_MAX, 2))
        if env == "PusherObstacle-v0":      # box and target rest 4 mm above each other amid the obstacles in the default row: moved out
            rows[:, 12:16] = rng.uniform(0.3, 0.5, (N_MAX, 4))
        self.rows = rows
        self.poses = {spe: P.poses(pi, self.orc, self.qa, rows, spe) for spe in SPES}
        self.D = {(spe, band): X.pair_dists(pi, *self.poses[spe], band) for spe in SPES for band in X.BANDS}

    def tensors(self, N, spe):
        import torch
        return torch.from_numpy(self.qa[:N]).cuda(), torch.from_numpy(self.rows[:(N + spe - 1) // spe]).cuda()

    def run(self, N, spe, band, K, stream=None, **kw):
        import torch
        tq, tr = self.tensors(N, spe)
        rep = self.bp.proximity(tq, tr, samples_per_env=spe, band=band, max_pairs=K, stream=stream, **kw)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in rep)


@pytest.fixture(scope="module", params=SUPPORTED_ENVS)
def world(request, oracle_mod):
    w = World(request.param, oracle_mod)
    yield w
    w.sc.close()


def test_inflated_class_pairs_are_in_band(world):
    """otherwise the tests below show nothing"""
    infl = X.inflated_pairs(world.pi.model)
    for band in X.BANDS:
        D = world.D[1, band]
        sep = (D > 0) & (D <= band)
        n = int(sep[:, infl].sum())
        print(world.env, "band", band, "separated pairs reported", int(sep.sum()), "of an inflated class", n)
        assert n >= 1, (world.env, band)
    # ... and there the exact table is not the inflated one
    assert (_bits(world.D[1, 0.05]) != _bits(P.pair_dists(world.pi, *world.poses[1], 0.05))).any()


def test_bit_identical_to_the_sequential_form(world):
    for band in X.BANDS:
        for K in (1, world.npair):
            for N in SIZES:
                for spe in SPES:
                    want = P.select(world.D[spe, band][:N], band, K)
                    got = world.run(N, spe, band, K, exact=True)
                    what = (world.env, band, K, N, spe)
                    for g, w, name in zip(got, want, ("clearance", "count", "pair", "dist")):
                        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
                        assert g.tobytes() == w.tobytes(), (what, name, int((g != w).sum()))


def test_validity_and_overlap_rows(world):
    import torch
    w = world
    thr = w.pi.spec.contact_threshold
    for spe in SPES:
        tq, tr = w.tensors(N_MAX, spe)
        valid = w.bp.is_valid(tq, tr, samples_per_env=spe)
        torch.cuda.synchronize()
        cl, cnt, pair, dist = w.run(N_MAX, spe, 0.05, w.npair, exact=True)
        assert np.array_equal(valid.cpu().numpy().astype(bool), cl > thr), (w.env, spe)
        # the rows with dist <= 0 carry exact=False's bits, and no overlap exact=False reports is missing (a dist of exactly 0.0 there
        # may be a SEPARATED pair whose inflated value max(band - depth, 0) was clamped: the exact route gives it its distance)
        _, _, pair0, dist0 = w.run(N_MAX, spe, 0.05, w.npair, exact=False)
        n_rows = 0
        for i in range(N_MAX):
            mine = {int(p): int(_bits(d)[0]) for p, d in zip(pair[i], dist[i]) if d <= 0}
            theirs = {int(p): int(_bits(d)[0]) for p, d in zip(pair0[i], dist0[i]) if d <= 0}
            assert all(theirs.get(p) == d for p, d in mine.items()), (w.env, spe, i, mine, theirs)
            assert all(p in mine for p, d in zip(pair0[i], dist0[i]) if d < 0), (w.env, spe, i, mine, theirs)
            n_rows += len(mine)
        assert n_rows > 20, n_rows


def test_margin_broad_phase_keeps_every_pair_in_band(world):
    """test_proximity_host's assertion with the exact table: no pair the un-culled sequential form reports is culled"""
    w = world
    m = w.pi.model
    gpos, gmat = w.poses[1]
    static = np.array([(gpos[:, g] == gpos[0, g]).all() for g in range(gpos.shape[1])])
    rb = P.rbound(m)
    kept = 0
    for band in X.BANDS:
        D = w.D[1, band]
        for i in range(N_MAX):
            cull = P.culled_band(m, rb, static, gpos[i], gmat[i], band)
            hit = D[i] != F.FAR
            assert not (hit & cull).any(), (w.env, band, i, np.nonzero(hit & cull)[0])
            kept += int(hit.sum())
    assert kept > 200


def test_two_runs_and_two_streams_write_the_same_bytes(world):
    import torch
    outs = [world.run(N_MAX, 5, 0.05, 3, stream=st, exact=True) for st in (None, None, torch.cuda.Stream(), torch.cuda.Stream())]
    for o in outs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o, outs[0]))


def test_default_path_is_exact_false(world):
    import torch
    a, b = world.run(N_MAX, 1, 0.05, 3), world.run(N_MAX, 1, 0.05, 3, exact=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    want = P.select(P.pair_dists(world.pi, *world.poses[1], 0.05), 0.05, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, want))
    tq, tr = world.tensors(64, 1)
    tb = torch.from_numpy(np.ascontiguousarray(world.qa[64:128])).cuda()
    m0, m1 = world.bp.motion_clearance(tq, tb, tr, samples_per_env=1, band=0.05), world.bp.motion_clearance(tq, tb, tr, samples_per_env=1, band=0.05, exact=False)
    torch.cuda.synchronize()
    for k in M.OUTPUTS[:-1]:
        assert getattr(m0, k).cpu().numpy().tobytes() == getattr(m1, k).cpu().numpy().tobytes(), k


def test_pair_level_kernel_has_the_bits_of_the_host_form():
    import torch
    from mopa_rl_amd.batch import geom_sep
    from mopa_rl_amd.scene import load_scene
    can = P.can_of(load_scene("sawyer_lift_obstacle"))
    cs = P.sep_case_list(can)
    cs = cs + [c.swapped() for c in cs if c.t2 != F.MESH]
    types, recs = F.recs_of(cs)
    tt, tr, tc = torch.from_numpy(types).cuda(), torch.from_numpy(recs).cuda(), torch.from_numpy(can).cuda()
    for band in X.BANDS:
        want, iters = X.host_sep(cs, can, band, iters=True)
        got = geom_sep(tt, tr, band, mesh_verts=tc, exact=True)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        bad = _bits(got) != _bits(want)
        assert not bad.any(), (band, [(cs[i].cls, cs[i].what, got[i], want[i]) for i in np.nonzero(bad)[0][:8]])
        # (the exact route reports at least the 8 cases per inflated class that test_band_membership counts at the smaller band)
        assert len(cs) > 1000 and (iters >= 0).all() and ((iters > 0) & (want != F.FAR)).sum() >= 64


@pytest.mark.parametrize("env", ["SawyerPushObstacle-v0", "SawyerLiftObstacle-v0"])
def test_clearance_reports(env, oracle_mod):
    """motion_clearance(exact=True) and path_clearance(exact=True) on motion_clearance_ref.mix_segments against the sequential forms
    with the exact pair table (Lift has mesh pairs)"""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from contacts_ref import full_state
    pi, orc, A, B, rows, _ = M.mix_segments(env)
    qa, qb, rows = np.array(A[:N_SEG]), np.array(B[:N_SEG]), np.array(rows[:N_SEG])
    sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
    bp = BatchPlanner(sc)
    ta, tb, tr = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), torch.from_numpy(rows).cuda()
    band = 0.05
    with X.exact_host():
        want = M.motion_clearance(pi, orc, qa, qb, rows, band, 1)
    infl = M.motion_clearance(pi, orc, qa[:65], qb[:65], rows[:65], band, 1)
    assert (_bits(want["clearance"][:65]) != _bits(infl["clearance"])).any()         # the exact table matters on these segments
    for N in (65, N_SEG):
        rep = bp.motion_clearance(ta[:N].contiguous(), tb[:N].contiguous(), tr[:N].contiguous(), samples_per_env=1, band=band, states=True, exact=True)
        torch.cuda.synchronize()
        for k in M.OUTPUTS:
            g, w = getattr(rep, k).cpu().numpy(), want[k][:N]
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (env, N, k, int((g != w).sum()))
    # paths of 0 .. 3 vertices made of the segments: qa[e] -> qb[e] -> qa[e + 1] on row e
    E = 48
    hp = np.zeros((E, 3, sc.nq))
    for e in range(E):
        for j, q in enumerate((qa[e], qb[e], qa[e + 1])):
            hp[e, j] = full_state(pi, q, rows[e])
    hl = (np.arange(E) % 4).astype(np.int32)
    with X.exact_host():
        pw = M.path_clearance(pi, orc, hp, hl, band)
    got = bp.path_clearance(torch.from_numpy(hp).cuda(), torch.from_numpy(hl).cuda(), band=band, exact=True)
    torch.cuda.synchronize()
    for k in ("clearance", "seg_min", "k_min", "pair_min", "mean_vertex_clearance"):
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == pw[k].dtype and g.tobytes() == pw[k].tobytes(), (env, k, g, pw[k])
    # the single-segment and single-state forms
    a, b = full_state(pi, qa[3], rows[3]), full_state(pi, qb[3], rows[3])
    one = sc.motion_clearance_state(a, b, band, exact=True)
    assert _bits(one["clearance"]) == _bits(want["clearance"][3]) and one["k_min"] == want["k_min"][3] and one["pair_min"] == want["pair_min"][3]
    cl, lst = sc.proximity_state(b, band, 4, exact=True)
    assert _bits(cl) == _bits(want["end_clearance"][3])
    sc.close()
