"""The chunk loop of the expanded-motion pipeline (csrc/mopa_motion.inc: motion_for_chunks over motion_expand_chunk) under
check_motion, the motion report and the clearance report.  A default chunk holds ~10^7 segments, so only MOPA_MOTION_CHUNK (read
once, at scene creation) lets a test run a second chunk: two scenes of one description, one with the default chunk and one with
chunks of 1000 segments, must write the same bytes.  That covers the offset `first` into every output and the env index
(first + i) / samples_per_env of k_motion_expand: samples_per_env = 7 does not divide 1000, so chunk boundaries fall inside an env's
group of segments, and every env has a passive row of its own.  Push only: the chunk arithmetic does not depend on the scene.
No test here provokes a fault: every input is a valid call."""
import numpy as np
import pytest

import motion_clearance_ref as M
import proximity_ref as P

pytestmark = pytest.mark.gpu
ENV = "SawyerPushObstacle-v0"
CHUNK = 1000
SPE = 7
BAND = 0.01                 # (proximity_ref.BANDS, test_motion_clearance_gpu.py)
N_ONE = 64                  # the prefix that runs with one segment per chunk
REPORT_OUT = ("valid", "n_states", "first_bad", "last_valid_t", "last_valid_q", "first_bad_q")
BLOCKER_OUT = ("count", "pair", "dist")
IN_THE_WAY = 37             # every 37th env has the cube in its first segment's way


def chunk_inputs(n):
    """(pi, qa [n, na], qb [n, na], rows [ceil(n / SPE), nq], row0 [nq]): motion_clearance_ref.mix_segments tiled to n segments, SPE
    to an env; every env row is the shared row row0 with the cube (the free body) moved in the plane by its own offset, which
    changes clearances and no verdict -- so in every IN_THE_WAY-th env the cube sits where the end state of the env's first segment
    has a claw, which blocks that segment at least"""
    pi, orc, A, B, rows, _ = M.mix_segments(ENV)
    m = pi.model
    idx = np.arange(n) % len(A)
    qa, qb = np.ascontiguousarray(A[idx]), np.ascontiguousarray(B[idx])
    row0 = np.array(rows[0])
    assert (rows == row0).all()
    E = (n + SPE - 1) // SPE
    env_rows = np.repeat(row0[None], E, axis=0)
    free, = np.nonzero(np.asarray(m.jnt_type) == 0)
    assert len(free) == 1
    a = int(m.jnt_qposadr[free[0]])
    env_rows[:, a:a + 2] += np.random.default_rng(47).normal(0.0, 0.03, (E, 2))
    way = np.arange(3, E, IN_THE_WAY)
    claw = [m.all_geom_names[i] for i in m.geom_mjid].index("rightclaw_it")
    env_rows[way, a:a + 3] = P.poses(pi, orc, qb[way * SPE], env_rows[way], 1)[0][:, claw]
    assert len(np.unique(env_rows, axis=0)) == E
    return pi, qa, qb, env_rows, row0


def assert_mixed(valid, valid_row0, n_near):
    """the outputs of the default chunk are not trivially equal: valid and blocked segments, segments with and without a state in
    band, and at least two env rows under which a verdict is not the shared row's"""
    assert 8 <= int(valid.sum()) <= len(valid) - 8
    assert int((n_near > 0).sum()) >= 8 and int((n_near == 0).sum()) >= 8
    changed = np.unique(np.nonzero(valid != valid_row0)[0] // SPE)
    assert len(changed) >= 2, changed


class World:
    def __init__(self):
        import torch
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        pi = M.mix_segments(ENV)[0]
        self.scenes = {}
        for chunk in (None, CHUNK, 1):
            with pytest.MonkeyPatch.context() as mp:
                if chunk is None:
                    mp.delenv("MOPA_MOTION_CHUNK", raising=False)
                else:
                    mp.setenv("MOPA_MOTION_CHUNK", str(chunk))
                sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
                sc.contact_scene()          # (the clearance report's scene is created on first use: under the same setting)
            self.scenes[chunk] = sc
        self.bp = {k: BatchPlanner(sc) for k, sc in self.scenes.items()}
        sc = self.scenes[None]
        lo, hi = 1, 1 << 20         # the smallest batch that takes the expanded form
        assert sc.motion_kernel(hi) == "k_motion_expand"
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if sc.motion_kernel(mid) == "k_motion_expand" else (mid + 1, hi)
        self.n_min = lo
        self.N = lo + 301
        self.pi, qa, qb, rows, row0 = chunk_inputs(self.N)
        self.qa, self.qb, self.rows = (torch.from_numpy(x).cuda() for x in (qa, qb, rows))
        self.rows0 = torch.from_numpy(np.repeat(row0[None], len(rows), axis=0)).cuda()

    def close(self):
        for sc in self.scenes.values():
            sc.close()


@pytest.fixture(scope="module")
def world(oracle_mod):
    w = World()
    yield w
    w.close()


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, np.nonzero(np.atleast_2d((g != w).T).any(axis=0))[0][:8])


def _clearance(bp, qa, qb, rows, band):
    import torch
    rep = bp.motion_clearance(qa, qb, rows, samples_per_env=SPE, band=band, states=True)
    torch.cuda.synchronize()
    return {k: getattr(rep, k).cpu().numpy() for k in M.OUTPUTS}


def test_chunked_scenes_write_the_same_bytes(world):
    import torch
    w = world
    N = w.N
    for chunk in (None, CHUNK):
        assert w.scenes[chunk].motion_kernel(N) == "k_motion_expand" and w.scenes[chunk].motion_kernel(w.n_min - 1) == "k_check_motion"
    assert N >= 4 * CHUNK + 1 and (N % CHUNK) % 256 != 0 and CHUNK % SPE != 0        # five chunks or more, a ragged last one
    out = {}
    for chunk in (None, CHUNK):
        bp = w.bp[chunk]
        valid = bp.check_motion(w.qa, w.qb, w.rows, samples_per_env=SPE)
        rep = bp.motion_report(w.qa, w.qb, w.rows, samples_per_env=SPE, states=True, max_contacts=2)
        torch.cuda.synchronize()
        o = {"check_motion": {"valid": valid.cpu().numpy()},
             "motion_report": {**{k: getattr(rep, k).cpu().numpy() for k in REPORT_OUT}, **{k: getattr(rep.blockers, k).cpu().numpy() for k in BLOCKER_OUT}}}
        for band in (0.0, BAND):
            o["motion_clearance", band] = _clearance(bp, w.qa, w.qb, w.rows, band)
        out[chunk] = o
    whole = out[None]
    assert whole["check_motion"]["valid"].tobytes() == whole["motion_report"]["valid"].tobytes()
    valid_row0 = w.bp[None].check_motion(w.qa, w.qb, w.rows0, samples_per_env=SPE)
    torch.cuda.synchronize()
    assert_mixed(whole["check_motion"]["valid"], valid_row0.cpu().numpy(), whole["motion_clearance", BAND]["n_near"])
    assert int((whole["motion_report"]["count"] > 0).sum()) >= 8
    for what in whole:
        _same(out[CHUNK][what], whole[what], what)


def test_one_segment_per_chunk(world):
    """MOPA_MOTION_CHUNK=1 on a prefix, the clearance report: every chunk is one segment in one scan block (nb = 1)"""
    w = world
    qa, qb, rows = w.qa[:N_ONE], w.qb[:N_ONE], w.rows[:(N_ONE + SPE - 1) // SPE]
    for band in (0.0, BAND):
        want = _clearance(w.bp[None], qa, qb, rows, band)
        assert (want["n_near"] > 0).any() and (want["n_states"] > 1).any()
        _same(_clearance(w.bp[1], qa, qb, rows, band), want, ("chunk 1", band))
