"""The device-side state count of K1 (mopa_is_valid_batch_counted, the entry point the batched pull-back feeds its candidate rows
through) on all four envs, against the CPU oracle on bytes: every launch plan k1_plan gives it -- dual dispatch (both validity
launches enqueued, each reads the count, one leaves at once), the lane-per-state launch alone (MOPA_NO_DUAL_DISPATCH, a scene
pinned to the third generation), the mesh gate with its row list, the row list's overflow and the fallback pass (Lift), the baked
pair drain (Push) and the refusals -- at the counts either side of every hand-over, verdict-only and with depths.  States from the
count on are neither read nor written, and the launch directly behind a counted one finds the self-resetting tile counter at zero.

N = T + 64 + 37 with T = max(64, 36 * CUs), the smallest batch at which dual dispatch exists; 7 states per env row, so tiles
straddle env rows; every count is a prefix of one oracle run over the N states."""
import ctypes as C

import numpy as np
import pytest

from conftest import SUPPORTED_ENVS, sample_states
from contacts_ref import full_state, ignored_mask

pytestmark = pytest.mark.gpu

SPE = 7
FILL_VALID = 7
FILL_MD = 0x7FF8DEAD0000BEEF          # one NaN bit pattern no kernel produces
LIFT = "SawyerLiftObstacle-v0"
PUSH = "SawyerPushObstacle-v0"
PUSHER = "PusherObstacle-v0"
SEEDS = {PUSH: 11, LIFT: 12, "SawyerAssemblyObstacle-v0": 13, PUSHER: 14}      # chosen on the CPU with the oracle, for 256 CUs: check_composition holds
MOPA_ERR_UNSUPPORTED = 2


def lane_min(n_cu):
    """k1_lane_min of an unpinned scene: from this many states on a batch goes to the lane-per-state kernel"""
    return max(64, 36 * int(n_cu))


def counts_of(T, N):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, N - 37, N - 1, N]


class Batch:
    """N mixed states on ceil(N / 7) env rows that all differ, and the oracle's verdicts and depths of all of them (one run); CPU only"""

    def __init__(self, env, n_cu, oracle_mod):
        from mopa_rl_amd.scene import planner_inputs
        self.env = env
        self.pi = pi = planner_inputs(env)
        m = pi.model
        self.T = T = lane_min(n_cu)
        self.N = N = T + 64 + 37
        self.E = E = (N + SPE - 1) // SPE
        self.orc = orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
        seed = SEEDS[env]
        rng = np.random.default_rng(seed)
        n_uni = N // 8 if env == PUSHER else N // 2       # (Pusher's arm sweeps its obstacles over most of its joint ranges)
        qa = np.concatenate([sample_states(pi, N - n_uni, seed + 100, "near")[0], sample_states(pi, n_uni, seed + 200, "uniform")[0]])
        qa = np.ascontiguousarray(qa[rng.permutation(N)])
        rows = np.repeat(sample_states(pi, 1, 3)[1], E, axis=0)
        for name in ("rc_close", "lc_close"):             # the gripper slides, inside their ranges
            if name in m.jnt_names:
                j = m.joint_name2id(name)
                rows[:, int(m.jnt_qposadr[j])] = rng.uniform(m.jnt_range[j][0], m.jnt_range[j][1], size=E)
        for j in np.nonzero(np.asarray(m.jnt_type) == 0)[0]:          # a free body: moved in the plane, row by row
            a = int(m.jnt_qposadr[j])
            rows[:, a:a + 2] += rng.normal(0.0, 0.03, (E, 2))
        if env == PUSHER:       # box and target rest 4 mm above each other amid the obstacles in the default row: moved out
            rows[:, 12:16] = rng.uniform(0.3, 0.5, (E, 4))
        if env == LIFT:         # the can (a convex mesh) parked around the gripper of two envs in three; their states jitter around one arm pose
            ca = m.get_joint_qpos_addr("cube")
            names = [m.all_geom_names[i] for i in m.geom_mjid]
            claw = [i for i, n in enumerate(names) if "claw" in n or "finger" in n][0]
            for e in range(E):
                if e % 3 == 2:
                    continue
                lo, hi = e * SPE, min(N, (e + 1) * SPE)
                base = qa[lo].copy()
                qa[lo:hi] = np.clip(base + rng.normal(0, 0.05, (hi - lo, len(base))), pi.jnt_minimum, pi.jnt_maximum)
                gpos, _ = orc.fk(full_state(pi, base, rows[e]))
                rows[e, ca:ca + 3] = gpos[claw] + rng.normal(0, 0.04, 3)
                quat = rng.normal(size=4)
                rows[e, ca + 3:ca + 7] = quat / np.linalg.norm(quat)
        self.qa, self.rows = qa, np.ascontiguousarray(rows)
        self.ov, self.omd = orc.is_valid_batch(qa, self.rows, samples_per_env=SPE, nthreads=0)
        for a in (self.qa, self.rows, self.ov, self.omd):
            a.setflags(write=False)

    def check_composition(self):
        """what the counts need of the batch: both verdicts among the first 63 states and among the states [T, N) -- the tiles the
        wave-per-state launch and the last, partial tiles of the lane-per-state launch decide --, all env rows different, and on
        Lift a mesh pair at or below the threshold in the first 64 states and in [T, N) (the oracle's pair distances)"""
        T, N, ov = self.T, self.N, self.ov
        for lo, hi in ((0, 63), (T, N)):
            assert 0 < int(ov[lo:hi].sum()) < hi - lo, (self.env, lo, hi, int(ov[lo:hi].sum()))
        assert len(np.unique(self.rows, axis=0)) == self.E
        if self.env == LIFT:
            from mopa_rl_amd.mjcf import GEOM_MESH
            m, pi = self.pi.model, self.pi
            g = int(np.where(m.geom_type == GEOM_MESH)[0][0])
            mesh_pairs = np.nonzero((np.asarray(m.pair_geom) == g).any(axis=1) & ~ignored_mask(pi))[0]
            for lo, hi in ((0, 64), (T, N)):        # 165 states in all
                hit = [bool((self.orc.pair_dist(full_state(pi, self.qa[i], self.rows[i // SPE]))[mesh_pairs] <= pi.spec.contact_threshold).any())
                       for i in range(lo, hi)]
                assert any(hit), (lo, hi)


_WORLDS = {}


def _world(env, oracle_mod):
    """the batch of one env on the device and its two scenes: as the library chooses ("auto"), and pinned to the third-generation
    lane-per-state kernel ("v5": threshold 64, every count goes to the lane kernel, no dual dispatch); built once per env"""
    import torch
    from test_gpu_parity import _scene_with_kernel
    if env not in _WORLDS:
        b = Batch(env, torch.cuda.get_device_properties(0).multi_processor_count, oracle_mod)
        pi = b.pi
        mk = lambda k: _scene_with_kernel(k, pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
        b.scenes = {"auto": mk(None), "v5": mk("v5")}
        b.tq, b.tr = torch.from_numpy(b.qa.copy()).cuda(), torch.from_numpy(b.rows.copy()).cuda()
        _WORLDS[env] = b
    return _WORLDS[env]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    import torch
    yield
    torch.cuda.synchronize()
    for b in _WORLDS.values():
        for s in b.scenes.values():
            s.close()
    _WORLDS.clear()


@pytest.fixture(scope="module", params=SUPPORTED_ENVS)
def world(request, oracle_mod):
    return _world(request.param, oracle_mod)


@pytest.fixture(scope="module")
def lift(oracle_mod):
    return _world(LIFT, oracle_mod)


def _filled(N, want_md):
    """outputs that hold the fill: a launch that skips a state leaves it there (memory fresh from the allocator may hold an earlier
    call's correct bytes)"""
    import torch
    valid = torch.full((N,), FILL_VALID, dtype=torch.uint8, device="cuda")
    return valid, (torch.full((N,), FILL_MD, dtype=torch.int64, device="cuda") if want_md else None)


def _read(valid, md):
    return valid.cpu().numpy(), (md.cpu().numpy().view(np.uint64) if md is not None else None)


def _counted(w, sc, n, want_md, plain_after=False):
    """one counted call through the C ABI on pre-filled outputs and -- with nothing in between, not even a synchronisation -- a plain
    call over all N states on the same scene and stream; returns (rc, valid bytes, depth bits or None, the plain call's outputs)"""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr, _stream_handle
    N = w.N
    valid, md = _filled(N, want_md)
    nd = torch.tensor([n], dtype=torch.int64, device="cuda")
    rc = _lib.lib().mopa_is_valid_batch_counted(sc.handle, _ptr(w.tq), _ptr(w.tr), N, SPE, _ptr(valid), _ptr(md) if want_md else None, _ptr(nd),
                                                _stream_handle(None))
    after = None
    if plain_after:
        v2, md2 = _filled(N, want_md)
        _lib.check(_lib.lib().mopa_is_valid_batch(sc.handle, _ptr(w.tq), _ptr(w.tr), N, SPE, _ptr(v2), _ptr(md2) if want_md else None, _stream_handle(None)))
        after = _read(v2, md2)
    return (rc,) + _read(valid, md) + (after,)


def _assert_counted(w, form, n, want_md, what=""):
    """the prefix equals the oracle, everything from n on holds the fill, and the full-N call behind it equals the oracle"""
    what = (w.env, form, "count", n, "depths" if want_md else "verdict-only", what)
    rc, valid, md, after = _counted(w, w.scenes[form], n, want_md, plain_after=True)
    assert rc == 0, what
    assert np.array_equal(valid[:n], w.ov[:n]), (what, int((valid[:n] != w.ov[:n]).sum()))
    assert (valid[n:] == FILL_VALID).all(), (what, "verdict bytes written past the count", int((valid[n:] != FILL_VALID).sum()))
    if want_md:
        want = w.omd.view(np.uint64)
        assert np.array_equal(md[:n], want[:n]), (what, int((md[:n] != want[:n]).sum()))
        assert (md[n:] == np.uint64(FILL_MD)).all(), (what, "depths written past the count", int((md[n:] != np.uint64(FILL_MD)).sum()))
        assert np.array_equal(after[1], want), (what, "the full launch behind it: depths", int((after[1] != want).sum()))
    assert np.array_equal(after[0], w.ov), (what, "the full launch behind it", int((after[0] != w.ov).sum()))
    return valid, md


def test_batch_composition(world):
    world.check_composition()


@pytest.mark.parametrize("form", ["auto", "v5"])
def test_launch_plan(world, form):
    """what the library reports of the plans under test: the lane-per-state kernel at N on both scenes, below T the wave-per-state
    kernel on the unpinned scene only; Push is a baked scene whose verdict-only plan drains two tiles at a time"""
    from mopa_rl_amd import _lib
    w, sc = world, world.scenes[form]
    assert sc.valid_kernel(w.N) == "k_is_valid_v5" and sc.valid_kernel(w.T) == "k_is_valid_v5"
    assert sc.valid_kernel(w.T - 1) == ("k_is_valid" if form == "auto" else "k_is_valid_v5")
    assert sc.valid_kernel(64) == ("k_is_valid" if form == "auto" and w.T > 64 else "k_is_valid_v5")
    tpd = []
    for want_md in (0, 1):
        t, cap = C.c_int32(), C.c_int32()
        assert _lib.lib().mopa_scene_k1_drain_plan(sc.handle, w.N, want_md, C.byref(t), C.byref(cap)) == 0
        tpd.append(t.value)
    baked = _lib.lib().mopa_scene_k1_baked(sc.handle)
    print(w.env, form, "T", w.T, "N", w.N, "kernel at N", sc.valid_kernel(w.N), "baked", baked, "tiles_per_drain (verdict-only, depths)", tpd)
    if w.env == PUSH and form == "auto":
        assert baked >= 1 and tpd[0] == 2
    assert all(t in (1, 2) for t in tpd)


@pytest.mark.parametrize("want_md", [False, True], ids=["verdicts", "depths"])
@pytest.mark.parametrize("form", ["auto", "v5"])
def test_counts_equal_the_oracle_prefix(world, form, want_md):
    for n in counts_of(world.T, world.N):
        _assert_counted(world, form, n, want_md)


def test_without_dual_dispatch_the_same_bytes(world, monkeypatch):
    """MOPA_NO_DUAL_DISPATCH (read per call): the lane-per-state launch alone serves every count of the unpinned scene"""
    w = world
    for want_md in (False, True):
        for n in (1, w.T - 1, w.T):
            monkeypatch.delenv("MOPA_NO_DUAL_DISPATCH", raising=False)
            dual = _assert_counted(w, "auto", n, want_md, "dual dispatch")
            monkeypatch.setenv("MOPA_NO_DUAL_DISPATCH", "1")
            single = _assert_counted(w, "auto", n, want_md, "MOPA_NO_DUAL_DISPATCH")
            assert dual[0].tobytes() == single[0].tobytes()
            assert not want_md or dual[1].tobytes() == single[1].tobytes()


@pytest.mark.parametrize("cap", [0, 64])
@pytest.mark.parametrize("form", ["auto", "v5"])
def test_lift_row_list_caps_under_a_count(lift, form, cap, monkeypatch):
    """MOPA_MESH_ROWS_CAP (read per call) = 0: no row list, every state with a mesh pair within reach goes through the state-list
    pass; 64: the row list overflows.  Both lists are built up to the count only.  (Lift alone has mesh pairs.)"""
    w = lift
    monkeypatch.setenv("MOPA_MESH_ROWS_CAP", str(cap))
    for want_md in (False, True):
        for n in (0, 65, w.T - 1, w.T + 1, w.N):
            _assert_counted(w, form, n, want_md, f"row cap {cap}")


def test_refusals(world):
    """a scene without the third-generation lane-per-state kernel (pinned to the wave-per-state kernel, or to the second generation --
    on Lift that is also the mesh scene without the gate) refuses the count: MOPA_ERR_UNSUPPORTED, nothing launched, nothing written"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr, _stream_handle
    from test_gpu_parity import _scene_with_kernel
    w, pi = world, world.pi
    for pin in ("v1", "v2"):
        sc = _scene_with_kernel(pin, pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
        for want_md in (False, True):
            for n in (0, 65, w.N):
                rc, valid, md, _ = _counted(w, sc, n, want_md)
                assert rc == MOPA_ERR_UNSUPPORTED, (w.env, pin, n)
                assert b"lane-per-state kernel" in _lib.lib().mopa_last_error(), (w.env, pin, _lib.lib().mopa_last_error())
                assert (valid == FILL_VALID).all() and (md is None or (md == np.uint64(FILL_MD)).all()), (w.env, pin, n)
        v, d = _filled(w.N, True)
        _lib.check(_lib.lib().mopa_is_valid_batch(sc.handle, _ptr(w.tq), _ptr(w.tr), w.N, SPE, _ptr(v), _ptr(d), _stream_handle(None)))
        v, d = _read(v, d)
        assert np.array_equal(v, w.ov) and np.array_equal(d, w.omd.view(np.uint64)), (w.env, pin)
        sc.close()
