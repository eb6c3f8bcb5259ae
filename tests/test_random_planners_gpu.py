"""The planner family off the shipped scenes: on the scenes and query sets of planner_cases.py (1 to 12 active coordinates, SO(2) and
a slide at active index >= 8, passive coordinates inside the tree, free bodies, mesh pairs, 454 pairs, no pair at all) RRT-Connect in
each of its builds, keep_state / resume, the race, RRT*, RRT* under the clearance objective, the three K9 kernels stand-alone and
behind a planner launch, and the single-query host forms are bit-identical to the sequential references; the K9 capacities of seven
scenes are the parent's.  Every comparison is on bit patterns, no tolerance is involved.  test_random_planners_host.py shows on the
references alone that these cases reach the branches they are for.  No test here launches something that is expected to fault: the
refusals are host-side argument checks.

The clearance references take, on the CPU, 1.8 s (band 0) and 2.7 s (1 cm) for the four queries x 100 iterations of seed 22 and 1.7 s
and 3.7 s for the three of `mesh`; every other reference of this file takes at most 1.7 s per scene."""
import numpy as np
import pytest

import planner_cases as PC
import race_ref
import rrtstar_ref as R
from test_race_gpu import _assert_equal as _assert_race
from test_shortcut_gpu import _run as _run_shortcut
from test_simplify_gpu import _assert_rows, _bits
from test_smooth_gpu import _run as _run_smooth
from test_star_clearance_gpu import _assert_equal as _assert_clear
from test_star_gpu import _assert_equal as _assert_star

pytestmark = pytest.mark.gpu

UNSUPPORTED = 2         # MOPA_ERR_UNSUPPORTED
# `full` (64 moving geoms, 454 pairs): the four multi-state slabs of a planner workgroup do not fit the LDS next to the scene.
# RRT-Connect, the race and the smoothing level of K9 refuse the scene before any launch; RRT* and the other two K9 levels run.
NO_PLANNER_LDS = ("full",)
K9_NAMES = ("simplify_paths", "shortcut_paths", "smooth_paths")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(res):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def _assert_connect(got, want, what=""):
    """got / want: (path, path_len, status, n_checks) as numpy"""
    assert np.array_equal(got[2], want[2]), f"{what}: status differs\n{got[2]}\n{want[2]}"
    assert np.array_equal(got[3], want[3]), f"{what}: n_checks differs\n{got[3]}\n{want[3]}"
    _assert_rows(got[0], got[1], want[0], want[1], what)


class Ctx:
    def __init__(self, O, key):
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        self.key = key
        self.w = PC.world(O, key)
        self.scene = _lib.Scene(*self.w.args, range_=self.w.range, seed=0, device=0)
        self.bp = BatchPlanner(self.scene)
        self.connect = tuple(_cuda(a) for a in PC.connect_set(O, key)[:2])
        self.star = tuple(_cuda(a) for a in PC.star_set(O, key)[:2])


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    made = {}

    def get(key):
        if key not in made:
            made[key] = Ctx(oracle_mod, key)
        return made[key]
    yield get
    for c in made.values():
        c.scene.close()


# ---------------- 1. RRT-Connect, every build ----------------
# (MOPA_PLAN_BUILD, MOPA_PLAN_NN_CAP, keywords of plan)
BUILDS = [("w1", None, {}), ("w1", "0", {}), ("w1", "64", {}), ("w2", None, {"max_workgroups": -1}), ("wg", None, {}), ("wg", "0", {}),
          ("wg", "64", {}), ("wg", None, {"max_workgroups": 3})]


@pytest.mark.parametrize("key", PC.KEYS, ids=str)
def test_rrt_connect_in_every_build(oracle_mod, ctx, key, monkeypatch, capfd):
    """status, path_len, rows and n_checks of every build equal orc.plan's; the launch line says that the workgroup-per-query build ran
    where it was asked for on up to 8 coordinates, and that it did not on more (the knob falls back there and still agrees)"""
    from mopa_rl_amd import _lib
    c = ctx(key)
    want = PC.connect_ref(oracle_mod, key)
    E = len(want[1])
    monkeypatch.setenv("MOPA_DEBUG", "1")
    for build, cap, kw in BUILDS:
        if key in NO_PLANNER_LDS:
            monkeypatch.setenv("MOPA_PLAN_BUILD", build)
            with pytest.raises(_lib.MopaError, match="error 4: planner LDS does not fit"):
                c.bp.plan(*c.connect, seed=PC.CONNECT_SEED, **PC.CONNECT, **kw)
            assert "plan launch" not in capfd.readouterr().err
            continue
        monkeypatch.setenv("MOPA_PLAN_BUILD", build)
        if cap is None:
            monkeypatch.delenv("MOPA_PLAN_NN_CAP", raising=False)
        else:
            monkeypatch.setenv("MOPA_PLAN_NN_CAP", cap)
        capfd.readouterr()
        got = _np(c.bp.plan(*c.connect, seed=PC.CONNECT_SEED, **PC.CONNECT, **kw))
        err = capfd.readouterr().err
        what = f"{key} {build} cap {cap} {kw}"
        _assert_connect(got, want, what)
        assert f"[mopa] plan launch: {E} queries" in err, (what, err)
        ran_wg = "plan launch (workgroup per query)" in err
        assert ran_wg == (build == "wg" and c.w.na <= 8), (what, err)
        if ran_wg:
            n_wg = int(err.split("(workgroup per query): ")[1].split(" queries, ")[1].split(" workgroups")[0])
            assert n_wg == (3 if kw else E) and (cap is None or f"mirror {cap} nodes" in err), (what, err)
    assert (want[2] == 0).sum() >= 3


# ---------------- 2. keep_state / resume ----------------
@pytest.mark.parametrize("key,first", [(k, f) for k, fs in PC.FIRST_ITERS.items() for f in fs], ids=str)
def test_continuation_of_a_permuted_subset(oracle_mod, ctx, key, first):
    """a launch with `first` iterations, then the unsolved queries in another order through PlanState.rows: together the single launch"""
    c = ctx(key)
    want = PC.connect_ref(oracle_mod, key)
    s, g = c.connect
    prm = dict(seed=PC.CONNECT_SEED, max_nodes=PC.CONNECT["max_nodes"], max_path=PC.CONNECT["max_path"])
    p1 = c.bp.plan(s, g, max_iters=first, keep_state=True, **prm)
    got = _np(p1[:4])
    todo = np.nonzero(got[2] == R.PLAN_NO_EXACT)[0]
    todo = todo[np.random.default_rng(5).permutation(len(todo))]
    if first < 100:
        assert len(todo) >= 4, (key, first, got[2])
    if len(todo):
        idx = _cuda(todo.astype(np.int64))
        p2 = _np(c.bp.plan(s[idx].contiguous(), g[idx].contiguous(), max_iters=PC.CONNECT["max_iters"], resume=p1[4].rows(idx), env_ids=idx, **prm))
        if first < 100:
            assert (p2[2] == 0).sum() >= 3, "the continuation solves queries"
        for a, b in zip(got, p2):
            a[todo] = b
    _assert_connect(got, want, f"{key}: {first} iterations + continuation of {todo.tolist()}")


# ---------------- 3. the race ----------------
@pytest.mark.parametrize("key", PC.KEYS, ids=str)
def test_race_equals_the_reference(oracle_mod, ctx, key):
    from mopa_rl_amd import _lib
    c = ctx(key)
    s, g = c.connect
    if key in NO_PLANNER_LDS:
        with pytest.raises(_lib.MopaError, match="error 4: planner LDS does not fit"):
            c.bp.plan_race(s, g, portfolio=PC.PORTFOLIO, seed=PC.RACE_SEED, **PC.CONNECT)
        return
    want = race_ref.as_arrays(PC.race_reference(oracle_mod, key), PC.CONNECT["max_path"], c.scene.nq)
    got = _np(c.bp.plan_race(s, g, portfolio=PC.PORTFOLIO, want_info=True, seed=PC.RACE_SEED, **PC.CONNECT))
    _assert_race(got, want, str(key))
    E = len(want[1])
    assert ((got[6][:, 0] >= 0) & (got[6][:, 0] <= PC.PORTFOLIO - 1)).all() and (got[6][:, 1] <= want[7]).all() and (got[6][:, 1] >= got[3]).all()
    # a reordered subset under its own ids and seeds: the rows of the full run
    sub = np.array([E - 1, 2, 0, E - 3, 4])
    idx = _cuda(sub.astype(np.int64))
    seeds = _cuda(np.full(len(sub), PC.RACE_SEED, dtype=np.int64))
    part = _np(c.bp.plan_race(s[idx].contiguous(), g[idx].contiguous(), portfolio=PC.PORTFOLIO, want_info=True, seed=999, env_id_base=555, env_ids=idx,
                              seeds=seeds, **PC.CONNECT))
    _assert_race(part, [a[sub] for a in want], f"{key} subset")


# ---------------- 4. RRT* ----------------
STAR = dict(max_iters=PC.STAR_ITERS, max_path=PC.STAR_PATH, seed=PC.STAR_SEED)


@pytest.mark.parametrize("key", PC.KEYS, ids=str)
def test_star_equals_the_reference(oracle_mod, ctx, key):
    """path, length, status, cost and the eight info columns; the threshold / bias variant; one workgroup; a second run"""
    c = ctx(key)
    s, g = c.star
    full = _np(c.bp.plan_star(s, g, want_info=True, **STAR))
    _assert_star(full, PC.star_ref(oracle_mod, key), str(key))
    variant = _np(c.bp.plan_star(s, g, want_info=True, **PC.VARIANT, **STAR))
    _assert_star(variant, PC.star_ref(oracle_mod, key, True), f"{key} threshold 0.15, bias 0.2")
    one = _np(c.bp.plan_star(s, g, want_info=True, max_workgroups=1, **STAR))
    again = _np(c.bp.plan_star(s, g, want_info=True, **STAR))
    for x, y, z in zip(full, one, again):
        assert x.tobytes() == y.tobytes() == z.tobytes()


@pytest.mark.parametrize("key", [22, "long_chain"], ids=str)
def test_star_synthetic_cases(oracle_mod, ctx, key):
    """a tree of 48 nodes that fills up, and a goal whose chain does not fit max_path = 2, on more than 8 coordinates"""
    c = ctx(key)
    cases, sid = PC.star_synthetic(oracle_mod, key)
    for name, (s, g, kw) in cases.items():
        kw = dict(dict(max_path=PC.STAR_PATH, max_nodes=None), **kw)
        want = R.plan_star_batch(c.w.orc, s[None], g[None], c.w.range, PC.STAR_ITERS, kw["max_nodes"], kw["max_path"], seed=PC.STAR_SEED, env_id_base=sid)
        got = _np(c.bp.plan_star(_cuda(s[None].copy()), _cuda(g[None].copy()), max_iters=PC.STAR_ITERS, seed=PC.STAR_SEED, env_id_base=sid,
                                 want_info=True, **kw))
        _assert_star(got, want, f"{key} {name}")
        if name == "full_tree":
            assert got[4][0, 1] == 48 and got[4][0, 7] >= 1
        else:
            assert got[2][0] == R.PLAN_NO_EXACT and got[4][0, 4] >= 1


# ---------------- 5. RRT* under the clearance objective ----------------
@pytest.mark.parametrize("band", PC.CLEAR_BANDS)
@pytest.mark.parametrize("key", list(PC.CLEAR_QUERIES), ids=str)
def test_star_clearance_equals_the_reference(oracle_mod, ctx, key, band):
    c = ctx(key)
    s, g = PC.clear_set(oracle_mod, key)
    want = PC.clear_ref(oracle_mod, key, band)
    got = _np(c.bp.plan_star_clearance(_cuda(s), _cuda(g), band, max_iters=PC.CLEAR_ITERS, max_path=PC.STAR_PATH, seed=PC.STAR_SEED, want_info=True,
                                       **PC.VARIANT))
    _assert_clear(got, want, f"{key} band {band}")
    assert (want[2] == 0).any()


# ---------------- 6. K9 ----------------
def _k9_run(bp, level, path, plen, status, **kw):
    """the level's entry on copies of numpy arrays -> (path, plen, info) as numpy"""
    import torch
    if level == 1:
        return _run_shortcut(bp, path, plen, status, **kw)
    if level == 2:
        return _run_smooth(bp, path, plen, status, **kw)
    p, n = _cuda(path), _cuda(plen)
    info = bp.simplify_paths(p, n, _cuda(status), want_info=True, **kw)
    torch.cuda.synchronize()
    return p.cpu().numpy(), n.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("key", PC.KEYS, ids=str)
def test_k9_stand_alone_on_the_oracles_paths(oracle_mod, ctx, key):
    """rows up to the new length, lengths and every info column of the three levels; skipped paths keep their bytes"""
    from mopa_rl_amd import _lib
    c = ctx(key)
    path, plen, status, _ = PC.connect_ref(oracle_mod, key)
    skipped = [e for e in range(len(plen)) if status[e] != 0 or plen[e] < 3]
    for level in (0, 1, 2):
        want = PC.k9_ref(oracle_mod, key, level)
        if level == 2 and key in NO_PLANNER_LDS:
            with pytest.raises(_lib.MopaError, match=r"error 2: path smoothing: max_path beyond what the per-wave LDS lists hold \(0\)"):
                _k9_run(c.bp, level, path, plen, status, seed=PC.K9_SEED, passes=PC.K9[level][1])
            continue
        got = _k9_run(c.bp, level, path, plen, status, seed=PC.K9_SEED, passes=PC.K9[level][1])
        _assert_rows(got[0], got[1], want[0], want[1], f"{key} level {level}")
        assert np.array_equal(got[2], want[2]), f"{key} level {level}: info differs\n{got[2]}\n{want[2]}"
        for e in skipped:
            assert np.array_equal(_bits(got[0][e]), _bits(path[e])) and got[1][e] == plen[e] and not got[2][e].any(), (key, level, e)
        assert (want[1] != plen).any()


@pytest.mark.parametrize("planner", ["plan", "plan_race", "plan_star"])
@pytest.mark.parametrize("key", [3, 22], ids=str)
def test_k9_switches_behind_a_launch(ctx, key, planner):
    """the three switches behind a planner launch = the stand-alone pass on that launch's own output (the race: with the winners' seeds)"""
    import torch
    from mopa_rl_amd.batch import k9_entry, k9_passes
    c = ctx(key)
    s, g = c.star if planner == "plan_star" else c.connect
    prm = {"plan": dict(seed=PC.CONNECT_SEED, **PC.CONNECT), "plan_race": dict(seed=PC.RACE_SEED, portfolio=PC.PORTFOLIO, **PC.CONNECT),
           "plan_star": STAR}[planner]
    launch = getattr(c.bp, planner)
    base = launch(s, g, **prm)
    torch.cuda.synchronize()
    assert int(((base[2] == 0) & (base[1] >= 3)).sum()) >= 4
    changed = 0
    for flags in (dict(vertex_simplify=True), dict(vertex_simplify=True, path_shortcut=True), dict(vertex_simplify=True, path_shortcut=True, path_smooth=True)):
        sw = (flags.get("vertex_simplify", False), flags.get("path_shortcut", False), flags.get("path_smooth", False))
        path, plen = base[0].clone(), base[1].clone()
        getattr(c.bp, k9_entry(*sw))(path, plen, base[2], seed=prm["seed"], seeds=base[5] if planner == "plan_race" else None,
                                      passes=k9_passes(sw[0], 3, sw[1], sw[2]))
        got = _np(launch(s, g, **flags, **prm))
        want = _np((path, plen))
        _assert_rows(got[0], got[1], want[0], want[1], f"{key} {planner} {flags}")
        for a, b in zip(got[2:], _np(base[2:])):
            assert a.tobytes() == b.tobytes(), "status, counts, cost, winner stay the planner's"
        changed += int(not torch.equal(path, base[0]))
    assert changed == 3, "a K9 level changed nothing"


# ---------------- 7. the single-query host forms ----------------
@pytest.mark.parametrize("key", [22, "one_active"], ids=str)
def test_single_query_forms_equal_their_batch_rows(oracle_mod, ctx, key):
    c = ctx(key)
    s, g, names = PC.connect_set(oracle_mod, key)
    want = PC.connect_ref(oracle_mod, key)
    races = PC.race_reference(oracle_mod, key)
    for e in (0, 3, len(names) - 1, len(names) - 2):
        st, rows, chk = c.scene.plan(s[e], g[e], PC.CONNECT["max_iters"], PC.CONNECT["max_nodes"], PC.CONNECT["max_path"], seed=PC.CONNECT_SEED, env_id=e)
        assert (st, chk, len(rows)) == (want[2][e], want[3][e], want[1][e]) and np.array_equal(_bits(rows), _bits(want[0][e, :want[1][e]])), (key, e)
        st, rows, chk, win, wseed, info = c.scene.plan_race(s[e], g[e], PC.PORTFOLIO, PC.CONNECT["max_iters"], PC.CONNECT["max_nodes"],
                                                            PC.CONNECT["max_path"], seed=PC.RACE_SEED, env_id=e)
        r = races[e]
        assert (st, chk, win, wseed, int(info[2])) == (r.status, r.n_checks, r.winner, r.win_seed, r.iters), (key, e)
        assert np.array_equal(_bits(rows), _bits(r.rows))
    s, g, names = PC.star_set(oracle_mod, key)
    ref = PC.star_ref(oracle_mod, key)
    for e in (0, 4, len(names) - 1, len(names) - 2):
        st, rows, cost, info = c.scene.plan_star(s[e], g[e], PC.STAR_ITERS, max_path=PC.STAR_PATH, seed=PC.STAR_SEED, env_id=e)
        assert st == ref[2][e] and np.array_equal(_bits(rows), _bits(ref[0][e, :ref[1][e]])) and np.array_equal(info, ref[4][e]), (key, e)
        assert np.array_equal(_bits([cost]), _bits([ref[3][e]]))


# ---------------- 8. capacities and refusals ----------------
# key -> (mopa_simplify_paths_max_path, mopa_shortcut_paths_max_path, mopa_smooth_paths_max_path) of the library of commit 8ea59a7
# ("Tests: servo dynamics and IK on random body trees; pin host limits"), read off on an MI355X
PARENT_CAPS = {"full": (3866, 1431, 0), "small_entry_cap": (3893, 1443, 0), "slab_centres": (4886, 1815, 117), "crowded_owner": (5820, 2174, 1693),
               "long_chain": (5424, 2006, 806), "one_active": (6487, 2424, 1970), "no_pairs": (6580, 2460, 2068)}
REFUSAL = ("path simplification: max_path beyond", "path shortcutting: max_path beyond", "path smoothing: max_path beyond")


@pytest.mark.parametrize("key", PC.CAPACITY_KEYS, ids=str)
def test_k9_capacities_are_the_parents(oracle_mod, ctx, key):
    """the three capacities guard the LDS layouts (they are not re-derived here): strictly ordered, a launch at the capacity (at 4096
    where it is larger) equals the reference on two short paths, one row more is refused before anything is launched"""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    import simplify_ref
    c = ctx(key)
    w = c.w
    L = _lib.lib()
    h = c.scene.handle
    caps = (L.mopa_simplify_paths_max_path(h), L.mopa_shortcut_paths_max_path(h), L.mopa_smooth_paths_max_path(h))
    print(key, "capacities", caps)
    assert caps == PARENT_CAPS.get(key), (key, caps)
    assert caps[0] > caps[1] > caps[2]
    # two out-and-back paths of 5 rows along the first free straight line of the sample
    q0, q1 = next((a, b) for a, b in zip(w.good[0::2], w.good[1::2]) if w.free(a, b) and w.dist(a, b) > 0.3)
    rows = simplify_ref.out_and_back(q0, q1, 3, w.act, w.row)[:5]
    entries = (L.mopa_simplify_paths_batch, L.mopa_shortcut_paths_batch, L.mopa_smooth_paths_batch)
    for level, cap in enumerate(caps):
        plen = np.full(2, 5, dtype=np.int32)
        passes = (4 << level) - 1
        if cap >= 5:
            mp = min(cap, 4096)
            path = np.zeros((2, mp, w.orc.nq))
            path[:, :5] = rows
            want = PC.K9[level][0](w.orc, path, plen, None, seed=5, passes=passes)
            p, n = _cuda(path), _cuda(plen)
            info = getattr(c.bp, K9_NAMES[level])(p, n, None, seed=5, passes=passes, want_info=True)
            torch.cuda.synchronize()
            _assert_rows(p.cpu().numpy(), n.cpu().numpy(), want[0], want[1], f"{key} level {level} at max_path {mp}")
            assert np.array_equal(info.cpu().numpy(), want[2])
        else:
            assert cap == 0 and level == 2, "the scene's LDS leaves the smoothing level no room: every max_path is refused"
        # one row more than the capacity (the 5 rows of the paths where there is no capacity): refused by the argument check
        cap1 = max(cap + 1, 5)
        over = torch.zeros(2, cap1, w.orc.nq, dtype=torch.float64, device="cuda")
        over[:, :5] = _cuda(rows)
        n = _cuda(plen)
        rc = entries[level](h, 2, cap1, _ptr(over), _ptr(n), None, 5, 0, None, None, passes, *((16,) if level else ()), None, None)
        assert rc == UNSUPPORTED and REFUSAL[level].encode() in L.mopa_last_error() and f"({cap})".encode() in L.mopa_last_error(), (key, level, rc, L.mopa_last_error())
        torch.cuda.synchronize()
        assert (n.cpu().numpy() == 5).all() and np.array_equal(_bits(over[:, :5].cpu().numpy()), _bits(np.repeat(rows[None], 2, axis=0))), "a refused call launched something"
