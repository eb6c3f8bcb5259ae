"""The planner cases of planner_cases.py on the CPU: the sequential references alone (the oracle's `plan`, race_ref, rrtstar_ref and
the three K9 references) reach, on scenes that are none of the shipped ones, the branches test_random_planners_gpu.py compares the
kernels on -- so that file cannot pass on empty work -- and every path they return is a path.  Each assertion message names the
counts reached; the counts at the time of writing stand next to the conditions."""
import math

import numpy as np
import pytest

import planner_cases as PC
import rrtstar_ref as R
import smooth_ref
from simplify_ref import dist
from test_star_host import _check_tree


def _changed(before, after):
    """indices of the paths a K9 reference changed (another length, or other bits in the rows that stay)"""
    path, plen = before
    return [e for e in range(len(plen)) if after[1][e] != plen[e] or not np.array_equal(after[0][e, :after[1][e]], path[e, :after[1][e]])]


def test_the_keys_reach_the_scene_dependent_branches(oracle_mod):
    """na on either side of 8 and at 1 and 8, passive coordinates inside the tree, mesh pairs, no pair at all, SO(2) and a slide at
    active index >= 8"""
    from mopa_rl_amd.mjcf import GEOM_MESH, JNT_SLIDE
    w = {k: PC.world(oracle_mod, k) for k in PC.KEYS}
    na = {k: w[k].na for k in PC.KEYS}
    assert na == {"one_active": 1, "serial": 5, "tile_posed": 5, "mesh": 5, 3: 8, "full": 8, "deep_branches": 10, "long_chain": 12, 22: 10,
                  "no_pairs": 3, "slab_centres": 7}, na
    assert w[3].orc.nq == 25 and w["long_chain"].orc.nq == 25 and w["one_active"].orc.nq == 10
    assert len(w["tile_posed"].pi.passive_joint_idx) == 11 and len(w["mesh"].pi.passive_joint_idx) == 16
    m = w["mesh"].m
    assert sum(GEOM_MESH in (m.geom_type[a], m.geom_type[b]) for a, b in m.pair_geom) >= 2
    assert w["no_pairs"].orc.npair == 0 and w["full"].orc.npair == 454 and w["slab_centres"].orc.npair == 428
    assert [i for i, f in enumerate(w[3].so2) if f] == [0, 5] and [i for i, f in enumerate(w[22].so2) if f] == [9] and w["serial"].so2[3]
    m22 = w[22].m
    jtype = lambda m, adr: int(m.jnt_type[[j for j in range(len(m.jnt_type)) if int(m.jnt_qposadr[j]) == int(adr)][0]])
    assert jtype(m22, w[22].act[8]) == JNT_SLIDE
    for k, ww in w.items():
        assert (len(ww.bad) == 0) == (k in PC.FREE_FILL), (k, len(ww.bad))


@pytest.mark.parametrize("key", PC.KEYS, ids=str)
def test_connect_sets_are_what_they_are_named(oracle_mod, key):
    w = PC.world(oracle_mod, key)
    s, g, names = PC.connect_set(oracle_mod, key)
    path, plen, st, chk = PC.connect_ref(oracle_mod, key)
    assert 6 <= len(names) <= 14 and len(names) == len(s)
    n_blocked = 0
    for e, name in enumerate(names):
        a, b = s[e, w.act], g[e, w.act]
        if name == "blocked":
            n_blocked += not w.free(a, b)
        elif name == "seam":
            c = PC.SEAM[key]
            assert a[c] > 2.2 and b[c] < -2.2 and w.valid(a) and w.valid(b)
        elif name == "invalid_goal":
            assert not w.valid(b) and w.valid(a) and st[e] == R.PLAN_INVALID_GOAL
        else:
            assert not w.valid(a) and w.valid(b) and st[e] == R.PLAN_NO_EXACT and plen[e] == 0
    assert n_blocked == (0 if key in PC.FREE_FILL else PC.N_BLOCKED), (key, n_blocked)
    assert (st == 0).sum() >= 3, (key, st.tolist())                      # 4 .. 12 per key
    assert chk.max() > 100


def test_race_cases(oracle_mod):
    """per key >= 3 solved queries (3 on slab_centres, 4 .. 12 elsewhere), an unsolved valid query somewhere (17 over the set), winners
    other than member 0 (38 of 61 solved), a query only another member solves (2)"""
    unsolved = other = rescued = solved = 0
    for key in PC.RACE_KEYS:
        races = PC.race_reference(oracle_mod, key)
        _, _, names = PC.connect_set(oracle_mod, key)
        n = sum(r.status == 0 for r in races)
        assert n >= 3, f"{key}: {n} solved"
        solved += n
        unsolved += sum(r.status == R.PLAN_NO_EXACT and nm in ("blocked", "seam") for r, nm in zip(races, names))
        other += sum(r.winner > 0 for r in races)
        rescued += sum(r.status == 0 and r.members[0].status != 0 for r in races)
        assert [r.status for r, nm in zip(races, names) if nm == "invalid_goal"] == [R.PLAN_INVALID_GOAL]
    assert unsolved >= 1 and other >= 8 and rescued >= 1, f"unsolved {unsolved}, winner != 0 in {other} of {solved} solved, rescued {rescued}"
    print(f"race: solved {solved}, unsolved {unsolved}, winner != 0 {other}, solved by another member only {rescued}")


def test_star_cases(oracle_mod):
    """per key a solved query and a rewire; over the set both statuses, a descendant update, and under the variant a query with two
    goal nodes"""
    statuses, desc, two_goals, counts = set(), 0, 0, {}
    for key in PC.KEYS:
        path, plen, st, cost, info, res = PC.star_ref(oracle_mod, key)
        _, _, names = PC.star_set(oracle_mod, key)
        real = np.array([nm in ("near", "seam") for nm in names])
        assert (st[real] == 0).any(), f"{key}: no solved query"
        assert info[:, 3].sum() >= 1, f"{key}: no rewire"
        statuses |= set(st[real].tolist())
        desc += int(info[:, 6].sum())
        v = PC.star_ref(oracle_mod, key, True)
        two_goals += int((v[4][:, 4] >= 2).sum())
        counts[key] = (int((st == 0).sum()), int(info[:, 3].sum()))
        assert ((info[:, 5] >= 0) == (st == 0)).all() and (info[real, 0] == PC.STAR_ITERS).all()
    assert statuses == {R.PLAN_OK, R.PLAN_NO_EXACT}, statuses
    assert desc >= 1 and two_goals >= 1, (desc, two_goals)
    print(f"RRT*: (solved, rewires) per key {counts}; descendant updates {desc}; variant queries with >= 2 goal nodes {two_goals}")


@pytest.mark.parametrize("key", [22, "long_chain"], ids=str)
def test_star_synthetic_cases_on_more_than_8_coordinates(oracle_mod, key):
    w = PC.world(oracle_mod, key)
    assert w.na > 8
    cases, e = PC.star_synthetic(oracle_mod, key)
    s, g, kw = cases["full_tree"]
    full = R.plan_star(w.orc, s, g, w.range, PC.STAR_ITERS, max_path=PC.STAR_PATH, seed=PC.STAR_SEED, stream_id=e, **kw)
    assert full.info[1] == 48 and full.info[7] >= 1, f"{key}: nodes {full.info[1]}, iterations on a full tree {full.info[7]}"
    _check_tree(w.orc, full, s)
    s, g, kw = cases["short_max_path"]
    short = R.plan_star(w.orc, s, g, w.range, PC.STAR_ITERS, seed=PC.STAR_SEED, stream_id=e, **kw)
    assert short.status == R.PLAN_NO_EXACT and short.info[4] >= 1 and len(short.rows) == 0, "a goal node exists, its chain has more than 2 rows"


def test_each_k9_level_changes_paths(oracle_mod):
    """per key and level a path that changes; over the set splices (level 1), moved vertices and dropped midpoints (level 2)"""
    splices = moved = dropped = 0
    for key in PC.RACE_KEYS:
        path, plen, st, _ = PC.connect_ref(oracle_mod, key)
        for level in (0, 1, 2):
            k = PC.k9_ref(oracle_mod, key, level)
            n = len(_changed((path, plen), k))
            assert n >= 1, f"{key} level {level}: no path changes"
            skipped = [e for e in range(len(plen)) if st[e] != 0 or plen[e] < 3]
            for e in skipped:
                assert k[1][e] == plen[e] and not k[2][e].any() and np.array_equal(k[0][e], path[e])
        splices += int(PC.k9_ref(oracle_mod, key, 1)[2][:, 3].sum())
        info = PC.k9_ref(oracle_mod, key, 2)[2]
        moved, dropped = moved + int(info[:, 7].sum()), dropped + int(info[:, 8].sum())
    assert splices >= 1 and moved >= 1 and dropped >= 1, f"splices {splices}, moved {moved}, dropped {dropped}"
    print(f"K9: splices {splices}, vertices moved {moved}, midpoints dropped {dropped}")


def _seam_steps(w, rows, c):
    return int((np.abs(np.diff(rows[:, w.act[c]])) > math.pi).sum())


def test_seed_22_paths_cross_the_seam_at_active_index_9(oracle_mod):
    w = PC.world(oracle_mod, 22)
    _, _, names = PC.connect_set(oracle_mod, 22)
    path, plen, st, _ = PC.connect_ref(oracle_mod, 22)
    smooth = PC.k9_ref(oracle_mod, 22, 2)
    races = PC.race_reference(oracle_mod, 22)
    seam = [e for e, nm in enumerate(names) if nm == "seam"]
    assert len(seam) == PC.N_SEAM and all(st[e] == 0 for e in seam) and all(races[e].status == 0 for e in seam), (st[seam], [races[e].status for e in seam])
    for e in seam:
        assert _seam_steps(w, path[e, :plen[e]], 9) >= 1, f"query {e}: the planner's path does not cross the seam"
        assert _seam_steps(w, smooth[0][e, :smooth[1][e]], 9) >= 1, f"query {e}: the smoothed path does not cross the seam"
        assert _seam_steps(w, races[e].rows, 9) >= 1
    # RRT* on the same pairs: solved ones cross as well
    _, sl, sst, _, _, _ = PC.star_ref(oracle_mod, 22, True)
    sp = PC.star_ref(oracle_mod, 22, True)[0]
    _, _, snames = PC.star_set(oracle_mod, 22)
    sseam = [e for e, nm in enumerate(snames) if nm == "seam" and sst[e] == 0]
    assert len(sseam) >= 3 and all(_seam_steps(w, sp[e, :sl[e]], 9) >= 1 for e in sseam), sseam


def test_the_comparison_can_fail(oracle_mod):
    """the references of seed 22's seam queries with so2 = all False, and with deep_branches' sample bounds (10 coordinates as well),
    give other rows"""
    w = PC.world(oracle_mod, 22)
    s, g, names = PC.star_set(oracle_mod, 22)
    ref = PC.star_ref(oracle_mod, 22, True)
    seam = [e for e, nm in enumerate(names) if nm == "seam"]
    no_wrap = [False] * w.na
    other = R.sample_bounds(PC.world(oracle_mod, "deep_branches").m, PC.world(oracle_mod, "deep_branches").orc.active_idx)
    assert other != R.sample_bounds(w.m, w.orc.active_idx)
    n_so2 = n_bounds = 0
    for e in seam:
        kw = dict(max_path=PC.STAR_PATH, seed=PC.STAR_SEED, stream_id=e, **PC.VARIANT)
        a = R.plan_star(w.orc, s[e], g[e], w.range, PC.STAR_ITERS, so2=no_wrap, **kw)
        b = R.plan_star(w.orc, s[e], g[e], w.range, PC.STAR_ITERS, bounds=other, **kw)
        want = ref[0][e, :ref[1][e]]
        n_so2 += not (len(a.rows) == len(want) and np.array_equal(a.rows, want))
        n_bounds += not (len(b.rows) == len(want) and np.array_equal(b.rows, want))
    assert n_so2 == len(seam) and n_bounds == len(seam), (n_so2, n_bounds)
    # K9: the smoothing of the oracle's seam paths without the wrap (rows and info columns: paths that end as start -> goal differ in
    # their counts only)
    cs, cg, cnames = PC.connect_set(oracle_mod, 22)
    path, plen, st, _ = PC.connect_ref(oracle_mod, 22)
    want = PC.k9_ref(oracle_mod, 22, 2)
    n_k9 = 0
    for e in [e for e, nm in enumerate(cnames) if nm == "seam"]:
        sm = smooth_ref.SmoothSimplifier(w.orc, path[e, :plen[e]], PC.K9_SEED, e, 0.005, no_wrap, path.shape[1])
        sm.run(15, 16)
        out = sm.result_rows()
        n_k9 += not (len(out) == want[1][e] and np.array_equal(out, want[0][e, :want[1][e]]) and tuple(want[2][e]) == tuple(sm.info()))
    assert n_k9 >= 1, n_k9
    print(f"so2 off changes {n_so2} of {len(seam)} RRT* seam queries, foreign bounds {n_bounds}, smoothing without the wrap {n_k9}")


@pytest.mark.parametrize("key", PC.KEYS, ids=str)
def test_every_returned_path_is_a_path(oracle_mod, key):
    """endpoints exact (or within the goal threshold), every segment passes check_motion, passive columns are the start row's"""
    w = PC.world(oracle_mod, key)
    passive = np.setdiff1d(np.arange(w.orc.nq), w.act)

    def check(rows, start, goal, threshold=0.0, what=""):
        assert len(rows) >= 2 and np.array_equal(rows[0], start), what
        d = dist(rows[-1, w.act], goal[w.act], w.so2)
        assert d <= threshold and (threshold > 0 or np.array_equal(rows[-1, w.act], goal[w.act])), (what, d)
        for k in range(len(rows) - 1):
            assert w.orc.check_motion(start, rows[k, w.act], rows[k + 1, w.act])[0], f"{what}: segment {k} fails the motion check"
        assert np.array_equal(rows[:, passive], np.repeat(start[None, passive], len(rows), axis=0)), what
    n = 0
    s, g, _ = PC.connect_set(oracle_mod, key)
    path, plen, st, _ = PC.connect_ref(oracle_mod, key)
    outs = [("plan", path, plen, st)]
    if key in PC.RACE_KEYS:
        races = PC.race_reference(oracle_mod, key)
        outs += [(f"K9 level {lv}",) + tuple(PC.k9_ref(oracle_mod, key, lv)[:2]) + (st,) for lv in (0, 1, 2)]
        for e, r in enumerate(races):
            if r.status == 0:
                check(r.rows, s[e], g[e], what=f"{key} race {e}")
                n += 1
    for what, p, l, status in outs:
        for e in np.nonzero(status == 0)[0]:
            check(p[e, :l[e]], s[e], g[e], what=f"{key} {what} {e}")
            n += 1
    s, g, _ = PC.star_set(oracle_mod, key)
    for variant in (False, True):
        p, l, status, cost, info, res = PC.star_ref(oracle_mod, key, variant)
        for e in np.nonzero(status == 0)[0]:
            check(p[e, :l[e]], s[e], g[e], PC.VARIANT["goal_threshold"] if variant else 0.0, f"{key} RRT* {variant} {e}")
            n += 1
        if key in ("deep_branches", "long_chain"):
            for e, r in enumerate(res):
                if r.tree is not None:
                    _check_tree(w.orc, r, s[e])
    assert n >= 6, n


# na -> the smallest n with k_of(na, n) > 64, the neighbours a wave holds: n + 1 > exp(64 / (1.1 e (1 + 1 / na))); no tree a launch
# can hold reaches it from two coordinates on
FIRST_N_BEYOND_64 = {1: 44442, 2: 1574208, 3: 9369038, 4: 27319623, 5: 55760649, 6: 92822117, 7: 136032979, 8: 183125859, 9: 232291889,
                     10: 282188584, 11: 331864351, 12: 380669200}


def test_k_table_of_the_library_is_pythons_for_1_to_12_coordinates():
    """mopa_plan_star_k(na, n, 1.1) = rrtstar_ref.k_of(na, n) for n = 1 .. 4097 and on either side of the first n beyond 64 neighbours"""
    from mopa_rl_amd import _lib
    L = _lib.lib()
    for na in range(1, 13):
        for n in range(1, 4098):
            assert L.mopa_plan_star_k(na, n, R.REWIRE_FACTOR) == R.k_of(na, n), (na, n)
        n = FIRST_N_BEYOND_64[na]
        assert n == int(math.exp(64.0 / R.k_rrt(na)))
        got = (L.mopa_plan_star_k(na, n - 1, R.REWIRE_FACTOR), L.mopa_plan_star_k(na, n, R.REWIRE_FACTOR))
        assert got == (R.k_of(na, n - 1), R.k_of(na, n)) == (R.K_MAX, R.K_MAX + 1), (na, n, got)
