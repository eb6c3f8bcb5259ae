"""The scene compiler and the oracle off the four shipped scenes, host side (no GPU): on random body trees and on one directed scene
per decision of the compiler (random_scenes.py) the oracle's FK equals an independent composition, every scene compiles into a save-slot
program in which no body continues from another body's pose, the set reaches the compiler states it is meant to reach (asserted), the
oracle's verdicts are mixed and every pair class decides some state, the states of the exact-route GPU tests hold separated pairs that
gjk_distance answers for; and malformed models -- the ones that used to crash the compiler
included -- are refused with a status and a message by the export and by the create entry points, in this process."""
import copy
import functools
import json
import os

import numpy as np
import pytest

import random_scenes as RS
from contacts_ref import ignored_mask
from test_oracle_fk import _rot, independent_fk
from mopa_rl_amd.mjcf import JNT_FREE, JNT_HINGE, JNT_SLIDE

KEYS = list(RS.DIRECTED) + list(RS.HOST_SEEDS)
N_STATES, SPE = 229, 50
PRIMITIVE_CLASSES = ["plane-sphere", "plane-capsule", "plane-cylinder", "plane-box", "sphere-sphere", "sphere-capsule", "sphere-cylinder",
                     "sphere-box", "capsule-capsule", "capsule-cylinder", "capsule-box", "cylinder-cylinder", "cylinder-box", "box-box"]


def _args(key):
    m, pi = RS.scene(key)
    return m, pi, (m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)


@functools.lru_cache(maxsize=None)
def _export(key):
    from mopa_rl_amd import _lib
    return _lib.k1_export(*_args(key)[2])


def _hdr(ex, field):
    from mopa_rl_amd import _lib
    off = _lib.lib().mopa_scene_hdr_offset(field.encode())
    assert off >= 0, field
    return int(np.frombuffer(ex["hdr"].tobytes()[off:off + 4], dtype=np.int32)[0])


def _ints(ex, field, n):
    o = _hdr(ex, field)
    return ex["ints"][o:o + n]


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        monkeypatch.delenv(k)


# ---------------- the oracle is a usable reference off the shipped scenes ----------------
@pytest.mark.parametrize("key", KEYS)
def test_oracle_fk_matches_independent_composition(key, oracle_mod):
    m, pi, args = _args(key)
    orc = oracle_mod.OracleScene(*args)
    rows = RS.env_rows(pi, 3, 5)
    qa = RS.sample(pi, 3, 5)
    for i in range(3):
        q = RS.full_state(pi, qa[i], rows[i])
        xpos, xquat = orc.fk_bodies(q)
        P, Rw = independent_fk(m, q)
        np.testing.assert_allclose(xpos, P, rtol=0, atol=2e-12)
        for b in range(len(m.body_names)):
            np.testing.assert_allclose(_rot(xquat[b]).as_matrix(), Rw[b].as_matrix(), rtol=0, atol=2e-12)
        gpos, gmat = orc.fk(q)
        for g in range(len(m.geom_type)):
            b = m.geom_body[g]
            np.testing.assert_allclose(gpos[g], P[b] + Rw[b].apply(m.geom_pos[g]), rtol=0, atol=2e-12)
            np.testing.assert_allclose(gmat[g], (Rw[b] * _rot(m.geom_quat[g])).as_matrix(), rtol=0, atol=2e-12)


def test_the_generator_emits_what_it_promises():
    kinds = set()
    for key in KEYS:
        m, pi, _ = _args(key)
        nb = len(m.body_names)
        for b in range(1, nb):                              # depth-first body order
            a = b - 1
            while a > m.body_parent[b]:
                a = m.body_parent[a]
            assert a == m.body_parent[b], key
        assert (np.diff(m.geom_body) >= 0).all() and (np.diff(m.geom_mjid) > 0).all(), key
        static = np.ones(nb, dtype=bool)
        for b in range(1, nb):
            static[b] = m.body_jntnum[b] == 0 and static[m.body_parent[b]]
        for a, b in m.pair_geom:
            assert a != b and m.geom_type[a] <= m.geom_type[b] and not (static[m.geom_body[a]] and static[m.geom_body[b]]), key
            assert m.geom_body[a] != m.geom_body[b] or key == "same_body_pair", key
        np.testing.assert_allclose(np.linalg.norm(m.body_quat, axis=1), 1.0, atol=1e-15)
        np.testing.assert_allclose(np.linalg.norm(m.geom_quat, axis=1), 1.0, atol=1e-15)
        np.testing.assert_allclose(np.linalg.norm(m.jnt_axis, axis=1), 1.0, atol=1e-15)
        assert len(pi.ref_joint_pos_indexes) >= 1
        assert all(m.jnt_type[list(m.jnt_qposadr).index(a)] in (JNT_HINGE, JNT_SLIDE) for a in pi.ref_joint_pos_indexes)
        if isinstance(key, int):
            assert not np.array_equal(m.geom_mjid, np.arange(len(m.geom_mjid))) or len(m.geom_mjid) < 4
            again = RS.random_scene(key)[0]
            assert again.to_json() == m.to_json()          # deterministic from the seed
            kinds |= {"two joints"} if (m.body_jntnum == 2).any() else set()
            kinds |= {"welded inside"} if any(m.body_jntnum[b] == 0 and not static[b] for b in range(1, nb)) else set()
            kinds |= {"ref"} if (m.jnt_ref != 0).any() else set()
            kinds |= {"anchor"} if (m.jnt_pos != 0).any() else set()
            kinds |= {"centred"} if any((m.jnt_pos[j] == 0).all() for j in range(len(m.jnt_type)) if m.jnt_type[j] != JNT_FREE) else set()
            kinds |= {f"free{int((m.jnt_type == JNT_FREE).sum())}"}
            kinds |= {"tilted plane"} if any(t == 0 and m.geom_body[g] != 0 for g, t in enumerate(m.geom_type)) else set()
            kinds |= {"ignored"} if pi.ignored_contacts else set()
            kinds |= {"passive hinge"} if any(m.jnt_type[j] != JNT_FREE and m.jnt_qposadr[j] in pi.passive_joint_idx for j in range(len(m.jnt_type))) else set()
            kinds |= {f"type{int(t)}" for t in m.geom_type}
    assert kinds >= {"two joints", "welded inside", "ref", "anchor", "centred", "free0", "free1", "free2", "tilted plane", "ignored", "passive hinge",
                     "type0", "type2", "type3", "type5", "type6"}


# ---------------- every scene compiles, and into a right save-slot program ----------------
def slot_violations(ex):
    """the bodies that would continue from a wrong pose: mb_load -2 = the parent is static, -1 = the parent is body k - 1, s >= 0 = slot s,
    which must hold the parent at that point of the walk"""
    nmb = _hdr(ex, "nmb")
    par, load, save = (_ints(ex, f, nmb) for f in ("o_mb_parent", "o_mb_load", "o_mb_save"))
    slot, bad = {}, []
    for k in range(nmb):
        if load[k] == -2:
            ok = par[k] < 0
        elif load[k] == -1:
            ok = par[k] == k - 1
        else:
            ok = 0 <= load[k] < _hdr(ex, "n_save") and slot.get(int(load[k])) == par[k]
        if not ok:
            bad.append(k)
        if save[k] >= 0:
            assert save[k] < _hdr(ex, "n_save")
            slot[int(save[k])] = k
    return bad


@pytest.mark.parametrize("key", KEYS)
def test_compiles_into_a_right_slot_program(key):
    ex = _export(key)                                       # (a refusal raises: no scene may be skipped)
    assert slot_violations(ex) == []
    m, pi, _ = _args(key)
    assert _hdr(ex, "na") == len(pi.ref_joint_pos_indexes) and _hdr(ex, "nq") == m.nq
    # the chains the planner's FK and the wave-per-state kernel walk: root-most moving ancestor first, each item the parent of the next
    nmb = _hdr(ex, "nmb")
    par = _ints(ex, "o_mb_parent", nmb)
    adr, ln = _ints(ex, "o_chain_adr", nmb), _ints(ex, "o_chain_len", nmb)
    items = ex["ints"][_hdr(ex, "o_chain_items"):]
    for k in range(nmb):
        c = items[adr[k]:adr[k] + ln[k]]
        assert c[-1] == k and par[c[0]] < 0 and all(par[c[i + 1]] == c[i] for i in range(len(c) - 1)), (key, k)


def _facts(key):
    ex = _export(key)
    na, nmj = _hdr(ex, "na"), _hdr(ex, "nmj")
    jt, qsrc = _ints(ex, "o_mj_type", nmj), _ints(ex, "o_mj_qsrc", nmj)
    return dict(n_save=_hdr(ex, "n_save"), n_pas_b=_hdr(ex, "n_pas_b"), n_pas_lv=_hdr(ex, "n_pas_lv"), cen_lds=ex["cen_lds"], use_v5=ex["use_v5"],
                cap=_hdr(ex, "v5_ent_cap"), pfk_maxlen=_hdr(ex, "pfk_maxlen"), na=na, nmg=ex["nmg"], npair=_hdr(ex, "npair"),
                so2=int(_ints(ex, "o_act_so2", na).sum()), active_slide=bool(((jt == JNT_SLIDE) & (qsrc < na)).any()),
                n_mesh_pairs=ex["n_mesh_pairs"], fingerprint="%016x" % ex["fingerprint"])


def test_the_set_reaches_the_compiler_states():
    F = {key: _facts(key) for key in KEYS}
    saves = {min(f["n_save"], 3) for f in F.values()}
    assert saves == {0, 1, 2, 3}
    assert F["serial"]["n_save"] == 0 and F["deep_branches"]["n_save"] >= 3
    assert F["tile_posed"]["n_pas_b"] >= 4 and F["tile_posed"]["n_pas_lv"] >= 2
    assert F["no_tile_poses"]["n_pas_b"] == 0 and F["no_tile_poses"]["n_pas_lv"] == 0
    assert F["long_chain"]["pfk_maxlen"] == 0 and all(f["pfk_maxlen"] > 0 or f["nmg"] == 0 for k, f in F.items() if k != "long_chain")
    assert 9 <= F["wide"]["na"] <= 13 and F["wide"]["so2"] >= 1
    assert F["full"]["nmg"] == 64
    assert not F["crowded_owner"]["use_v5"] and not F["far"]["use_v5"]
    assert sum(f["use_v5"] for f in F.values()) >= len(F) - 2         # ... and nothing else turns the third generation off
    assert F["slab_centres"]["use_v5"] and not F["slab_centres"]["cen_lds"] and F["slab_centres"]["n_mesh_pairs"] == 0
    assert F["serial"]["use_v5"] and F["serial"]["cen_lds"]
    assert F["small_entry_cap"]["use_v5"] and F["small_entry_cap"]["cap"] < 1024 and F["serial"]["cap"] == 1024
    assert F["mesh"]["n_mesh_pairs"] > 0
    assert F["no_moving_geoms"]["nmg"] == 0 and F["no_moving_geoms"]["npair"] == 0
    assert F["no_pairs"]["npair"] == 0 and F["no_pairs"]["nmg"] > 0
    assert F["one_active"]["na"] == 1
    assert any(f["so2"] for f in F.values()) and any(f["active_slide"] for f in F.values())
    # why the two scenes lose the third generation: a crowded owner, a far geom
    m, pi, _ = _args("crowded_owner")
    owner = np.maximum(*np.asarray(m.pair_geom).T)
    assert np.bincount(owner).max() > 64
    m, pi, _ = _args("far")
    assert np.abs(m.body_pos).max() > 32.0
    # none of these scenes is a baked one (the baked kernels are fingerprint-gated)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_build.json")) as f:
        recorded = {rec["fingerprint"] for env in json.load(f).values() for rec in env.values()}
    assert not recorded & {f["fingerprint"] for f in F.values()}
    assert len({f["fingerprint"] for f in F.values()}) == len(F)


# ---------------- the sampled states are a mix, and every pair class decides some of them ----------------
def test_state_mix_and_deciding_pair_classes(oracle_mod):
    from mopa_rl_amd.scene import pair_classes
    n_valid = n = 0
    deciding = {}
    for key in KEYS:
        m, pi, args = _args(key)
        orc = oracle_mod.OracleScene(*args)
        rows, qa = RS.env_rows(pi, (N_STATES + SPE - 1) // SPE, 7), RS.sample(pi, N_STATES, 7)
        v, md = orc.is_valid_batch(qa, rows, samples_per_env=SPE, nthreads=0)
        n_valid, n = n_valid + int(v.sum()), n + len(v)
        if not len(m.pair_geom):
            continue
        cls, ign = pair_classes(m), ignored_mask(pi)
        for i in range(0, N_STATES, 4):
            d = orc.pair_dist(RS.full_state(pi, qa[i], rows[i // SPE]))
            d[ign] = 1.0e10
            p = int(d.argmin())
            if d[p] < 0.0:                                  # the pair that sets the state's min_dist
                assert d[p] == md[i]
                deciding[cls[p]] = deciding.get(cls[p], 0) + 1
    print("valid", n_valid, "of", n, "deciding", deciding)
    assert 0.10 * n <= n_valid <= 0.90 * n
    for c in PRIMITIVE_CLASSES + ["plane-mesh"]:
        assert deciding.get(c, 0) >= 1, c
    assert any(c.endswith("-mesh") and not c.startswith("plane") for c in deciding)


# ---------------- the states of the exact-route tests reach the route ----------------
def test_the_exact_route_is_reached(oracle_mod):
    """sequential form alone: per scene of RS.EXACT_KEYS the separated pairs of an inflated class (box-box, cylinder-*, *-mesh) that the
    exact table reports inside the 5 cm band over RS.exact_states -- the pairs gjk_distance answers for -- and, at 1 cm, likewise.  A scene
    without one is listed: at most a quarter of the scenes, and none of the scenes that are there for a reason."""
    import proximity_exact_ref as X
    import proximity_ref as P
    none, tilted = [], []
    for key in RS.EXACT_KEYS:
        m, pi, args = _args(key)
        orc = oracle_mod.OracleScene(*args)
        qa, rows, spe = RS.exact_states(pi)
        assert len(qa) == RS.N_EXACT
        gpos, gmat = P.poses(pi, orc, qa, rows, spe)
        infl = X.inflated_pairs(m)
        n = {}
        for band in X.BANDS:
            De, Di = X.pair_dists(pi, gpos, gmat, band), P.pair_dists(pi, gpos, gmat, band)
            n[band] = int(((De > 0) & (De <= band))[:, infl].sum())
            # the exact table is not the inflated one wherever such a pair is counted, and is the inflated one on every other class
            assert n[band] == 0 or (De.view(np.uint64) != Di.view(np.uint64))[:, infl].any(), (key, band)
            assert np.array_equal(De[:, ~infl].view(np.uint64), Di[:, ~infl].view(np.uint64)), (key, band)
        print(key, "separated pairs of an inflated class in band:", n, "of", int(infl.sum()), "such pairs x", len(qa), "states")
        if n[0.05] == 0:
            none.append(key)
        elif any(t == 0 and m.geom_body[g] != 0 for g, t in enumerate(m.geom_type)):
            tilted.append(key)
    print("scenes without such a pair:", none, "; tilted-plane scenes with one:", tilted)
    assert len(none) <= len(RS.EXACT_KEYS) // 4, none
    assert not {"mesh", "full", "slab_centres"} & set(none) and tilted, (none, tilted)


# ---------------- malformed models are refused, by the export and by scene creation ----------------
def bfs_reorder(m):
    """the same model with its bodies renumbered breadth-first (a parent still comes before its children), geoms kept in body order"""
    nb = len(m.body_parent)
    order, i = [0], 0
    while i < len(order):
        order += [b for b in range(1, nb) if m.body_parent[b] == order[i]]
        i += 1
    new = np.empty(nb, dtype=np.int64)
    new[order] = np.arange(nb)
    m2 = copy.copy(m)
    for k in ("body_pos", "body_quat", "body_jntnum"):
        setattr(m2, k, getattr(m, k)[order])
    m2.body_parent = np.array([new[m.body_parent[b]] if b else 0 for b in order], dtype=np.int32)
    jorder = [j for b in order for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b])]
    for k in ("jnt_type", "jnt_qposadr", "jnt_axis", "jnt_pos", "jnt_ref", "jnt_limited", "jnt_range"):
        setattr(m2, k, getattr(m, k)[jorder])
    m2.jnt_body = np.array([new[m.jnt_body[j]] for j in jorder], dtype=np.int32)
    adr, c = [], 0
    for b in order:
        adr.append(c if m.body_jntnum[b] else -1)
        c += int(m.body_jntnum[b])
    m2.body_jntadr = np.array(adr, dtype=np.int32)
    gb = new[m.geom_body]
    go = np.argsort(gb, kind="stable")
    inv = np.empty(len(go), dtype=np.int64)
    inv[go] = np.arange(len(go))
    for k in ("geom_type", "geom_size", "geom_pos", "geom_quat"):
        setattr(m2, k, getattr(m, k)[go])
    m2.geom_body = gb[go].astype(np.int32)
    pg = inv[np.asarray(m.pair_geom, dtype=np.int64)]
    swap = m2.geom_type[pg[:, 0]] > m2.geom_type[pg[:, 1]]
    pg[swap] = pg[swap][:, ::-1]
    m2.pair_geom = pg.astype(np.int32)
    return m2


def _static_geoms(m):
    nb = len(m.body_names)
    static = np.ones(nb, dtype=bool)
    for b in range(1, nb):
        static[b] = m.body_jntnum[b] == 0 and static[m.body_parent[b]]
    return [g for g in range(len(m.geom_type)) if static[m.geom_body[g]] and m.geom_type[g] != 0]


def _with(m, field, index, value):
    m2 = copy.copy(m)
    a = np.array(getattr(m, field), copy=True)
    a[index] = value
    setattr(m2, field, a)
    return m2


def _add_pair(m, a, b):
    if max(a, b) < len(m.geom_type) and m.geom_type[a] > m.geom_type[b]:
        a, b = b, a
    m2 = copy.copy(m)
    m2.pair_geom = np.vstack([m.pair_geom, [[a, b]]]).astype(np.int32)
    return m2


def _malformed():
    """name -> (model, passive list, status code, a piece of the message)"""
    m, pi = RS.scene("deep_branches")
    pas = pi.passive_joint_idx
    nb, nq = len(m.body_names), m.nq
    st = _static_geoms(m)
    moving = [g for g in range(len(m.geom_type)) if g not in st and m.geom_type[g] != 0]
    last_joint_body = int(np.nonzero(m.body_jntnum)[0][-1])
    out = {
        "static-static pair": (_add_pair(m, st[0], st[1]), pas, 1, "two static geoms"),
        "pair (g, g), g static": (_add_pair(m, st[0], st[0]), pas, 1, "one geom twice"),
        "pair (g, g), g moving": (_add_pair(m, moving[0], moving[0]), pas, 1, "one geom twice"),
        "pair_geom beyond ngeom": (_add_pair(m, moving[0], len(m.geom_type)), pas, 1, "pair_geom out of range"),
        "geom_body beyond nbody": (_with(m, "geom_body", -1, nb + 5), pas, 1, "geom_body out of range"),
        "geom_body negative": (_with(m, "geom_body", 0, -1), pas, 1, "geom_body out of range"),
        "body_parent beyond nbody": (_with(m, "body_parent", nb - 1, nb + 3), pas, 1, "body_parent"),
        "body_parent negative": (_with(m, "body_parent", nb - 1, -1), pas, 1, "body_parent"),
        "body_parent[b] == b": (_with(m, "body_parent", nb - 2, nb - 2), pas, 1, "body_parent"),
        "body_parent[b] > b": (_with(m, "body_parent", nb - 2, nb - 1), pas, 1, "body_parent"),
        "body_jntnum beyond njnt": (_with(m, "body_jntnum", last_joint_body, 50), pas, 1, "body_jntadr + body_jntnum out of range"),
        "body_jntadr beyond njnt": (_with(m, "body_jntadr", last_joint_body, len(m.jnt_type)), pas, 1, "body_jntadr + body_jntnum out of range"),
        "body_jntnum negative": (_with(m, "body_jntnum", last_joint_body, -2), pas, 1, "body_jntadr + body_jntnum out of range"),
        "jnt_qposadr beyond nq": (_with(m, "jnt_qposadr", 0, nq + 3), pas, 1, "jnt_qposadr out of range"),
        "jnt_qposadr negative": (_with(m, "jnt_qposadr", 0, -1), pas, 1, "jnt_qposadr out of range"),
        "bodies breadth-first": (bfs_reorder(m), pas, 2, "bodies are not in depth-first order"),
    }
    free = int(np.nonzero(m.jnt_type == JNT_FREE)[0][0])
    out["free joint with 6 slots left"] = (_with(m, "jnt_qposadr", free, nq - 6), pas, 1, "jnt_qposadr out of range")
    mm, pim = RS.scene("mesh")
    g = int(np.nonzero(mm.geom_type == 7)[0][0])
    out["geom_dataid beyond nmesh"] = (_with(mm, "geom_dataid", g, 5), pim.passive_joint_idx, 1, "without a convex hull")
    out["geom_dataid negative"] = (_with(mm, "geom_dataid", g, -1), pim.passive_joint_idx, 1, "without a convex hull")
    nodes = [RS.node(p, ngeom=8) for p in (-1, 0, 1, 1, 0, 4, 4)] + [RS.node(-1, ngeom=7)]
    m65, pi65 = RS.build("full_plus_one", 107, nodes, n_static=3, n_free=1, free_geoms=2, gscale=0.5, scale=0.3, pair_keep=0.25)
    out["65 moving geoms"] = (m65, pi65.passive_joint_idx, 4, "more than 64 moving collidable geoms")
    return out


MALFORMED = ["static-static pair", "pair (g, g), g static", "pair (g, g), g moving", "pair_geom beyond ngeom", "geom_body beyond nbody",
             "geom_body negative", "body_parent beyond nbody", "body_parent negative", "body_parent[b] == b", "body_parent[b] > b",
             "body_jntnum beyond njnt", "body_jntadr beyond njnt", "body_jntnum negative", "jnt_qposadr beyond nq", "jnt_qposadr negative",
             "bodies breadth-first", "free joint with 6 slots left", "geom_dataid beyond nmesh", "geom_dataid negative", "65 moving geoms"]


def test_the_list_of_malformed_models_is_complete():
    assert sorted(_malformed()) == sorted(MALFORMED)
    m, _ = RS.scene("deep_branches")
    b = bfs_reorder(m)
    assert (b.body_parent[1:] < np.arange(1, len(b.body_parent))).all() and not np.array_equal(b.body_parent, m.body_parent)


@pytest.mark.parametrize("case", MALFORMED)
def test_malformed_models_are_refused(case):
    import ctypes as C
    from mopa_rl_amd import _lib
    model, passive, code, text = _malformed()[case]
    with pytest.raises(_lib.MopaError) as e:
        _lib.k1_export(model, passive, [], RS.CONTACT_THRESHOLD)
    assert str(e.value).startswith(f"libmopa_hip error {code}: ") and text in str(e.value), str(e.value)
    # scene creation compiles on the host before it looks for a device: the same refusal, with or without a GPU
    desc, keep, _, _ = _lib.scene_desc(model, passive, [], RS.CONTACT_THRESHOLD)
    h = C.c_void_p()
    assert _lib.lib().mopa_scene_create(C.byref(desc), C.byref(h)) == code and not h.value
    assert text in _lib.lib().mopa_last_error().decode()
    with pytest.raises(_lib.MopaError) as e:
        _lib.Scene(model, passive, [], RS.CONTACT_THRESHOLD)
    assert str(e.value).startswith(f"libmopa_hip error {code}: ") and text in str(e.value), str(e.value)
