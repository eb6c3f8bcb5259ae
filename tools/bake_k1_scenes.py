#!/usr/bin/env python3
"""Bake committed scenes into k_is_valid_v5: writes mopa_rl_amd/csrc/mopa_valid_v5_baked.inc (committed, generated source).

Each scene is loaded the way the library's callers load it (scene.planner_inputs + _lib.Scene's pair pruning and cull
radii), the host half of mopa_scene_create runs on it (mopa_scene_k1_export: no device), and what k_is_valid_v5 reads
of the FP32 pair table and of the moving-body program (forward kinematics) goes into a traits struct as compile-time
constants, with the scene's fingerprint (FNV-1a over both blobs, the pair table and the header).  mopa_scene_create
launches the baked instantiation only for a scene whose fingerprint matches; every other scene -- the full-pair-list sibling (Scene.full), other thresholds, custom scenes --
keeps the generic kernel.  The output depends on nothing but the inputs: two runs give the same bytes.

    python tools/bake_k1_scenes.py [--out PATH]      (then rebuild: make -C mopa_rl_amd/csrc)
"""
from __future__ import annotations

import argparse
import hashlib
import os
import struct
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

# the scene tables must not depend on A/B knobs of the caller's environment (MOPA_V5_*, MOPA_PRUNE_PAIRS, ...)
for _k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
    del os.environ[_k]

from mopa_rl_amd import _lib  # noqa: E402
from mopa_rl_amd.scene import ENV_SPECS, SCENE_DIR, planner_inputs  # noqa: E402

OUT = os.path.join(ROOT, "mopa_rl_amd", "csrc", "mopa_valid_v5_baked.inc")
# (env, traits name): the headline scene.  A scene is added here only once its baked kernel has been measured no slower
# than the generic one (tools/scene_bench.py).
SCENES = [("SawyerPushObstacle-v0", "K1Baked_SawyerPushObstacle")]
# tiles per narrow-phase drain (TR::kTilesPerDrain; scenes not named: 1).  2 only where the pair drain has been measured faster
# than 1 on the bench batch (DESIGN.md "Pair drain").
TILES_PER_DRAIN = {"SawyerPushObstacle-v0": 2}


def fnv1a64(chunks) -> int:
    f = 0xCBF29CE484222325
    for b in chunks:
        for x in b:
            f = ((f ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return f


def fingerprint(ex: dict) -> int:
    """The library's k1_fingerprint restated: the header's last three doubles (range, resolution, nn_eps: planner fields)
    hashed as zeros."""
    hdr = bytearray(ex["hdr"].tobytes())
    hdr[-24:] = bytes(24)
    return fnv1a64([ex["dbl"].tobytes(), ex["ints"].tobytes(), ex["tab"].tobytes(), bytes(hdr)])


def scene_args(env: str):
    pi = planner_inputs(env)
    return pi, (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)


class Unsupported(Exception):
    """The scene is outside what the baked kernel supports: it keeps the generic one."""


J_FREE, J_SLIDE, J_HINGE = 0, 2, 3


def hdr_int(ex: dict, field: str) -> int:
    """An int field of the exported header, at the offset the library reports for it (offsetof, not restated here)."""
    off = _lib.lib().mopa_scene_hdr_offset(field.encode())
    if off < 0:
        raise KeyError(f"SceneHdr has no field {field!r}")
    return int(ex["hdr"][off: off + 4].view("<i4")[0])


def hdr_double(ex: dict, field: str) -> float:
    off = _lib.lib().mopa_scene_hdr_offset(field.encode())
    if off < 0:
        raise KeyError(f"SceneHdr has no field {field!r}")
    return float(ex["hdr"][off: off + 8].view("<f8")[0])


def fk_program(ex: dict) -> dict:
    """The moving-body program of k_is_valid_v5's phase 1, read from the exported blobs (the bytes the fingerprint covers):
    per body its record of the packed int blob and its 14 doubles (as 64-bit patterns), per moving geom its local pose, the
    static frames, the active values' references and the passive coordinates' qpos addresses.  Raises Unsupported for a
    scene the baked walk does not cover."""
    if not (ex["use_v5"] and ex["cen_lds"]):
        raise Unsupported("not a scene of the baked instantiation (third-generation kernel, centres in LDS)")
    if ex["n_mesh_pairs"] != 0:
        raise Unsupported(f"{ex['n_mesh_pairs']} mesh pairs (the baked instantiation has no mesh gate)")
    H = {f: hdr_int(ex, f) for f in ("na", "nq", "n_pq", "nmb", "nmg", "nsf", "n_save", "n_pas_b", "n_dbl", "n_int", "o_mbr", "o_mbd",
                                     "o_mgd", "o_sf_pos", "o_sf_quat", "o_sf_mat", "o_act_ref", "o_pq_adr")}
    ints, bits = ex["ints"].astype("<i4"), ex["dbl"].astype("<f8").view("<u8")
    if H["n_dbl"] != len(bits) or H["n_int"] != len(ints) or H["nmg"] != ex["nmg"]:
        raise Unsupported("header does not describe the exported blobs")
    na, nmb, nmg, n_pq, n_save = H["na"], H["nmb"], H["nmg"], H["n_pq"], H["n_save"]
    if na > 8:
        raise Unsupported(f"{na} active values (the walk's hoisted sines cover 8)")
    if H["n_pas_b"] > 0:
        raise Unsupported(f"{H['n_pas_b']} tile-posed bodies (phase 0 is not baked)")
    pq_adr = [int(x) for x in ints[H["o_pq_adr"]: H["o_pq_adr"] + n_pq]]
    bodies, bd = [], []
    for k in range(nmb):
        jn, _jntadr, load, sf, save, mgadr, mgnum, w = (int(x) for x in ints[H["o_mbr"] + 8 * k: H["o_mbr"] + 8 * k + 8])
        jt, jp0, src = w & 0x7F, (w >> 7) & 1, w >> 8
        if jn > 1:
            raise Unsupported(f"moving body {k} has {jn} joints (the baked walk takes one at most)")
        if jn == 1 and jt not in (J_FREE, J_SLIDE, J_HINGE):
            raise Unsupported(f"moving body {k}: joint type {jt}")
        if jn == 1 and jt == J_FREE and not (src >= na and src - na + 7 <= n_pq
                                             and pq_adr[src - na: src - na + 7] == list(range(pq_adr[src - na], pq_adr[src - na] + 7))):
            raise Unsupported(f"moving body {k}: free joint coordinates not contiguous")
        if jn == 1 and not 0 <= src < na + n_pq:
            raise Unsupported(f"moving body {k}: value slot {src}")
        if not (load >= -2 and load < n_save and save < n_save and (load != -2 or 0 <= sf < H["nsf"]) and (k > 0 or load == -2 or jt == J_FREE)
                and 0 <= mgadr and mgadr + mgnum <= nmg):
            raise Unsupported(f"moving body {k}: record {[jn, load, sf, save, mgadr, mgnum]} out of range")
        bodies.append([load, sf, save, mgadr, mgnum, jn, jt, jp0, src])
        bd.append([int(x) for x in bits[H["o_mbd"] + 16 * k: H["o_mbd"] + 16 * k + 14]])
    gd = [[int(x) for x in bits[H["o_mgd"] + 8 * m: H["o_mgd"] + 8 * m + 7]] for m in range(nmg)]
    sf = [[int(x) for x in bits[H["o_sf_pos"] + 3 * i: H["o_sf_pos"] + 3 * i + 3]] + [int(x) for x in bits[H["o_sf_quat"] + 4 * i: H["o_sf_quat"] + 4 * i + 4]]
          + [int(x) for x in bits[H["o_sf_mat"] + 9 * i: H["o_sf_mat"] + 9 * i + 9]] for i in range(H["nsf"])]
    act_ref = [int(x) for x in bits[H["o_act_ref"]: H["o_act_ref"] + na]]
    return {"na": na, "nq": H["nq"], "nmb": nmb, "n_pq": n_pq, "n_save": n_save, "bodies": bodies, "bd": bd, "gd": gd, "sf": sf, "act_ref": act_ref, "pq_adr": pq_adr}


RESIDENT_CLASSES = (4, 5, 8)      # PC_SPHERE_SPHERE, PC_SPHERE_CAPSULE, PC_CAPSULE_CAPSULE: closed-form routines of a few dozen operations
RESIDENT_MAX = 2
RESIDENT_MIN_SURVIVAL = 0.75
RESIDENT_SAMPLE, RESIDENT_SEED = 2048, 20


def resident_sample(pi, env: str, n: int, seed: int):
    """Full qpos rows of the seeded sample behind the residency choice: active joints half uniform in the joint box, half near
    the initial pose; gripper slides uniform in their range and the free-jointed object at its nominal pose + U(+-0.05) in xy
    (the passive block of bench.make_inputs, drawn per state)."""
    from mopa_rl_amd.scene import default_qpos
    m = pi.model
    rng = np.random.default_rng(seed)
    row = default_qpos(env, m)
    act = np.asarray(pi.ref_joint_pos_indexes)
    lo, hi = np.asarray(pi.jnt_minimum), np.asarray(pi.jnt_maximum)
    q = np.repeat(row[None], n, axis=0)
    qa = rng.uniform(lo, hi, size=(n, len(act)))
    qa[n // 2:] = np.clip(row[act] + rng.normal(0.0, 0.3, size=(n - n // 2, len(act))), lo, hi)
    q[:, act] = qa
    for name in ("rc_close", "lc_close"):
        if name in m.jnt_names:
            j = m.joint_name2id(name)
            a, (r0, r1) = int(m.jnt_qposadr[j]), m.jnt_range[j]
            q[:, a] = rng.uniform(r0, r1, size=n)
    free = [int(m.jnt_qposadr[j]) for j in range(len(m.jnt_names)) if int(m.jnt_type[j]) == J_FREE]
    if free:
        q[:, free[0]: free[0] + 2] += rng.uniform(-0.05, 0.05, size=(n, 2))
    return q


def moving_pairs(ex: dict, tab, padr, nmov):
    """The table's moving-moving entries: (owner slot M, entry K of the owner, partner slot, pair class, owner is geom 2)."""
    out = []
    for m in range(ex["nmg"]):
        for k in range(nmov[m]):
            fl = int(tab[8 * (padr[m] + k) + 7])
            assert (fl >> 13) & 1, "an entry of the moving group without a moving partner"
            out.append((m, k, (fl >> 14) & 0xFF, (fl >> 8) & 0xF, (fl >> 12) & 1))
    return out


def survival_rates(pi, ex: dict, tab, padr, pairs, q):
    """Share of the states `q` (full qpos rows) in which pass A's sphere test keeps each of `pairs`: the oracle's geom
    centres rounded to FP32 against the table's own FP32 squared cull radius."""
    from oracle import oracle as O
    orc = O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    o = hdr_int(ex, "o_mg_geom")
    mg = [int(g) for g in ex["ints"][o: o + ex["nmg"]]]
    cen = np.stack([orc.fk(row)[0][mg] for row in q]).astype(np.float32)       # [n][nmg][3]
    rates = []
    for (m, k, ps, _code, _g2) in pairs:
        rs2 = np.float32(tab[8 * (padr[m] + k) + 3: 8 * (padr[m] + k) + 4].view("<f4")[0])
        d = cen[:, m] - cen[:, ps]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        rates.append(float(np.count_nonzero(~(d2 > rs2))) / len(q))
    return rates


def resident_pairs(env: str, pi, ex: dict, fk: dict, tab, padr, nmov) -> list:
    """The scene's resident pairs (at most RESIDENT_MAX, by survival rate): moving-moving pairs of a closed-form class that pass A
    keeps in at least RESIDENT_MIN_SURVIVAL of a seeded sample of states -- the baked walk evaluates them in place, on full lanes,
    instead of sending them through survivor bit, entry, compaction, gather and batch.  A speed heuristic: residency changes where
    a pair is evaluated, never the result.  (Baked scenes have no tile-posed geoms: fk_program refuses them.)
    Per pair: owner slot M, table entry K, geom slots in routine order (type 1 <= type 2, as v5_flush orders them), class, both
    types, both sizes as 64-bit patterns of the exported blob, survival in percent (rounded down)."""
    # the walk poses the moving geoms in slot order: "first / second posed" below is the smaller / larger slot
    adr = [b[3] for b in fk["bodies"] if b[4] > 0]
    assert adr == sorted(adr), "moving geoms are not posed in slot order"
    cand = [p for p in moving_pairs(ex, tab, padr, nmov) if p[3] in RESIDENT_CLASSES]
    if not cand:
        return []
    rates = survival_rates(pi, ex, tab, padr, cand, resident_sample(pi, env, RESIDENT_SAMPLE, RESIDENT_SEED))
    order = sorted(range(len(cand)), key=lambda i: (-rates[i], cand[i][0], cand[i][1]))
    o_geom, o_rec, o_type = hdr_int(ex, "o_mg_geom"), hdr_int(ex, "o_g_rec"), hdr_int(ex, "o_g_type")
    ints, bits = ex["ints"].astype("<i4"), ex["dbl"].astype("<f8").view("<u8")
    out = []
    for i in order[:RESIDENT_MAX]:
        if rates[i] < RESIDENT_MIN_SURVIVAL:
            break
        m, k, ps, code, owner_is_g2 = cand[i]
        sa, sb = (ps, m) if owner_is_g2 else (m, ps)
        ga, gb = int(ints[o_geom + sa]), int(ints[o_geom + sb])
        ta, tb = int(ints[o_type + ga]), int(ints[o_type + gb])
        assert ta <= tb and sa != sb
        size = [int(x) for x in bits[o_rec + 16 * ga + 12: o_rec + 16 * ga + 15]] + [int(x) for x in bits[o_rec + 16 * gb + 12: o_rec + 16 * gb + 15]]
        out.append({"row": [m, k, sa, sb, code, ta, tb], "size": size, "pct": int(100.0 * rates[i])})
    return out


SPARSE_SAMPLE, SPARSE_SEED = 4096, 29


def sparse_parents(fk: dict) -> list:
    """Parent of every moving body in the walk's program (-1: a static frame, or a free-jointed body, which takes its pose from the
    env row): `load` -1 is the body before, >= 0 the body that last filled that save slot."""
    parent, saved = [], {}
    for k, (load, _sf, save, _mgadr, _mgnum, jn, jt, _jp0, _src) in enumerate(fk["bodies"]):
        if jn == 1 and jt == J_FREE or load == -2:
            parent.append(-1)
        elif load == -1:
            parent.append(k - 1)
        else:
            parent.append(saved[load])
        if save >= 0:
            saved[save] = k
    return parent


def sparse_marks(index: int, env: str, pi, fk: dict, nmg: int, n: int = SPARSE_SAMPLE, seed: int = SPARSE_SEED) -> list:
    """Bodies the baked walk takes in its sparse form (mopa_valid_v5.inc, "Sparse form of the walk").  The sparse walk equals the
    dense one except for the sign of exact zeros, and a state with an exact zero in a stored pose component of a marked body's geom
    runs the dense walk again: a body is marked only if no stored component (position, quaternion) of its geoms, or of the geoms of
    any body below it, is an exact zero in the dense walk (scene #index of the loaded library) anywhere on a seeded sample of
    bench-like states (resident_sample) -- and, more cautious than the guard needs, no entry of the rotation matrix of such a
    quaternion either: an exact zero there is a pose on a structural symmetry (Push: the base bodies, whose axes stay parallel to the
    world's), one step from a stored zero.  Never a free-jointed body: its pose comes from the env row.  The marks are closed
    under descent by construction.  A speed heuristic: the marks change how often the guard trips, never the result."""
    import ctypes as C
    q = resident_sample(pi, env, n, seed)
    qa = np.ascontiguousarray(q[:, np.asarray(pi.ref_joint_pos_indexes)])
    out = np.full((n, nmg, 7), np.nan)
    rc = _lib.lib().mopa_k1_baked_fk_pose_host(index, n, qa.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise SystemExit(f"{env}: the loaded library has no baked scene #{index} to sample the dense walk of (build it first)")
    w, x, y, z = (out[:, :, 3 + i] for i in range(4))
    # (the entries of quat2mat, operation for operation: what the narrow phase forms from a stored quaternion)
    mat = np.stack([((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                    2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x),
                    2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z], axis=-1)
    geom_zero = (out == 0.0).any(axis=(0, 2)) | (mat == 0.0).any(axis=(0, 2))            # [nmg]
    parent = sparse_parents(fk)
    nmb = fk["nmb"]
    zero = [bool(geom_zero[b[3]: b[3] + b[4]].any()) for b in fk["bodies"]]
    for k in range(nmb - 1, -1, -1):                      # a body's zeros count against everything above it
        if parent[k] >= 0 and zero[k]:
            zero[parent[k]] = True
    free = [b[5] == 1 and b[6] == J_FREE for b in fk["bodies"]]
    marks = [not zero[k] and not free[k] for k in range(nmb)]
    assert all(marks[k] or not marks[parent[k]] for k in range(nmb) if parent[k] >= 0), "marks not closed under descent"
    return marks


G_CAPSULE, G_CYLINDER = 3, 5
K_CULL_EPS = np.float32(2.0e-5)                 # kCullEps of mopa_valid_v5.inc
K_AXIS_STEP = np.uint32(0x3A802009).view(np.float32)   # kAxisStep


def axis_extents(ex: dict, tab, padr, nmov, nstat) -> dict:
    """Axis owners of the scene -- moving capsules / cylinders with static non-plane partners -- and what pass A needs to test
    those partners' world AABBs against the owner's per-axis reach r + hl |a_i| instead of its bounding radius (mopa_valid_v5.inc,
    "Axis extents"): per moving geom slot the owner's index (-1: none), hl (FP32 bits) and the clamp ax_max; per table entry
    the three constants c_i' = (float)H_i + ((float)r + kCullEps), in the FP32 arithmetic that builds the table's own
    c_i = (float)H_i + ((float)rbound + kCullEps) (checked here against the table).  ax_max: the largest FP32 a for which the
    kernel's c_i' + hl a -- FP32 product, FP32 sum, as numpy's float32 computes them -- stays <= c_i for every static pair and axis of
    the owner (both operations are monotone in a, so it holds for every smaller a too)."""
    nmg = ex["nmg"]
    o_geom, o_rec, o_type, o_aabb, o_mgd = (hdr_int(ex, f) for f in ("o_mg_geom", "o_g_rec", "o_g_type", "o_g_aabb", "o_mgd"))
    ints, dbl = ex["ints"].astype("<i4"), ex["dbl"].astype("<f8")
    f32 = lambda w: np.uint32(w).view(np.float32)
    bits = lambda f: int(np.float32(f).view(np.uint32))
    slot, hl_bits, amax_bits, etab = [-1] * nmg, [0] * nmg, [0] * nmg, [0] * (3 * (len(tab) - 3 * nmg) // 8)
    n_ax = 0
    for m in range(nmg):
        g = int(ints[o_geom + m])
        if int(ints[o_type + g]) not in (G_CAPSULE, G_CYLINDER) or nstat[m] == 0:
            continue
        r, hl = np.float32(dbl[o_rec + 16 * g + 12]), np.float32(dbl[o_rec + 16 * g + 13])
        rg_old, rg_new = np.float32(dbl[o_mgd + 8 * m + 7]) + K_CULL_EPS, r + K_CULL_EPS
        both = []
        for k in range(nmov[m], nmov[m] + nstat[m]):
            e = padr[m] + k
            pg = int(tab[8 * e + 7]) & 0xFF
            for i in range(3):
                H = np.float32(dbl[o_aabb + 3 * pg + i])
                c_old, c_new = np.float32(H + rg_old), np.float32(H + rg_new)
                assert bits(c_old) == int(tab[8 * e + 4 + i]), f"slot {m} entry {k}: the table's half extent is not (float)H + rg"
                etab[3 * e + i] = bits(c_new)
                both.append((c_old, c_new))
        a = np.float32(1023.0) * K_AXIS_STEP            # the largest value pass A unpacks
        guess = np.float32(min((float(co) - float(cn)) / float(hl) for co, cn in both)) * np.float32(1.0 + 1e-6)
        a = min(a, guess)
        while any(np.float32(cn + np.float32(hl * a)) > co for co, cn in both):
            a = np.nextafter(a, np.float32(0.0))
        assert a > 0
        slot[m], hl_bits[m], amax_bits[m] = n_ax, bits(hl), bits(a)
        n_ax += 1
    return {"n_ax": n_ax, "slot": slot, "hl": hl_bits, "amax": amax_bits, "tab": etab,
            "n_pairs": sum(nstat[m] for m in range(nmg) if slot[m] >= 0)}


def bake(env: str, name: str, index: int) -> str:
    pi, args = scene_args(env)
    ex = _lib.k1_export(*args)
    fp = fingerprint(ex)
    if fp != ex["fingerprint"]:
        raise SystemExit(f"{env}: fingerprint {fp:016x} != the library's {ex['fingerprint']:016x}")
    try:
        fk = fk_program(ex)
    except Unsupported as e:
        raise SystemExit(f"{env}: cannot be baked: {e}")
    nmg = ex["nmg"]
    tab = ex["tab"].astype("<i4").view("<u4")
    n5 = (len(tab) - 3 * nmg) // 8
    cnt = tab[8 * n5: 8 * n5 + nmg]
    padr = [int(tab[8 * n5 + nmg + 2 * m]) for m in range(nmg)]
    pnum = [int(tab[8 * n5 + nmg + 2 * m + 1]) for m in range(nmg)]
    nmov = [int(c & 0xFF) for c in cnt]
    nstat = [int((c >> 8) & 0xFF) for c in cnt]
    npl = [int((c >> 16) & 0xFF) for c in cnt]
    assert all(a + b + c == p for a, b, c, p in zip(nmov, nstat, npl, pnum)) and max(pnum) <= 64
    path = os.path.join(SCENE_DIR, ENV_SPECS[env].scene + ".json")
    sha = hashlib.sha256(open(path, "rb").read()).hexdigest()
    thr = hdr_double(ex, "thr")

    def ints(v):
        return "{" + ", ".join(str(x) for x in v) + "}"

    def u64(v):
        return "{" + ", ".join(f"0x{x:016x}ull" for x in v) + "}"

    L = [f"// {env}: mopa_rl_amd/scenes/{os.path.basename(path)} (sha256 {sha}),",
         f"// contact threshold {thr!r}, pair pruning and cull radii from the scene's meta; {nmg} moving geoms, {n5} table entries",
         f"struct {name} {{",
         "    static constexpr bool kBaked = true;",
         "    // consecutive 64-state tiles a wave walks and culls before ONE narrow-phase drain evaluates their entries together",
         f"    static constexpr int kTilesPerDrain = {TILES_PER_DRAIN.get(env, 1)};",
         f"    static constexpr unsigned long long kFingerprint = 0x{fp:016x}ull;",
         f"    static constexpr int nmg = {nmg};",
         f"    static constexpr int padr[nmg] = {ints(padr)};",
         f"    static constexpr int pnum[nmg] = {ints(pnum)};",
         f"    static constexpr int nmov[nmg] = {ints(nmov)};",
         f"    static constexpr int nstat[nmg] = {ints(nstat)};",
         f"    static constexpr int npl[nmg] = {ints(npl)};",
         "    // FP32 pair table, 8 words per entry, as the library builds it: [0..2] partner centre / plane point (moving partners: [0]",
         "    // inscribed-ball bound), [3] squared cull radius / plane offset, [4..6] AABB half extents / plane normal, [7] flags",
         f"    static constexpr unsigned tab[{8 * n5}] = {{"]
    for m in range(nmg):
        L.append(f"        // geom slot {m}: {nmov[m]} moving + {nstat[m]} static + {npl[m]} plane partners")
        for e in range(padr[m], padr[m] + pnum[m]):
            L.append("        " + ", ".join(f"0x{int(w):08x}u" for w in tab[8 * e: 8 * e + 8]) + ",")
    L.append("    };")
    n_save, n_pq = max(fk["n_save"], 1), max(fk["n_pq"], 1)      # (array sizes: at least 1)
    L += ["    // forward kinematics (phase 1): the moving-body program of the generic walk, doubles as 64-bit patterns",
          f"    static constexpr int nmb = {fk['nmb']}, na = {fk['na']}, nq = {fk['nq']}, n_pq = {n_pq}, n_save = {n_save}, nsf = {len(fk['sf'])};",
          "    // per moving body: load (-2 static frame, -1 the body before, >= 0 save slot), static frame, save slot, first moving geom,",
          "    // moving geoms, joints, joint type, anchor at the body origin, value slot (< na active, else passive na + k)",
          "    static constexpr int fk_body[nmb][9] = {"]
    L += [f"        {ints(b)}," for b in fk["bodies"]]
    L += ["    };", "    // per moving body: pos[3] quat[4] joint axis[3] joint pos[3] joint ref", "    static constexpr unsigned long long fk_bd[nmb][14] = {"]
    L += [f"        {u64(b)}," for b in fk["bd"]]
    L += ["    };", "    // per moving geom: local pos[3] quat[4]", "    static constexpr unsigned long long fk_gd[nmg][7] = {"]
    L += [f"        {u64(g)}," for g in fk["gd"]]
    L += ["    };", "    // static frames: pos[3] quat[4] mat[9]", "    static constexpr unsigned long long fk_sf[nsf][16] = {"]
    L += [f"        {u64(f)}," for f in fk["sf"]]
    L += ["    };",
          f"    static constexpr unsigned long long fk_act_ref[na] = {u64(fk['act_ref'])};",
          f"    static constexpr int fk_pq_adr[n_pq] = {ints(fk['pq_adr'] + [0] * (n_pq - fk['n_pq']))};",
          "    // bodies the walk takes in its sparse form (products with the exact zeros and ones above left out, guarded at run time):",
          f"    // no exact zero in a stored pose (or its rotation matrix) of theirs or below them on {SPARSE_SAMPLE} seeded states (seed {SPARSE_SEED}); never a free-jointed body",
          "    static constexpr bool fk_sparse[nmb] = {" + ", ".join("true" if x else "false" for x in sparse_marks(index, env, pi, fk, nmg)) + "};"]
    res = resident_pairs(env, pi, ex, fk, tab, padr, nmov)
    n_res = max(len(res), 1)
    L += ["    // resident pairs (evaluated inside the walk, skipped by pass A): owner slot M, table entry K, geom slots in routine order",
          "    // (type 1 <= type 2), pair class, both types; then both sizes.  Chosen by pass A's survival rate on a seeded sample:",
          "    // " + (", ".join(f"({r['row'][0]}, {r['row'][1]}) kept in {r['pct']} %" for r in res) or "none"),
          f"    static constexpr int n_res = {len(res)};",
          f"    static constexpr int res[{n_res}][7] = {{" + ", ".join(ints(r["row"]) for r in res or [{"row": [-1, -1, 0, 0, 0, 0, 0]}]) + "};",
          f"    static constexpr unsigned long long res_size[{n_res}][6] = {{" + ", ".join(u64(r["size"]) for r in res or [{"size": [0] * 6}]) + "};"]
    ax = axis_extents(ex, tab, padr, nmov, nstat)

    def u32(v):
        return "{" + ", ".join(f"0x{x:08x}u" for x in v) + "}"

    L += [f"    // axis owners (moving capsules / cylinders with static non-plane partners: {ax['n_ax']} geoms, {ax['n_pairs']} of the {sum(nstat)} static pairs):",
          "    // per moving geom slot its word in the tile's axis table (-1: none), hl and the clamp of |axis| (FP32 bits); per table entry",
          "    // the static partner's AABB half extents + r + kCullEps (FP32 bits; 0: not a static pair of an axis owner)",
          f"    static constexpr int n_ax = {ax['n_ax']};",
          f"    static constexpr int ax_slot[nmg] = {ints(ax['slot'])};",
          f"    static constexpr unsigned ax_hl[nmg] = {u32(ax['hl'])};",
          f"    static constexpr unsigned ax_max[nmg] = {u32(ax['amax'])};",
          f"    static constexpr unsigned ax_tab[{3 * n5}] = {{"]
    for m in range(nmg):
        for e in range(padr[m], padr[m] + pnum[m]):
            L.append("        " + ", ".join(f"0x{w:08x}u" for w in ax["tab"][3 * e: 3 * e + 3]) + ",")
    L += ["    };", "};"]
    return "\n".join(L)


def generate() -> str:
    parts = ["// mopa_valid_v5_baked.inc -- GENERATED by tools/bake_k1_scenes.py: do not edit.  Inputs: the scene files named below,",
             "// the scene compiler (mopa_scene_build.inc) that builds the tables.  Included by mopa_valid_v5.inc.",
             "// Regenerate after changing either; tests/test_k1_baked_host.py checks that this file is current.",
             ""]
    for i, (env, name) in enumerate(SCENES):
        parts.append(bake(env, name, i + 1))
        parts.append("")
    parts.append("// X(index from 1, traits): every baked scene")
    parts.append("#define MOPA_K1_BAKED_SCENES(X) " + " ".join(f"X({i + 1}, {name})" for i, (_, name) in enumerate(SCENES)))
    return "\n".join(parts) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    txt = generate()
    with open(a.out, "w") as f:
        f.write(txt)
    print(f"wrote {a.out} ({len(txt)} bytes)")


if __name__ == "__main__":
    main()
