#!/usr/bin/env python3
"""Bake committed scenes into k_is_valid_v5: writes mopa_rl_amd/csrc/mopa_valid_v5_baked.inc (committed, generated source).

Each scene is loaded the way the library's callers load it (scene.planner_inputs + _lib.Scene's pair pruning and cull
radii), the host half of mopa_scene_create runs on it (mopa_scene_k1_export: no device), and what k_is_valid_v5 reads
of the FP32 pair table goes into a traits struct as compile-time constants, with the scene's fingerprint (FNV-1a over
both blobs, the pair table and the header).  mopa_scene_create launches the baked instantiation only for a scene whose
fingerprint matches; every other scene -- the full-pair-list sibling (Scene.full), other thresholds, custom scenes --
keeps the generic kernel.  The output depends on nothing but the inputs: two runs give the same bytes.

    python tools/bake_k1_scenes.py [--out PATH]      (then rebuild: make -C mopa_rl_amd/csrc)
"""
from __future__ import annotations

import argparse
import hashlib
import os
import struct
import sys

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


def bake(env: str, name: str) -> str:
    pi, args = scene_args(env)
    ex = _lib.k1_export(*args)
    fp = fingerprint(ex)
    if fp != ex["fingerprint"]:
        raise SystemExit(f"{env}: fingerprint {fp:016x} != the library's {ex['fingerprint']:016x}")
    if not (ex["use_v5"] and ex["cen_lds"] and ex["n_mesh_pairs"] == 0):
        raise SystemExit(f"{env}: not a scene of the baked instantiation (third-generation kernel, centres in LDS, no mesh pairs)")
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
    thr = struct.unpack("<d", ex["hdr"].tobytes()[-32:-24])[0]

    def ints(v):
        return "{" + ", ".join(str(x) for x in v) + "}"

    L = [f"// {env}: mopa_rl_amd/scenes/{os.path.basename(path)} (sha256 {sha}),",
         f"// contact threshold {thr!r}, pair pruning and cull radii from the scene's meta; {nmg} moving geoms, {n5} table entries",
         f"struct {name} {{",
         "    static constexpr bool kBaked = true;",
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
    L.append("};")
    return "\n".join(L)


def generate() -> str:
    parts = ["// mopa_valid_v5_baked.inc -- GENERATED by tools/bake_k1_scenes.py: do not edit.  Inputs: the scene files named below,",
             "// the host half of mopa_scene_create (mopa_hip.hip) that builds the tables.  Included by mopa_valid_v5.inc.",
             "// Regenerate after changing either; tests/test_k1_baked_host.py checks that this file is current.",
             ""]
    for env, name in SCENES:
        parts.append(bake(env, name))
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
