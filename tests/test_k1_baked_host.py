"""Baked K1 scenes, host side (no GPU): the host export of the scene tables, the fingerprint that selects a baked
instantiation, and the generated mopa_valid_v5_baked.inc being current and reproducible."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENV = "SawyerPushObstacle-v0"


def _args(env=ENV, model=None):
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(env, model)
    return pi, (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        monkeypatch.delenv(k)


def test_export_runs_without_a_device_and_matches_the_baked_fingerprint():
    import bake_k1_scenes as B
    from mopa_rl_amd import _lib
    _, args = _args()
    ex = _lib.k1_export(*args)
    assert ex["use_v5"] and ex["cen_lds"] and ex["n_mesh_pairs"] == 0
    assert len(ex["dbl"]) > 0 and len(ex["ints"]) > 0 and len(ex["tab"]) == 8 * ((len(ex["tab"]) - 3 * ex["nmg"]) // 8) + 3 * ex["nmg"]
    assert B.fingerprint(ex) == ex["fingerprint"]
    inc = open(B.OUT).read()
    baked = [int(x, 16) for x in re.findall(r"kFingerprint = 0x([0-9a-f]{16})ull", inc)]
    assert ex["fingerprint"] in baked
    # planner settings are not part of what K1 reads
    assert _lib.k1_export(*args, range_=0.37, resolution=0.01)["fingerprint"] == ex["fingerprint"]


def test_generator_is_deterministic_and_the_committed_file_is_current(tmp_path):
    import bake_k1_scenes as B
    a, b = B.generate(), B.generate()
    assert a == b
    out = tmp_path / "baked.inc"
    out.write_text(a)
    assert out.read_bytes() == open(B.OUT, "rb").read(), "mopa_valid_v5_baked.inc is stale: run tools/bake_k1_scenes.py"


def test_other_scenes_get_other_fingerprints():
    from mopa_rl_amd import _lib
    pi, args = _args()
    fp = _lib.k1_export(*args)["fingerprint"]
    # the full-pair-list sibling (Scene.full), another threshold
    assert _lib.k1_export(*args, prune_pairs=False)["fingerprint"] != fp
    assert _lib.k1_export(*args[:3], args[3] - 1e-3)["fingerprint"] != fp
    # one constant of the model moved by one ULP: a static geom's size
    m = pi.model
    g = 0
    old = m.geom_size[g, 0]
    try:
        m.geom_size[g, 0] = np.nextafter(old, np.inf)
        assert _lib.k1_export(*args)["fingerprint"] != fp
    finally:
        m.geom_size[g, 0] = old
    assert _lib.k1_export(*args)["fingerprint"] == fp
