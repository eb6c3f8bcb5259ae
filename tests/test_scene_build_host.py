"""The scene compiler's output, host side (no GPU): for every supported env and every creation-time setting, the blobs, the FP32
pair table, the header, the fingerprint, the launch facts and the `[mopa] scene:` line (the K1 policy: LDS sizes, entry caps,
centre placement, tile-posed counts) equal the recorded ones byte for byte; and what the compiler refuses, it refuses with the
same code and text.

tests/golden/scene_build.json is recorded by running this module as a script (it rewrites the file from the library in use:
MOPA_HIP_LIB selects the build)."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import SUPPORTED_ENVS  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_build.json")

ENVS = SUPPORTED_ENVS
# name -> (environment variables, Scene keyword arguments)
SETTINGS = {
    "default": ({}, {}),
    "kernel_v1": ({"MOPA_VALID_KERNEL": "v1"}, {}),
    "kernel_v2": ({"MOPA_VALID_KERNEL": "v2"}, {}),
    "kernel_v5": ({"MOPA_VALID_KERNEL": "v5"}, {}),
    "centres_lds": ({"MOPA_V5_CENTRES": "lds"}, {}),
    "centres_slab": ({"MOPA_V5_CENTRES": "slab"}, {}),
    "no_tile_poses": ({"MOPA_V5_NO_TILE_POSES": "1"}, {}),
    "tile_min_1": ({"MOPA_V5_TILE_MIN": "1"}, {}),
    "no_pruning": ({}, {"prune_pairs": False}),
}


def _args(env):
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(env)
    return pi, (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)


def _record(ex, err):
    """what the fixture holds of one export + the stderr text of the call"""
    lines = [ln for ln in err.splitlines() if ln.startswith("[mopa] scene:")]
    assert len(lines) == 2, err            # k1_export compiles the scene twice (sizes, then contents)
    assert lines[0] == lines[1]
    rec = {k: hashlib.sha256(np.ascontiguousarray(ex[k]).tobytes()).hexdigest() for k in ("dbl", "ints", "tab", "hdr")}
    rec.update(fingerprint="%016x" % ex["fingerprint"], use_v5=ex["use_v5"], cen_lds=ex["cen_lds"], n_mesh_pairs=ex["n_mesh_pairs"],
               nmg=ex["nmg"], scene_line=lines[0])
    return rec


def _clear_knobs(setenv, delenv):
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        delenv(k)
    setenv("MOPA_DEBUG", "1")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("env", ENVS)
def test_compiler_output_is_the_recorded_one(env, setting, golden, monkeypatch, capfd):
    from mopa_rl_amd import _lib
    _clear_knobs(monkeypatch.setenv, monkeypatch.delenv)
    envvars, kw = SETTINGS[setting]
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    _, args = _args(env)
    capfd.readouterr()
    ex = _lib.k1_export(*args, **kw)
    got = _record(ex, capfd.readouterr().err)
    want = golden[env][setting]
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], f"{env} / {setting}: {k}"


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(ENVS)
    for env in ENVS:
        assert sorted(golden[env]) == sorted(SETTINGS)
    # the settings do reach the compiler: each knob changes something it should somewhere
    push, lift, asm = golden["SawyerPushObstacle-v0"], golden["SawyerLiftObstacle-v0"], golden["SawyerAssemblyObstacle-v0"]
    assert push["default"]["use_v5"] and not push["kernel_v2"]["use_v5"] and not push["kernel_v1"]["use_v5"]
    assert push["default"]["cen_lds"] and not push["centres_slab"]["cen_lds"]
    assert lift["default"]["n_mesh_pairs"] > 0 and not lift["centres_lds"]["cen_lds"]
    assert asm["default"]["scene_line"] != asm["no_tile_poses"]["scene_line"]
    assert push["default"]["tab"] != push["no_pruning"]["tab"]


def _refusal(env, mutate):
    """the MopaError text of a description the compiler refuses"""
    from mopa_rl_amd import _lib
    pi, (model, passive, ignored, thr) = _args(env)
    with pytest.raises(_lib.MopaError) as e:
        mutate(_lib, model, list(passive), ignored, thr)
    return str(e.value)


def test_refusals_keep_code_and_text(monkeypatch):
    _clear_knobs(monkeypatch.setenv, monkeypatch.delenv)
    monkeypatch.delenv("MOPA_DEBUG")
    env = "SawyerPushObstacle-v0"
    msg = _refusal(env, lambda L, m, pas, ign, thr: L.k1_export(m, pas, ign, 0.01))
    assert msg == "libmopa_hip error 2: contact_threshold > 0 is not supported (the broad phase culls at zero margin)"
    msg = _refusal(env, lambda L, m, pas, ign, thr: L.k1_export(m, pas + [m.nq], ign, thr))
    assert msg == "libmopa_hip error 1: passive_qpos_idx out of range"

    def ellipsoid(L, m, pas, ign, thr):
        g = int(np.asarray(m.pair_geom).reshape(-1, 2)[0, 0])
        old = m.geom_type[g]
        try:
            m.geom_type[g] = 4
            L.k1_export(m, pas, ign, thr, prune_pairs=False)
        finally:
            m.geom_type[g] = old
    msg = _refusal(env, ellipsoid)
    assert msg == "libmopa_hip error 2: collidable geom type 4 (ellipsoid/hfield) is not supported"
    # precedence among the checks: the threshold is looked at before the passive list
    msg = _refusal(env, lambda L, m, pas, ign, thr: L.k1_export(m, pas + [m.nq], ign, 0.01))
    assert msg.endswith("contact_threshold > 0 is not supported (the broad phase culls at zero margin)")


class _StderrText:
    """file descriptor 2 into a temporary file (the line is printed by the native library)"""

    def __enter__(self):
        sys.stderr.flush()
        self._saved = os.dup(2)
        self._tmp = tempfile.TemporaryFile(mode="w+b")
        os.dup2(self._tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self._saved, 2)
        os.close(self._saved)
        self._tmp.seek(0)
        self.text = self._tmp.read().decode()
        self._tmp.close()


def _write_fixture():
    from mopa_rl_amd import _lib
    out = {}
    for env in ENVS:
        out[env] = {}
        _, args = _args(env)
        for setting, (envvars, kw) in SETTINGS.items():
            _clear_knobs(os.environ.__setitem__, os.environ.__delitem__)
            os.environ.update(envvars)
            with _StderrText() as cap:
                ex = _lib.k1_export(*args, **kw)
            out[env][setting] = _record(ex, cap.text)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN} from {_lib.LIB_PATH}")


if __name__ == "__main__":
    _write_fixture()
