"""Host side of the replay sink (mopa_rl_amd/replay.py, csrc/mopa_replay.inc): the two symbols, the C ABI's argument checks
(all before any launch, so a box without a GPU observes them), the sampler's draw rule and the numpy reference ring the GPU
tests compare against.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from replay_ref import NAN_PATTERN, RefRing, draw_index, pack_rows, width
from reuse_ref import rng_key, rng_uniform_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


def test_symbols_declared_and_exported():
    from mopa_rl_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mopa_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for sym in ("mopa_replay_append", "mopa_replay_sample"):
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} is not declared in include/mopa_hip.h"
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)


def test_argument_errors_are_status_codes_before_any_launch():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    keep = (C.c_double * 8)()
    buf = C.cast(keep, C.c_void_p)         # (never dereferenced: every call below fails its checks first)

    def append(capacity=257, D=5, A=7, ring=buf, state=buf, n=4, mask=None, count=None, col=buf, ac_ld=7, ac_type=None, packed=None, work=buf):
        return L.mopa_replay_append(capacity, D, A, ring, state, n, mask, count, col, col, ac_ld, col, col, col, 1, col, ac_type, packed, work, None)

    def sample(capacity=257, D=5, A=7, ring=buf, state=buf, B=4, n_batches=1, out=buf, idx=buf):
        return L.mopa_replay_sample(capacity, D, A, ring, state, B, n_batches, 0, 0, 0, out, idx, None)

    def refused(rc, word):
        msg = L.mopa_last_error()
        assert rc == INVALID_ARG and word in msg, (rc, msg)

    for call in (append, sample):
        for capacity in (0, -3):
            refused(call(capacity=capacity), b"capacity < 1")
        refused(call(D=0), b"D < 1")
        refused(call(A=0), b"A < 1")
        refused(call(ring=None), b"null")
        refused(call(state=None), b"null")
    refused(append(work=None), b"null")
    refused(append(col=None), b"null source column")
    refused(append(ac_ld=6), b"ac_ld < A")
    refused(append(n=-1), b"n < 0")
    refused(append(mask=buf, count=buf), b"both a mask and a count")
    refused(append(packed=buf, col=None, mask=buf), b"packed")
    refused(append(packed=buf, col=None, count=buf), b"packed")
    refused(append(packed=buf), b"both a packed source and columns")
    refused(sample(B=0), b"B < 1")
    refused(sample(n_batches=0), b"n_batches < 1")
    refused(sample(out=None), b"null")
    refused(sample(idx=None), b"null")
    # an append of no rows is complete without a launch
    assert append(n=0) == 0


def test_draw_rule_stays_in_range_and_hits_both_ends():
    assert draw_index(0.0, 5) == 0 and draw_index(1.0 - 2.0 ** -53, 5) == 4
    assert draw_index(1.0, 5) == 4                                        # (a product that reaches `size` is held by the min())
    key = rng_key(7, 0)
    for size in (1, 2, 3, 5, 257):
        got = [draw_index(rng_uniform_k(key, i), size) for i in range(40 * size)]
        assert min(got) == 0 and max(got) == size - 1
    # the ring's draws: counter = rows drawn so far, whatever the batch sizes
    a, b = RefRing(9, 2, 1, seed=3), RefRing(9, 2, 1, seed=3)
    for r in (a, b):
        r.append_rows(np.arange(6 * r.W, dtype=np.float32).reshape(6, r.W))
    one = a.sample(4, n_batches=2)
    two = [b.sample(4), b.sample(4)]
    assert np.array_equal(one[1], np.concatenate([t[1] for t in two])) and np.array_equal(one[0], np.concatenate([t[0] for t in two]))
    assert a.draws == b.draws == 8 and one[1].min() >= 0 and one[1].max() < 6
    assert np.array_equal(one[0][:, 0], one[1] * a.W)


def _numbered(n, W, first=0):
    """rows whose entries name (row number, column)"""
    return (np.arange(first, first + n, dtype=np.float32)[:, None] * 128.0 + np.arange(W, dtype=np.float32)[None, :])


def test_reference_ring_wraps_and_keeps_the_newest():
    D, A = 3, 2
    W = width(D, A)
    r = RefRing(7, D, A, fill=NAN_PATTERN)
    assert r.size == 0 and (r.ring.view(np.uint32) == NAN_PATTERN).all()
    r.append_rows(_numbered(5, W))
    assert list(r.state) == [5, 5] and np.array_equal(r.ring[:5], _numbered(5, W)) and (r.ring.view(np.uint32)[5:] == NAN_PATTERN).all()
    r.append_rows(_numbered(4, W, first=5))                      # rows 5, 6 -> ring 5, 6; rows 7, 8 -> ring 0, 1
    assert list(r.state) == [9, 7]
    assert np.array_equal(r.ring[:, 0] / 128.0, [7, 8, 2, 3, 4, 5, 6])
    # an oversized append keeps its last `capacity` rows, each ring row written once, at the places a row-by-row append leaves them
    r.append_rows(_numbered(17, W, first=100))
    one = RefRing(7, D, A)
    one.total = 9
    for k in range(17):
        one.append_rows(_numbered(1, W, first=100 + k))
    assert list(r.state) == list(one.state) == [26, 7] and np.array_equal(r.ring, one.ring)
    assert sorted(r.ring[:, 0] / 128.0) == list(range(110, 117))
    # a count keeps the head of the source, a mask its marked rows in ascending order
    before = r.ring.copy()
    assert r.append_rows(_numbered(4, W), count=0) == 0 and r.append_rows(_numbered(4, W), mask=np.zeros(4, dtype=np.uint8)) == 0
    assert list(r.state) == [26, 7] and np.array_equal(r.ring, before)
    assert r.append_rows(_numbered(4, W, first=200), count=9) == 4
    assert r.append_rows(_numbered(6, W, first=300), mask=[0, 1, 0, 0, 3, 1]) == 3
    assert np.array_equal(r.ring[np.arange(26, 33) % 7, 0] / 128.0, [200, 201, 202, 203, 301, 304, 305])


def test_reference_rows_and_records():
    D, A = 3, 2
    rng = np.random.default_rng(0)
    n = 6
    ob, ob_next, ac, rew = rng.normal(size=(n, D)), rng.normal(size=(n, D)), rng.normal(size=(n, A + 1)), rng.normal(size=n)
    done, intra, ac_type = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 40, size=n), rng.integers(0, 3, size=n).astype(np.int32)
    rows = pack_rows(D, A, ob, ac, rew, done, intra, ob_next, ac_type=ac_type)
    assert rows.dtype == np.float32 and rows.shape == (n, width(D, A))
    assert np.array_equal(rows[:, D:D + A], ac[:, :A].astype(np.float32)) and np.array_equal(rows[:, D + A + 3], ac_type)
    assert np.array_equal(rows[:, D + A + 2], intra) and np.array_equal(rows[:, -D:], ob_next.astype(np.float32))
    # narrowing is round-to-nearest-even: halfway between two floats goes to the even one
    assert pack_rows(1, 1, [[1.0 + 2.0 ** -24]], [[1.0 + 3 * 2.0 ** -24]], [0.0], [0], [0], [[0.0]])[0, :2].tolist() == [1.0, 1.0 + 2.0 ** -22]
    # an exchange record with a stepped column stores what the masked column source stores, with ac_type 0
    stepped = np.array([1, 0, 1, 1, 0, 1], dtype=np.float32)
    a, b = RefRing(4, D, A), RefRing(4, D, A)
    a.append_records(pack_rows(D, A, ob, ac, rew, done, intra, ob_next, stepped=stepped))
    b.append_rows(pack_rows(D, A, ob, ac, rew, done, intra, ob_next), mask=stepped)
    assert list(a.state) == list(b.state) == [4, 4] and np.array_equal(a.ring.view(np.uint32), b.ring.view(np.uint32))


def test_device_buffer_refuses_the_host():
    """no CPU fallback: a buffer or a tensor on the host is an error, not a slow path"""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.replay import DeviceReplayBuffer
    with pytest.raises(_lib.MopaError, match="no CPU fallback"):
        DeviceReplayBuffer(257, 5, 7, "cpu")
    with pytest.raises(_lib.MopaError, match="no CPU fallback"):
        DeviceReplayBuffer(257, 5, 7, torch.device("cpu"), seed=3)
    with pytest.raises(_lib.MopaError, match="not on a GPU"):
        DeviceReplayBuffer._on_device("append_step", None, torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(_lib.MopaError, match="at least 1"):
        DeviceReplayBuffer(0, 5, 7, "cuda")
