"""Host reference of the replay sink (mopa_rl_amd/replay.py, csrc/mopa_replay.inc) for test_replay_host.py and
test_replay_gpu.py: a numpy ring with the library's rules -- row layout, narrowing, selection, destination, oversize rule,
state -- and the sampler's draws from reuse_ref.py's counter RNG."""
import numpy as np

from reuse_ref import rng_key, rng_uniform_k

NAN_PATTERN = 0x7FC0BEEF       # a quiet NaN with a payload: what a never-written ring row holds in the tests


def width(D, A):
    return 2 * D + A + 4


def pack_rows(D, A, ob, ac, rew, done, intra, ob_next, ac_type=None, stepped=None):
    """the float32 rows [n, W] of a column source: ob | ac[:, :A] | rew | done | intra_steps | ac_type (0 without one) | ob_next;
    with `stepped` that column holds it instead (an exchange record).  numpy's astype(float32) rounds to nearest even."""
    n = len(rew)
    rows = np.zeros((n, width(D, A)), dtype=np.float32)
    rows[:, :D] = np.asarray(ob, dtype=np.float64).astype(np.float32)
    rows[:, D:D + A] = np.asarray(ac, dtype=np.float64)[:, :A].astype(np.float32)
    rows[:, D + A] = np.asarray(rew, dtype=np.float64).astype(np.float32)
    rows[:, D + A + 1] = np.asarray(done).astype(np.float32)
    rows[:, D + A + 2] = np.asarray(intra).astype(np.float32)
    if stepped is not None:
        rows[:, D + A + 3] = np.asarray(stepped).astype(np.float32)
    elif ac_type is not None:
        rows[:, D + A + 3] = np.asarray(ac_type).astype(np.float32)
    rows[:, D + A + 4:] = np.asarray(ob_next, dtype=np.float64).astype(np.float32)
    return rows


def draw_index(u, size):
    """randint(0, size) from a uniform of [0, 1): min(int(u * size), size - 1)"""
    return min(int(u * float(size)), size - 1)


class RefRing:
    def __init__(self, capacity, D, A, seed=0, stream_id=0, fill=None):
        self.capacity, self.D, self.A, self.W = int(capacity), int(D), int(A), width(D, A)
        self.ring = np.zeros((self.capacity, self.W), dtype=np.float32)
        if fill is not None:
            self.ring.view(np.uint32)[:] = fill
        self.total = 0
        self.key = rng_key(int(seed), int(stream_id))
        self.draws = 0

    @property
    def size(self):
        return min(self.total, self.capacity)

    @property
    def state(self):
        return np.array([self.total, self.size], dtype=np.int64)

    def append_rows(self, rows, mask=None, count=None):
        """rows [n, W] float32 as `pack_rows` forms them; mask [n] (non-zero keeps) or count (rows 0 .. min(count, n) - 1)"""
        assert mask is None or count is None
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, self.W)
        n = len(rows)
        if mask is not None:
            kept = rows[np.asarray(mask).reshape(n) != 0]
        elif count is not None:
            kept = rows[:min(max(int(count), 0), n)]
        else:
            kept = rows
        m = len(kept)
        for k in range(max(m - self.capacity, 0), m):
            self.ring.view(np.uint32)[(self.total + k) % self.capacity] = kept[k].view(np.uint32)
        self.total += m
        return m

    def append_records(self, records):
        """exchange records: column D + A + 3 is the mask; the stored ac_type is 0"""
        records = np.array(records, dtype=np.float32).reshape(-1, self.W)
        col = self.D + self.A + 3
        mask = records[:, col] != 0
        records[:, col] = 0.0
        return self.append_rows(records, mask=mask)

    def sample(self, B, n_batches=1):
        """(rows [B * n_batches, W] float32, idx int64), the draw counter moved on"""
        total = B * n_batches
        out = np.zeros((total, self.W), dtype=np.float32)
        idx = np.full(total, -1, dtype=np.int64)
        size = self.size
        for i in range(total):
            if size > 0:
                idx[i] = draw_index(rng_uniform_k(self.key, self.draws + i), size)
                out.view(np.uint32)[i] = self.ring.view(np.uint32)[idx[i]]
        self.draws += total
        return out, idx
