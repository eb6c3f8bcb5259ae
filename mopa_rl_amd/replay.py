"""The replay sink: a device-resident transition ring that is fed and sampled without a read-back (library calls
mopa_replay_append / mopa_replay_sample, csrc/mopa_replay.inc; DESIGN section 4 "Replay sink").

The reference's trainer runs `runner.run(every_steps=1)` (rl/trainer.py:280), so every rollout it hands to
`ReplayBuffer.store_episode` holds exactly one transition -- the agent step's own and each relabelled one -- and
`RandomSampler` (rl/dataset.py:51-84) picks a stored rollout uniformly, then t = randint(1) = 0: a uniform draw over the
stored transitions of a ring that overwrites the oldest.  That is what this class is, for the columns the learner reads
(rl/sac_agent.py:412-422), stored as the float32 the learner converts them to:

    row = ob[D] | ac[A] | rew | done | intra_steps | ac_type | ob_next[D]          (W = 2 * D + A + 4)

-- the width of a `dist.TransitionExchange` record, with `ac_type` where that record has `stepped`.  An append is at
most two launches and a sample is one, on the current stream; only `__len__` waits for the device."""
from __future__ import annotations

from . import _lib

M64 = 0xFFFFFFFFFFFFFFFF


def _torch():
    import torch
    return torch


class DeviceReplayBuffer:
    """Ring of `capacity` transitions of an env with `obs_dim` observation and `ac_dim` action entries on `device`.
    `seed` keys the sampler's counter RNG (stream `stream_id`; draw i of the buffer's life takes counter i).
    The ring is shared state: feed and sample one buffer from one stream (or order the streams yourself)."""

    def __init__(self, capacity: int, obs_dim: int, ac_dim: int, device, seed: int = 0, stream_id: int = 0):
        torch = _torch()
        self.capacity, self.obs_dim, self.ac_dim = int(capacity), int(obs_dim), int(ac_dim)
        if self.capacity < 1 or self.obs_dim < 1 or self.ac_dim < 1:
            raise _lib.MopaError("DeviceReplayBuffer: capacity, obs_dim and ac_dim are at least 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MopaError("DeviceReplayBuffer: the buffer lives on a GPU (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.width = 2 * self.obs_dim + self.ac_dim + 4
        self.seed, self.stream_id = int(seed) & M64, int(stream_id) & M64
        self.draws = 0                       # rows drawn so far = the next draw's counter
        self.ring = torch.zeros(self.capacity, self.width, dtype=torch.float32, device=self.device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._work = None

    # ---- checks

    @staticmethod
    def _on_device(what: str, *tensors):
        """a tensor on the host is an error, not a slow path"""
        for x in tensors:
            if x is not None and not getattr(x, "is_cuda", False):
                raise _lib.MopaError(f"DeviceReplayBuffer.{what}: a tensor is not on a GPU (there is no CPU fallback)")

    def _col(self, what, name, x, n, dtypes, width=None):
        torch = _torch()
        if x.dtype == torch.bool:
            x = x.view(torch.uint8)
        shape = (n,) if width is None else (n, width)
        if x.dtype not in dtypes or tuple(x.shape) != shape or x.device != self.device:
            raise _lib.MopaError(f"DeviceReplayBuffer.{what}: {name} is {x.dtype} {tuple(x.shape)} on {x.device}, "
                                 f"not {' / '.join(str(d) for d in dtypes)} {shape} on {self.device}")
        return x.contiguous()

    def _scratch(self, n):
        if self._work is None or self._work.numel() < n + 2:
            self._work = _torch().empty(n + 2, dtype=_torch().int64, device=self.device)
        return self._work

    # ---- feeding

    def _append_columns(self, what, n, ob, ac, rew, done, intra, ob_next, ac_type, mask=None, count=None):
        torch = _torch()
        self._on_device(what, ob, ac, rew, done, intra, ob_next, ac_type, mask, count)
        f64 = (torch.float64,)
        ob = self._col(what, "ob", ob, n, f64, self.obs_dim)
        ob_next = self._col(what, "ob_next", ob_next, n, f64, self.obs_dim)
        rew = self._col(what, "rew", rew.reshape(-1), n, f64)
        done = self._col(what, "done", done.reshape(-1), n, (torch.uint8,))
        intra = self._col(what, "intra_steps", intra.reshape(-1), n, (torch.int64, torch.int32))
        if ac.dim() != 2 or int(ac.shape[0]) != n or int(ac.shape[1]) < self.ac_dim or ac.dtype != torch.float64 or ac.device != self.device:
            raise _lib.MopaError(f"DeviceReplayBuffer.{what}: ac is {ac.dtype} {tuple(ac.shape)}, not float64 [{n}, >= {self.ac_dim}] on {self.device}")
        if ac.stride(1) != 1 or (n > 1 and ac.stride(0) < self.ac_dim):
            ac = ac.contiguous()
        ac_ld = int(ac.stride(0)) if n > 1 else max(int(ac.shape[1]), self.ac_dim)
        if ac_type is not None:
            ac_type = self._col(what, "ac_type", ac_type.reshape(-1), n, (torch.int32, torch.int64))
            if ac_type.dtype != torch.int32:
                ac_type = ac_type.to(torch.int32)
        if mask is not None:
            mask = self._col(what, "mask", mask.reshape(-1), n, (torch.uint8,))
        if count is not None:
            count = self._col(what, "count", count.reshape(-1), 1, (torch.int64,))
        work = self._scratch(n)
        stream = torch.cuda.current_stream(self.device)
        ptr = lambda x: x.data_ptr() if x is not None else None
        _lib.check(_lib.lib().mopa_replay_append(
            self.capacity, self.obs_dim, self.ac_dim, self.ring.data_ptr(), self.state.data_ptr(), n, ptr(mask), ptr(count), ptr(ob), ptr(ac), ac_ld,
            ptr(rew), ptr(done), ptr(intra), int(intra.dtype == torch.int64), ptr(ob_next), ptr(ac_type), None, work.data_ptr(), stream.cuda_stream))
        for x in (ob, ac, rew, done, intra, ob_next, ac_type, mask, count, work):      # (tensors of another stream's allocator pool)
            if x is not None:
                x.record_stream(stream)

    def append_step(self, out):
        """the dict of `BatchMoPARollout.agent_step`: the transitions of the envs that `stepped` (every env when the dict has no
        such entry), in env order; `ac[:, :ac_dim]`, and `ac_type` if the dict has one"""
        n = int(out["ob"].shape[0])
        self._append_columns("append_step", n, out["ob"], out["ac"], out["rew"], out["done"], out["intra_steps"], out["ob_next"],
                             out.get("ac_type"), mask=out.get("stepped"))

    def append_reuse(self, rb):
        """a `ReuseBatch` of `reuse_transitions_device`: its rows 0 .. min(count, rb.cap) - 1, by its device-side count"""
        self._append_columns("append_reuse", rb.cap, rb.ob, rb.ac, rb.rew, rb.done, rb.intra_steps, rb.ob_next, rb.ac_type, count=rb.count)

    def append_records(self, records):
        """float32 exchange records [n, W] (the buffer `dist.TransitionExchange.pack` fills, or the gathered [world * E, W] one
        behind `result`): the rows whose `stepped` column is non-zero; the stored `ac_type` is 0"""
        torch = _torch()
        self._on_device("append_records", records)
        if records.dim() != 2 or int(records.shape[1]) != self.width or records.dtype != torch.float32 or records.device != self.device:
            raise _lib.MopaError(f"DeviceReplayBuffer.append_records: records are {records.dtype} {tuple(records.shape)}, not float32 [n, {self.width}] "
                                 f"on {self.device}")
        records = records.contiguous()
        n = int(records.shape[0])
        stream = torch.cuda.current_stream(self.device)
        work = self._scratch(n)
        _lib.check(_lib.lib().mopa_replay_append(
            self.capacity, self.obs_dim, self.ac_dim, self.ring.data_ptr(), self.state.data_ptr(), n, None, None, None, None, 0, None, None, None, 0,
            None, None, records.data_ptr(), work.data_ptr(), stream.cuda_stream))
        records.record_stream(stream)
        work.record_stream(stream)

    # ---- sampling

    def _views(self, rows, idx):
        o, a = self.obs_dim, self.ac_dim
        return {"ob": rows[:, :o], "ac": rows[:, o:o + a], "rew": rows[:, o + a], "done": rows[:, o + a + 1], "intra_steps": rows[:, o + a + 2],
                "ac_type": rows[:, o + a + 3], "ob_next": rows[:, o + a + 4:], "idx": idx, "rows": rows}

    def empty_sample(self, batch_size: int, n_batches: int = 1):
        """storage of a `sample(batch_size, n_batches)` result, nothing drawn: what `sample(..., into=...)` takes"""
        torch = _torch()
        total = max(int(batch_size), 0) * max(int(n_batches), 0)
        return self._views(torch.empty(total, self.width, dtype=torch.float32, device=self.device),
                           torch.empty(total, dtype=torch.int64, device=self.device))

    def sample(self, batch_size: int, n_batches: int = 1, into=None):
        """`n_batches * batch_size` uniform draws over the stored transitions (one launch, no read-back): a dict of views --
        ob, ac, rew, done, intra_steps, ac_type, ob_next -- of one float32 tensor [n_batches * batch_size, W] (`rows`; batch b is
        rows b * batch_size .. (b + 1) * batch_size - 1), and `idx` (int64), the ring rows drawn.  The draw counter advances by the
        rows drawn, so two calls of B draw what one call of 2 B draws.  An empty buffer gives zero rows and idx = -1.
        into   a previous result of the same size, whose storage is written again"""
        torch = _torch()
        B, nb = int(batch_size), int(n_batches)
        total = max(B, 0) * max(nb, 0)
        if into is None:
            into = self.empty_sample(B, nb)
            rows, idx = into["rows"], into["idx"]
        else:
            rows, idx = into["rows"], into["idx"]
            self._on_device("sample", rows, idx)
            if (tuple(rows.shape) != (total, self.width) or tuple(idx.shape) != (total,) or rows.dtype != torch.float32 or idx.dtype != torch.int64
                    or not rows.is_contiguous() or not idx.is_contiguous() or rows.device != self.device or idx.device != self.device):
                raise _lib.MopaError("DeviceReplayBuffer.sample: `into` has other shapes than this call")
        stream = torch.cuda.current_stream(self.device)
        _lib.check(_lib.lib().mopa_replay_sample(self.capacity, self.obs_dim, self.ac_dim, self.ring.data_ptr(), self.state.data_ptr(), B, nb,
                                                 self.seed, self.stream_id, self.draws & M64, rows.data_ptr(), idx.data_ptr(), stream.cuda_stream))
        rows.record_stream(stream)
        idx.record_stream(stream)
        self.draws += total
        return into

    # ---- size, checkpoint

    @property
    def size_dev(self):
        """number of stored transitions as a device scalar (a view of state[1]): no read-back"""
        return self.state[1]

    def __len__(self) -> int:
        """number of stored transitions.  The one place of this class that reads back, and so waits for the device."""
        return int(self.state[1].item())

    def state_dict(self):
        """ring, state and draw counter (the reference checkpoints its replay buffer: rl/trainer.py:183-219)"""
        return {"ring": self.ring.clone(), "state": self.state.clone(), "draws": int(self.draws), "seed": self.seed, "stream_id": self.stream_id,
                "capacity": self.capacity, "obs_dim": self.obs_dim, "ac_dim": self.ac_dim}

    def load_state_dict(self, sd):
        torch = _torch()
        if (int(sd["capacity"]), int(sd["obs_dim"]), int(sd["ac_dim"])) != (self.capacity, self.obs_dim, self.ac_dim):
            raise _lib.MopaError("DeviceReplayBuffer.load_state_dict: the checkpoint is of another capacity, obs_dim or ac_dim")
        ring, state = sd["ring"], sd["state"]
        if tuple(ring.shape) != (self.capacity, self.width) or ring.dtype != torch.float32 or tuple(state.shape) != (2,) or state.dtype != torch.int64:
            raise _lib.MopaError("DeviceReplayBuffer.load_state_dict: ring / state of another shape or type")
        self.ring.copy_(ring, non_blocking=True)
        self.state.copy_(state, non_blocking=True)
        self.draws, self.seed, self.stream_id = int(sd["draws"]), int(sd["seed"]) & M64, int(sd["stream_id"]) & M64
