"""Planner jobs of the batched rollout: one RRT-Connect launch (K3) and the way of its rows to executable trajectories -- un-wrap of
`SamplingBasedPlanner.plan` / `PlannerAgent.plan`, densification of rl/sac_agent.py:216-233, its fallback planners (:300-306) -- as a
typed record (`PlanJob`) that `PlannerJobs` drives through five stages.  The array form of the path post-processing is numpy functions
of this module, which has no device dependency of its own: CPU tensors, no stream, `device_paths=False` run without a GPU."""
import contextlib
from dataclasses import dataclass, field
from functools import partialmethod
from typing import Any, Optional

import numpy as np

from . import _lib
from .agent_planning import _torch, seam_steps_np, simple_interpolate_batch, wrap_unlimited

RRT, DEVICE, SPLIT, SIMPLE, MAIN = "rrt", "device", "split", "simple", "main"      # PlanJob.stage
BUCKETS = (6, 12, 24, 48)      # path-length edges of the split of a long job (`split_rows`)


def unwrap_rows(start, P, seam_idx):
    """SamplingBasedPlanner.plan rebuilds the trajectory from successive differences (:71-99): tr[k] = tr[k-1] + (states[k] - states[k-1]),
    tr[0] = start (PlannerAgent drops row 0).  np.add.accumulate is that strictly sequential sum, for one path ([nq], [L, nq]) or all
    paths of a job at once ([R, nq], [R, L, nq]; rows past a path's length hold garbage)."""
    return np.add.accumulate(np.concatenate([start[..., None, :], seam_steps_np(P, seam_idx)], axis=-2), axis=-2)


def long_segments(T, nrow, n: int, ac_scale: float):
    """(path, waypoint) index arrays of the steps of T [R, W + 1, nq] (row 0 = start, `nrow` waypoints each) that exceed ac_scale in
    one of the first n joints: waypoint i minus its predecessor (rl/sac_agent.py:220-225)"""
    step = T[:, 1:, :n] - T[:, :-1, :n]
    far = ((step < -ac_scale) | (step > ac_scale)).any(axis=2)
    far &= np.arange(far.shape[1])[None, :] < nrow[:, None]
    return np.nonzero(far)


def densify_cut(T, seg_r, seg_i, n: int, ac_scale: float, clip_state, valid):
    """cut every long segment by the straight-line rule (steps <= 0.8 ac_scale from its clipped start, then its end), all interior states
    validated in one call of `valid(rows [S, nq]) -> bool [S]`.  Returns (starts, ends, count [S], walk [S, K, nq], fb: the segments
    with an invalid interior state)."""
    starts = clip_state(T[seg_r, seg_i])                                        # :266 clip_qpos on every segment start
    ends = T[seg_r, seg_i + 1]
    bound = ac_scale * 0.8
    diff = ends[:, :n] - starts[:, :n]
    ratio = np.maximum(np.where(diff > bound, diff / bound, 0.0), np.where(diff < -bound, diff / -bound, 0.0))
    scale = np.maximum(ratio.max(axis=1), 1.0)
    count = scale.astype(np.int64)                                              # int(): truncation
    per_step = diff / scale[:, None]
    K = int(count.max())
    walk = np.repeat(starts[:, None, :], K, axis=1)
    acc = starts[:, :n].copy()
    for k in range(K):                                                          # K dependent additions, as the scalar rule
        acc = acc + per_step
        walk[:, k, :n] = acc
    live = np.arange(K)[None, :] < count[:, None]
    verdict = np.ones((len(seg_r), K), dtype=bool)
    verdict[live] = valid(walk[live])
    return starts, ends, count, walk, list(np.nonzero(~verdict.all(axis=1))[0])


def assemble(hp: "HostPaths", M: int, nq: int):
    """the final trajectories of a job's M rows: ([M, L, nq] padded, lengths -- 0 for the failed rows) + the flags.  Waypoint i of
    path r becomes `pieces[r, i]` rows: itself, or -- densified -- its cut (count interior states + the waypoint), or a fallback path."""
    good, T, nrow = hp.good, hp.T, hp.nrow
    if not len(good):
        return (np.zeros((M, 1, nq)), np.zeros(M, dtype=np.int64)) + hp.flags
    R, W = T.shape[0], T.shape[1] - 1
    seg_r, seg_i = hp.seg_r, hp.seg_i
    pieces = (np.arange(W)[None, :] < nrow[:, None]).astype(np.int64)
    seg_len = np.zeros(len(seg_r), dtype=np.int64)
    if len(seg_r):
        seg_len[:] = hp.count + 1
        for k, rep in hp.replacement.items():
            seg_len[k] = len(rep)
        pieces[seg_r, seg_i] = seg_len
    off = np.cumsum(pieces, axis=1) - pieces                       # first output row of waypoint i
    length = pieces.sum(axis=1)
    out = np.zeros((R, max(1, int(length.max())), nq))
    r_idx, i_idx = np.nonzero(np.arange(W)[None, :] < nrow[:, None])
    out[r_idx, off[r_idx, i_idx] + pieces[r_idx, i_idx] - 1] = T[r_idx, i_idx + 1]      # every piece ends in its waypoint
    if len(seg_r):
        kk = np.nonzero(np.array([k not in hp.replacement for k in range(len(seg_r))]))[0]
        if len(kk):
            cnt = hp.count[kk]
            kr = np.repeat(kk, cnt)                                                      # (segment, interior state c) pairs
            c = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            out[seg_r[kr], off[seg_r[kr], seg_i[kr]] + c] = hp.walk[kr, c]
        for k, rep in hp.replacement.items():
            o = off[seg_r[k], seg_i[k]]
            out[seg_r[k], o:o + len(rep)] = rep
    traj = np.zeros((M, out.shape[1], nq))
    ln = np.zeros(M, dtype=np.int64)
    traj[good], ln[good] = out, length
    return (traj, ln) + hp.flags


def split_rows(plen_h):
    """A finished launch's paths are post-processed as padded [rows, longest path, nq] arrays; a few long paths among many short
    ones would make that mostly padding: the rows of a job by path-length bucket (`BUCKETS`), one index array per bucket in use"""
    edges = np.searchsorted(np.array(BUCKETS), plen_h, side="left")
    return [np.nonzero(edges == b)[0] for b in np.unique(edges)]


def join_results(results, rows, M: int, nq: int):
    """the result of a job of M rows from those of its buckets (`rows[b]` = the job's rows in bucket b)"""
    L = max(r[0].shape[1] for r in results)
    traj, ln = np.zeros((M, L, nq)), np.zeros(M, dtype=np.int64)
    flags = [np.zeros(M, dtype=bool) for _ in range(3)]
    for (tr, l, *fl), rw in zip(results, rows):
        traj[rw, :tr.shape[1]], ln[rw] = tr, l
        for f, g in zip(flags, fl):
            f[rw] = g
    return (traj, ln) + tuple(flags)


def merge_paths(traj_t, lens, tr_j, ln_j, rows):
    """write a job's padded trajectories (tr_j [M, L, nq], ln_j [M]; 0 = no path; tensors or host arrays) into rows `rows` (index
    tensor) of traj_t / lens (torch; traj_t is widened when a job's paths are longer)"""
    torch = _torch()
    L = int(tr_j.shape[1])
    if L > traj_t.shape[1]:
        traj_t = torch.cat([traj_t, torch.zeros(traj_t.shape[0], L - traj_t.shape[1], traj_t.shape[2], dtype=traj_t.dtype, device=traj_t.device)], dim=1)
    traj_t[rows, :L] = torch.as_tensor(tr_j, device=traj_t.device)
    lens[rows] = torch.as_tensor(ln_j, device=traj_t.device)
    return traj_t, lens


@dataclass(slots=True)
class HostPaths:
    """host working set of a job whose rows are post-processed in numpy (stages "rrt" without device paths, "simple", "main")"""
    ids_h: Any                  # env ids and step counts of the job's rows (fallback queries: stream ids and seeds)
    steps_h: Any
    flags: tuple                # (success, valid, exact) bool [M]
    good: Any                   # rows with a path (status 0); T, nrow, seg_r index into these
    T: Any = None               # [R, W + 1, nq] un-wrapped rows, row 0 = the start; nrow [R] waypoints per path
    nrow: Any = None
    seg_r: Any = None           # long segment k: waypoint seg_i[k] of path seg_r[k]
    seg_i: Any = None
    starts: Any = None          # per segment: clipped start, end, interior states (`densify_cut`)
    ends: Any = None
    count: Any = None
    walk: Any = None
    fb: list = field(default_factory=list)                 # segments still waiting for a fallback planner
    replacement: dict = field(default_factory=dict)        # segment -> the rows a fallback planner (or [end]) gave it


@dataclass(slots=True)
class PlanJob:
    """One planner launch on its way to trajectories.  Stream and allocator obligations live in `stream`, `event`, `built`, `held`
    and `post_on_main`."""
    ids: Any                    # [M] int64 env rows of the queries (row of the rollout, not the global id)
    cur: Any                    # [M, nq] start states as the caller holds them (clipped, NOT wrapped) / targets
    target: Any
    steps: Any                  # [M] int64 step count of every env when its query was made (seeds of the fallback planners)
    stream: Any = None          # side stream the launch and (unless post_on_main) its post-processing run on; None: the caller's
    iters: int = 0              # iteration budget of the launch (below the full budget: a first-phase launch)
    stage: str = RRT            # RRT -> [DEVICE | SPLIT | SIMPLE -> MAIN]; what `event` / the outputs below belong to
    event: Any = None           # recorded on `stream` behind the current stage's launches; None: nothing to wait for
    path: Any = None            # outputs of the current stage's planner launch: [M', max_path, nq], [M'] int32, [M'] int32
    plen: Any = None
    status: Any = None
    retry: bool = False         # a full-budget launch of queries a first-phase launch left unsolved (pooled or chained)
    pstate: Any = None          # PlanState a first-phase launch kept for the retry of its unsolved queries
    chain: Optional["PlanJob"] = None          # the continuation queued behind this first-phase launch on its stream (all its rows)
    post_on_main: bool = False  # the stream is busy with the continuation: post-process on the caller's stream
    lazy: Any = None            # (chain job, rows): this job IS rows `rows` of that continuation; gathered when `event` has passed
    built: Any = None           # event on the caller's stream behind the ops that made ids / cur / ...; `stream` waits for it first
    unwrapped: bool = False     # `path` went through the device un-wrap already (row 0 = cur)
    bucketed: bool = False      # one path-length bucket of a split job: not split again, not post-processed on the device
    sub: Optional["PlanJob"] = None            # DEVICE: the rows that need the fallback planners, through the host form; `sub_rows`
    subs: Optional[list] = None                # SPLIT: one job per bucket; `sub_rows[b]` = this job's rows in bucket b
    sub_rows: Any = None
    dev: Any = None             # DEVICE: [traj, length, ok, valid, exact] device tensors before the sub-job's rows are merged
    result: Any = None          # (traj [M, L, nq], length [M], success, valid, exact): numpy, or device tensors (device paths)
    held: Any = None            # tensors a side-stream launch reads, held until that launch has been waited for (`event`)
    host: Optional[HostPaths] = None

    def subset(self, rows, stream, width=None, **flags):
        """the job of the rows `rows` (index tensor) of this one's finished launch (the first `width` rows of their paths)"""
        return PlanJob(self.ids[rows], self.cur[rows], self.target[rows], self.steps[rows], stream=stream, plen=self.plen[rows],
                       status=self.status[rows], path=self.path[rows] if width is None else self.path[rows, :width], **flags)

    @classmethod
    def continuation(cls, first: "PlanJob", rows, iters: int):
        """the queries `rows` of `first` whose continuation already runs behind it on its stream: a job finished at the second event"""
        return cls(first.ids[rows], first.cur[rows], first.target[rows], first.steps[rows], stream=first.stream, iters=iters,
                   event=first.chain.event, retry=True, lazy=(first.chain, rows))


class PlannerJobs:
    """Launches planner jobs and drives them through their stages (`launch`, `advance`, `finish`); `plan` is `SACAgent.plan`.
      stage RRT     results of the main RRT-Connect launch: sentinel decoding, the un-wrapped trajectory, densification: a path
                    segment longer than ac_scale in some joint is cut by the straight-line rule from its clipped start; all
                    interior states of all segments are validated in ONE launch.  With `cfg.device_paths` on the device (DEVICE)
      stage DEVICE  ... is enqueued; queries that met an invalid interior state go through the host form as a sub-job
      stage SPLIT   host form of more than 64 rows: one sub-job per path-length bucket
      stage SIMPLE  the (rare) segments with an invalid interior state: simple planner, one batched launch (:300-303)
      stage MAIN    those it could not connect: main planner, one batched launch (:304-306); else the segment stays [end]"""

    def __init__(self, cfg, bp, bp_simple, limits, valid, n: int, nq: int, seam_idx, seam_mask: int, E: int, main_iters: int,
                 simple_iters: int, device):
        self.cfg, self.bp, self.bp_simple, self.limits, self.valid = cfg, bp, bp_simple, limits, valid
        self.n, self.nq, self.seam_idx, self.seam_mask, self.E = n, nq, seam_idx, seam_mask, E
        self.main_iters, self.simple_iters, self.device = main_iters, simple_iters, device

    def _plan(self, stage, start, goal, ids, seeds, iters, stream=None, **side):
        """`BatchPlanner.plan` of the main planner (or, stage SIMPLE, the simple one) with its K9 flags; on a side stream with
        cfg.planner_workgroups and what `side` says (keep_state / resume / exclusive / max_workgroups)"""
        cfg = self.cfg
        bp, pre = (self.bp_simple, "simple_planner_") if stage == SIMPLE else (self.bp, "")
        kw = dict(max_iters=iters, max_nodes=cfg.max_nodes, max_path=cfg.max_path, seed=cfg.seed, env_ids=ids, seeds=seeds,
                  vertex_simplify=getattr(cfg, pre + "vertex_simplify"), path_shortcut=getattr(cfg, pre + "path_shortcut"))
        if getattr(cfg, pre + "path_smooth"):       # (flag off: the launches get the keywords they always got)
            kw["path_smooth"] = True
        if stream is not None:
            kw.update({"stream": stream, "max_workgroups": cfg.planner_workgroups, **side})
        return bp.plan(start, goal, **kw)

    def launch(self, cur, target, ids, steps, seeds=None, stream=None, iters=None, keep=False, resume=None, chain=False):
        """RRT-Connect (K3) for the envs `ids` whose straight line is blocked (:205-209): asynchronous, optionally on a side stream.  A query's
        sample stream is keyed by (cfg.seed + the env's own step count, env id): an env's plans do not depend on which envs are planned with it or
        when.  `keep`: the launch keeps its trees (job.pstate); `chain`: the full-budget continuation of its unsolved queries goes behind it (job.chain)."""
        torch, cfg = _torch(), self.cfg
        if seeds is None:
            seeds = (steps + cfg.seed).contiguous()
        gids = (ids + int(cfg.env_id_base)).contiguous() if cfg.env_id_base else ids       # the planner's stream id: the GLOBAL env id
        job = PlanJob(ids, cur, target, steps, stream=stream, iters=self.main_iters if iters is None else int(iters))
        if self.seam_idx:       # the planner sees the wrapped endpoints; job.cur stays the caller's state
            cur, target = wrap_unlimited(cur, self.seam_idx).contiguous(), wrap_unlimited(target, self.seam_idx).contiguous()
        if stream is None:
            job.path, job.plen, job.status = self._plan(MAIN, cur, target, gids, seeds, job.iters)[:3]
            return job
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            full = (resume is not None or not keep) and job.iters == self.main_iters
            res = self._plan(MAIN, cur, target, gids, seeds, job.iters, stream, keep_state=keep, resume=resume,
                             exclusive=cfg.planner_exclusive >= 2 or (cfg.planner_exclusive == 1 and full))
            job.path, job.plen, job.status = res[:3]
            job.pstate = res[4] if keep else None      # trees + counters of the queries this budget leaves unsolved
            job.event = torch.cuda.Event()      # (chained: the quick queries' results are complete HERE)
            job.event.record(stream)
            if chain:
                rb = self._plan(MAIN, cur, target, gids, seeds, self.main_iters, stream, resume=res[4], exclusive=cfg.planner_exclusive >= 1,
                                max_workgroups=cfg.planner_chain_workgroups or cfg.planner_workgroups)
                job.chain = PlanJob(ids, job.cur, job.target, steps, stream=stream, iters=self.main_iters, event=torch.cuda.Event(),
                                    path=rb[0], plen=rb[1], status=rb[2], retry=True)
                job.chain.event.record(stream)
                job.post_on_main = True
            for t in (cur, target, ids, gids, seeds):
                t.record_stream(stream)
        return job

    def advance(self, job: PlanJob, wait: bool):
        """Drive a job through its stages; True: finished (job.result is set).  `wait` (lock-step): every stage is waited for; else False where a launch has not finished."""
        while True:
            done = getattr(self, "_stage_" + job.stage)(job, wait)      # None: the job went on to another stage
            if done is not None:
                return done

    def finish(self, job: PlanJob):
        self.advance(job, wait=True)
        return job.result

    @staticmethod
    def _ready(job, wait):
        if job.event is not None:
            if wait:
                job.event.synchronize()
            elif not job.event.query():
                return False
        return True

    @staticmethod
    def _rows_h(job, plen_h):
        path_h = job.path[:, :max(1, int(plen_h.max()))].cpu().numpy()         # the [max_path] tail of every row is unused
        path_h[np.arange(path_h.shape[1])[None, :] >= plen_h[:, None]] = 0.0   # ... and holds whatever the allocator left
        return path_h

    def _stage_rrt(self, job, wait):
        torch, cfg, n = _torch(), self.cfg, self.n
        if not self._ready(job, wait):
            return False
        if cfg.device_paths and self.nq <= 64 and not job.bucketed and not job.unwrapped:
            self._enqueue_device(job)
            return self._stage_device(job, wait, just_enqueued=True)
        plen_h, st_h = job.plen.cpu().numpy(), job.status.cpu().numpy()
        if len(plen_h) > 64 and not job.bucketed:
            job.sub_rows, job.stage = split_rows(plen_h), SPLIT
            job.subs = [job.subset(torch.as_tensor(r, device=job.path.device), job.stream, width=max(1, int(plen_h[r].max())), bucketed=True,
                                   unwrapped=job.unwrapped) for r in job.sub_rows]
            return None
        path_h, cur_h = self._rows_h(job, plen_h), job.cur.cpu().numpy()
        ok = st_h == 0         # sentinel rows (sampling_based_planner.py:64-69): -5 goal invalid, -4 no exact solution
        good, empty = np.where(ok)[0], np.zeros(0, dtype=np.int64)
        hp = job.host = HostPaths(job.ids.cpu().numpy(), job.steps.cpu().numpy(), (ok, st_h != _lib.PLAN_INVALID_GOAL, st_h != _lib.PLAN_NO_EXACT),
                                  good, nrow=empty, seg_r=empty, seg_i=empty)
        if len(good):
            # (rows that went through mopa_paths_unwrap_batch already have row 0 = cur)
            hp.T = path_h[good] if job.unwrapped else unwrap_rows(cur_h[good], path_h[good], self.seam_idx)
            hp.nrow = plen_h[good] - 1
            if cfg.interpolation and hp.T.shape[1] > 1:
                hp.seg_r, hp.seg_i = long_segments(hp.T, hp.nrow, n, cfg.ac_scale)
        if len(hp.seg_r):
            valid_np = lambda rows: self.valid(torch.tensor(rows, device=self.device)).cpu().numpy()
            hp.starts, hp.ends, hp.count, hp.walk, hp.fb = densify_cut(hp.T, hp.seg_r, hp.seg_i, n, cfg.ac_scale, self.limits.clip_state_np, valid_np)
        return self._fallback_or_done(job, SIMPLE)

    def _fallback_or_done(self, job, stage):
        """the segments left in host.fb go to the fallback planner of `stage` (one launch); none left: the job is done"""
        torch, cfg, hp, dev = _torch(), self.cfg, job.host, self.device
        if not hp.fb:
            job.result = assemble(hp, len(hp.ids_h), self.nq)
            return True
        iters, base = (self.simple_iters, 1) if stage == SIMPLE else (self.main_iters, 2)
        starts = wrap_unlimited(torch.tensor(hp.starts[hp.fb], device=dev), self.seam_idx)
        ends = wrap_unlimited(torch.tensor(hp.ends[hp.fb], device=dev), self.seam_idx)
        rows = hp.good[hp.seg_r[hp.fb]]
        total = int(cfg.env_id_total) if cfg.env_id_total else self.E
        ids = torch.tensor(total * base + int(cfg.env_id_base) + hp.ids_h[rows], dtype=torch.int64, device=dev)
        seeds = torch.tensor(cfg.seed + hp.steps_h[rows], dtype=torch.int64, device=dev)
        job.stage = stage
        if job.stream is None:
            job.path, job.plen, job.status = self._plan(stage, starts, ends, ids, seeds, iters)[:3]
        else:
            job.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(job.stream):
                job.path, job.plen, job.status = self._plan(stage, starts, ends, ids, seeds, iters, job.stream)[:3]
                job.held = (starts, ends, ids, seeds)
                job.event = torch.cuda.Event()
                job.event.record(job.stream)
        return None

    def _fallback_back(self, job, wait, then=None):
        """a fallback stage came back: rows = host.fb.  A solved segment gets the planner's rows (SamplingBasedPlanner.plan: start +
        running sum of successive differences; PlannerAgent drops row 0); the others go on to stage `then`, or (None) stay [end]"""
        if not self._ready(job, wait):
            return False
        hp = job.host
        plen_h, st_h = job.plen.cpu().numpy(), job.status.cpu().numpy()
        path_h = self._rows_h(job, plen_h)
        left = []
        for r, k in enumerate(hp.fb):
            if st_h[r] == 0:
                hp.replacement[k] = unwrap_rows(hp.starts[k], path_h[r, :plen_h[r]], self.seam_idx)[1:]
            elif then is not None:
                left.append(k)
            else:
                hp.replacement[k] = hp.ends[k][None]
        hp.fb = left
        return self._fallback_or_done(job, then)

    _stage_simple = partialmethod(_fallback_back, then=MAIN)
    _stage_main = partialmethod(_fallback_back, then=None)

    def _stage_split(self, job, wait):
        if not all([sub.result is not None or self.advance(sub, wait) for sub in job.subs]):      # (a list: every sub-job is advanced)
            return False
        job.result = join_results([s.result for s in job.subs], job.sub_rows, len(job.plen), self.nq)
        return True

    def _enqueue_device(self, job):
        """Stage RRT with the path post-processing on the device (batch.postprocess_paths: three small launches around one
        validity launch on the job's stream; one read-back of two totals); job.result will hold device tensors."""
        from .batch import postprocess_paths
        torch, cfg = _torch(), self.cfg
        on = lambda s: torch.cuda.stream(s) if s is not None else contextlib.nullcontext()
        if job.lazy is not None:        # continuation half of a chained launch: its rows of the continuation's outputs
            (src, rows), job.lazy = job.lazy, None
            if job.stream is not None and job.built is not None:
                job.stream.wait_event(job.built)
                job.built = None
            with on(job.stream):
                job.path, job.plen, job.status = src.path[rows], src.plen[rows], src.status[rows]
        pstream = None if job.post_on_main else job.stream
        if job.post_on_main:
            for x in (job.path, job.plen, job.status, job.cur):
                x.record_stream(torch.cuda.current_stream())
        with on(pstream):
            out, ln, need = postprocess_paths(job.path, job.plen, job.status, job.cur, self.n, cfg.ac_scale, cfg.interpolation, self.limits,
                                              self.valid, stream=pstream, seam_mask=self.seam_mask)
            st = job.status        # sentinel rows (sampling_based_planner.py:64-69): -5 goal invalid, -4 no exact solution
            job.dev = [out, ln, st == 0, st != _lib.PLAN_INVALID_GOAL, st != _lib.PLAN_NO_EXACT]
            rows = torch.nonzero(need).flatten()
            if len(rows):
                job.sub, job.sub_rows = job.subset(rows, pstream, unwrapped=True), rows
            job.event = torch.cuda.Event() if pstream is not None else None
            if job.event is not None:
                job.event.record(pstream)
        job.stage = DEVICE

    def _stage_device(self, job, wait, just_enqueued=False):
        # the launches of _enqueue_device (and the sub-job, if any) have to be finished.  Right after they were enqueued what is left is one small
        # assemble launch (the read-backs waited for the rest): waiting those microseconds out here saves the job, and its envs, a whole call
        torch = _torch()
        if not self._ready(job, wait or (just_enqueued and job.sub is None)):
            return False
        out, ln, ok, v, e = job.dev
        if job.sub is not None:
            if not self.advance(job.sub, wait):
                return False
            tr_s, ln_s = (torch.as_tensor(x, device=out.device) for x in job.sub.result[:2])
            if tr_s.shape[1] > out.shape[1]:
                out = torch.cat([out, torch.zeros(out.shape[0], tr_s.shape[1] - out.shape[1], self.nq, dtype=out.dtype, device=out.device)], dim=1)
            out[job.sub_rows, :tr_s.shape[1]] = tr_s
            ln[job.sub_rows] = ln_s
        job.result = (out, ln, ok, v, e)
        return True

    def plan(self, cur, target, env_ids, t_env):
        """`SACAgent.plan` (rl/sac_agent.py:198-235) for M envs, synchronously; `t_env` [E] int64: the step count of every env.
        Returns (traj [M, L, nq] tensor, length [M] int64 -- 0 where the plan failed --, and the boolean numpy arrays success,
        interpolation, valid, exact).  Only the envs that needed RRT-Connect are post-processed and written into their rows."""
        torch = _torch()
        cfg, M, cur = self.cfg, cur.shape[0], self.limits.clip_state(cur)
        traj_t, tlen, succ, _ = simple_interpolate_batch(self.bp, cur, target, cfg.ac_scale, list(range(self.n)))
        succ_h = succ.cpu().numpy()
        success, interpolation, valid, exact = succ_h.copy(), np.ones(M, dtype=bool), succ_h.copy(), succ_h.copy()
        lens = torch.where(succ, tlen.to(torch.int64), torch.zeros_like(tlen, dtype=torch.int64))
        fail = np.where(~succ_h)[0]
        if len(fail) == 0:
            return traj_t, lens, success, interpolation, valid, exact
        fi = torch.as_tensor(fail, device=cur.device)
        cur_f, tgt_f, ids = cur[fi].contiguous(), target[fi].contiguous(), env_ids[fi].contiguous()
        seeds = (t_env[ids] + cfg.seed).contiguous()
        tr_j, ln_j, s_j, v_j, e_j = self.finish(self.launch(cur_f, tgt_f, ids, t_env[ids].clone(), seeds))
        s_j, v_j, e_j = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (s_j, v_j, e_j))
        interpolation[fail] = False
        success[fail], valid[fail], exact[fail] = s_j, v_j, e_j
        traj_t, lens = merge_paths(traj_t, lens, tr_j, ln_j, fi)
        return traj_t, lens, success, interpolation, valid, exact
