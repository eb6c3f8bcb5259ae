"""Batched rollout step of MoPA-RL: the body of `MoPARolloutRunner.run`'s inner loop
(reference rl/mopa_rollouts.py:70-375) for E envs at once, on the batched pieces of this package.

One call of :meth:`BatchMoPARollout.agent_step` is one iteration of the reference's `while not done` loop for every
env: the policy action either is executed directly (`env.step(ac / omega)`, :336-356) or -- some |ac_j| > omega
(`is_planner_ac`, rl/sac_agent.py:148-153) -- is turned into a joint-space target (:116-131), pulled back while
invalid (:133-143), planned to (`SACAgent.plan`, rl/sac_agent.py:198-235: straight-line pre-check, then RRT-Connect,
then densification of the planner path) and executed waypoint by waypoint with `env.step(.., is_planner=True)` while
the SMDP reward `sum_i gamma^i r_i` and `intra_steps` are accumulated (:152-199); a failed plan costs one env step with
the current reward (:303-334).  Counters `mp / rl / interpolation / mp_fail / approximate / invalid` are kept per env.

Action spaces: joint-space MoPA-SAC, and MoPA + IK (`use_ik_target`: Cartesian displacement + rotation quaternion of the
ik_target site, turned into a joint displacement by the batched damped-LS IK -- BASELINE config 5; on an env with a 2-D world
box, PusherObstacle-v0, the 2 Cartesian entries alone and a position-only IK -- scripts/2d/mopa_ik.sh), and `discrete_action`
(the policy's `ac_type` head routes a step, :86-88,106-111,349).  Envs: the three Sawyer
obstacle envs (7 arm entries per action, Lift adds the gripper entry, which a planner step applies at
the last waypoint of its path, :163-167) and PusherObstacle-v0 (4 joints, joint0 UNLIMITED: query endpoints are wrapped into
(-3.14, 3.14) before planning and the returned steps un-wrapped across the seam, as `SamplingBasedPlanner.plan` does --
`wrap_unlimited`, `seam_steps_np`, `mopa_paths_unwrap_seam_batch`; `RolloutConfig.for_env` carries config/pusher.py).  The `reuse_data` relabelling (:204-300) -- extra transitions between random
pairs of waypoints of an executed path -- is fed by `agent_step(..., record=True)`: `reuse_transitions_device()` relabels all envs
in three launches and leaves the transitions on the device (a `ReuseBatch`), `reuse_transitions()` is the same rule as a host loop
over envs and draws (the checker of the device form; tests/test_reuse_gpu.py compares the two bit for bit).
The env is the KINEMATIC one (kinematic_env.py) -- not dynamics parity.

Where the work runs: every validity check (targets, pull-back, interpolated states, densification) and every
RRT-Connect query is one batched GPU launch over all envs that need it; env steps are one K4 launch per waypoint index.
The ragged bookkeeping of planner paths (a minority of envs per step) is done on the host in numpy with the same
arithmetic as the scalar code, so that results equal the per-env reference loop bit for bit (tests/test_gpu_rollout.py).
RNG streams: the RRT-Connect query of env e at agent step t uses (seed + t, stream e); the fallback planners inside the
densification use streams E + e (simple planner) and 2E + e (main planner); e is the GLOBAL env id (`env_id_base` + row) and
E the global env count (`env_id_total`), so a sharded rollout draws what the unsharded one draws.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import _lib
from .agent_planning import (JointLimits, action_to_displacement, displacement_to_action, interpolation_steps, max_interpolation_steps,
                             is_planner_action, seam_steps_np, simple_interpolate_batch, wrap_unlimited)
from .batch import BatchPlanner, _torch
from .plan_jobs import PlanJob, PlannerJobs, merge_paths
from .planner import ITERS_PER_SECOND
from .kinematic_env import KIND_PUSHER
from .scene import ENV_SPECS, planner_inputs

COUNTERS = ("mp", "rl", "interpolation", "mp_fail", "approximate", "invalid")


@dataclass
class RolloutConfig:
    """Defaults restated from the reference: config/__init__.py:24-110 (mopa section), config/sawyer.py:76-112,
    config/motion_planner.py:4-70.  `RolloutConfig.for_env(name)` fills the env-specific ones (config/pusher.py differs)."""
    omega: float = 0.7
    ac_space_type: str = "piecewise"
    action_range: float = 0.5
    ac_scale: float = 0.05
    invalid_target_handling: bool = True
    num_trials: int = 100
    step_size: float = 0.02
    interpolation: bool = True
    discount_factor: float = 0.99
    timelimit: float = 1.0
    simple_planner_timelimit: float = 0.05
    range: float = 0.1
    simple_planner_range: float = 0.05
    joint_margin: float = 0.001
    contact_threshold: float = -0.002
    max_nodes: int = 1024
    max_path: int = 256
    seed: int = 1234
    # K9: OMPL's two vertex-removing simplifier passes (reduceVertices, collapseCloseVertices) directly behind every launch of the
    # main / the simple planner (`BatchPlanner.plan(vertex_simplify=True)`); un-wrap and densification then work on the shorter
    # rows.  Not the reference's is_simplified (shortcutPath and the B-spline smoothing have their own flags below).
    vertex_simplify: bool = False
    simple_planner_vertex_simplify: bool = False
    # K9 shortcutPath in front of those passes (`BatchPlanner.plan(path_shortcut=True)`): the launch behind the planner's cuts
    # corners through the interior of segments, so the executed rows include states that are no planner rows
    path_shortcut: bool = False
    simple_planner_path_shortcut: bool = False
    # K9 smoothBSpline between shortcutPath and those passes (`BatchPlanner.plan(path_smooth=True)`): the launch behind the
    # planner's is `smooth_paths`; with all three flags it runs PathSimplifier::simplify's schedule without its wall clock
    path_smooth: bool = False
    simple_planner_path_smooth: bool = False
    # data-parallel runs (sample streams keyed by (seed, GLOBAL env id, iteration), so results do not depend on how
    # the envs are sharded): this rank's envs are rows env_id_base .. env_id_base + E - 1 of env_id_total envs in all
    # (rank * E and world * E; 0 total = this rank alone)
    env_id_base: int = 0
    env_id_total: int = 0
    # MoPA + IK action space (config/__init__.py --use_ik_target / --ik_target; rl/trainer.py:93-125): the policy outputs a
    # Cartesian displacement of the ik_target site (3) + a rotation quaternion (4) [+ the gripper entry]
    async_planner: bool = False       # RRT-Connect on side streams; envs waiting for a query sit out (see agent_step)
    planner_streams: int = 3          # RRT-Connect launches in flight at most (async_planner)
    planner_job_cap: int = 2048       # queries per asynchronous launch at most (the rest waits for the next free stream)
    planner_min_job: int = 1024       # queries an asynchronous launch waits for while other launches are in flight
    planner_first_iters: int = 300    # asynchronous launches first run with this iteration budget; the queries it does not solve
                                      # (a few %) are launched again with the full budget, among their kind.  A query's outcome
                                      # is a function of its endpoints and sample stream only, and a budget only ends the loop:
                                      # the second run retraces the first and goes on, so results are those of one full run --
                                      # but the many quick queries no longer wait for (or hold wave slots next to) the few that
                                      # take 2000 iterations.  0: one launch with the full budget
    device_paths: bool = True         # planner rows -> trajectories (un-wrap, densification) on the device (batch.postprocess_paths);
                                      # False: the array-operation form on the host (also serves the rare queries whose
                                      # densification needs the fallback planners)
    planner_chain: int = 1            # a first-phase launch is followed, on the same stream and with no host in between, by the
                                      # launch that continues its unsolved queries with the full budget (the kernel skips the
                                      # settled ones): the quick queries are picked up at an event between the two, the
                                      # budget-exhausting ones never wait in a retry pool.  0: pooled retry launches (round 2's form)
    planner_workgroups: int = 128     # persistent workgroups of an asynchronous launch.  A planner wave holds 256 registers (two
                                      # per SIMD): launches that took every slot would stall the main stream's kernels for their
                                      # whole bulk phase.  3 streams x 128 measured best on Push (tools/rollout_ab.sh: 1.03 M agent
                                      # steps/s; 3 x 64: 0.79 M, 2 x 256: 0.93 M)
    planner_chain_workgroups: int = 0 # workgroups of the continuation launch behind a first-phase launch (0: planner_workgroups).  With planner_exclusive
                                      # >= 1 that launch runs the workgroup-per-query build of K3 (four waves on a budget-exhausting query, the CU to itself):
                                      # few workgroups keep the CUs it takes away from the main stream's kernels few
    planner_exclusive: int = 0        # 1: the full-budget launches (continuation of a first-phase launch / pooled retries), 2: every asynchronous
                                      # planner launch keeps its CUs to itself (C ABI `exclusive_cu`): the one-wave-per-SIMD build of K3 with the
                                      # FP32 tree mirror in the CU's whole LDS (a budget-exhausting query: 41 instead of 46+ ms)
    discrete_action: bool = False     # --discrete_action (config/__init__.py:110; rl/mopa_rollouts.py:86-88,106-111,349): the policy's
                                      # `ac_type` head (1 = planner), not the action's magnitude, routes a step; direct actions
                                      # are then NOT divided by omega
    use_graphs: bool = False          # async_planner, joint-space actions, record=False: the fixed-shape halves of a call (policy
                                      # action -> target -> pull-back -> straight-line pre-check; execution + bookkeeping when no
                                      # planner launch finished in the call) are captured once as HIP graphs and replayed -- ~90
                                      # launches of host dispatch per call become two.  The returned tensors are then the graphs'
                                      # static buffers: valid until the next call
    walk_chunk: int = 0               # dynamics envs (a waypoint = one 75-sub-step physics launch whose time does not depend on how
                                      # many envs take part): a call executes at most this many waypoints per env; envs still on
                                      # their path are busy -- they sit out the policy's action of the following calls like envs
                                      # waiting for a query -- and complete their agent step in the call their walk ends in.  Every
                                      # env goes through the same transitions; launches stay full instead of draining towards the
                                      # longest path of the call.  0: a call walks every path to its end
    fused: bool = True                # the elementwise bookkeeping of a call as six library kernels (mopa_rollout_stage) instead of
                                      # ~170 torch launches; False: the torch form (the two agree bit for bit, tests/test_gpu_rollout.py)
    use_ik_target: bool = False
    ik_target: str = "grip_site"
    min_world_size: tuple = (-1.2, -1.2, 0.0)        # env/sawyer/sawyer.py:52-53
    max_world_size: tuple = (1.2, 1.2, 2.0)
    # (the Cartesian width of the IK action is len(min_world_size), rl/trainer.py:93-110: 3 + a rotation quaternion for the Sawyer envs; a
    #  2-D world box -- PusherObstacle-v0 -- makes it 2 entries and NO quaternion, and the IK position-only: scripts/2d/mopa_ik.sh)

    @property
    def n_cart(self) -> int:
        return len(self.min_world_size)

    @property
    def ik_has_quat(self) -> bool:
        """rl/trainer.py:100-104: the action has its `quat` entry only when the world box is 3-D"""
        return len(self.min_world_size) == 3

    @classmethod
    def for_env(cls, env_name: str, **over):
        """the config the reference builds for `env_name`: config/sawyer.py / config/pusher.py / config/motion_planner.py defaults as
        restated in scene.ENV_SPECS (Pusher: ac_scale 0.1, action_range 1.0, range 0.2, simple_planner_range 0.1,
        simple_planner_timelimit 0.02, step_size 0.04, joint_margin 0, contact_threshold -0.0015), then `over`."""
        from .scene import ENV_SPECS
        sp = ENV_SPECS[env_name]
        kw = dict(omega=sp.omega, action_range=sp.action_range, ac_scale=sp.ac_scale, num_trials=sp.num_trials, step_size=sp.step_size,
                  timelimit=sp.timelimit, simple_planner_timelimit=sp.simple_planner_timelimit, range=sp.range,
                  simple_planner_range=sp.simple_planner_range, joint_margin=sp.joint_margin, contact_threshold=sp.contact_threshold)
        if over.get("use_ik_target"):
            kw.update(IK_ENV_DEFAULTS.get(env_name, {}))
        kw.update(over)
        return cls(**kw)


# what `use_ik_target` reads from the env and its launch script where they differ from the Sawyer defaults of RolloutConfig:
# PusherObstacle-v0 (scripts/2d/mopa_ik.sh: --ik_target fingertip; env/pusher/pusher_obstacle.py:34-35: a 2-D world box)
IK_ENV_DEFAULTS = {"PusherObstacle-v0": dict(ik_target="fingertip", min_world_size=(-0.41, -0.41), max_world_size=(0.41, 0.41))}


def reuse_transitions(out, cfg, n_arm: int, rng, max_reuse_data: int = 30, grip_qpos_idx=None):
    """The `reuse_data` relabelling of rl/mopa_rollouts.py:204-300 on the record of one `agent_step(..., record=True)`:
    for every env that executed a planner path with more than 3 waypoints, up to min(len, max_reuse_data) random
    (start, goal) waypoint pairs become extra transitions  ob_list[start] --inverse-displacement action--> ob_list[goal]
    with reward (meta_rew[goal] - meta_rew[start]) * gamma^-(start+1), done = done_list[goal],
    intra_steps = goal - start - 1, kept only if the relabelled action is a planner action inside [-1, 1].
    `rng`: a numpy RandomState-like object (`randint(low, high)`) shared by all envs, or a callable env -> such an object
    (the reference draws from the global np.random, one env per process).
    `grip_qpos_idx`: qpos address of the first gripper joint for envs whose action has a gripper entry (Lift, dof 8):
    `env.form_action` appends that joint's difference (env/sawyer/sawyer.py:283-299), `valid_action` checks the whole vector,
    `is_planner_ac` the arm entries.
    Returns a list of dicts (env, start, goal, ob, ac, rew, done, intra_steps, ob_next) of numpy values."""
    rec = out["record"]
    if cfg.use_ik_target:
        # With use_ik_target the reference never moves target_qpos off curr_qpos (BatchMoPARollout._seg_pre), so a planner step
        # executes the two waypoints of a zero-length line and `len(ob_list) > 3` (:222) never holds: the IK branch of the
        # relabelling (:247-262, cart_list / quat_list) cannot be reached.  Anything longer here is not the reference's rollout.
        if bool((rec["n_exec"] > 3).any()):
            raise NotImplementedError("reuse_data relabelling for the IK action space (cart_list / quat_list, rl/mopa_rollouts.py:247-262)")
        return []
    if grip_qpos_idx is None and int(out["ac"].shape[1]) > n_arm:
        raise ValueError("the env's action has a gripper entry: pass grip_qpos_idx (BatchMoPARollout.reuse_transitions does)")
    ac_type = out["ac_type"].cpu().numpy() if (cfg.discrete_action and "ac_type" in out) else None
    ob, mr, dn, wp = (rec[k].cpu().numpy() for k in ("ob", "meta_rew", "done", "waypoint"))
    nexec = rec["n_exec"].cpu().numpy()
    extra = []
    for e in np.where(nexec > 3)[0]:
        draw = rng(int(e)) if callable(rng) else rng
        L = int(nexec[e])
        seen = set()
        for _ in range(min(L, max_reuse_data)):
            start = draw.randint(low=0, high=L - 1)
            if start + 1 > L - 1:
                continue
            goal = draw.randint(low=start + 1, high=L)
            if (start, goal) in seen:
                continue
            seen.add((start, goal))
            # env.form_action(traj[goal], traj[start]) -> pi.invert_displacement
            ac = displacement_to_action(wp[e, goal, :n_arm] - wp[e, start, :n_arm], cfg.ac_scale, cfg.omega, cfg.action_range,
                                        cfg.ac_space_type)
            is_planner = bool(np.any(ac < -cfg.omega) or np.any(ac > cfg.omega))
            if grip_qpos_idx is not None:
                ac = np.concatenate([ac, [wp[e, goal, grip_qpos_idx] - wp[e, start, grip_qpos_idx]]])
            in_box = bool(np.all(ac >= -1.0) and np.all(ac <= 1.0))
            if not (is_planner and in_box):
                continue
            rew = (mr[e, goal] - mr[e, start]) * cfg.discount_factor ** (-(start + 1))
            extra.append({"env": int(e), "start": start, "goal": goal, "ob": ob[e, start], "ac": ac, "rew": float(rew),
                          "done": int(dn[e, goal]), "intra_steps": goal - start - 1, "ob_next": ob[e, goal]})
            if ac_type is not None:       # `inter_subgoal_ac["ac_type"] = ac["ac_type"]` (rl/mopa_rollouts.py:266-267)
                extra[-1]["ac_type"] = int(ac_type[e])
    return extra


def draw_reuse_pairs(n_exec, max_reuse_data: int, rng):
    """The (start, goal) draws of `reuse_transitions` as a table [E, max_reuse_data, 2] int32 (numpy) for
    `BatchMoPARollout.reuse_transitions_device(..., pairs=...)`: `rng` (one object, or a callable env -> object) is consumed
    exactly as the host loop consumes it -- the same `randint` calls in the same order, envs with more than 3 executed
    waypoints only, min(n_exec, max_reuse_data) draws per env -- so the draws of a numpy RandomState (the reference's) reach
    the device.  A draw the host loop skips (no room for a goal; a pair its env drew before) is (-1, -1)."""
    nexec = n_exec.cpu().numpy() if hasattr(n_exec, "cpu") else np.asarray(n_exec)
    table = np.full((len(nexec), int(max_reuse_data), 2), -1, dtype=np.int32)
    for e in np.where(nexec > 3)[0]:
        draw = rng(int(e)) if callable(rng) else rng
        L = int(nexec[e])
        seen = set()
        for i in range(min(L, max_reuse_data)):
            start = draw.randint(low=0, high=L - 1)
            if start + 1 > L - 1:
                continue
            goal = draw.randint(low=start + 1, high=L)
            if (start, goal) in seen:
                continue
            seen.add((start, goal))
            table[e, i] = (start, goal)
    return table


@dataclass
class ReuseBatch:
    """What `BatchMoPARollout.reuse_transitions_device` returns: the relabelled transitions as device tensors.  `count` [1] int64
    is the number kept (the true number, also when it exceeds the capacity `cap` = rows of the other tensors); rows
    0 .. min(count, cap) - 1 are the transitions, ordered by env, then draw, as the host function lists them; rows behind them
    hold whatever the buffers held before.  `ac_type` is None unless the rollout has the discrete head."""
    count: "object"
    env: "object"
    start: "object"
    goal: "object"
    ob: "object"
    ac: "object"
    rew: "object"
    done: "object"
    intra_steps: "object"
    ob_next: "object"
    ac_type: "object" = None

    @property
    def cap(self) -> int:
        return int(self.env.shape[0])

    def to_list(self):
        """the host function's list of dicts of numpy values (the one place that reads back, and so waits for the device)"""
        n = min(int(self.count.cpu()[0]), self.cap)
        col = {k: getattr(self, k)[:n].cpu().numpy() for k in ("env", "start", "goal", "ob", "ac", "rew", "done", "intra_steps", "ob_next")}
        ac_type = self.ac_type[:n].cpu().numpy() if self.ac_type is not None else None
        out = []
        for r in range(n):
            out.append({"env": int(col["env"][r]), "start": int(col["start"][r]), "goal": int(col["goal"][r]), "ob": col["ob"][r],
                        "ac": col["ac"][r], "rew": float(col["rew"][r]), "done": int(col["done"][r]),
                        "intra_steps": int(col["intra_steps"][r]), "ob_next": col["ob_next"][r]})
            if ac_type is not None:
                out[-1]["ac_type"] = int(ac_type[r])
        return out


_INV_DISC = {}


def reuse_transitions_device(out, cfg, n_arm: int, max_reuse_data: int = 30, grip_qpos_idx=None, pairs=None, cap=None, env_mask=None,
                             into=None, t: int = 0):
    """`reuse_transitions` on the device (library call mopa_reuse_batch: three launches on the current stream, no read-back
    and no synchronisation): the record of `agent_step(..., record=True)` -> a `ReuseBatch` of device tensors whose rows are the
    host function's list, bit for bit and in its order (tests/test_reuse_gpu.py).
    pairs     [E, max_reuse_data, 2] int32 (numpy or device tensor; `draw_reuse_pairs` builds it from a RandomState-like
              object): draw i of env e; (-1, -1) and out-of-range entries emit nothing.  None: the draws come from the
              library's counter RNG on the device, key (cfg.seed + t, stream 3 * env_id_total + global env id) -- behind the
              planners' streams e, E + e, 2E + e --, counters 2i and 2i + 1 through randint(low, high) = low + min(int(u * (high -
              low)), high - low - 1): a sharded rollout draws what the unsharded one draws.
    cap       rows of the result (default E * max_reuse_data, which always suffices); `count` holds the true number either way
    env_mask  [E] bool / uint8: envs with a zero entry emit nothing (a `walk_chunk` rollout: the record of an env is complete
              only in the call in which it `stepped`)
    into      a ReuseBatch of the same shapes whose tensors are written (no allocation); rows beyond the count stay as they are
    The IK action space raises NotImplementedError (see `reuse_transitions`: the reference cannot reach that branch)."""
    torch = _torch()
    rec = out["record"]
    if cfg.use_ik_target:
        raise NotImplementedError("reuse_data relabelling for the IK action space (cart_list / quat_list, rl/mopa_rollouts.py:247-262)")
    if grip_qpos_idx is None and int(out["ac"].shape[1]) > n_arm:
        raise ValueError("the env's action has a gripper entry: pass grip_qpos_idx (BatchMoPARollout.reuse_transitions_device does)")
    normal = cfg.ac_space_type == "normal"
    if not normal and cfg.ac_space_type != "piecewise":
        raise NotImplementedError(cfg.ac_space_type)
    R = int(max_reuse_data)
    grip = -1 if grip_qpos_idx is None else int(grip_qpos_idx)
    dof = int(n_arm) + (1 if grip >= 0 else 0)
    ob, mr, dn, nexec = rec["ob"].contiguous(), rec["meta_rew"].contiguous(), rec["done"].contiguous(), rec["n_exec"].contiguous()
    wp = rec["waypoint"].contiguous()
    if not ob.is_cuda:
        raise _lib.MopaError("reuse_transitions_device: the record is not on a GPU (there is no CPU fallback; reuse_transitions is the host form)")
    E, L, D = (int(x) for x in ob.shape)
    f64 = torch.float64
    if (tuple(wp.shape[:2]) != (E, L) or tuple(mr.shape) != (E, L) or tuple(dn.shape) != (E, L) or tuple(nexec.shape) != (E,) or dn.dtype != torch.uint8
            or nexec.dtype != torch.int64 or ob.dtype != f64 or mr.dtype != f64 or wp.dtype != f64):
        raise _lib.MopaError("reuse_transitions_device: not a record of agent_step(..., record=True)")
    dev = ob.device
    ac_type = out["ac_type"].reshape(-1).to(torch.int32).contiguous() if (cfg.discrete_action and "ac_type" in out) else None
    if env_mask is not None:
        env_mask = env_mask.to(torch.uint8).contiguous()
        if tuple(env_mask.shape) != (E,):
            raise _lib.MopaError("reuse_transitions_device: env_mask is not [E]")
    if pairs is not None:
        pairs = torch.as_tensor(pairs, dtype=torch.int32).to(dev).contiguous()
        if tuple(pairs.shape) != (E, R, 2):
            raise _lib.MopaError(f"reuse_transitions_device: pairs is not [E, max_reuse_data, 2] = {(E, R, 2)}")
    cap = E * R if cap is None else int(cap)
    if into is None:
        rows = max(cap, 0)
        mk = lambda *sh, dt=f64: torch.empty(*sh, dtype=dt, device=dev)
        into = ReuseBatch(count=mk(1, dt=torch.int64), env=mk(rows, dt=torch.int32), start=mk(rows, dt=torch.int32), goal=mk(rows, dt=torch.int32),
                          ob=mk(rows, D), ac=mk(rows, dof), rew=mk(rows), done=mk(rows, dt=torch.uint8), intra_steps=mk(rows, dt=torch.int32),
                          ob_next=mk(rows, D), ac_type=mk(rows, dt=torch.int32) if ac_type is not None else None)
    elif into.cap != cap or tuple(into.ob.shape) != (cap, D) or tuple(into.ac.shape) != (cap, dof) or (into.ac_type is None) != (ac_type is None):
        raise _lib.MopaError("reuse_transitions_device: `into` has other shapes than this call")
    key = (str(dev), L, float(cfg.discount_factor))
    inv = _INV_DISC.get(key)
    if inv is None:      # gamma^-(start + 1) as the host function forms it, once per record length
        inv = _INV_DISC[key] = torch.tensor([cfg.discount_factor ** (-(k + 1)) for k in range(L)], dtype=f64, device=dev)
    work = torch.empty(2 * max(E, 1), dtype=torch.int64, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    # the constants of agent_planning.displacement_to_action, formed as its expressions form them (Python doubles)
    c1 = 1.0 if normal else (cfg.action_range - cfg.ac_scale) / (1.0 - cfg.ac_scale)
    c2 = 1.0 if normal else (1.0 - cfg.ac_scale) / (1.0 - cfg.omega)
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().mopa_reuse_batch(
        E, L, D, int(wp.shape[2]), int(n_arm), dof, grip, ptr(ob), ptr(mr), ptr(dn), ptr(wp), ptr(nexec), ptr(ac_type), ptr(env_mask),
        cfg.ac_scale, cfg.omega, cfg.omega / cfg.ac_scale, c1, c2, cfg.action_range, int(normal), ptr(inv), R, ptr(pairs),
        (int(cfg.seed) + int(t)) & 0xFFFFFFFFFFFFFFFF, int(cfg.env_id_base), int(cfg.env_id_total) or E, cap, ptr(work), ptr(into.count),
        ptr(into.env), ptr(into.start), ptr(into.goal), ptr(into.ac), ptr(into.rew), ptr(into.done), ptr(into.intra_steps), ptr(into.ob),
        ptr(into.ob_next), ptr(into.ac_type), stream.cuda_stream))
    for x in (ob, mr, dn, wp, nexec, ac_type, env_mask, pairs, inv, work):      # (tensors of another stream's allocator pool)
        if x is not None:
            x.record_stream(stream)
    return into


_SIDE_STREAMS = {}


def _side_streams(dev, n):
    """The planner's side streams, shared by every rollout object of the process: the GPU runs only a few hardware queues
    side by side (4 by default), streams beyond that share a queue with another stream and a 48 ms planner launch then sits
    in front of the main stream's kernels -- so streams are created once per device and handed out again."""
    torch = _torch()
    pool = _SIDE_STREAMS.setdefault(str(dev), [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


def ik_targets_torch(site_pos, site_mat, ac, action_range, world_lo, world_hi):
    """The IK problem of `ik_displacement` as array operations (what `BatchIK.targets` computes in one launch): returns (target_cart, target_quat)."""
    torch = _torch()
    lo = torch.tensor(world_lo, dtype=torch.float64, device=ac.device)
    hi = torch.tensor(world_hi, dtype=torch.float64, device=ac.device)
    target_cart = torch.minimum(torch.maximum(site_pos + action_range * ac[:, :3], lo), hi).contiguous()
    m = site_mat.to(torch.float32).to(torch.float64)                      # np.array(rmat, dtype=np.float32)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i, j] for i in range(3) for j in range(3))
    tr = m00 + m11 + m22
    # closed-form quaternion, branch on the largest of (trace, m00, m11, m22) for conditioning
    qw = torch.stack([1.0 + tr, m21 - m12, m02 - m20, m10 - m01], dim=1)
    qx = torch.stack([m21 - m12, 1.0 + m00 - m11 - m22, m01 + m10, m02 + m20], dim=1)
    qy = torch.stack([m02 - m20, m01 + m10, 1.0 - m00 + m11 - m22, m12 + m21], dim=1)
    qz = torch.stack([m10 - m01, m02 + m20, m12 + m21, 1.0 - m00 - m11 + m22], dim=1)
    pick = torch.stack([tr, m00, m11, m22], dim=1).argmax(dim=1)
    q = torch.stack([qw, qx, qy, qz], dim=1)[torch.arange(len(m), device=m.device), pick]      # (w, x, y, z), unnormalised
    q = q / q.norm(dim=1, keepdim=True)
    q = torch.where(q[:, :1] < 0, -q, q)
    tq = torch.stack([q[:, 0], q[:, 1], q[:, 2], q[:, 2]], dim=1)                               # [[3, 0, 1, 1]] of (x, y, z, w)
    aq = ac[:, 3:7] / ac[:, 3:7].norm(dim=1, keepdim=True)
    aw, ax, ay, az = tq.unbind(1)
    bw, bx, by, bz = aq.unbind(1)
    target_quat = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                               aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=1).contiguous()
    return target_cart, target_quat


def ik_targets_pos_np(site_pos, ac, n_cart: int, action_range: float, world_lo, world_hi):
    """The position-only IK target in the reference's own numpy words (rl/mopa_rollouts.py:91-98, then :684-690 for a 2-D world box):
    the checker of `BatchIK.targets_pos` (bit for bit).  site_pos [E, 3], ac [E, >= n_cart] -> target_cart [E, 3]."""
    site_pos, ac = np.asarray(site_pos, dtype=np.float64), np.asarray(ac, dtype=np.float64)
    lo, hi = np.asarray(world_lo, dtype=np.float64), np.asarray(world_hi, dtype=np.float64)
    cart = np.clip(site_pos[:, :n_cart] + action_range * ac[:, :n_cart], lo, hi)
    return np.concatenate((cart, site_pos[:, n_cart:]), axis=1)


def sit_out_action(ac, alive, use_ik_target: bool, has_quat: bool = True):
    """The action `run_episode` hands to `agent_step`: the policy's rows for the envs still in their episode, a neutral row for the
    envs that sit out.  Neutral is all zeros -- except, with `use_ik_target`, the rotation entries ac[3:7]: `k_ik_targets` divides them
    by their norm as the reference does (rl/mopa_rollouts.py:696), so they are the identity quaternion (1, 0, 0, 0); a zero row would
    make the IK target, the joint displacement and from there `env.qpos` of the env NaN.  An IK action without a quaternion
    (`has_quat=False`: a 2-D world box, RolloutConfig.ik_has_quat) has nothing to divide by: its neutral row is all zeros too."""
    torch = _torch()
    neutral = torch.zeros_like(ac, dtype=torch.float64)
    if use_ik_target and has_quat:
        neutral[:, 3] = 1.0
    return torch.where(alive[:, None], ac.to(torch.float64), neutral).contiguous()


class BatchMoPARollout:
    def reuse_transitions(self, out, rng, max_reuse_data: int = 30):
        """`reuse_transitions` on a recorded step of this rollout, with the env's gripper joint supplied where its action has
        a gripper entry (Lift)"""
        f = self.env.facts
        grip = int(f.grip_qpos_idx[0]) if self.ac_dim > self.n and len(f.grip_qpos_idx) else None
        return reuse_transitions(out, self.cfg, self.n, rng, max_reuse_data=max_reuse_data, grip_qpos_idx=grip)

    def reuse_transitions_device(self, out, max_reuse_data: int = 30, pairs=None, cap=None, env_mask=None, into=None):
        """`reuse_transitions_device` on a recorded step of this rollout: the gripper joint is supplied as in
        `reuse_transitions`; without `pairs` the draws are keyed by (cfg.seed + self.t, cfg.env_id_base, cfg.env_id_total or E)
        -- `self.t` as it stands when this is called.  Runs on the current stream; returns a `ReuseBatch`."""
        f = self.env.facts
        grip = int(f.grip_qpos_idx[0]) if self.ac_dim > self.n and len(f.grip_qpos_idx) else None
        return reuse_transitions_device(out, self.cfg, self.n, max_reuse_data=max_reuse_data, grip_qpos_idx=grip, pairs=pairs, cap=cap,
                                        env_mask=env_mask, into=into, t=self.t)

    def __init__(self, env, cfg: Optional[RolloutConfig] = None):
        torch = _torch()
        self.env = env
        self.cfg = cfg if cfg is not None else RolloutConfig()
        if abs(env.ac_scale - self.cfg.ac_scale) > 0:
            raise _lib.MopaError("env.ac_scale and RolloutConfig.ac_scale differ")
        spec = ENV_SPECS[env.env_name]
        pi = planner_inputs(env.env_name, env.model)
        # unlimited joints (`non_limited_idx`, rl/trainer.py:80-82; Pusher: joint0): SamplingBasedPlanner wraps a query's start and
        # goal into (-3.14, 3.14) there before planning and takes the returned steps across the seam the short way round
        # (motion_planners/sampling_based_planner.py:51-55,60-99) -- `wrap_unlimited` / the seam mask of the path post-processing
        self._seam_idx = [int(i) for i in pi.non_limited_idx]
        self._seam_mask = sum(1 << i for i in self._seam_idx)
        self.pi = pi
        dev_index = env.device.index if env.device.index is not None else -1
        mk = lambda r: _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, self.cfg.contact_threshold, range_=r,
                                  seed=self.cfg.seed, device=dev_index)
        self.scene, self.simple_scene = mk(self.cfg.range), mk(self.cfg.simple_planner_range)
        self.bp, bp_simple = BatchPlanner(self.scene), BatchPlanner(self.simple_scene)
        self.E, self.nq, self.n = env.E, env.nq, env.n_arm
        self.arm = list(int(i) for i in env.facts.arm_qpos_idx)
        assert self.arm == list(range(self.n)), "the reference slices qpos[:n] (rl/sac_agent.py:275-278)"
        f = env.facts
        dev, f64 = env.device, torch.float64
        self.limits = JointLimits(f.qpos_min, f.qpos_max, f.qpos_limited, self.cfg.joint_margin, device=dev)
        self.counters: Dict[str, "object"] = {k: torch.zeros(self.E, dtype=torch.int64, device=dev) for k in COUNTERS}
        self.t_env = torch.zeros(self.E, dtype=torch.int64, device=dev)     # agent steps every env has completed
        self._t = 0
        self._t_dev = torch.zeros((), dtype=torch.int64, device=dev)         # the same counter on the device (captured launches read it)
        self.busy = torch.zeros(self.E, dtype=torch.bool, device=dev)        # env waits for an RRT-Connect query (async_planner)
        self._jobs = []          # PlanJobs in flight (plan_jobs.py)
        # created on first use: profiling dict (set from outside) + its last mark, HIP graphs, fused step struct, walk_chunk state, pool counts
        self.timing = self._mark_t = self._graphs = self._fs = self._walk = self._count_ring = self._count_free = self._pool_counts = None
        # blocked envs waiting for the next RRT-Connect launch: mask + their (clipped) current state and target
        self._pool_mask = torch.zeros(self.E, dtype=torch.bool, device=dev)
        self._res = None      # per-env parking buffers of planner state between a first-phase launch and its retry (_park_state)
        self._retry_mask = torch.zeros(self.E, dtype=torch.bool, device=dev)     # ... and those whose first, short launch ran out
        self._wait_since = torch.zeros(self.E, dtype=torch.int64, device=dev)    # call in which an env started to wait
        self.n_retried = torch.zeros((), dtype=torch.int64, device=dev)
        self._q_cur = torch.zeros(self.E, self.nq, dtype=torch.float64, device=dev)
        self._q_tgt = torch.zeros(self.E, self.nq, dtype=torch.float64, device=dev)
        self._k_interp = max_interpolation_steps(self.cfg.action_range, self.cfg.ac_scale)
        self._interp_overflow = torch.zeros((), dtype=torch.bool, device=dev)
        self._disc = {}
        # a state that is certainly valid (the env's initial pose): stands in for the rows a launch has no business with
        self._safe_q = torch.tensor(np.asarray(env.init_qpos_row, dtype=np.float64)[None], device=dev)
        if not bool(self._valid(self._safe_q)[0]):
            raise _lib.MopaError("the env's initial pose is not a valid state")
        self._streams = _side_streams(dev, max(1, self.cfg.planner_streams)) if self.cfg.async_planner else []
        self._next_stream = 0
        self.main_iters = max(1, int(round(self.cfg.timelimit * ITERS_PER_SECOND)))
        self.simple_iters = max(1, int(round(self.cfg.simple_planner_timelimit * ITERS_PER_SECOND)))
        self.jobs = PlannerJobs(self.cfg, self.bp, bp_simple, self.limits, self._valid, self.n, self.nq, self._seam_idx, self._seam_mask, self.E,
                                self.main_iters, self.simple_iters, dev)
        self.ik = None
        if self.cfg.use_ik_target:
            from .ik import BatchIK
            self.ik = BatchIK(env.model, self.cfg.ik_target, spec.robot_joints, device=dev_index)
            self._world_lo = torch.tensor(self.cfg.min_world_size, dtype=f64, device=dev)
            self._world_hi = torch.tensor(self.cfg.max_world_size, dtype=f64, device=dev)
            # `_cart2dispalcement` clips the IK result against env._jnt_minimum/_jnt_maximum[jnt_indices] (float64; unlimited
            # joints carry +-3.14 there, env/base.py:85-86) -- only the arm entries are read back
            self._ik_lo = torch.tensor(f.qpos_min[self.arm], dtype=f64, device=dev)
            self._ik_hi = torch.tensor(f.qpos_max[self.arm], dtype=f64, device=dev)
            if self.cfg.n_cart not in (2, 3) or len(self.cfg.max_world_size) != self.cfg.n_cart:
                raise _lib.MopaError("min_world_size / max_world_size must both hold 2 or 3 entries")
            if not self.cfg.ik_has_quat and env.action_dim != self.n:
                raise NotImplementedError("a position-only IK action with further action entries (no such env in the reference)")
        # Cartesian entries of the IK action: 3 + the rotation quaternion, or the 2 of a 2-D world box without one
        self._ik_ac = (self.cfg.n_cart + (4 if self.cfg.ik_has_quat else 0)) if self.cfg.use_ik_target else 0
        self.ac_dim = (self._ik_ac if self.cfg.use_ik_target else self.n) + (env.action_dim - self.n)
        self._pend_ob = torch.zeros(self.E, env.obs_dim, dtype=f64, device=dev)      # ob / ac of the step a busy env is in
        self._pend_ac = torch.zeros(self.E, self.ac_dim, dtype=f64, device=dev)
        self._ac_type_in = torch.zeros(self.E, dtype=torch.int64, device=dev)      # discrete_action: this call's ac_type / that of a pending step
        self._pend_type = torch.zeros(self.E, dtype=torch.int64, device=dev)
        # contact force (`env.get_contact_force()` after every env.step, rl/mopa_rollouts.py:538-539, :636-637): on the envs whose contacts run
        # behind a constraint solver (K7 / K8) the env accumulates it per launch on the device; `_cf_mark` = the accumulator when an
        # env's agent step began, so a step's force is total - mark however its env.steps were spread over launches and calls
        self._cf_mark = None
        if getattr(env, "has_contact_solver", None) is not None and env.has_contact_solver():
            if env.contact_force is None:
                env.enable_contact_force()
            self._cf_mark = env.contact_force_total.clone()

    # ------------------------------------------------------------------
    def close(self):
        self.scene.close()
        self.simple_scene.close()

    def clip_qpos(self, q):
        """`SACAgent.clip_qpos` (rl/sac_agent.py:237-260) per row, with the float32 limits the agents hold."""
        return self.limits.clip_state(q)

    def ik_displacement(self, ac, cur):
        """`MoPARolloutRunner._cart2dispalcement` (rl/mopa_rollouts.py:87-99,681-728) for E envs: the policy's Cartesian action
        -> joint displacement of the arm through the damped-LS IK (K5).
            target_cart = clip(site_xpos + action_range * ac[:3], world box)
            target_quat = mulQuat(q_site[(w, x, y, y)], ac[3:7] / |ac[3:7]|)      # the reference indexes [3, 0, 1, 1] (sic)
            qpos_from_site_pose(ik_env, ik_target, target_cart, target_quat, robot_joints, max_steps=100, tol=1e-2)
            displacement = clip(result, joint limits)[arm] - curr[arm]
        q_site is the site's orientation as `util.env.mat2quat` returns it: from the float32-rounded rotation matrix, sign
        w >= 0.  (The reference takes the dominant eigenvector of the 4 x 4 K-matrix; for a rotation matrix that is the
        closed-form quaternion used here, to the float32 rounding of the matrix -- a 1e-7 effect on the target.)"""
        torch = _torch()
        cfg = self.cfg
        if not cfg.ik_has_quat:
            # a 2-D world box (PusherObstacle-v0): no `quat` entry, target_quat=None, the site's own z appended to the 2-D target
            # (:684-699) -- the whole pre-step in one launch (`BatchIK.displacement_pos`; cur is read, not written)
            return self.ik.displacement_pos(cur.contiguous(), ac, cfg.n_cart, cfg.action_range, cfg.min_world_size, cfg.max_world_size,
                                            self._ik_lo, self._ik_hi, max_steps=100, tol=1e-2)
        site_pos, site_mat = self.ik.site_pose(cur.contiguous())
        # (one launch; the module's `ik_targets_torch` is the array-operation form it replaced -- ~70 elementwise launches per call -- kept as
        #  the checker of tests/test_gpu_ik.py)
        target_cart, target_quat = self.ik.targets(site_pos, site_mat, ac, cfg.action_range, cfg.min_world_size, cfg.max_world_size)
        q_ik = cur.clone()
        self.ik.solve(q_ik, target_cart, target_quat, max_steps=100, tol=1e-2)
        arm_t = torch.minimum(torch.maximum(q_ik[:, :self.n], self._ik_lo), self._ik_hi)
        return arm_t - cur[:, :self.n]

    def _valid(self, q):
        return self.bp.is_valid(q[:, self.arm].contiguous(), q.contiguous(), samples_per_env=1).bool()

    # ------------------------------------------------------------------
    @property
    def t(self) -> int:
        """agent steps taken (lock-step count); part of the planner's sample-stream key.  Assigning it puts every env at that
        step (tests replay recorded steps)."""
        return self._t

    @t.setter
    def t(self, value: int):
        self._t = int(value)
        self._t_dev.fill_(int(value))
        self.t_env.fill_(int(value))

    def plan(self, cur, target, env_ids):
        """`SACAgent.plan` (rl/sac_agent.py:198-235) for M envs, synchronously: `PlannerJobs.plan` with this rollout's step counts"""
        return self.jobs.plan(cur, target, env_ids, self.t_env)

    # ------------------------------------------------------------------
    def agent_step(self, ac, record: bool = False, ac_type=None):
        """One agent step for all E envs.  ac: float64 [E, >= self.ac_dim] GPU tensor (policy output in [-1, 1]).
        Returns a dict of GPU tensors: ob [E,obs_dim] (before), ac (the action each transition belongs to), ob_next
        [E,obs_dim], rew [E] (SMDP return of the step), done [E] uint8, intra_steps [E] int64, is_planner [E] bool, success [E]
        (env success flag), `path_len`, `plan_ok`, and `stepped` [E] bool: the envs that completed an agent step in this call.
        On an env with contacts behind a constraint solver (K7 / K8) also `contact_force` [E]: `env.get_contact_force()` summed over
        every env.step of the agent step (all waypoints of a planner path, rl/mopa_rollouts.py:538-539) -- parity unpinned.
        record=True adds `record`: per executed waypoint k the obs after it, the running SMDP return, the done flag and
        the waypoint itself ([E, L, ...]; `n_exec` [E] = waypoints actually executed) -- the `ob_list / meta_rew_list /
        done_list / traj` of the reference, input of `reuse_transitions`.

        Lock-step (default): every env steps in every call; the call returns when the slowest RRT-Connect query of the step is
        done.  `cfg.async_planner`: the RRT-Connect queries of a call run on side streams while the call returns; their envs
        are `busy` -- they sit out the following calls (their rows of `ac` are ignored) -- until their query has finished, and
        complete their step (path execution or the failed-plan step) in the first call after that.  Envs are independent and a
        query's sample stream is keyed by the env's own step count, so each env goes through the same sequence of transitions
        either way; only their interleaving differs.  Rows of the outputs are meaningful where `stepped`."""
        if self.cfg.discrete_action:
            if ac_type is None:
                raise _lib.MopaError("discrete_action: agent_step needs the policy's ac_type [E] (1 = motion planner, 0 = direct)")
            self._ac_type_in.copy_(ac_type.reshape(-1))
        if self.cfg.use_graphs and not record and self.timing is None:
            return self._agent_step_graphs(ac)
        if self._cf_mark is not None:      # envs that begin an agent step in this call (a reset since the last one has zeroed their total)
            self._cf_mark.copy_(_torch().where(self.busy, self._cf_mark, self.env.contact_force_total))
        bag = self._seg_pre(ac)
        self._seg_plan(bag)
        res = self._seg_exec(bag, record)
        self._t += 1
        return res

    def _agent_step_graphs(self, ac, warmup: int = 2):
        """agent_step with the two fixed-shape parts replayed from HIP graphs (cfg.use_graphs).  The first `warmup` calls run
        eagerly on the stream the graphs are then captured on -- so that every per-stream scratch buffer of the library
        exists before capture --, the capture itself is the execution of its call (capture, then replay)."""
        torch = _torch()
        if self.cfg.use_ik_target or not self.cfg.async_planner:
            raise _lib.MopaError("use_graphs serves the asynchronous joint-space rollout")
        if getattr(self.env, "dynamics", False):
            # waypoint execution through the physics loops over a data-dependent path length on the host: not capturable
            raise _lib.MopaError("use_graphs serves the kinematic env (a dynamics env executes waypoints step by step on the host)")
        G = self._graphs
        main = torch.cuda.current_stream(self.env.device)
        if G is None:
            G = self._graphs = {"calls": 0, "stream": torch.cuda.Stream(device=self.env.device), "pool": torch.cuda.graph_pool_handle(),
                                "ac": torch.zeros(self.E, ac.shape[1], dtype=torch.float64, device=self.env.device),
                                "pre": None, "exec": None}
        st = G["stream"]
        if G["calls"] < warmup:
            G["calls"] += 1
            st.wait_stream(main)
            with torch.cuda.stream(st):
                bag = self._seg_pre(ac)
                self._seg_plan(bag)
                res = self._seg_exec(bag, False)
            for v in res.values():
                v.record_stream(main)
            main.wait_stream(st)
            self._t += 1
            return res
        G["ac"].copy_(ac)
        import os as _os
        which = _os.environ.get("MOPA_ROLLOUT_GRAPHS", "both")       # pre | exec | both: bisecting knob
        if which == "exec":
            bag = self._seg_pre(G["ac"])
            self._seg_plan(bag)
            res = self._seg_exec(bag, False)
            self._t += 1
            return res
        if G["pre"] is None:
            st.wait_stream(main)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=G["pool"], stream=st, capture_error_mode="relaxed"):
                G["bag"] = self._seg_pre(G["ac"])
            G["pre"] = g
        G["pre"].replay()
        bag = dict(G["bag"])
        self._seg_plan(bag)
        if which == "both" and bag["n_finished"] == 0 and bag["traj_pad"] is G["bag"]["traj_pad"]:
            bag["finished"] = None       # (the all-false mask is then created inside the graph: a static buffer)
            if G["exec"] is None:
                st.wait_stream(main)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=G["pool"], stream=st, capture_error_mode="relaxed"):
                    G["res"] = self._seg_exec(bag, False)
                G["exec"] = g
            G["exec"].replay()
            res = G["res"]
        else:
            res = self._seg_exec(bag, False)
        self._t += 1
        return res

    def _mark(self, name):
        tm = self.timing     # optional dict: phase -> seconds (each mark synchronises; profiling only)
        if tm is None:
            return
        import time as _time
        torch = _torch()
        torch.cuda.current_stream().synchronize()    # the main stream only: planner launches on side streams go on
        now = _time.perf_counter()
        if self._mark_t is not None and name is not None:
            tm[name] = tm.get(name, 0.0) + now - self._mark_t
        self._mark_t = now

    # The three parts of a call.  _seg_pre and _seg_exec have fixed shapes, touch persistent state only IN PLACE and read no
    # Python-side counters, so they can be captured as graphs; _seg_plan is host logic (planner launches, pick-ups).
    def _seg_pre(self, ac):
        """policy action -> planner / direct, target, pull-back, straight-line pre-check; blocked envs join the pool"""
        torch = _torch()
        env, cfg, E, n = self.env, self.cfg, self.E, self.n
        mark = self._mark
        mark(None)
        if cfg.fused:
            return self._seg_pre_fused(ac)
        busy0 = self.busy.clone()
        active = ~busy0
        prev_ob = torch.where(busy0[:, None], self._pend_ob, env.obs)
        ac_tr = torch.where(busy0[:, None], self._pend_ac, ac[:, :self.ac_dim])
        cur = env.qpos.clone()
        if cfg.use_ik_target:
            # MoPA + IK: the action is Cartesian; its joint displacement decides planner / direct and IS the direct action
            a = self.ik_displacement(ac, cur)
            extra_ac = ac_tr[:, self._ik_ac:self._ik_ac + (env.action_dim - n)]
            mark("ik")
        else:
            a = ac[:, :n].contiguous()
            extra_ac = ac_tr[:, n:env.action_dim]
        if cfg.discrete_action:
            # the discrete head decides (rl/mopa_rollouts.py:86-88,106-111); a busy env's pending step keeps its own type
            ac_type = torch.where(busy0, self._pend_type, self._ac_type_in)
            is_pl = (ac_type != 0) & active
        else:
            ac_type = None
            is_pl = is_planner_action(a, cfg.omega) & active
        # Everything below works on all E rows with masks -- no index lists, so no host read-back of how many envs take which
        # branch.  Rows that are not planner actions carry a known-valid dummy state through the validity launches; nothing of
        # theirs is used.
        safe = self._safe_q
        if cfg.use_ik_target:
            # (with use_ik_target the reference never moves target_qpos off curr_qpos -- :113-131 is skipped and
            # `_cart2dispalcement` keeps its result local --, so a planner step plans from the current state to itself: two
            # zero-motion env steps.  Reproduced as is.)
            target = cur
        else:
            target = cur.clone()
            target[:, :n] += action_to_displacement(a, cfg.ac_scale, cfg.omega, cfg.action_range, cfg.ac_space_type)
            target = self.limits.clip_target(target)          # np.clip to the joint limits, unlimited entries restored (:121-131)
        target = torch.where(is_pl[:, None], target, safe).contiguous()
        if cfg.invalid_target_handling:
            target, _, tv = self.bp.pullback(torch.where(is_pl[:, None], cur, safe).contiguous(), target, cfg.step_size, cfg.num_trials)
            tv = tv.bool()
        else:
            tv = self._valid(target)
        mark("target")
        bad_target = (is_pl & ~tv).to(torch.int64)       # invalid target: success, valid, exact = False, False, True
        self.counters["mp_fail"] += bad_target
        self.counters["invalid"] += bad_target
        pv = is_pl & tv
        # ---- SACAgent.plan: straight-line pre-check for all of them in one launch (:198-204) ----
        cur_v = torch.where(pv[:, None], self.clip_qpos(cur), safe).contiguous()
        tgt_v = torch.where(pv[:, None], target, safe).contiguous()
        traj_i, tlen, succ, nst = simple_interpolate_batch(self.bp, cur_v, tgt_v, cfg.ac_scale, self.arm, fixed_steps=self._k_interp)
        # a line that needs more than the fixed width (cur outside its limits by more than action_range) is not executed as a
        # truncated walk: it goes the planner's way; drain() still reports it
        over = nst > self._k_interp
        self._interp_overflow |= over.any()
        succ = succ & ~over
        plan_ok = pv & succ
        self.counters["interpolation"] += plan_ok.to(torch.int64)
        traj_pad = torch.where(plan_ok[:, None, None], traj_i, torch.zeros_like(traj_i))
        path_len = torch.where(plan_ok, tlen.to(torch.int64), torch.zeros_like(tlen, dtype=torch.int64))
        mark("interpolate")
        # ---- the blocked ones go to RRT-Connect; lock-step waits for it below, async_planner does not ----
        blocked = pv & ~succ
        self._q_cur.copy_(torch.where(blocked[:, None], cur_v, self._q_cur))
        self._q_tgt.copy_(torch.where(blocked[:, None], tgt_v, self._q_tgt))
        self._pool_mask |= blocked
        self._wait_since.copy_(torch.where(blocked, self._t_dev.expand_as(self._wait_since), self._wait_since))
        self.busy |= blocked
        self._pend_ob.copy_(torch.where(blocked[:, None], prev_ob, self._pend_ob))
        self._pend_ac.copy_(torch.where(blocked[:, None], ac_tr, self._pend_ac))
        if cfg.discrete_action:
            self._pend_type.copy_(torch.where(blocked, ac_type, self._pend_type))
        return {"ac_type": ac_type, "active": active, "prev_ob": prev_ob, "ac_tr": ac_tr, "a": a, "extra_ac": extra_ac, "is_pl": is_pl, "plan_ok": plan_ok,
                "traj_pad": traj_pad, "path_len": path_len, "n_finished": 0}

    def _park_state(self, ps, jid, again):
        """the planner state (trees, counters) of a first-phase launch's unsolved queries -> the per-env parking buffers"""
        torch = _torch()
        from .batch import PlanState
        E, w = self.E, 2 * ps.max_nodes * ps.na
        if self._res is None:
            dev = ps.state.device
            self._res = PlanState(torch.empty(E * w + 8, dtype=torch.float64, device=dev), torch.empty(E * 2 * ps.max_nodes, dtype=torch.int32, device=dev),
                                  torch.zeros(E, 4, dtype=torch.int64, device=dev), ps.max_nodes, ps.na)
        rows = torch.nonzero(again).flatten()
        if len(rows) == 0:
            return
        env_rows = jid[rows]
        n = ps.state.shape[0]
        self._res.tree_q[:E * w].view(E, w)[env_rows] = ps.tree_q[:n * w].view(n, w)[rows]
        self._res.tree_p.view(E, 2 * ps.max_nodes)[env_rows] = ps.tree_p.view(n, 2 * ps.max_nodes)[rows]
        self._res.state[env_rows] = ps.state[rows]
        for x in (ps.tree_q, ps.tree_p, ps.state):
            x.record_stream(torch.cuda.current_stream())

    def _pick_rows(self, mask, kind_in_flight, min_job, cap):
        """the waiting envs of `mask` that go into a launch now, taken out of the mask: (ids ascending, start rows, target rows, step
        counts, seeds), or None -- nothing waits, or too few while a launch of their kind is in flight (the pool waits for company)"""
        torch, cfg = _torch(), self.cfg
        if cfg.fused and cfg.async_planner and mask.is_cuda:
            # the pick-up in one library launch (ids ascending as torch.nonzero lists them, mask cleared, start / target rows, step counts
            # and seeds gathered) when the count lies within [what a launch waits for, the launch's cap]; one read-back as before
            picked = self._pool_pick(mask, 1 if not kind_in_flight else min_job, cap)
            if picked[0] == 0 or (picked[1] is None and picked[0] <= cap):
                return None
            if picked[1] is not None:
                return picked[1:]
        bi = torch.nonzero(mask).flatten()
        if not (len(bi) and (not cfg.async_planner or len(bi) >= min_job or not kind_in_flight)):
            return None
        if cfg.async_planner and len(bi) > cap:
            # the envs that have waited longest go first (a plain prefix would starve the high env indices whenever more wait than a launch takes)
            bi = bi[torch.argsort(self._wait_since[bi], stable=True)[:cap]]
        bi = bi.contiguous()
        mask[bi] = False
        cur, tgt, seeds = self._q_cur[bi].contiguous(), self._q_tgt[bi].contiguous(), (self.t_env[bi] + cfg.seed).contiguous()
        return bi, cur, tgt, self.t_env[bi].clone(), seeds

    def _seg_plan(self, bag):
        """RRT-Connect launches for the pooled envs, pick-up of the launches that are done (host logic, dynamic shapes)"""
        torch, cfg = _torch(), self.cfg
        # One K3 launch takes about as long for 40 queries as for 4000 (its time is the latency of the slowest query), so the
        # waiting envs of several calls share a launch: a job starts only when a side stream has no job in flight (and only
        # then the waiting envs are listed: the one read-back of this part).
        two_phase = cfg.async_planner and 0 < cfg.planner_first_iters < self.main_iters
        for retry in ((False, True) if two_phase else (False,)):
            used = {j.stream for j in self._jobs}
            side = next((st for st in self._streams if st not in used), None)      # (lock-step: there are no side streams)
            if side is None and cfg.async_planner:
                break
            # (a launch costs the host about as much as a call: with several streams free, small pools wait for company
            # unless nothing of their kind is in flight)
            kind_in_flight = any(j.retry == retry for j in self._jobs)
            min_job = cfg.planner_min_job // 4 if retry else cfg.planner_min_job
            known = self._pool_counts_known() if cfg.async_planner else None
            if known is not None:
                # listing the waiting envs reads their number back (the host waits for the stream): only in calls in which
                # the count an earlier call left behind says a launch is due
                if not (known[int(retry)] >= min_job or (known[int(retry)] > 0 and not kind_in_flight)):
                    continue
            picked = self._pick_rows(self._retry_mask if retry else self._pool_mask, kind_in_flight, min_job,
                                     cfg.planner_job_cap // 4 if retry else cfg.planner_job_cap)
            if picked is None:
                continue
            if bool(self._interp_overflow):
                raise _lib.MopaError(f"a straight-line pre-check needed more than {self._k_interp} steps (targets further than "
                                     "action_range from the current state?)")
            bi, cur_p, tgt_p, steps_p, seeds_p = picked
            # a first-phase launch keeps its trees; the retry launch of its unsolved queries continues from them (parked per
            # env in between) instead of retracing the first iterations -- or, chained, goes behind it on its stream
            first = two_phase and not retry and side is not None
            res_in = None
            if retry and self._res is not None:
                from .batch import PlanState
                res_in = PlanState(self._res.tree_q, self._res.tree_p, self._res.state, cfg.max_nodes, self._res.na).rows(bi)
            job = self.jobs.launch(cur_p, tgt_p, bi, steps_p, seeds_p, stream=side, keep=first, resume=res_in,
                                   iters=cfg.planner_first_iters if (two_phase and not retry) else self.main_iters,
                                   chain=bool(cfg.planner_chain) and first and cfg.device_paths and self.nq <= 64)
            job.retry = retry
            self._jobs.append(job)
        # ---- RRT-Connect jobs that are done (lock-step: all of them) ----
        bag["finished"] = torch.zeros(self.E, dtype=torch.bool, device=self.env.device) if self._jobs else None
        jobs, self._jobs = self._jobs, []
        for job in jobs:
            if self.jobs.advance(job, wait=not cfg.async_planner):
                self._fold(job, bag)
            else:
                self._jobs.append(job)
        self._mark("plan")

    def _fold(self, job, bag):
        """a finished job's rows -> plan_ok / traj_pad / path_len of the call, `busy` and the counters; the queries a first-phase launch
        left unsolved go on to their retry (pooled: `_retry_mask`; chained: a job of their own joins `_jobs`)"""
        torch, dev, plan_ok, path_len = _torch(), self.env.device, bag["plan_ok"], bag["path_len"]
        tr_j, ln_j, s_j, v_j, e_j = job.result
        if job.stream is not None:
            # results allocated on the job's side stream are read by this stream's launches below: tell the allocator,
            # or the next job could be handed their memory while those launches are still queued
            for x in job.result:
                if hasattr(x, "record_stream"):
                    x.record_stream(torch.cuda.current_stream())
        jid, t = job.ids, lambda x: torch.as_tensor(x, device=dev)
        s_t, v_t, e_t = t(s_j), t(v_j), t(e_j)
        # (everything below is index arithmetic over the job's rows with a `fin` mask -- no boolean-mask indexing: each `x[mask]` is a
        #  torch.nonzero underneath, three launches, a memset and a read-back the host waits for)
        fin = None
        if job.iters < self.main_iters:
            # first-phase launch: "no exact solution" may only mean that the short budget ran out -- those queries run
            # again with the full budget (their envs stay busy); everything else is final
            again = ~s_t & ~e_t
            if job.chain is not None:
                rows = torch.nonzero(again).flatten()
                if len(rows):
                    nxt = PlanJob.continuation(job, rows, self.main_iters)
                    # its tensors come from THIS stream's ops (nonzero, gathers) and are read on the side stream later:
                    # an event the side stream waits for, and the allocator told about the second reader
                    nxt.built = torch.cuda.Event()
                    nxt.built.record(torch.cuda.current_stream())
                    if job.stream is not None:
                        for x in (nxt.ids, nxt.cur, nxt.target, nxt.steps, rows):
                            x.record_stream(job.stream)
                    self._jobs.append(nxt)
            else:
                self._retry_mask[jid] = self._retry_mask[jid] | again
                if job.pstate is not None:
                    self._park_state(job.pstate, jid, again)
            self.n_retried = self.n_retried + again.sum()
            fin = ~again
        ok_f = s_t if fin is None else (s_t & fin)
        bad_f = ~s_t if fin is None else (~s_t & fin)
        bag["finished"][jid] = True if fin is None else fin
        bag["n_finished"] += 1
        plan_ok[jid] = s_t if fin is None else torch.where(fin, s_t, plan_ok[jid])
        self.counters["mp"].index_add_(0, jid, ok_f.to(self.counters["mp"].dtype))
        self.counters["mp_fail"].index_add_(0, jid, bad_f.to(self.counters["mp_fail"].dtype))
        self.counters["approximate"].index_add_(0, jid, (bad_f & ~e_t).to(self.counters["approximate"].dtype))
        self.counters["invalid"].index_add_(0, jid, (bad_f & ~v_t).to(self.counters["invalid"].dtype))
        ln_t = t(ln_j)
        if fin is not None:      # (the rows of the queries that run again keep their length 0: their trajectory rows are never read)
            ln_t = torch.where(fin, ln_t.to(path_len.dtype), path_len[jid])
        bag["traj_pad"], bag["path_len"] = merge_paths(bag["traj_pad"], path_len, t(tr_j), ln_t, jid)
        self.busy[jid] = False if fin is None else (self.busy[jid] & ~fin)

    def _seg_exec(self, bag, record: bool = False):
        """direct steps, failed-plan steps and waypoint execution; counters and the returned transition"""
        torch = _torch()
        env, cfg, E, n = self.env, self.cfg, self.E, self.n
        dev = env.device
        mark = self._mark
        active, is_pl, a, extra_ac = bag["active"], bag["is_pl"], bag["a"], bag["extra_ac"]
        plan_ok, traj_pad, path_len, prev_ob, ac_tr = bag["plan_ok"], bag["traj_pad"], bag["path_len"], bag["prev_ob"], bag["ac_tr"]
        finished = bag.get("finished")
        if finished is None:
            finished = torch.zeros(E, dtype=torch.bool, device=dev)
        chunked = cfg.walk_chunk > 0 and getattr(env, "dynamics", False)
        if cfg.fused and not chunked:
            return self._seg_exec_fused(bag, record)
        direct = active & ~is_pl
        self.counters["rl"] += direct.to(torch.int64)
        sitting = self.busy & ~finished            # still waiting for their query (or on a walk): nothing of theirs is touched
        stepped = ~sitting
        # ---- direct execution (:336-356) and failed plans (:303-334: reward of the current state, one env step) in one launch
        # (:349-352: with the discrete head the direct action goes to the env as it is, otherwise rescaled by 1 / omega)
        act0 = torch.where(direct[:, None], a if cfg.discrete_action else a / torch.full_like(a, cfg.omega), torch.zeros_like(a))
        if env.action_dim > n:          # Lift: the gripper entry is passed through unscaled (:340-343)
            act0 = torch.cat([act0, torch.where(direct[:, None], extra_ac, torch.zeros_like(extra_ac))], dim=1)
        act0 = act0.contiguous()
        flags = torch.where(direct, 1, torch.where(plan_ok | sitting, 2, 0)).to(torch.uint8).contiguous()
        is_pl_out = is_pl | finished
        last_extra = extra_ac[:, 0].contiguous() if env.action_dim > n else None
        rec = None
        if chunked:
            # (the direct / failed-plan steps share a launch with the first waypoint of every env on a walk)
            rew, done, intra, rec, path_len, plan_ok, is_pl_out, stepped = self._walk_chunk(bag, act0, flags, record, sitting, is_pl_out, last_extra)
        else:
            env._launch(act0, False, flags)
            rew = torch.where(plan_ok, torch.zeros_like(env.reward), env.reward)
            done = torch.where(plan_ok, torch.zeros_like(env.done), env.done)
            intra = torch.zeros(E, dtype=torch.int64, device=dev)
            # ---- waypoint execution (:152-199)
            L = traj_pad.shape[1]
            if record:
                rec = {"ob": torch.zeros(E, L, env.obs.shape[1], dtype=torch.float64, device=dev),
                       "meta_rew": torch.zeros(E, L, dtype=torch.float64, device=dev),
                       "done": torch.zeros(E, L, dtype=torch.uint8, device=dev),
                       "waypoint": traj_pad, "n_exec": torch.zeros(E, dtype=torch.int64, device=dev)}
            # one launch: every env walks its own waypoints until its path ends or a step reports done (envs without a path: length 0)
            disc = self._disc_pow(L)
            rew, done = rew.contiguous(), done.to(torch.uint8).contiguous()
            env.exec_trajectories(traj_pad.contiguous(), torch.where(plan_ok, path_len, torch.zeros_like(path_len)).contiguous(), disc,
                                  rew, done, intra, rec={k: rec[k] for k in ("ob", "meta_rew", "done", "n_exec")} if rec else None,
                                  last_extra=last_extra)
        mark("execute")
        if chunked:
            env.has_prev.copy_(torch.where(self._walk["on"], env.has_prev, torch.zeros_like(env.has_prev)))
        else:
            env.has_prev.zero_()                                 # env._reset_prev_state()
        self.t_env += stepped.to(torch.int64)
        self._t_dev += 1
        res = {"ob": prev_ob, "ac": ac_tr, "ob_next": env.obs.clone(), "rew": rew, "done": done, "intra_steps": intra,
               "is_planner": is_pl_out, "success": env.success.clone(), "path_len": path_len, "plan_ok": plan_ok, "stepped": stepped}
        if cfg.discrete_action:
            res["ac_type"] = bag["ac_type"]
        if rec is not None:
            res["record"] = rec
        return self._cf_out(res)

    # ---- the same two parts with the elementwise work in the library's bookkeeping kernels (cfg.fused) ----
    def _fused_struct(self):
        torch = _torch()
        if self._fs is not None:
            return self._fs
        import ctypes as C
        env, cfg = self.env, self.cfg
        if _lib.lib().mopa_rollout_step_size() != C.sizeof(_lib.MopaRolloutStep):
            raise _lib.MopaError("MopaRolloutStep: the binding's layout differs from the library's")
        S = self._fs = _lib.MopaRolloutStep()
        S.E, S.nq, S.n_arm, S.ac_dim, S.adim, S.obs_dim, S.K = self.E, self.nq, self.n, self.ac_dim, env.action_dim, env.obs.shape[1], self._k_interp
        S.discrete, S.normal_space = int(cfg.discrete_action), int(cfg.ac_space_type == "normal")
        if cfg.ac_space_type not in ("normal", "piecewise"):
            raise NotImplementedError(cfg.ac_space_type)
        S.omega, S.ac_scale, S.action_range = cfg.omega, cfg.ac_scale, cfg.action_range
        S.omega_over_scale, S.one_minus_omega, S.range_minus_scale = cfg.omega / cfg.ac_scale, 1 - cfg.omega, cfg.action_range - cfg.ac_scale
        lim = self.limits
        self._fs_keep = [t.contiguous() for t in (lim.lo, lim.hi, lim.lo_state, lim.hi_state, lim.lo_shrunk, lim.hi_shrunk, self._safe_q.reshape(-1))]
        for k, t in zip(("lim_lo", "lim_hi", "lo_state", "hi_state", "lo_shrunk", "hi_shrunk", "safe_q"), self._fs_keep):
            setattr(S, k, t.data_ptr())
        if self._interp_overflow.dtype != torch.bool:
            raise _lib.MopaError("interp_overflow must be a bool scalar")
        return S

    def _fused_bind(self, **tensors):
        """device addresses of this call's tensors -> the step struct (None -> NULL); every tensor must be contiguous"""
        S = self._fs
        for k, t in tensors.items():
            if t is None:
                setattr(S, k, None)
                continue
            if not t.is_contiguous():
                raise _lib.MopaError(f"rollout step buffer {k} is not contiguous")
            setattr(S, k, t.data_ptr())

    def _pool_pick(self, mask, min_n: int, cap: int):
        """mopa_rollout_pool_pick on the current stream: (count, ids, start rows, target rows, step counts, seeds) of the envs whose `mask` byte is
        set -- the last five None when the count is outside [min_n, cap] (nothing was touched then)."""
        torch = _torch()
        from .batch import _stream_handle
        dev = mask.device
        ids = torch.empty(cap, dtype=torch.int64, device=dev)
        cur = torch.empty(cap, self.nq, dtype=torch.float64, device=dev)
        tgt = torch.empty(cap, self.nq, dtype=torch.float64, device=dev)
        steps = torch.empty(cap, dtype=torch.int64, device=dev)
        seeds = torch.empty(cap, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().mopa_rollout_pool_pick(self.E, self.nq, int(min_n), int(cap), mask.data_ptr(), self._q_cur.data_ptr(), self._q_tgt.data_ptr(),
                                                     self.t_env.data_ptr(), int(self.cfg.seed), ids.data_ptr(), cur.data_ptr(), tgt.data_ptr(),
                                                     steps.data_ptr(), seeds.data_ptr(), cnt.data_ptr(), _stream_handle(None)))
        n = int(cnt.item())
        if n < min_n or n > cap:
            return n, None, None, None, None, None
        return n, ids[:n], cur[:n], tgt[:n], steps[:n], seeds[:n]

    def _pool_counts_known(self):
        """(envs waiting for a planner launch, for a retry launch) as of the latest earlier call whose bookkeeping has finished
        on the device, or None (torch form of the calls / no such call yet): copied to pinned memory behind each call"""
        ring = self._count_ring
        if not ring:
            return None
        for k in range(len(ring) - 1, -1, -1):
            if ring[k][0].query():
                self._count_free.extend(ring[:k])             # older entries (finished before this one, same stream) are recycled
                del ring[:k]
                return [int(x) for x in ring[0][1]]
        return None

    def _pool_counts_push(self):
        torch = _torch()
        if self._count_ring is None:
            self._count_ring, self._count_free = [], []
        ring = self._count_ring
        # at most two calls enqueued ahead of the device: the planner's pick-ups are decided on the host's clock, and a host
        # far ahead would enqueue calls in which envs sit out although their query has long finished
        pending = [r for r in ring if not r[0].query()]
        if len(pending) >= 2:
            pending[0][0].synchronize()
        while len(ring) > 4:
            self._count_free.append(ring.pop(0))
        ev, host = self._count_free.pop() if self._count_free else (torch.cuda.Event(), torch.zeros(2, dtype=torch.int64).pin_memory())
        host.copy_(self._pool_counts, non_blocking=True)
        ev.record(torch.cuda.current_stream())
        ring.append((ev, host))

    def _fused_stage(self, stage):
        import ctypes as C
        from .batch import _stream_handle
        _lib.check(_lib.lib().mopa_rollout_stage(C.byref(self._fs), int(stage), _stream_handle(None)))

    def _seg_pre_fused(self, ac):
        torch = _torch()
        from .batch import _ptr, _stream_handle
        env, cfg, E, n, nq = self.env, self.cfg, self.E, self.n, self.nq
        dev, f64, u8, i64 = env.device, torch.float64, torch.bool, torch.int64
        mark = self._mark
        S = self._fused_struct()
        ac = ac if ac.is_contiguous() else ac.contiguous()
        if ac.dtype != f64 or ac.shape[0] != E or ac.shape[1] < self.ac_dim:
            raise _lib.MopaError("agent_step: ac must be float64 [E, >= ac_dim]")
        a_in = None
        if cfg.use_ik_target:
            a_in = self.ik_displacement(ac, env.qpos.clone()).contiguous()
            mark("ik")
        em = lambda *sh, dt=f64: torch.empty(*sh, dtype=dt, device=dev)
        n_extra = env.action_dim - n
        B = {"prev_ob": em(E, S.obs_dim), "ac_tr": em(E, self.ac_dim), "a": em(E, n), "extra_ac": em(E, max(n_extra, 1)),
             "target": em(E, nq), "cur_m": em(E, nq), "cur_v": em(E, nq), "tgt_v": em(E, nq), "traj": em(E, self._k_interp + 1, nq),
             "active": em(E, dt=u8), "is_pl": em(E, dt=u8), "pv": em(E, dt=u8), "plan_ok": em(E, dt=u8),
             "ac_type": em(E, dt=i64) if cfg.discrete_action else None, "path_len": em(E, dt=i64)}
        S.ac_stride = int(ac.shape[1])
        c = self.counters
        self._fused_bind(qpos=env.qpos, obs=env.obs, reward=env.reward, done=env.done, success=env.success, has_prev=env.has_prev,
                         busy=self.busy, pool_mask=self._pool_mask, interp_overflow=self._interp_overflow, wait_since=self._wait_since,
                         t_dev=self._t_dev, t_env=self.t_env, pend_type=self._pend_type, q_cur=self._q_cur, q_tgt=self._q_tgt,
                         pend_ob=self._pend_ob, pend_ac=self._pend_ac, c_rl=c["rl"], c_interp=c["interpolation"], c_mp_fail=c["mp_fail"],
                         c_invalid=c["invalid"], ac=ac, ac_type_in=self._ac_type_in, a_in=a_in, **B)
        self._fused_stage(0)
        if cfg.invalid_target_handling:
            trials = em(E, dt=torch.int32)
            tv = em(E, dt=torch.uint8)
            _lib.check(_lib.lib().mopa_pullback_batch(self.scene.handle, _ptr(B["cur_m"]), _ptr(B["target"]), E, float(cfg.step_size), int(cfg.num_trials),
                                                      _ptr(trials), _ptr(tv), _stream_handle(None)))
        else:
            tv = self._valid(B["target"]).contiguous()
        mark("target")
        self._fused_bind(tv=tv)
        self._fused_stage(1)
        tlen, ok, nst = em(E, dt=torch.int32), em(E, dt=torch.uint8), em(E, dt=torch.int32)
        _lib.check(_lib.lib().mopa_interpolate_batch(self.scene._h, E, n, self._k_interp, _ptr(B["cur_v"]), _ptr(B["tgt_v"]), float(cfg.ac_scale),
                                                     _ptr(B["traj"]), _ptr(tlen), _ptr(ok), _ptr(nst), _stream_handle(None)))
        self._fused_bind(tlen=tlen, ok=ok, nst=nst)
        self._fused_stage(2)
        mark("interpolate")
        self._fs_call = (ac, a_in, tv, tlen, ok, nst)          # alive until the call's last stage has been enqueued
        return {"ac_type": B["ac_type"], "active": B["active"], "prev_ob": B["prev_ob"], "ac_tr": B["ac_tr"], "a": B["a"],
                "extra_ac": B["extra_ac"][:, :n_extra] if n_extra else B["extra_ac"][:, :0], "is_pl": B["is_pl"], "plan_ok": B["plan_ok"],
                "traj_pad": B["traj"], "path_len": B["path_len"], "n_finished": 0, "_extra_buf": B["extra_ac"]}

    def _seg_exec_fused(self, bag, record: bool = False):
        torch = _torch()
        env, cfg, E, n = self.env, self.cfg, self.E, self.n
        dev, f64, u8, i64 = env.device, torch.float64, torch.bool, torch.int64
        mark = self._mark
        S = self._fs
        em = lambda *sh, dt=f64: torch.empty(*sh, dtype=dt, device=dev)
        traj_pad, plan_ok, path_len = bag["traj_pad"], bag["plan_ok"], bag["path_len"]
        lift = env.action_dim > n
        X = {"act0": em(E, env.action_dim), "flags": em(E, dt=torch.uint8), "sitting": em(E, dt=u8), "stepped": em(E, dt=u8),
             "is_pl_out": em(E, dt=u8), "plen_m": em(E, dt=i64), "last_extra": em(E) if lift else None, "rew": em(E),
             "done_out": em(E, dt=torch.uint8), "intra": em(E, dt=i64), "ob_next": em(E, S.obs_dim), "success_out": em(E, dt=env.success.dtype)}
        # (the planner's pick-ups may have replaced plan_ok / path_len rows in place and widened traj_pad)
        counting = cfg.async_planner and not cfg.use_graphs
        if counting and self._pool_counts is None:
            self._pool_counts = torch.zeros(2, dtype=i64, device=dev)
        self._fused_bind(finished=bag.get("finished"), plan_ok=plan_ok, path_len=path_len, active=bag["active"], is_pl=bag["is_pl"], a=bag["a"],
                         extra_ac=bag["_extra_buf"], retry_mask=self._retry_mask if counting else None,
                         pool_counts=self._pool_counts if counting else None, **X)
        self._fused_stage(3)
        env._launch(X["act0"], False, X["flags"])
        self._fused_stage(4)
        rec = None
        L = traj_pad.shape[1]
        if record:
            rec = {"ob": torch.zeros(E, L, env.obs.shape[1], dtype=f64, device=dev), "meta_rew": torch.zeros(E, L, dtype=f64, device=dev),
                   "done": torch.zeros(E, L, dtype=torch.uint8, device=dev), "waypoint": traj_pad, "n_exec": torch.zeros(E, dtype=i64, device=dev)}
        env.exec_trajectories(traj_pad if traj_pad.is_contiguous() else traj_pad.contiguous(), X["plen_m"], self._disc_pow(L), X["rew"], X["done_out"],
                              X["intra"], rec={k: rec[k] for k in ("ob", "meta_rew", "done", "n_exec")} if rec else None, last_extra=X["last_extra"])
        mark("execute")
        self._fused_stage(5)
        if counting:
            self._pool_counts_push()
        self._fs_call = None
        res = {"ob": bag["prev_ob"], "ac": bag["ac_tr"], "ob_next": X["ob_next"], "rew": X["rew"], "done": X["done_out"], "intra_steps": X["intra"],
               "is_planner": X["is_pl_out"], "success": X["success_out"], "path_len": path_len, "plan_ok": plan_ok, "stepped": X["stepped"]}
        if cfg.discrete_action:
            res["ac_type"] = bag["ac_type"]
        if rec is not None:
            res["record"] = rec
        return self._cf_out(res)

    def _cf_out(self, res):
        """`contact_force` of the envs that completed their agent step: the env's accumulator minus its value when the step began"""
        if self._cf_mark is None:
            return res
        torch = _torch()
        tot, st = self.env.contact_force_total, res["stepped"].bool()
        res["contact_force"] = torch.where(st, tot - self._cf_mark, torch.zeros_like(tot))
        self._cf_mark.copy_(torch.where(st, tot, self._cf_mark))
        return res

    def _disc_pow(self, L):
        disc = self._disc.get(L)
        if disc is None:
            disc = self._disc[L] = _torch().tensor([self.cfg.discount_factor ** k for k in range(L)], dtype=_torch().float64, device=self.env.device)
        return disc

    def _walk_chunk(self, bag, act0, flags0, record, sitting, is_pl_out, last_extra):
        """cfg.walk_chunk (dynamics env): the paths handed out in this call join the persistent walk state; every env on a walk
        advances by at most walk_chunk waypoints, each a physics launch over all envs on a walk -- the first of them also
        carries this call's direct and failed-plan steps (act0 / flags0).  The envs whose walk ended complete their agent
        step, the others stay busy.  Per env the arithmetic is that of one uninterrupted walk."""
        torch = _torch()
        env, cfg, E, n = self.env, self.cfg, self.E, self.n
        dev = env.device
        plan_ok, traj_pad, path_len = bag["plan_ok"], bag["traj_pad"], bag["path_len"]
        L = int(traj_pad.shape[1])
        W = self._walk
        if W is None:
            z = lambda *sh, dt=torch.float64: torch.zeros(*sh, dtype=dt, device=dev)
            W = self._walk = {"on": z(E, dt=torch.bool), "traj": z(E, L, self.nq), "len": z(E, dt=torch.int64), "pos": z(E, dt=torch.int64),
                              "rew": z(E), "done": z(E, dt=torch.uint8), "intra": z(E, dt=torch.int64), "is_pl": z(E, dt=torch.bool),
                              "extra": z(E), "rec": None}
        if L > W["traj"].shape[1]:                                   # a longer path than any before: widen (rare)
            grow = lambda x: torch.cat([x, torch.zeros(E, L - x.shape[1], *x.shape[2:], dtype=x.dtype, device=dev)], dim=1)
            W["traj"] = grow(W["traj"])
            if W["rec"] is not None:
                for k in ("ob", "meta_rew", "done"):
                    W["rec"][k] = grow(W["rec"][k])
        Lw = int(W["traj"].shape[1])
        if L < Lw:
            traj_pad = torch.cat([traj_pad, torch.zeros(E, Lw - L, self.nq, dtype=traj_pad.dtype, device=dev)], dim=1)
        on0 = W["on"]
        new = plan_ok & ~sitting                                     # paths handed out in this call (straight lines, finished queries)
        zi = torch.zeros_like(W["len"])
        W["traj"].copy_(torch.where(new[:, None, None], traj_pad, W["traj"]))
        W["len"].copy_(torch.where(new, torch.clamp(path_len, max=Lw), torch.where(on0, W["len"], zi)))
        W["pos"].copy_(torch.where(on0, W["pos"], zi))
        W["rew"].copy_(torch.where(on0, W["rew"], torch.zeros_like(W["rew"])))
        W["done"].copy_(torch.where(on0, W["done"], torch.zeros_like(W["done"])))
        W["intra"].copy_(torch.where(on0, W["intra"], zi))
        W["is_pl"].copy_(torch.where(on0, W["is_pl"], is_pl_out))
        if last_extra is not None:
            W["extra"].copy_(torch.where(new, last_extra, W["extra"]))
        rec = None
        if record:
            if W["rec"] is None:
                W["rec"] = {"ob": torch.zeros(E, Lw, env.obs.shape[1], dtype=torch.float64, device=dev),
                            "meta_rew": torch.zeros(E, Lw, dtype=torch.float64, device=dev),
                            "done": torch.zeros(E, Lw, dtype=torch.uint8, device=dev), "n_exec": torch.zeros(E, dtype=torch.int64, device=dev)}
            rec = W["rec"]
            fresh = ~on0
            rec["ob"].copy_(torch.where(fresh[:, None, None], torch.zeros_like(rec["ob"]), rec["ob"]))
            rec["meta_rew"].copy_(torch.where(fresh[:, None], torch.zeros_like(rec["meta_rew"]), rec["meta_rew"]))
            rec["done"].copy_(torch.where(fresh[:, None], torch.zeros_like(rec["done"]), rec["done"]))
            rec["n_exec"].copy_(torch.where(fresh, torch.zeros_like(rec["n_exec"]), rec["n_exec"]))
        disc = self._disc_pow(Lw)
        ext = W["extra"] if last_extra is not None else None
        # the launch runs with planner-step semantics (the action IS the displacement): a direct action's arm entries are
        # multiplied by ac_scale here instead of in the kernel -- the same one multiplication.  (Pusher: `desired_state = prev +
        # action` in both step forms, env/pusher/pusher_obstacle.py:262-266 -- nothing to multiply.)
        other = act0.clone()
        if env.kind != KIND_PUSHER:
            other[:, :n] = act0[:, :n] * torch.full_like(act0[:, :n], cfg.ac_scale)
        walked = env.walk_round(W["traj"], W["len"], W["pos"], disc, W["rew"], W["done"], W["intra"], rec, ext, other_action=other, other_flags=flags0)
        rew1, done1 = env.reward.clone(), env.done.clone()           # of the envs that took their direct / failed-plan step
        if cfg.walk_chunk > 1:
            env.exec_trajectories(W["traj"], W["len"], disc, W["rew"], W["done"], W["intra"], rec=rec, last_extra=ext, pos=W["pos"],
                                  chunk=cfg.walk_chunk - 1)
        still = W["pos"] < W["len"]
        # envs on a walk are busy: the following calls ignore the policy's rows for them; the transition's first half is parked
        # exactly as for envs waiting for a query
        self._pend_ob.copy_(torch.where(still[:, None], bag["prev_ob"], self._pend_ob))
        self._pend_ac.copy_(torch.where(still[:, None], bag["ac_tr"], self._pend_ac))
        if cfg.discrete_action:
            self._pend_type.copy_(torch.where(still, bag["ac_type"], self._pend_type))
        self.busy.copy_((self.busy & ~on0) | still)
        W["on"] = still
        stepped = (~sitting | on0) & ~still
        walker = on0 | new
        out_rec = None
        if record:
            out_rec = {k: v.clone() for k, v in rec.items()}
            out_rec["waypoint"] = W["traj"].clone()
        return (torch.where(walker, W["rew"], rew1), torch.where(walker, W["done"], done1.to(torch.uint8)), W["intra"].clone(), out_rec,
                torch.where(walker, W["len"], path_len), plan_ok | on0, W["is_pl"].clone(), stepped)

    def drain(self):
        """wait for every RRT-Connect launch in flight (async_planner); their envs complete their step in a following agent_step"""
        for job in self._jobs:
            if job.event is not None:
                job.event.synchronize()

    def run_episode(self, policy, max_step: int = 10000, is_train: bool = True, random_exploration: bool = False, reset: bool = True):
        """`MoPARolloutRunner.run_episode` (reference rl/mopa_rollouts.py:401-678: the evaluation loop -- ONE episode, `while not done
        and ep_len < max_step`, every agent step the same routing as `run`) for all E envs at once: each env runs one episode from
        `env.reset()` (`reset=False`: from the state the env is in) and sits out once its episode is over: it gets the neutral action
        of `sit_out_action`, nothing of it is recorded any more, and after every call it is put back into the state its episode ended
        in -- when the loop returns, `env.qpos` is `qpos_final` and `env.obs` the final obs of every env.  Lock-step only: a call is one
        agent step of every env still in its episode.

        policy(ob [E, obs_dim], is_train=..., random_exploration=...) -> ac [E, >= ac_dim] (float64, in [-1, 1]; with
        `discrete_action` a pair (ac, ac_type [E])) -- the batched `pi.act` (:432-437).

        What differs from `run`, as in the reference: the per-step reward of a planner step is the PLAIN sum of its waypoints'
        rewards (`meta_rew += reward`, :540 -- not the discounted SMDP return of :171), a failed plan is one step with the current
        reward (:594-611), no `reuse_data` transitions.  Returns (rollout, ep_info):
          rollout  ob [T + 1, E, obs_dim] (row t = the obs an env's t-th agent step started from; the row after its last step = the
                   final obs: `rollout.add({"ob": ll_ob})`, :661), ac [T, E, ac_dim], rew [T, E], done [T, E] uint8, valid [T, E] bool
                   (env e took an agent step in call t), n_steps [E], qpos_final [E, nq] (the state each episode ended in) -- the reference's
                   evaluation rollout holds ob / ac of planner steps only (:577-585 against :648-653), this one of every step;
          ep_info  len, rew (:663-670), success (the env's `episode_success`), and the six counters (:671), one entry per env.
        On an env with contacts behind a constraint solver (K7 / K8) ep_info also holds `contact_force` (:538-539, :636-637: the sum of
        `env.get_contact_force()` over every env.step of the episode) and `avg_conntact_force` (the reference's key, :669-675: that sum
        / len) -- from the restated solver, PARITY UNPINNED against MuJoCo; a kinematic env has no contact forces and reports neither
        key.  `max_step` below the
        env's own episode cap would cut a path between two waypoints (:575): build the env with that cap instead."""
        torch = _torch()
        env, cfg, E = self.env, self.cfg, self.E
        if cfg.async_planner:
            raise _lib.MopaError("run_episode is the lock-step evaluation loop (async_planner=False)")
        if max_step < env.max_episode_steps:
            raise _lib.MopaError(f"max_step {max_step} < the env's max_episode_steps {env.max_episode_steps}: make the env with that episode cap")
        dev = env.device
        if reset:
            env.reset()
        gamma, disc_cache = cfg.discount_factor, self._disc
        cfg.discount_factor, self._disc = 1.0, {}
        try:
            alive = torch.ones(E, dtype=torch.bool, device=dev)
            ep_len = torch.zeros(E, dtype=torch.int64, device=dev)
            ep_rew = torch.zeros(E, dtype=torch.float64, device=dev)
            cnt = {k: torch.zeros(E, dtype=torch.int64, device=dev) for k in COUNTERS}
            success = torch.zeros(E, dtype=torch.bool, device=dev)
            ep_cf = torch.zeros(E, dtype=torch.float64, device=dev) if self._cf_mark is not None else None
            obs, acs, rews, dones, valids = [], [], [], [], []
            last_ob, last_q = env.obs.clone(), env.qpos.clone()
            while True:
                got = policy(env.obs.clone(), is_train=is_train, random_exploration=random_exploration)
                ac, ac_type = got if cfg.discrete_action else (got, None)
                ac = sit_out_action(ac, alive, cfg.use_ik_target, cfg.ik_has_quat)
                if ac_type is not None:
                    ac_type = torch.where(alive, ac_type.reshape(-1).to(torch.int64), torch.zeros(E, dtype=torch.int64, device=dev))
                before = {k: self.counters[k].clone() for k in COUNTERS}
                out = self.agent_step(ac, ac_type=ac_type)
                ep_len += torch.where(alive, out["intra_steps"] + 1, torch.zeros_like(ep_len))
                ep_rew += torch.where(alive, out["rew"], torch.zeros_like(ep_rew))
                if ep_cf is not None:
                    ep_cf += torch.where(alive, out["contact_force"], torch.zeros_like(ep_cf))
                for k in COUNTERS:
                    cnt[k] += torch.where(alive, self.counters[k] - before[k], torch.zeros_like(cnt[k]))
                success |= alive & out["success"].bool()
                obs.append(torch.where(alive[:, None], out["ob"], last_ob))
                acs.append(out["ac"].clone())
                rews.append(torch.where(alive, out["rew"], torch.zeros_like(out["rew"])))
                dones.append(torch.where(alive, out["done"].to(torch.uint8), torch.zeros_like(out["done"], dtype=torch.uint8)))
                valids.append(alive.clone())
                last_ob = torch.where(alive[:, None], out["ob_next"], last_ob)
                last_q = torch.where(alive[:, None], env.qpos, last_q)
                # (the step a sitting-out env took with its neutral action is undone: with `use_ik_target` that action still moves the arm --
                #  the IK aims at the [3, 0, 1, 1]-indexed site quaternion --, and a drifting env could end up anywhere)
                env.qpos.copy_(last_q)
                env.obs.copy_(last_ob)
                alive = alive & ~(out["done"].bool() | (ep_len >= max_step))
                if not bool(alive.any()):         # (one host read per agent step: this is the evaluation loop, not the training one)
                    break
            obs.append(last_ob)
        finally:
            cfg.discount_factor, self._disc = gamma, disc_cache
        valid = torch.stack(valids)
        # row n_steps[e] of `ob` = env e's final obs; rows beyond it repeat it
        ob_t = torch.stack(obs)
        rollout = {"ob": ob_t, "ac": torch.stack(acs), "rew": torch.stack(rews), "done": torch.stack(dones), "valid": valid,
                   "n_steps": valid.sum(0), "qpos_final": last_q}
        ep_info = {"len": ep_len, "rew": ep_rew, "success": success, **cnt}
        if ep_cf is not None:
            ep_info["contact_force"] = ep_cf
            ep_info["avg_conntact_force"] = ep_cf / ep_len.to(torch.float64)
        return rollout, ep_info
