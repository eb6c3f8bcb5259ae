"""PyKinematicPlanner -- the drop-in boundary object.

Mirrors the Cython class of the reference (motion_planners/planner.pyx:31-52):
same constructor arguments (14, positional), same three methods, same return
conventions (``plan`` returns a list of rows, or ``[[-5]*nq]`` when the goal is
invalid / ``[[-4]*nq]`` when no exact solution was found --
motion_planners/KinematicPlanner.cpp:181-184,249-250).  The work happens in
libmopa_hip.so on the GPU; there is no CPU path.

Differences that cannot be hidden (DESIGN.md "Semantics"):
  * ``timelimit`` seconds are converted to an RRT-Connect iteration budget
    (``ITERS_PER_SECOND`` per second) -- the reference stops on wall-clock and
    is therefore not reproducible;
  * ``algo == b"rrt_connect"`` and ``algo == b"rrt_star"`` are implemented.
    ``b"rrt"`` -- which means RRT* in the reference,
    KinematicPlanner.cpp:89,99-101 -- keeps raising: RRT* (K3b)
    has the name ``b"rrt_star"`` here.  With it ``opt`` must be ``""`` or
    ``path_length`` (the only objective built), ``threshold`` is the goal
    threshold, the goal bias is OMPL's default 0.05 whatever ``goal_bias``
    says, and every ``plan`` spends its whole iteration budget.  The
    maximize-min-clearance objective needs a band, for which the 14
    constructor arguments have no slot: it is chosen after construction
    with the attributes ``objective = "maximize_min_clearance"`` and
    ``clearance_band`` ("K3b under the clearance
    objective"; a stated deviation from OMPL: the cost is the pair
    (clearance, then L1 length)), and ``plan`` then leaves the clearance
    in ``last_cost`` and the length in ``last_length``.  The planner stays
    on the inflated (margin-rule) distances: ``path_clearance(rows,
    exact=True)`` of a returned path is never lower than the planner's
    clearance, up to kGjkTol = 1e-6; equality of bits holds with
    ``exact=False`` only;
  * ``opt``, ``num_actions``, ``goal_bias``, ``simplified_duration`` are
    accepted and ignored exactly as the reference ignores them
    (KinematicPlanner.cpp:42-61); ``is_simplified=True`` is rejected
    (PathSimplifier is randomised and time-bounded).  The part of it that can
    be stated exactly -- the two vertex-removing passes reduceVertices and
    collapseCloseVertices (K9) -- runs behind the attribute
    ``vertex_simplify`` (default False; not a constructor argument, the
    reference's 14 stay as they are), and shortcutPath, with the stub
    checks of DESIGN.md, behind the attribute ``path_shortcut``, and
    smoothBSpline, with the outer-half checks of DESIGN.md, behind the
    attribute ``path_smooth``.  The three together are ``simplify()``'s
    schedule without its wall clock; checkAndRepair is not built (every
    segment of a result has itself passed the motion check);
  * ``glue_bodies = [body_a, body_b]`` (names, str or bytes) plans with
    ``body_b`` -- the manipulated object, a body with one free joint --
    attached to ``body_a``: ``plan`` attaches at the start state,
    ``isValidState`` at the state itself, and the free-joint columns of a
    solved path hold the object's pose at every waypoint (the weld form of
    the reference's GlueTransformation).  Built for
    rrt_connect with ``portfolio == 1`` and no K9 switch; the reference's
    two-slide branch (Pusher's box) is not built.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .scene import load_scene

#: RRT-Connect iterations granted per second of the reference's ``timelimit``
ITERS_PER_SECOND = int(os.environ.get("MOPA_ITERS_PER_SECOND", "2000"))
MAX_NODES = int(os.environ.get("MOPA_MAX_NODES", "4096"))
MAX_PATH = int(os.environ.get("MOPA_MAX_PATH", "1024"))


def _to_str(b) -> str:
    return b.decode("utf-8") if isinstance(b, (bytes, bytearray)) else str(b)


class PyKinematicPlanner:
    def __init__(self, xml_filename, algo, num_actions, opt, threshold, _range, passive_joint_idx, glue_bodies,
                 ignored_contacts, contact_threshold, goal_bias, is_simplified, simplified_duration, seed):
        self.xml_filename = _to_str(xml_filename)
        self.algo = _to_str(algo)
        self.num_actions = int(num_actions)
        self.opt = _to_str(opt)
        self.threshold = float(threshold)
        self._range = float(_range)
        self.passive_joint_idx = [int(i) for i in passive_joint_idx]
        self.glue_bodies = list(glue_bodies)
        self.ignored_contacts = [(int(a), int(b)) for a, b in ignored_contacts]
        self.contact_threshold = float(contact_threshold)
        self.isSimplified = bool(is_simplified)
        self.simplifiedDuration = float(simplified_duration)
        self.seed = int(seed)
        if self.glue_bodies:
            if len(self.glue_bodies) != 2 or not all(isinstance(b, (str, bytes, bytearray)) for b in self.glue_bodies):
                raise NotImplementedError("glue_bodies: only the empty list and two body names [body_a, body_b] (str or bytes) are implemented")
            self.glue_bodies = [_to_str(b) for b in self.glue_bodies]
        if self.algo not in ("rrt_connect", "rrt_star"):
            raise NotImplementedError(f"algo={self.algo!r}: only 'rrt_connect' and 'rrt_star' (the reference's 'rrt' = RRT*) are implemented")
        if self.algo == "rrt_star" and self.opt not in ("", "path_length"):
            raise NotImplementedError(f"opt={self.opt!r}: RRT* is built with the path-length objective only")
        if self.isSimplified:
            raise NotImplementedError("is_simplified=True (OMPL PathSimplifier) is not implemented; its two vertex-removing passes "
                                      "(reduceVertices, collapseCloseVertices), its shortcutPath and its smoothBSpline are: set "
                                      "the attributes vertex_simplify = True, path_shortcut = True and / or path_smooth = True "
                                      "(the three together are simplify()'s schedule without its wall clock)")
        #: K9: plan() runs reduceVertices + collapseCloseVertices over the solved path (`vertex_simplify_passes`: 1 / 2 / 3)
        self.vertex_simplify = False
        self.vertex_simplify_passes = 3
        #: K9: plan() runs shortcutPath over the solved path, in front of the vertex passes when `vertex_simplify` is set too
        self.path_shortcut = False
        #: K9: plan() runs smoothBSpline over the solved path, behind shortcutPath and in front of the vertex passes
        self.path_smooth = False
        #: K3 race: with rrt_connect, plan() runs `portfolio` seeded members per query and returns the winner's path (DESIGN.md "K3 race")
        self.portfolio = 1
        #: K3b: with rrt_star, "path_length" or "maximize_min_clearance" (band-limited: `clearance_band`, finite, >= 0 and above the
        #: contact threshold, has to be set too).  plan() then optimises the pair (clearance, then L1 length): DESIGN.md section 4
        self.objective = "path_length"
        self.clearance_band = None
        self._check_glue_combination()
        self._model = load_scene(self.xml_filename)
        self._scene = _lib.Scene(self._model, self.passive_joint_idx, self.ignored_contacts, self.contact_threshold,
                                 range_=self._range, resolution=0.005, seed=self.seed)
        #: the scene plan() and isValidState() run on: with glue_bodies the glued sibling (closed with `_scene`)
        self._query_scene = self._scene.glued(*self.glue_bodies) if self.glue_bodies else self._scene
        self._plan_count = 0
        self._status_scene = self._query_scene      # the scene the last plan() ran on: getPlannerStatus() reads it
        self._batch = None          # the BatchPlanner of `_scene`, made on first use (path_clearance)
        #: RRT*: the cost of the last plan()'s path: its L1 length, +inf when it found none; under the clearance objective its
        #: clearance, -inf when it found none, and `last_length` holds the L1 length
        self.last_cost = float("inf")
        self.last_length = float("inf")

    # -- reference API -----------------------------------------------------
    def isValidState(self, state_vec) -> bool:
        return self._query_scene.is_valid_state(np.asarray(state_vec, dtype=np.float64))

    def plan(self, start_vec, goal_vec, timelimit) -> List[List[float]]:
        start = np.asarray(start_vec, dtype=np.float64)
        goal = np.asarray(goal_vec, dtype=np.float64)
        max_iters = max(1, int(round(float(timelimit) * ITERS_PER_SECOND)))
        # every plan() call of one planner object draws a fresh sample stream
        k9_seed = self.seed
        self._status_scene = self._query_scene
        self._check_glue_combination()
        if int(self.portfolio) > 1 and self.algo == "rrt_star":
            raise NotImplementedError("portfolio > 1 is built for rrt_connect only (RRT* always spends its whole budget: nothing to race)")
        if self.objective not in ("path_length", "maximize_min_clearance"):
            raise ValueError(f"objective={self.objective!r}: 'path_length' or 'maximize_min_clearance'")
        if self.objective == "maximize_min_clearance":
            self._check_clearance_combination()
            self._status_scene = self._scene.contact_scene()       # the scene with the full pair list, as the clearance report runs on
            status, path, self.last_cost, self.last_length, _ = self._status_scene.plan_star_clearance(
                start, goal, float(self.clearance_band), max_iters=max_iters, max_nodes=max_iters + 1, max_path=MAX_PATH, seed=self.seed,
                env_id=self._plan_count, goal_bias=_lib.STAR_GOAL_BIAS, goal_threshold=self.threshold)
        elif self.algo == "rrt_star":
            # goal bias: OMPL's default 0.05, not the constructor's `goal_bias` -- the reference never forwards that argument to
            # the planner it builds (KinematicPlanner.cpp:42-120); the goal threshold is the constructor's `threshold`
            status, path, self.last_cost, _ = self._scene.plan_star(start, goal, max_iters=max_iters, max_nodes=max_iters + 1, max_path=MAX_PATH,
                                                                    seed=self.seed, env_id=self._plan_count, goal_bias=_lib.STAR_GOAL_BIAS,
                                                                    goal_threshold=self.threshold)
        elif int(self.portfolio) > 1:
            # the simplifier draws from the winner's stream
            status, path, _, _, k9_seed, _ = self._scene.plan_race(start, goal, int(self.portfolio), max_iters=max_iters, max_nodes=MAX_NODES,
                                                                   max_path=MAX_PATH, seed=self.seed, env_id=self._plan_count)
        else:
            status, path, _ = self._query_scene.plan(start, goal, max_iters=max_iters, max_nodes=MAX_NODES, max_path=MAX_PATH,
                                                     seed=self.seed, env_id=self._plan_count)
        if (self.vertex_simplify or self.path_shortcut or self.path_smooth) and status == _lib.PLAN_OK and len(path) >= 3:
            path = self._simplify(path, self._plan_count, k9_seed)
        self._plan_count += 1
        nq = self._scene.nq
        if status == _lib.PLAN_INVALID_GOAL:
            return [[-5.0] * nq]
        if status != _lib.PLAN_OK:
            return [[-4.0] * nq]
        return path.tolist()

    def _check_glue_combination(self) -> None:
        """glue_bodies is built for plain rrt_connect: the combinations that are not raise, naming themselves"""
        if not self.glue_bodies:
            return
        if self.algo == "rrt_star":
            raise NotImplementedError("glue_bodies with algo='rrt_star': glue is built for rrt_connect only")
        if int(self.portfolio) > 1:
            raise NotImplementedError("glue_bodies with portfolio > 1: the K3 race is not built for a glued scene")
        on = [n for n in ("vertex_simplify", "path_shortcut", "path_smooth") if getattr(self, n)]
        if on:
            raise NotImplementedError(f"glue_bodies with {' / '.join(on)}: path simplification (K9) is not built for a glued scene")

    def _check_clearance_combination(self) -> None:
        """objective = "maximize_min_clearance" is built for plain rrt_star with a band"""
        if self.glue_bodies:
            raise NotImplementedError("objective='maximize_min_clearance' with glue_bodies: RRT* is not built for a glued scene")
        if self.algo != "rrt_star":
            raise NotImplementedError(f"objective='maximize_min_clearance' with algo={self.algo!r}: the clearance objective is built for rrt_star only")
        on = [n for n in ("vertex_simplify", "path_shortcut", "path_smooth") if getattr(self, n)]
        if on:
            raise NotImplementedError(f"objective='maximize_min_clearance' with {' / '.join(on)}: a simplifier behind this planner would change "
                                      "the clearance it reports; simplify the returned path and call path_clearance instead")
        if self.clearance_band is None:
            raise ValueError("objective='maximize_min_clearance' needs clearance_band (finite, >= 0, above the contact threshold)")

    def _simplify(self, path: np.ndarray, stream_id: int, seed=None) -> np.ndarray:
        """K9 over one solved path: the draws come from the sample stream (seed, stream_id) the plan itself used (a race: the
        winner's seed)"""
        seed = self.seed if seed is None else seed
        import torch
        from .batch import BatchPlanner, k9_entry, k9_passes
        ordinal = self._scene.device_ordinal    # the scene's device (-1: the current one, where it was created)
        dev = torch.device("cuda", ordinal if ordinal >= 0 else torch.cuda.current_device())
        plen = torch.tensor([len(path)], dtype=torch.int32, device=dev)
        flags = (self.vertex_simplify, self.path_shortcut, self.path_smooth)
        cap = len(path)                 # the vertex passes only remove rows
        if self.path_smooth:            # a smoothing step nearly doubles the vertices: the largest capacity the kernel's lists hold
            cap = min(MAX_PATH, int(_lib.lib().mopa_smooth_paths_max_path(self._scene.handle)))
            if len(path) > cap:
                raise _lib.MopaError(f"path_smooth: the path has {len(path)} rows, the smoothing kernel holds {cap}")
        elif self.path_shortcut:        # a shortcut can add a vertex: the rows get the planner's own capacity
            cap = MAX_PATH
        rows = torch.zeros(1, cap, path.shape[1], dtype=torch.float64, device=dev)
        rows[0, :len(path)] = torch.from_numpy(np.ascontiguousarray(path)).to(dev)
        getattr(BatchPlanner(self._scene), k9_entry(*flags))(
            rows, plen, None, seed=seed, env_id_base=stream_id,
            passes=k9_passes(flags[0], self.vertex_simplify_passes, flags[1], flags[2]))
        return rows[0, :int(plen[0])].cpu().numpy()

    def getPlannerStatus(self) -> bytes:
        return self._status_scene.planner_status()

    # -- extras used by the batched host code --------------------------------
    @property
    def scene(self) -> "_lib.Scene":
        """the scene plan() and isValidState() run on: with glue_bodies the glued one, whose unbuilt entry points refuse.  The
        glued scene belongs to the ordinary one: `close()` below releases both"""
        return self._query_scene

    def close(self) -> None:
        self._scene.close()

    @property
    def model(self):
        return self._model

    def contacts(self, state_vec, frames: bool = False, manifold: bool = False, max_points: int = 4, point_cutoff: float = 0.0) -> List[Tuple]:
        """the pairs that make `state_vec` invalid -- (geom1_name, geom2_name, dist) with dist <= contact_threshold, what the
        reference's checker finds in d->contact[i] (mujoco_ompl_interface.cpp:917-978); empty for a valid state.
        frames=True: (geom1_name, geom2_name, dist, normal, pos), one contact frame per pair (`Scene.contacts_state`).
        manifold=True: (geom1_name, geom2_name, dist, normal, [(pos, dist_i), ...]), up to max_points contact points per pair
        (`Scene.contacts_state`).  With glue_bodies it raises: the contact report is not built for a glued scene"""
        if self.glue_bodies:
            raise NotImplementedError("contacts() with glue_bodies: the contact report is not built for a glued scene")
        if manifold:
            return self._scene.contacts_state(np.asarray(state_vec, dtype=np.float64), manifold=True, max_points=max_points, point_cutoff=point_cutoff)
        return self._scene.contacts_state(np.asarray(state_vec, dtype=np.float64), frames=frames)

    def proximity(self, state_vec, band: float, max_pairs: int = 8, exact: bool = False, witness: bool = False):
        """how far from collision `state_vec` is and which pairs are nearest: (clearance, [(geom1_name, geom2_name, dist), ...]),
        clearance saturating at `band`, the pairs with dist <= band nearest first (`Scene.proximity_state`); exact=True: GJK distances
        for disjoint box-box, cylinder and mesh pairs instead of the margin rule's; witness=True (needs exact=True): the entries
        become (geom1_name, geom2_name, dist, normal, p1, p2), the pair's two closest points and the unit vector from the first to
        the second.  With glue_bodies it raises: the proximity report is not built for a glued scene"""
        if witness and not exact:
            raise ValueError("witness=True needs exact=True: the inflated route's distance is not attained by two points of the shapes")
        if self.glue_bodies:
            raise NotImplementedError("proximity() with glue_bodies: the proximity report is not built for a glued scene")
        if witness:
            return self._scene.proximity_state(np.asarray(state_vec, dtype=np.float64), band, max_pairs, exact=exact, witness=True)
        return self._scene.proximity_state(np.asarray(state_vec, dtype=np.float64), band, max_pairs, exact=exact)

    def motion_report(self, start_vec, goal_vec, max_contacts: int = 0) -> dict:
        """where the straight line from `start_vec` to `goal_vec` (full qpos vectors; the passive entries are start_vec's) is
        blocked -- OMPL's checkMotion(s1, s2, lastValid): `valid`, `n_states`, `first_bad`, `last_valid_t`, `last_valid_q`,
        `first_bad_q`, and with max_contacts >= 1 `blockers`, the pairs that make the first blocked state invalid as
        (geom1_name, geom2_name, dist) (`Scene.motion_report_state`).  With glue_bodies it raises: the motion report is not built
        for a glued scene"""
        if self.glue_bodies:
            raise NotImplementedError("motion_report() with glue_bodies: the motion report is not built for a glued scene")
        return self._scene.motion_report_state(np.asarray(start_vec, dtype=np.float64), np.asarray(goal_vec, dtype=np.float64), max_contacts=max_contacts)

    def motion_clearance(self, start_vec, goal_vec, band: float, exact: bool = False) -> dict:
        """how near the straight line from `start_vec` to `goal_vec` (full qpos vectors; the passive entries are start_vec's) comes
        to collision -- OMPL's MinimaxObjective::motionCost under the clearance state cost: `clearance`, `n_states`, `n_near`,
        `k_min`, `t_min`, `pair` as (geom1_name, geom2_name), `pair_min`, `end_clearance`, `q_min` (`Scene.motion_clearance_state`);
        exact=True: over the state clearances of `proximity(..., exact=True)`.  With glue_bodies it raises: the clearance report is not built for a glued scene"""
        if self.glue_bodies:
            raise NotImplementedError("motion_clearance() with glue_bodies: the clearance report is not built for a glued scene")
        return self._scene.motion_clearance_state(np.asarray(start_vec, dtype=np.float64), np.asarray(goal_vec, dtype=np.float64), band,
                                                  exact=exact)

    def path_clearance(self, traj, band: float, exact: bool = False) -> dict:
        """the clearance of a path as `plan` returns it (a list of full qpos vectors): `clearance` (the smallest state clearance
        along it, vertex 0 included, saturating at band), `seg_min` (the first segment that attains it; -1: vertex 0 does, or
        nothing is within the band), `k_min`, `pair` as (geom1_name, geom2_name) or None, `pair_min`, `mean_vertex_clearance`
        (`BatchPlanner.path_clearance`); exact=True: with the exact route's distances -- for a path planned under
        objective = "maximize_min_clearance" never lower than the planner's clearance, up to 1e-6.  With glue_bodies it raises: the clearance report is not built for a glued scene"""
        if self.glue_bodies:
            raise NotImplementedError("path_clearance() with glue_bodies: the clearance report is not built for a glued scene")
        import torch
        from .batch import BatchPlanner
        rows = np.ascontiguousarray(np.asarray(traj, dtype=np.float64).reshape(-1, self._scene.nq))
        ordinal = self._scene.device_ordinal
        dev = torch.device("cuda", ordinal if ordinal >= 0 else torch.cuda.current_device())
        path = torch.from_numpy(rows[None] if len(rows) else np.zeros((1, 1, self._scene.nq))).to(dev).contiguous()
        plen = torch.tensor([len(rows)], dtype=torch.int32, device=dev)
        if self._batch is None:
            self._batch = BatchPlanner(self._scene)
        r = self._batch.path_clearance(path, plen, band=band, exact=exact)
        m = self._model
        pair = int(r.pair_min[0])
        g = np.asarray(m.pair_geom).reshape(-1, 2)
        name = lambda j: m.all_geom_names[int(m.geom_mjid[int(j)])]
        return {"clearance": float(r.clearance[0]), "seg_min": int(r.seg_min[0]), "k_min": int(r.k_min[0]), "pair_min": pair,
                "pair": (name(g[pair, 0]), name(g[pair, 1])) if pair >= 0 else None,
                "mean_vertex_clearance": float(r.mean_vertex_clearance[0])}
