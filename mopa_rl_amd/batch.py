"""Batched (device-resident) entry points over torch tensors.

torch is used only for device memory and streams: every call hands raw device
pointers to libmopa_hip.so through the C ABI (include/mopa_hip.h).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import numpy as np
from typing import Optional, Tuple

from . import _lib


def _torch():
    import torch
    return torch


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _check_f64(t, name, cols=None):
    torch = _torch()
    if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise _lib.MopaError(f"{name} must be a contiguous float64 tensor on the GPU")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise _lib.MopaError(f"{name} must have shape [*, {cols}], got {tuple(t.shape)}")


def _stream_handle(stream) -> C.c_void_p:
    if stream is not None:
        return C.c_void_p(stream.cuda_stream)
    # the current stream's raw handle without building a torch.cuda.Stream object (a dozen lookups per agent_step call:
    # ~9 us each through torch.cuda.current_stream(), well under 1 us this way)
    return C.c_void_p(_raw_stream_fn()())


_RAW_STREAM = None


def _raw_stream_fn():
    """the cheapest way this torch build offers to read the current stream's raw handle (chosen once): the private
    torch._C._cuda_getCurrentRawStream when it exists, else the documented torch.cuda.current_stream().cuda_stream"""
    global _RAW_STREAM
    if _RAW_STREAM is None:
        torch = _torch()
        tc = torch._C
        if os.environ.get("MOPA_STREAM_PUBLIC_API") != "1" and hasattr(tc, "_cuda_getCurrentRawStream") and hasattr(tc, "_cuda_getDevice"):
            _RAW_STREAM = lambda: tc._cuda_getCurrentRawStream(tc._cuda_getDevice())
        else:
            _RAW_STREAM = lambda: torch.cuda.current_stream().cuda_stream
    return _RAW_STREAM


class PlanState:
    """Trees, iteration and check counts a planner launch left behind for its queries (`BatchPlanner.plan(keep_state=True)`)."""

    def __init__(self, tree_q, tree_p, state, max_nodes: int, na: int):
        self.tree_q, self.tree_p, self.state, self.max_nodes, self.na = tree_q, tree_p, state, int(max_nodes), int(na)

    def rows(self, idx):
        """the state of the queries `idx` (int64 tensor), in that order -- what a continuing launch of those queries takes"""
        torch = _torch()
        E = self.state.shape[0]
        w = 2 * self.max_nodes * self.na
        tq = torch.empty(len(idx) * w + 8, dtype=torch.float64, device=self.tree_q.device)
        tq[:len(idx) * w].view(len(idx), w).copy_(self.tree_q[:E * w].view(E, w)[idx])
        return PlanState(tq, self.tree_p.view(E, 2 * self.max_nodes)[idx].contiguous().view(-1), self.state[idx].contiguous(),
                         self.max_nodes, self.na)

    @staticmethod
    def cat(parts):
        torch = _torch()
        p0 = parts[0]
        w = 2 * p0.max_nodes * p0.na
        n = sum(p.state.shape[0] for p in parts)
        tq = torch.empty(n * w + 8, dtype=torch.float64, device=p0.tree_q.device)
        o = 0
        for p in parts:
            k = p.state.shape[0] * w
            tq[o:o + k].copy_(p.tree_q[:k])
            o += k
        return PlanState(tq, torch.cat([p.tree_p for p in parts]), torch.cat([p.state for p in parts]), p0.max_nodes, p0.na)


class ContactReport:
    """`BatchPlanner.contacts`: per state the number of pairs at or below the cutoff (`count` [N] int32, not capped), their
    indices into `model.pair_geom` in ascending order (`pair` [N, K] int32, -1 in unused slots) and their signed distances
    (`dist` [N, K] float64, MOPA_FAR in unused slots).  With `frames=True` also ONE contact frame per record, that of the
    deepest contact: `normal` [N, K, 3], a unit vector from the pair's first geom (as `geoms()` orders them) towards its second,
    and `pos` [N, K, 3], the midpoint of the two witness points; 0.0 in unused slots.  Both are None otherwise.
    With `manifold=True` the same `normal` and, per record, a contact manifold of up to P points: `npoint` [N, K] int32 (the
    number of points under point_cutoff, at most 8, not capped by P; 0 in unused slots), `point_dist` [N, K, P] (ascending,
    deepest first; MOPA_FAR in unused slots) and `point_pos` [N, K, P, 3] (0.0 in unused slots); None otherwise.  `pos` stays
    tied to `frames=True`."""

    def __init__(self, count, pair, dist, model, normal=None, pos=None, npoint=None, point_dist=None, point_pos=None):
        self.count, self.pair, self.dist, self.model = count, pair, dist, model
        self.normal, self.pos = normal, pos
        self.npoint, self.point_dist, self.point_pos = npoint, point_dist, point_pos

    def __iter__(self):
        return iter((self.count, self.pair, self.dist))

    def geoms(self):
        """[N, K, 2] int64 numpy array: ids of the two geoms of every record among ALL geoms of the model (MuJoCo's geom ids,
        `model.geom_mjid`), -1 in unused slots"""
        return pair_geom_ids(self.model, self.pair.cpu().numpy())

    def names(self, i: int):
        """the records of state i as (geom1_name, geom2_name, dist)"""
        m = self.model
        n = min(int(self.count[i]), self.pair.shape[1])
        ids = pair_geom_ids(m, self.pair[i, :n].cpu().numpy())
        d = self.dist[i, :n].cpu().numpy()
        return [(m.all_geom_names[int(a)], m.all_geom_names[int(b)], float(x)) for (a, b), x in zip(ids, d)]


class ProximityReport:
    """`BatchPlanner.proximity`: per state `clearance` [N] float64 (min(band, the smallest pair distance): band when no pair is in
    band), `count` [N] int32 (the pairs with dist <= band, not capped) and the K nearest of them, ascending by (dist, pair index):
    `pair` [N, K] int32 indices into `model.pair_geom` (-1 in unused slots), `dist` [N, K] float64 (MOPA_FAR in unused slots).
    With witness=True also `p1` / `p2` [N, K, 3] float64 (world frame: a point of the pair's first geom and one of its second, at
    `dist` from each other; the contact frame's two witness points for a pair in overlap) and `normal` [N, K, 3] (the unit vector
    from p1 towards p2), 0.0 in unused slots; None otherwise."""

    def __init__(self, clearance, count, pair, dist, model, normal=None, p1=None, p2=None):
        self.clearance, self.count, self.pair, self.dist, self.model = clearance, count, pair, dist, model
        self.normal, self.p1, self.p2 = normal, p1, p2

    def __iter__(self):
        return iter((self.clearance, self.count, self.pair, self.dist))

    def geoms(self):
        """[N, K, 2] int64 numpy array of MuJoCo geom ids (`ContactReport.geoms`), -1 in unused slots"""
        return pair_geom_ids(self.model, self.pair.cpu().numpy())


class MotionReport:
    """`BatchPlanner.motion_report`: per segment `valid` [N] uint8 (the byte `check_motion` writes), `n_states` [N] int32 (c =
    max(validSegmentCount, 1): the states s_1 .. s_c that were due, s_c = qb), `first_bad` [N] int32 (the smallest k with s_k
    invalid, 0 if valid), `last_valid_t` [N] float64 ((first_bad - 1) / c, 1.0 if valid), and with states=True `last_valid_q` /
    `first_bad_q` [N, na] float64 (s_{first_bad - 1}, qa's bits when first_bad == 1, and s_{first_bad}; both qb for a valid
    segment), None otherwise.  `blockers`: a `ContactReport` of the states first_bad_q at the contact threshold (max_contacts >= 1:
    a blocked segment has count >= 1, a valid one the unused row), or None."""

    def __init__(self, valid, n_states, first_bad, last_valid_t, last_valid_q=None, first_bad_q=None, blockers=None):
        self.valid, self.n_states, self.first_bad, self.last_valid_t = valid, n_states, first_bad, last_valid_t
        self.last_valid_q, self.first_bad_q, self.blockers = last_valid_q, first_bad_q, blockers


class MotionClearance:
    """`BatchPlanner.motion_clearance`: per segment, over the states s_1 .. s_c `MotionReport` walks (s_c = qb; qa is not
    evaluated), `clearance` [N] float64 (the smallest state clearance, each saturating at band), `n_states` [N] int32 (c),
    `n_near` [N] int32 (states with a pair within the band), `k_min` [N] int32 (the smallest k whose state attains the clearance
    with a pair in band; 0: nothing within the band), `t_min` [N] float64 (k_min / c), `pair_min` [N] int32 (the nearest pair of
    s_k_min, index into `model.pair_geom`; -1 when k_min == 0), `end_clearance` [N] float64 (that of qb) and with states=True
    `q_min` [N, na] float64 (s_k_min; qb's bits when k_min == 0), None otherwise.  As `PathClearance.segments` it also carries
    `path_index` / `seg_index` [N] int64: segment i is seg_index[i] -> seg_index[i] + 1 of path path_index[i]."""

    def __init__(self, clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance, q_min, model, path_index=None, seg_index=None):
        self.clearance, self.n_states, self.n_near, self.k_min, self.t_min = clearance, n_states, n_near, k_min, t_min
        self.pair_min, self.end_clearance, self.q_min, self.model = pair_min, end_clearance, q_min, model
        self.path_index, self.seg_index = path_index, seg_index

    def geoms(self):
        """[N, 2] int64 numpy array of MuJoCo geom ids of `pair_min` (`ContactReport.geoms`), -1 where nothing is within the band"""
        return pair_geom_ids(self.model, self.pair_min.cpu().numpy())


class PathClearance:
    """`BatchPlanner.path_clearance`: per path `clearance` [E] float64 (min of vertex 0's state clearance and the segments'
    clearances; NaN for an unsolved query, path_len == 0), `seg_min` [E] int32 (the first segment that attains it; -1 when vertex
    0 does, which includes "nothing within the band"), `k_min` / `pair_min` [E] int32 (that segment's; 0 and vertex 0's pair when
    seg_min == -1), `mean_vertex_clearance` [E] float64 (the mean of the band-saturated clearances of the path's vertices, OMPL's
    PathGeometric::clearance(); NaN when path_len == 0) and `segments`, the `MotionClearance` of all segments of all paths."""

    def __init__(self, clearance, seg_min, k_min, pair_min, mean_vertex_clearance, segments):
        self.clearance, self.seg_min, self.k_min, self.pair_min = clearance, seg_min, k_min, pair_min
        self.mean_vertex_clearance, self.segments = mean_vertex_clearance, segments

    def geoms(self):
        """[E, 2] int64 numpy array of MuJoCo geom ids of `pair_min`, -1 where there is none"""
        return pair_geom_ids(self.segments.model, self.pair_min.cpu().numpy())


def pair_geom_ids(model, pair) -> np.ndarray:
    """pair indices (any shape, -1 = unused) -> [..., 2] MuJoCo geom ids of the pairs' geoms, -1 where unused"""
    pair = np.asarray(pair, dtype=np.int64)
    g = np.asarray(model.geom_mjid, dtype=np.int64)[np.asarray(model.pair_geom, dtype=np.int64).reshape(-1, 2)]
    out = g[np.clip(pair, 0, max(len(g) - 1, 0))] if len(g) else np.zeros(pair.shape + (2,), dtype=np.int64)
    out[pair < 0] = -1
    return out


def _pair_batch(types, recs):
    """The argument rule of the pair-level entry points: types [M, 2] int32 and recs [M, 2, 15] float64, both contiguous on
    the GPU -> (M, the device ordinal of recs)"""
    torch = _torch()
    _check_f64(recs, "recs")
    if types.dtype != torch.int32 or not types.is_cuda or not types.is_contiguous() or types.dim() != 2 or types.shape[1] != 2:
        raise _lib.MopaError("types must be a contiguous int32 GPU tensor [M, 2]")
    M = types.shape[0]
    if recs.numel() != M * 30:
        raise _lib.MopaError(f"recs must have shape [{M}, 2, 15], got {tuple(recs.shape)}")
    return M, int(recs.device.index if recs.device.index is not None else torch.cuda.current_device())


def geom_frames(types, recs, stream=None):
    """mopa_geom_frames_batch: M posed primitive pairs, one lane each -- types [M, 2] int32 (MuJoCo geom type codes, either
    order), recs [M, 2, 15] float64 (pos[3] mat[9] size[3] per geom), both contiguous on the GPU -> [M, 7] = dist, normal[3],
    pos[3]; the bits of `_lib.geom_frames_host`.  Meshes are not served at this level."""
    torch = _torch()
    M, dev = _pair_batch(types, recs)
    out = torch.empty(M, 7, dtype=torch.float64, device=recs.device)
    _lib.check(_lib.lib().mopa_geom_frames_batch(dev, M, _ptr(types), _ptr(recs), _ptr(out), _stream_handle(stream)))
    return out


def geom_sep(types, recs, band: float, mesh_verts=None, stream=None, exact: bool = False):
    """mopa_geom_sep_batch: M posed pairs, one lane each, as `geom_frames` takes them -> [M] band-limited signed distances, the
    bits of `_lib.geom_sep_host`; mesh_verts [n, 3] (float64, on the GPU): the hull of every geom of type 7.
    exact=True (mopa_geom_sep_exact_batch): the bits of `_lib.geom_sep_host(..., exact=True)`, the GJK distance of disjoint box-box,
    cylinder and mesh pairs"""
    torch = _torch()
    M, dev = _pair_batch(types, recs)
    nvert = 0
    if mesh_verts is not None:
        _check_f64(mesh_verts, "mesh_verts", 3)
        nvert = mesh_verts.shape[0]
    out = torch.empty(M, dtype=torch.float64, device=recs.device)
    fn = _lib.lib().mopa_geom_sep_exact_batch if exact else _lib.lib().mopa_geom_sep_batch
    _lib.check(fn(dev, M, _ptr(types), _ptr(recs), _ptr(mesh_verts) if nvert else None, nvert, float(band), _ptr(out), _stream_handle(stream)))
    return out


def geom_witness(types, recs, band: float, mesh_verts=None, stream=None):
    """mopa_geom_witness_batch: M posed pairs, one lane each, as `geom_sep` takes them -> [M, 10] = d, n[3], p1[3], p2[3]: the
    exact route's distance with the pair's two closest points and the unit vector between them, the bits of
    `_lib.geom_witness_host`"""
    torch = _torch()
    M, dev = _pair_batch(types, recs)
    nvert = 0
    if mesh_verts is not None:
        _check_f64(mesh_verts, "mesh_verts", 3)
        nvert = mesh_verts.shape[0]
    out = torch.empty(M, 10, dtype=torch.float64, device=recs.device)
    _lib.check(_lib.lib().mopa_geom_witness_batch(dev, M, _ptr(types), _ptr(recs), _ptr(mesh_verts) if nvert else None, nvert, float(band), _ptr(out),
                                                  _stream_handle(stream)))
    return out


def geom_manifolds(types, recs, point_cutoff: float = 0.0, max_points: int = 4, stream=None):
    """mopa_geom_manifolds_batch: M posed primitive pairs, one lane each, as `geom_frames` takes them -> (normal_dist [M, 4] =
    normal[3], dist; npoint [M] int32; points [M, P, 4] = pos[3], dist_i): the bits of `_lib.geom_manifolds_host`.  Meshes are
    not served at this level."""
    torch = _torch()
    M, dev = _pair_batch(types, recs)
    P = int(max_points)
    nd = torch.empty(M, 4, dtype=torch.float64, device=recs.device)
    npoint = torch.empty(M, dtype=torch.int32, device=recs.device)
    pts = torch.empty(M, max(P, 1), 4, dtype=torch.float64, device=recs.device)
    _lib.check(_lib.lib().mopa_geom_manifolds_batch(dev, M, _ptr(types), _ptr(recs), float(point_cutoff), P, _ptr(nd), _ptr(npoint), _ptr(pts),
                                                    _stream_handle(stream)))
    return nd, npoint, pts


def k9_passes(vertex_simplify, simplify_passes, path_shortcut, path_smooth) -> int:
    """The passes word of the K9 launch that the flags of `plan` select (bit 0 reduceVertices, bit 1 collapseCloseVertices, bit 2
    shortcutPath, bit 3 smoothBSpline); 0: no K9 launch."""
    vertex = int(simplify_passes) if vertex_simplify else 0
    if path_smooth:
        return 8 | (4 if path_shortcut else 0) | vertex
    return (4 if path_shortcut else 0) | vertex


def k9_entry(vertex_simplify, path_shortcut, path_smooth) -> Optional[str]:
    """The `BatchPlanner` method that takes that word: the kernel of the highest stage asked for; None when all flags are off."""
    return "smooth_paths" if path_smooth else "shortcut_paths" if path_shortcut else "simplify_paths" if vertex_simplify else None


class BatchPlanner:
    """N-state validity / motion checks and E-env RRT-Connect on one GPU."""

    def __init__(self, scene: "_lib.Scene"):
        self.scene = scene
        self.na = scene.na
        self.nq = scene.nq

    def _state_batch(self, q_active, qpos_env, samples_per_env, name="q_active"):
        """The one argument rule of a batch of states: q_active [N, na] and qpos_env [rows, nq] contiguous float64 on the GPU,
        samples_per_env >= 1 (None: N // rows) with ceil(N / samples_per_env) <= rows -> (N, samples_per_env)"""
        _check_f64(q_active, name, self.na)
        _check_f64(qpos_env, "qpos_env", self.nq)
        N, rows = q_active.shape[0], qpos_env.shape[0]
        spe = int(samples_per_env) if samples_per_env is not None else max(1, N // max(1, rows))
        if spe <= 0:
            raise _lib.MopaError("samples_per_env must be >= 1")
        if (N + spe - 1) // spe > rows:
            raise _lib.MopaError("qpos_env has fewer rows than ceil(N / samples_per_env)")
        return N, spe

    def _segment_batch(self, qa, qb, qpos_env, samples_per_env):
        """... and of a batch of segments qa[i] -> qb[i]: `_state_batch` of qa, and qb as long as qa"""
        N, spe = self._state_batch(qa, qpos_env, samples_per_env, "qa")
        _check_f64(qb, "qb", self.na)
        if qb.shape[0] != N:
            raise _lib.MopaError("qa and qb must hold the same number of segments")
        return N, spe

    # valid[i] for state i = qpos_env[i // samples_per_env] with active entries <- q_active[i]
    def is_valid(self, q_active, qpos_env, samples_per_env: Optional[int] = None, want_min_dist: bool = False,
                 out=None, stream=None, guard: bool = False, n_dev=None):
        """n_dev: int64 device tensor of one element, the number of states when only the device knows it (<= N; states from it on
        are neither read nor written; `out` then keeps what it held there).
        guard: states with a joint beyond its range + the pruning proof's guard band are re-evaluated with the full pair list
        (a device-side range test, one host read of the count; off on the hot paths, whose states are sampled / clipped inside
        the ranges -- `Scene.is_valid_state`, the reference's isValidState, always guards)."""
        torch = _torch()
        N, spe = self._state_batch(q_active, qpos_env, samples_per_env)
        valid = out if out is not None else torch.empty(N, dtype=torch.uint8, device=q_active.device)
        md = torch.empty(N, dtype=torch.float64, device=q_active.device) if want_min_dist else None
        if n_dev is not None:
            if guard or n_dev.dtype != torch.int64 or n_dev.numel() != 1 or n_dev.device != q_active.device:
                raise _lib.MopaError("n_dev: one int64 on the states' device, without guard")
            _lib.check(_lib.lib().mopa_is_valid_batch_counted(self.scene.handle, _ptr(q_active), _ptr(qpos_env), N, spe, _ptr(valid),
                                                              _ptr(md) if md is not None else None, _ptr(n_dev), _stream_handle(stream)))
            return (valid, md) if want_min_dist else valid
        _lib.check(_lib.lib().mopa_is_valid_batch(self.scene.handle, _ptr(q_active), _ptr(qpos_env), N, spe, _ptr(valid),
                                                  _ptr(md) if md is not None else None, _stream_handle(stream)))
        if guard and self.scene.npair_pruned and N:
            sc = self.scene
            dev = q_active.device
            if getattr(self, "_guard_t", None) is None or self._guard_t[0].device != dev:
                pos = {int(a): k for k, a in enumerate(sc.active_idx)}
                act = [k for k, a in enumerate(sc.guard_adr) if int(a) in pos]
                pas = [k for k, a in enumerate(sc.guard_adr) if int(a) not in pos]
                mk = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=dev)
                self._guard_t = (mk([pos[int(sc.guard_adr[k])] for k in act], torch.long), mk(sc.guard_lo[act], torch.float64), mk(sc.guard_hi[act], torch.float64),
                                 mk(sc.guard_adr[pas], torch.long), mk(sc.guard_lo[pas], torch.float64), mk(sc.guard_hi[pas], torch.float64))
            ia, la, ha, ip_, lp, hp = self._guard_t
            qa = q_active[:, ia]
            oor = ((qa < la) | (qa > ha)).any(dim=1)
            if len(ip_):
                qp = qpos_env[:, ip_]
                oor_env = ((qp < lp) | (qp > hp)).any(dim=1)
                oor = oor | oor_env[torch.arange(N, device=dev) // spe]
            rows = torch.nonzero(oor).flatten()
            if len(rows):
                if getattr(self, "_full_bp", None) is None:
                    self._full_bp = BatchPlanner(sc.full())
                r = self._full_bp.is_valid(q_active[rows].contiguous(), qpos_env[rows // spe].contiguous(), samples_per_env=1,
                                           want_min_dist=want_min_dist, stream=stream)
                if want_min_dist:
                    valid[rows], md[rows] = r[0], r[1]
                else:
                    valid[rows] = r
        return (valid, md) if want_min_dist else valid

    def contacts(self, q_active, qpos_env, samples_per_env: Optional[int] = None, cutoff: Optional[float] = None,
                 max_contacts: int = 16, stream=None, frames: bool = False, manifold: bool = False, max_points: int = 4,
                 point_cutoff: float = 0.0) -> ContactReport:
        """Which pairs are in contact, for every state of a batch (states as in `is_valid`): one record per non-ignored
        candidate pair with dist <= cutoff, ascending index into `model.pair_geom`; `count` is not capped by `max_contacts`,
        the records with the lowest indices are kept.  cutoff=None: the scene's contact_threshold, i.e. the pairs that make a
        state invalid; any other cutoff must be < 0.  Runs on the scene with the full pair list (`Scene.contact_scene`).
        frames=True: the report also carries `.normal` and `.pos` (one more launch; count / pair / dist are the same bytes).
        manifold=True: the report also carries `.normal`, `.npoint`, `.point_dist` and `.point_pos`: up to max_points (1..8)
        contact points per record with dist_i <= point_cutoff (>= cutoff), deepest first (one more launch behind the report;
        DESIGN.md section 4, "Contact manifolds", PARITY UNPINNED).  With both switches on the report runs once per switch and
        writes the same bytes both times."""
        torch = _torch()
        N, spe = self._state_batch(q_active, qpos_env, samples_per_env)
        K, P = int(max_contacts), int(max_points)
        k1, p1 = max(K, 1), max(P, 1)
        h = self.scene.contact_scene().handle
        dev = q_active.device
        f64 = lambda *shape: torch.empty(N, k1, *shape, dtype=torch.float64, device=dev)
        count = torch.empty(N, dtype=torch.int32, device=dev)
        pair = torch.empty(N, k1, dtype=torch.int32, device=dev)
        dist = f64()
        normal = f64(3) if (frames or manifold) else None
        pos = f64(3) if frames else None
        npoint = torch.empty(N, k1, dtype=torch.int32, device=dev) if manifold else None
        pdist, ppos = (f64(p1), f64(p1, 3)) if manifold else (None, None)
        cut = float(self.scene.contact_threshold if cutoff is None else cutoff)
        states = (h, _ptr(q_active), _ptr(qpos_env), N, spe)
        rows = (_ptr(count), _ptr(pair), _ptr(dist))
        sh = _stream_handle(stream)
        if frames:      # (the frames call first: both write the same normal bits, the manifold's stay)
            _lib.check(_lib.lib().mopa_contact_frames_batch(*states, cut, K, *rows, _ptr(normal), _ptr(pos), sh))
        if manifold:
            _lib.check(_lib.lib().mopa_contact_manifolds_batch(*states, cut, float(point_cutoff), K, P, *rows, _ptr(normal), _ptr(npoint), _ptr(pdist), _ptr(ppos), sh))
        if not (frames or manifold):
            _lib.check(_lib.lib().mopa_contacts_batch(*states, cut, K, *rows, sh))
        return ContactReport(count, pair, dist, self.scene.model, normal, pos, npoint, pdist, ppos)

    def proximity(self, q_active, qpos_env, samples_per_env: Optional[int] = None, band: float = 0.05, max_pairs: int = 8,
                  stream=None, exact: bool = False, witness: bool = False) -> ProximityReport:
        """How far from collision every state of a batch is, and which pairs are nearest (states as in `is_valid`): the signed
        distance of every non-ignored candidate pair at or below `band` (>= 0, metres); `clearance` saturates at band, `count`
        is not capped by `max_pairs`, the nearest pairs are kept.  A pair in overlap carries the contact report's bits; disjoint
        box-box, cylinder and mesh pairs get MuJoCo's margin rule, a conservative distance: never more than 1e-6 above the true
        one, below it by a shortfall that grows with band ("Proximity report").  exact=True
        (mopa_proximity_exact_batch): those pairs get their GJK distance instead -- true <= d <= true + 1e-6, the same bits at
        every band that reports the pair; everything else is unchanged ("Exact route").  One launch of its own on the scene with the
        full pair list (`Scene.contact_scene`); a glued scene raises.
        witness=True (needs exact=True; mopa_proximity_witness_batch): the report also carries `.normal`, `.p1` and `.p2`, where on
        the two shapes each reported distance is attained and in which direction (one more launch behind the report; clearance /
        count / pair / dist are the same bytes; "Witness points").  The inflated route's distance is not attained by any two
        points of the shapes, so witness=True with exact=False raises ValueError."""
        if witness and not exact:
            raise ValueError("witness=True needs exact=True: the inflated route's distance is not attained by two points of the shapes")
        if self.scene.glue is not None:
            raise NotImplementedError("the proximity report of a glued scene")
        torch = _torch()
        N, spe = self._state_batch(q_active, qpos_env, samples_per_env)
        K = int(max_pairs)
        sc = self.scene.contact_scene()
        dev = q_active.device
        clearance = torch.empty(N, dtype=torch.float64, device=dev)
        count = torch.empty(N, dtype=torch.int32, device=dev)
        pair = torch.empty(N, max(K, 1), dtype=torch.int32, device=dev)
        dist = torch.empty(N, max(K, 1), dtype=torch.float64, device=dev)
        if witness:
            normal, p1, p2 = (torch.empty(N, max(K, 1), 3, dtype=torch.float64, device=dev) for _ in range(3))
            _lib.check(_lib.lib().mopa_proximity_witness_batch(sc.handle, _ptr(q_active), _ptr(qpos_env), N, spe, float(band), K, _ptr(clearance), _ptr(count),
                                                               _ptr(pair), _ptr(dist), _ptr(normal), _ptr(p1), _ptr(p2), _stream_handle(stream)))
            return ProximityReport(clearance, count, pair, dist, self.scene.model, normal, p1, p2)
        fn = _lib.lib().mopa_proximity_exact_batch if exact else _lib.lib().mopa_proximity_batch
        _lib.check(fn(sc.handle, _ptr(q_active), _ptr(qpos_env), N, spe, float(band), K, _ptr(clearance), _ptr(count), _ptr(pair), _ptr(dist),
                      _stream_handle(stream)))
        return ProximityReport(clearance, count, pair, dist, self.scene.model)

    def clearance(self, q_active, qpos_env, samples_per_env: Optional[int] = None, band: float = 0.05, stream=None, exact: bool = False):
        """`proximity(...).clearance` alone: [N] float64, min(band, the smallest pair distance) of every state"""
        return self.proximity(q_active, qpos_env, samples_per_env, band=band, max_pairs=1, stream=stream, exact=exact).clearance

    def glue_attach(self, rows, stream=None):
        """glued scene (`Scene.glued`): rows [E, nq] -> their attached rows, copies whose free-joint slots of the carried body hold
        its offset (t, rq) under body_a at the row's own joint values (mopa_glue_attach_batch); `is_valid`, `check_motion` and `plan`
        do this internally"""
        torch = _torch()
        _check_f64(rows, "rows", self.nq)
        out = torch.empty_like(rows)
        _lib.check(_lib.lib().mopa_glue_attach_batch(self.scene.handle, _ptr(rows), rows.shape[0], _ptr(out), _stream_handle(stream)))
        return out

    def glue_rows(self, path, path_len, attached, stream=None):
        """glued scene: the carried body's pose at every waypoint into the free-joint columns of the rows r < path_len[e] of
        path [E, max_path, nq], in place (mopa_glue_rows_batch); `plan` does this internally"""
        torch = _torch()
        _check_f64(attached, "attached", self.nq)
        if (path.dtype != torch.float64 or not path.is_cuda or not path.is_contiguous() or path.dim() != 3 or path.shape[2] != self.nq
                or path.shape[0] != attached.shape[0]):
            raise _lib.MopaError("path must be a contiguous float64 GPU tensor [E, max_path, nq] with E = attached.shape[0]")
        if path_len.dtype != torch.int32 or not path_len.is_cuda or not path_len.is_contiguous() or path_len.shape != (path.shape[0],):
            raise _lib.MopaError("path_len must be a contiguous int32 GPU tensor [E]")
        _lib.check(_lib.lib().mopa_glue_rows_batch(self.scene.handle, _ptr(path), _ptr(path_len), _ptr(attached), path.shape[0], path.shape[1],
                                                   _stream_handle(stream)))
        return path

    def check_motion(self, qa, qb, qpos_env, samples_per_env: Optional[int] = None, stream=None):
        torch = _torch()
        N, spe = self._segment_batch(qa, qb, qpos_env, samples_per_env)
        valid = torch.empty(N, dtype=torch.uint8, device=qa.device)
        _lib.check(_lib.lib().mopa_check_motion_batch(self.scene.handle, _ptr(qa), _ptr(qb), _ptr(qpos_env), N, spe,
                                                      _ptr(valid), _stream_handle(stream)))
        return valid

    def motion_report(self, qa, qb, qpos_env, samples_per_env: Optional[int] = None, states: bool = True, max_contacts: int = 0,
                      stream=None) -> MotionReport:
        """Where every segment qa[i] -> qb[i] is blocked, and by which pairs (mopa_motion_report_batch; segments and env rows as
        in `check_motion`, whose bytes `.valid` holds): OMPL's checkMotion(s1, s2, lastValid) -- the first invalid state in
        ascending order, the last valid parameter and state before it -- see `MotionReport`.  states=False leaves the two [N, na]
        rows out.  max_contacts = K >= 1: `.blockers` is the contact report of the states first_bad_q at the scene's
        contact_threshold with that K, the bytes of `contacts(first_bad_q, qpos_env, max_contacts=K)` -- in the same call on a
        scene that holds the whole pair list, else on `Scene.contact_scene()` behind it.  The large-batch form
        (`Scene.motion_kernel`) synchronises the stream once per call, as `check_motion`'s does."""
        torch = _torch()
        N, spe = self._segment_batch(qa, qb, qpos_env, samples_per_env)
        K = int(max_contacts)
        if K < 0:
            raise _lib.MopaError("max_contacts must be >= 0")
        dev = qa.device
        valid = torch.empty(N, dtype=torch.uint8, device=dev)
        n_states = torch.empty(N, dtype=torch.int32, device=dev)
        first_bad = torch.empty(N, dtype=torch.int32, device=dev)
        t = torch.empty(N, dtype=torch.float64, device=dev)
        csc = self.scene.contact_scene() if K else None
        chained = K != 0 and csc is self.scene
        lvq = torch.empty(N, self.na, dtype=torch.float64, device=dev) if states else None
        fbq = torch.empty(N, self.na, dtype=torch.float64, device=dev) if (states or (K and not chained)) else None
        count = pair = dist = None
        if K:
            count = torch.empty(N, dtype=torch.int32, device=dev)
            pair = torch.empty(N, K, dtype=torch.int32, device=dev)
            dist = torch.empty(N, K, dtype=torch.float64, device=dev)
        opt = lambda x: _ptr(x) if x is not None else None
        sh = _stream_handle(stream)
        _lib.check(_lib.lib().mopa_motion_report_batch(self.scene.handle, _ptr(qa), _ptr(qb), _ptr(qpos_env), N, spe, _ptr(valid), _ptr(n_states),
                                                       _ptr(first_bad), _ptr(t), opt(lvq), opt(fbq), K if chained else 0,
                                                       opt(count) if chained else None, opt(pair) if chained else None,
                                                       opt(dist) if chained else None, sh))
        if K and not chained:
            _lib.check(_lib.lib().mopa_contacts_batch(csc.handle, _ptr(fbq), _ptr(qpos_env), N, spe, float(self.scene.contact_threshold), K,
                                                      _ptr(count), _ptr(pair), _ptr(dist), sh))
        blockers = ContactReport(count, pair, dist, self.scene.model) if K else None
        return MotionReport(valid, n_states, first_bad, t, lvq, fbq if states else None, blockers)

    def motion_clearance(self, qa, qb, qpos_env, samples_per_env: Optional[int] = None, band: float = 0.05, states: bool = False,
                         stream=None, exact: bool = False) -> MotionClearance:
        """How near every segment qa[i] -> qb[i] comes to collision, where along it and to which pair (mopa_motion_clearance_batch;
        segments and env rows as in `check_motion`): OMPL's MinimaxObjective::motionCost under the clearance state cost, over the
        states `motion_report` walks, each state's clearance and nearest pair being the bits of `proximity(..., max_pairs=1)` --
        see `MotionClearance`.  states=True adds the [N, na] rows q_min.  exact=True (mopa_motion_clearance_exact_batch): the bits of
        `proximity(..., max_pairs=1, exact=True)` per state.  Runs on the scene with the full pair list
        (`Scene.contact_scene`) and synchronises the stream once in the middle of the call (the state count is read back), as the
        large-batch `check_motion` does -- the last kernels are still in flight when it returns; N == 0 gives an empty report
        without a call; a glued scene raises."""
        if self.scene.glue is not None:
            raise NotImplementedError("the clearance report of a glued scene")
        torch = _torch()
        N, spe = self._segment_batch(qa, qb, qpos_env, samples_per_env)
        if not (math.isfinite(float(band)) and float(band) >= 0.0):
            raise _lib.MopaError("band must be finite and >= 0")
        sc = self.scene.contact_scene()
        dev = qa.device
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
        i32 = lambda: torch.empty(N, dtype=torch.int32, device=dev)
        clearance, t_min, end_clearance = f64(N), f64(N), f64(N)
        n_states, n_near, k_min, pair_min = i32(), i32(), i32(), i32()
        q_min = f64(N, self.na) if states else None
        if N == 0:      # (empty tensors have no address to pass: an empty report, no call)
            return MotionClearance(clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance, q_min, self.scene.model)
        fn = _lib.lib().mopa_motion_clearance_exact_batch if exact else _lib.lib().mopa_motion_clearance_batch
        _lib.check(fn(sc.handle, _ptr(qa), _ptr(qb), _ptr(qpos_env), N, spe, float(band), _ptr(clearance), _ptr(n_states), _ptr(n_near), _ptr(k_min),
                      _ptr(t_min), _ptr(pair_min), _ptr(end_clearance), _ptr(q_min) if states else None, _stream_handle(stream)))
        return MotionClearance(clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance, q_min, self.scene.model)

    def path_clearance(self, path, path_len, band: float = 0.05, stream=None, exact: bool = False) -> PathClearance:
        """The clearance of E planner paths (path [E, max_path, nq], path_len [E] int32, as `plan` returns them): the path cost of
        the minimax clearance objective with vertex 0 counted, where along the path it is attained and to which pair, and the mean
        clearance of the vertices -- see `PathClearance` and DESIGN.md section 4, "Clearance report".  The env row of a path is its
        row 0; the rows of an unsolved query (path_len == 0) are not read.  Torch plumbing around `motion_clearance` (all segments
        of all paths in one call) and `proximity` (the vertices 0 of the solved queries); the reductions are deterministic.
        Cost besides the pipeline's own read-back: `path_len` is copied to the host once (E int32, one more synchronisation of the
        stream) to lay out the segment list, and the mean is summed left to right by one small launch per column up to the
        longest path.  exact=True: both calls with exact=True."""
        if self.scene.glue is not None:
            raise NotImplementedError("the clearance report of a glued scene")
        torch = _torch()
        if path.dtype != torch.float64 or not path.is_cuda or not path.is_contiguous() or path.dim() != 3 or path.shape[2] != self.nq:
            raise _lib.MopaError("path must be a contiguous float64 GPU tensor [E, max_path, nq]")
        if path_len.dtype != torch.int32 or not path_len.is_cuda or not path_len.is_contiguous() or path_len.shape != (path.shape[0],):
            raise _lib.MopaError("path_len must be a contiguous int32 GPU tensor [E]")
        E, P = path.shape[0], path.shape[1]
        if P < 1:
            raise _lib.MopaError("path must hold at least one row per query")
        dev = path.device
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            hl = path_len.cpu().numpy().astype(np.int64)                   # the read-back
            if ((hl < 0) | (hl > P)).any():
                raise _lib.MopaError("path_len must lie in 0 .. max_path")
            nseg = np.maximum(hl - 1, 0)
            start = np.cumsum(nseg) - nseg
            to_dev = lambda a: torch.as_tensor(a, dtype=torch.long, device=dev)
            pe = to_dev(np.repeat(np.arange(E), nseg))                     # (path, j) of every segment, path by path, j ascending
            pj = to_dev(np.arange(int(nseg.sum())) - np.repeat(start, nseg))
            solved = to_dev(np.nonzero(hl >= 1)[0])
            act = to_dev(np.asarray(self.scene.active_idx))
            L = path_len.long()
            jj = torch.arange(P - 1, device=dev)
            pa = path[:, :, act]                                           # [E, P, na]
            seg = self.motion_clearance(pa[pe, pj].contiguous(), pa[pe, pj + 1].contiguous(), path[pe, 0].contiguous(), samples_per_env=1,
                                        band=band, stream=stream, exact=exact)
            seg.path_index, seg.seg_index = pe, pj
            v0 = torch.full((E,), float("nan"), dtype=torch.float64, device=dev)
            p0 = torch.full((E,), -1, dtype=torch.int32, device=dev)
            if len(solved):
                v = self.proximity(pa[solved, 0].contiguous(), path[solved, 0].contiguous(), samples_per_env=1, band=band, max_pairs=1, stream=stream,
                                   exact=exact)
                v0[solved], p0[solved] = v.clearance, v.pair[:, 0]
            segc = torch.full((E, P - 1), float("inf"), dtype=torch.float64, device=dev)
            segk = torch.zeros(E, P - 1, dtype=torch.int32, device=dev)
            segp = torch.full((E, P - 1), -1, dtype=torch.int32, device=dev)
            ende = torch.zeros(E, P - 1, dtype=torch.float64, device=dev)
            segc[pe, pj], segk[pe, pj], segp[pe, pj], ende[pe, pj] = seg.clearance, seg.k_min, seg.pair_min, seg.end_clearance
            clearance = torch.cat([v0[:, None], segc], dim=1).min(dim=1).values
            # the first segment that attains the minimum (not torch.min's index, whose tie rule is not specified)
            first = torch.where(segc == clearance[:, None], jj[None, :], P).min(dim=1).values if P > 1 else torch.full((E,), P, device=dev)
            at_v0 = (v0 == clearance) | (first >= P)
            seg_min = torch.where(at_v0, -1, first)
            g = seg_min.clamp(min=0)[:, None]
            zero = torch.zeros(E, dtype=torch.int32, device=dev)
            k_min = torch.where(at_v0, zero, segk.gather(1, g)[:, 0] if P > 1 else zero)
            pair_min = torch.where(at_v0, p0, segp.gather(1, g)[:, 0] if P > 1 else p0)
            acc = v0.clone()                                               # left to right: v_0, then the end state of segment 0, 1, ...
            for j in range(int(nseg.max()) if E else 0):                   # (the longest path's segments)
                acc = torch.where(L - 1 > j, acc + ende[:, j], acc)
            mean = acc / L.double()
            none = L <= 0                                                  # an unsolved query: NaN, -1, 0, -1, NaN
            nan = torch.full((E,), float("nan"), dtype=torch.float64, device=dev)
            clearance = torch.where(none, nan, clearance)
            mean = torch.where(none, nan, mean)
            seg_min = torch.where(none, -1, seg_min).int()
            k_min = torch.where(none, zero, k_min)
            pair_min = torch.where(none, torch.full_like(p0, -1), pair_min)
        return PathClearance(clearance, seg_min, k_min, pair_min, mean, seg)

    def plan(self, start, goal, max_iters: int = 2000, max_nodes: int = 1024, max_path: int = 256, seed: int = 0,
             env_id_base: int = 0, stream=None, env_ids=None, seeds=None, max_workgroups: int = 0, exclusive: bool = False,
             keep_state: bool = False, resume=None, vertex_simplify: bool = False,
             simplify_passes: int = 3, path_shortcut: bool = False,
             path_smooth: bool = False) -> Tuple["object", "object", "object", "object"]:
        """E independent RRT-Connect queries.  Returns (path[E,max_path,nq], path_len[E], status[E], n_checks[E]).
        env_ids (int64 [E] GPU tensor, optional): the sample-stream id of every query (default env_id_base + index).
        seeds (int64 [E] GPU tensor, optional): a seed per query instead of `seed`.
        max_workgroups: 0 = one persistent workgroup per CU (shortest lone launch), < 0 = as many as the chip holds (throughput:
        launches that overlap others), > 0 = explicit cap; exclusive: no other planner workgroup shares this launch's CUs
        (include/mopa_hip.h).
        keep_state: the launch keeps its trees in tensors of its own and returns a fifth element, a `PlanState` (tree_q, tree_p,
        state, max_nodes), from which a later launch with a larger `max_iters` continues the unsolved queries: `resume=` a
        PlanState whose rows are in this launch's query order (`PlanState.rows(idx)` gathers; same max_nodes, same seeds / ids).
        The continued run gives what one launch with the larger budget gives, without retracing the first iterations.
        vertex_simplify: the launch of `simplify_paths` (K9: OMPL's two vertex-removing passes, `simplify_passes` selects them) goes
        directly behind the planner's on the same stream with the same seed / ids / seeds, so the rows and `path_len` that come
        back are the simplified ones; `n_checks` stays the planner's own count.  A continuation leaves `path_len` 0 for the
        queries an earlier launch settled, so every query's final rows are simplified exactly once.
        path_shortcut: the launch of `shortcut_paths` (K9 with OMPL's shortcutPath in front) takes that place instead, with
        passes = 4 | (simplify_passes if vertex_simplify else 0): the rows that come back include states that are no planner
        rows, and `path_len` may have grown (never beyond max_path).
        path_smooth: the launch of `smooth_paths` (K9 with OMPL's smoothBSpline between shortcutPath and the vertex passes) takes
        that place instead, with passes = 8 | (4 if path_shortcut else 0) | (simplify_passes if vertex_simplify else 0); the three
        flags together are PathSimplifier::simplify's schedule without its wall clock."""
        torch = _torch()
        _check_f64(start, "start", self.nq)
        _check_f64(goal, "goal", self.nq)
        E = start.shape[0]
        dev = start.device
        ps = None
        if keep_state:
            na = self.scene.na
            ps = PlanState(torch.empty(E * 2 * max_nodes * na + 8, dtype=torch.float64, device=dev),
                           torch.empty(E * 2 * max_nodes, dtype=torch.int32, device=dev),
                           torch.zeros(E, 4, dtype=torch.int64, device=dev), int(max_nodes), na)
        if resume is not None and (resume.max_nodes != int(max_nodes) or resume.state.shape[0] != E):
            raise _lib.MopaError("resume: a PlanState of this launch's queries (same order, same max_nodes) is needed")
        path = torch.zeros(E, max_path, self.nq, dtype=torch.float64, device=dev)
        plen = torch.zeros(E, dtype=torch.int32, device=dev)
        status = torch.zeros(E, dtype=torch.int32, device=dev)
        nchk = torch.zeros(E, dtype=torch.int64, device=dev)
        if env_ids is not None and (env_ids.dtype != torch.int64 or not env_ids.is_cuda or not env_ids.is_contiguous()
                                    or tuple(env_ids.shape) != (E,)):
            raise _lib.MopaError("env_ids must be a contiguous int64 GPU tensor of shape [E]")
        if seeds is not None and (seeds.dtype != torch.int64 or not seeds.is_cuda or not seeds.is_contiguous() or tuple(seeds.shape) != (E,)):
            raise _lib.MopaError("seeds must be a contiguous int64 GPU tensor of shape [E]")
        prm = _lib.MopaPlanParams(int(max_iters), int(max_nodes), int(max_path), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  int(env_id_base), _ptr(env_ids) if env_ids is not None else None,
                                  _ptr(seeds) if seeds is not None else None, int(max_workgroups), 1 if exclusive else 0,
                                  _ptr(ps.tree_q) if ps else None, _ptr(ps.tree_p) if ps else None, _ptr(ps.state) if ps else None,
                                  _ptr(resume.tree_q) if resume is not None else None, _ptr(resume.tree_p) if resume is not None else None,
                                  _ptr(resume.state) if resume is not None else None)
        _lib.check(_lib.lib().mopa_plan_batch(self.scene.handle, _ptr(start), _ptr(goal), E, C.byref(prm), _ptr(path),
                                              _ptr(plen), _ptr(status), _ptr(nchk), _stream_handle(stream)))
        if resume is not None and stream is not None:
            for t in (resume.tree_q, resume.tree_p, resume.state):
                t.record_stream(stream)
        self._k9_behind(path, plen, status, seed, env_id_base, env_ids, seeds, vertex_simplify, simplify_passes, path_shortcut, path_smooth, stream)
        return (path, plen, status, nchk, ps) if keep_state else (path, plen, status, nchk)

    def plan_star(self, start, goal, max_iters: int = 2000, max_nodes: Optional[int] = None, max_path: int = 256, seed: int = 0,
                  env_id_base: int = 0, stream=None, env_ids=None, seeds=None, max_workgroups: int = 0,
                  goal_bias: float = _lib.STAR_GOAL_BIAS, goal_threshold: float = 0.0, rewire_factor: float = _lib.STAR_REWIRE_FACTOR,
                  want_info: bool = False, vertex_simplify: bool = False, simplify_passes: int = 3, path_shortcut: bool = False,
                  path_smooth: bool = False):
        """E independent RRT* queries (K3b: the reference's planner_type "rrt"; DESIGN.md "K3b RRT*").  Returns (path [E, max_path,
        nq], path_len [E], status [E], cost [E]) -- cost = the L1 length of the returned chain, +inf unless status is 0 -- and with
        `want_info` a fifth element, an int64 [E, 8] tensor: iterations run, nodes, motion checks, rewires, goal nodes, first goal
        iteration (-1: none), descendant cost updates, iterations that found the tree full.  The planner is anytime: every query
        spends all of `max_iters`.  max_nodes=None: max_iters + 1, which no query can fill.  goal_threshold: a new state this close
        to the goal (L1) is a goal node; 0 = the goal sample itself, drawn with probability `goal_bias` until one exists.
        env_ids / seeds / env_id_base / seed / stream: as for `plan`.  max_workgroups > 0 caps the persistent workgroups.
        vertex_simplify / simplify_passes / path_shortcut / path_smooth: exactly as in `plan`, the K9 launch goes behind this one on
        the same stream with the same seed / ids / seeds (its draws are disjoint from the planner's); `cost` stays the planner's."""
        torch = _torch()
        _check_f64(start, "start", self.nq)
        _check_f64(goal, "goal", self.nq)
        E = start.shape[0]
        dev = start.device
        for t, name in ((env_ids, "env_ids"), (seeds, "seeds")):
            if t is not None and (t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (E,)):
                raise _lib.MopaError(f"{name} must be a contiguous int64 GPU tensor of shape [E]")
        nodes = int(max_iters) + 1 if max_nodes is None else int(max_nodes)

        def alloc():
            return (torch.zeros(E, max_path, self.nq, dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.int32, device=dev),
                    torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.float64, device=dev),
                    torch.zeros(E, _lib.STAR_INFO_COLS, dtype=torch.int64, device=dev) if want_info else None)
        if stream is not None:
            with torch.cuda.stream(stream):
                path, plen, status, cost, info = alloc()
        else:
            path, plen, status, cost, info = alloc()
        prm = _lib.MopaStarParams(int(max_iters), max(nodes, 2), int(max_path), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_base),
                                  _ptr(env_ids) if env_ids is not None else None, _ptr(seeds) if seeds is not None else None,
                                  float(goal_bias), float(goal_threshold), float(rewire_factor), int(max_workgroups))
        _lib.check(_lib.lib().mopa_plan_star_batch(self.scene.handle, _ptr(start), _ptr(goal), E, C.byref(prm), _ptr(path), _ptr(plen),
                                                   _ptr(status), _ptr(cost), _ptr(info) if info is not None else None, _stream_handle(stream)))
        self._k9_behind(path, plen, status, seed, env_id_base, env_ids, seeds, vertex_simplify, simplify_passes, path_shortcut, path_smooth, stream)
        return (path, plen, status, cost, info) if want_info else (path, plen, status, cost)

    def plan_star_clearance(self, start, goal, band: float, max_iters: int = 2000, max_nodes: Optional[int] = None, max_path: int = 256,
                            seed: int = 0, env_id_base: int = 0, stream=None, env_ids=None, seeds=None, max_workgroups: int = 0,
                            goal_bias: float = _lib.STAR_GOAL_BIAS, goal_threshold: float = 0.0,
                            rewire_factor: float = _lib.STAR_REWIRE_FACTOR, want_info: bool = False):
        """E independent RRT* queries under the maximize-min-clearance objective, band-limited ("K3b under the
        clearance objective"): the planner that optimises what `path_clearance` measures.  Returns (path [E, max_path, nq], path_len
        [E], status [E], clearance [E], length [E]) and with `want_info` a sixth element, an int64 [E, 11] tensor: `plan_star`'s
        eight columns with motion evaluations in column 2, then the evaluations of the parent walk, those of the rewire step, and the
        rewires that strictly raised a clearance.  A chain's cost is the pair (clearance, larger is better; then L1 length, smaller
        is better): `clearance` is the bits of `path_clearance(path, path_len, band).clearance`, `length` the chain's L1 length;
        -inf and +inf unless status is 0.  `band`: finite, >= 0 and above the scene's contact threshold.  For equal seeds, ids and
        parameters the tree holds the nodes `plan_star` grows; where no evaluated motion is in band the result is `plan_star`'s.
        Every other keyword is `plan_star`'s.  Runs on the scene with the full pair list (`Scene.contact_scene`), as the clearance
        report does; a glued scene raises.  The K9 switches are not offered: a simplifier behind this planner would change the
        clearance it reports -- call `simplify_paths` and `path_clearance` on the result instead.
        The planner stays on the inflated (margin-rule) distances: `path_clearance(path, path_len, band, exact=True)`
        of a returned path is never lower than `clearance`, up to kGjkTol = 1e-6; equality of bits holds with exact=False only."""
        torch = _torch()
        _check_f64(start, "start", self.nq)
        _check_f64(goal, "goal", self.nq)
        E = start.shape[0]
        dev = start.device
        for t, name in ((env_ids, "env_ids"), (seeds, "seeds")):
            if t is not None and (t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (E,)):
                raise _lib.MopaError(f"{name} must be a contiguous int64 GPU tensor of shape [E]")
        nodes = int(max_iters) + 1 if max_nodes is None else int(max_nodes)

        def alloc():
            return (torch.zeros(E, max_path, self.nq, dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.int32, device=dev),
                    torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.float64, device=dev),
                    torch.zeros(E, dtype=torch.float64, device=dev),
                    torch.zeros(E, _lib.STAR_CLEARANCE_INFO_COLS, dtype=torch.int64, device=dev) if want_info else None)
        if stream is not None:
            with torch.cuda.stream(stream):
                path, plen, status, clearance, length, info = alloc()
        else:
            path, plen, status, clearance, length, info = alloc()
        prm = _lib.MopaStarParams(int(max_iters), max(nodes, 2), int(max_path), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_base),
                                  _ptr(env_ids) if env_ids is not None else None, _ptr(seeds) if seeds is not None else None,
                                  float(goal_bias), float(goal_threshold), float(rewire_factor), int(max_workgroups))
        # the scene with the full pair list, as the clearance report runs on (a glued scene goes to the library as it is, which refuses it)
        sc = self.scene if self.scene.glue is not None else self.scene.contact_scene()
        _lib.check(_lib.lib().mopa_plan_star_clearance_batch(sc.handle, _ptr(start), _ptr(goal), E, C.byref(prm), float(band), _ptr(path),
                                                             _ptr(plen), _ptr(status), _ptr(clearance), _ptr(length),
                                                             _ptr(info) if info is not None else None, _stream_handle(stream)))
        return (path, plen, status, clearance, length, info) if want_info else (path, plen, status, clearance, length)

    def plan_race(self, start, goal, portfolio: int = 4, max_iters: int = 2000, max_nodes: int = 1024, max_path: int = 256, seed: int = 0,
                  env_id_base: int = 0, env_ids=None, seeds=None, stream=None, max_workgroups: int = 0, no_abort: bool = False,
                  want_info: bool = False, vertex_simplify: bool = False, simplify_passes: int = 3, path_shortcut: bool = False,
                  path_smooth: bool = False):
        """E RRT-Connect queries, each run by `portfolio` (1 .. 256) members that share start, goal and stream id and differ in their
        seed only: member m runs (seed + m * 0x9E3779B97F4A7C15) mod 2^64, member 0 is exactly the query `plan` runs (K3 race,
        DESIGN.md).  The result of a query is that of ONE member: the solved one with the smallest (consumed checks, m) -- a rule that
        does not depend on timing; members that can no longer win stop early unless `no_abort`.  Returns (path [E, max_path, nq],
        path_len [E], status [E], n_checks [E] = the winner's, winner [E] int32 (-1: no member solved; n_checks and win_seed are
        then member 0's), win_seed [E] int64 (bit pattern of the winner's seed)) and with `want_info` a seventh element, an int64
        [E, 3] tensor: members cut, checks spent by all members until they stopped (both depend on timing unless `no_abort`), the
        winner's iterations (-1: none).  Tree scratch is E * portfolio * 2 * max_nodes * na doubles plus parents.
        env_ids / seeds / env_id_base / seed / stream / max_workgroups: as for `plan`, the launch policy applied to E * portfolio slots.
        vertex_simplify / simplify_passes / path_shortcut / path_smooth: as in `plan`, but the K9 launch draws with seeds=win_seed,
        the winner's stream."""
        torch = _torch()
        _check_f64(start, "start", self.nq)
        _check_f64(goal, "goal", self.nq)
        E = start.shape[0]
        dev = start.device
        for t, name in ((env_ids, "env_ids"), (seeds, "seeds")):
            if t is not None and (t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (E,)):
                raise _lib.MopaError(f"{name} must be a contiguous int64 GPU tensor of shape [E]")

        def alloc():
            return (torch.zeros(E, max_path, self.nq, dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.int32, device=dev),
                    torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int64, device=dev),
                    torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int64, device=dev),
                    torch.zeros(E, _lib.RACE_INFO_COLS, dtype=torch.int64, device=dev) if want_info else None)
        if stream is not None:
            with torch.cuda.stream(stream):
                path, plen, status, nchk, winner, wseed, info = alloc()
        else:
            path, plen, status, nchk, winner, wseed, info = alloc()
        prm = _lib.MopaRaceParams(int(max_iters), int(max_nodes), int(max_path), int(portfolio), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_base),
                                  _ptr(env_ids) if env_ids is not None else None, _ptr(seeds) if seeds is not None else None,
                                  int(max_workgroups), 1 if no_abort else 0)
        _lib.check(_lib.lib().mopa_plan_race_batch(self.scene.handle, _ptr(start), _ptr(goal), E, C.byref(prm), _ptr(path), _ptr(plen), _ptr(status),
                                                   _ptr(nchk), _ptr(winner), _ptr(wseed), _ptr(info) if info is not None else None,
                                                   _stream_handle(stream)))
        self._k9_behind(path, plen, status, seed, env_id_base, env_ids, wseed, vertex_simplify, simplify_passes, path_shortcut, path_smooth, stream)
        return (path, plen, status, nchk, winner, wseed, info) if want_info else (path, plen, status, nchk, winner, wseed)

    def simplify_paths(self, path, plen, status=None, seed: int = 0, env_id_base: int = 0, env_ids=None, seeds=None, passes: int = 3,
                       stream=None, want_info: bool = False):
        """K9, in place: OMPL's reduceVertices (passes bit 0) and collapseCloseVertices (bit 1) over the planner's rows -- `path`
        [E, max_path, nq] float64, `plen` [E] int32, `status` [E] int32 or None -- one wave per path, asynchronous, no read-back.
        Every surviving row is one of the input rows; they are compacted to the front and `plen` is rewritten (rows behind it are
        unspecified).  Paths with a non-zero status or fewer than 3 rows are not touched.  seed / env_id_base / env_ids / seeds: what
        `plan` was given (the draws come from the planner's sample stream of the query, at counters from 2^63 on).  shortcutPath,
        B-spline smoothing and checkAndRepair of OMPL's simplify() are not built.  Returns None, or with `want_info` an int64
        [E, 2] tensor: motion checks made, draws consumed (0 for untouched paths)."""
        return self._k9_rows_launch(_lib.lib().mopa_simplify_paths_batch, 2, path, plen, status, seed, env_id_base, env_ids, seeds, passes, None,
                                    stream, want_info)

    def shortcut_paths(self, path, plen, status=None, seed: int = 0, env_id_base: int = 0, env_ids=None, seeds=None, passes: int = 7,
                       max_rounds: int = 16, stream=None, want_info: bool = False):
        """K9 with shortcutPath, in place: OMPL's shortcutPath (passes bit 2) in front of reduceVertices (bit 0) and
        collapseCloseVertices (bit 1) -- arguments as for `simplify_paths`, one wave per path, asynchronous, no read-back.
        shortcutPath connects points inside segments, so rows that are no input rows appear (interpolated active entries, row 0's
        passive ones) and `plen` can grow, never beyond max_path; a splice is accepted only when the stubs next to a new interior
        point pass the motion check as well, so every segment of the result has passed it (DESIGN.md "K9 path simplification:
        shortcutPath").  Paths with a non-zero status, fewer than 3 rows or more than max_path are not touched.  `max_rounds`
        bounds the rounds of OMPL's schedule.  With bit 2 clear the result is `simplify_paths`'s.  smoothBSpline is
        `smooth_paths`; checkAndRepair is not built.  Returns None, or with `want_info` an int64 [E, 6] tensor: motion checks, draws, rounds,
        accepted shortcut splices, capacity skips, largest vertex count reached (0 for untouched paths)."""
        return self._k9_rows_launch(_lib.lib().mopa_shortcut_paths_batch, 6, path, plen, status, seed, env_id_base, env_ids, seeds, passes, max_rounds,
                                    stream, want_info)

    def smooth_paths(self, path, plen, status=None, seed: int = 0, env_id_base: int = 0, env_ids=None, seeds=None, passes: int = 15,
                     max_rounds: int = 16, stream=None, want_info: bool = False):
        """K9 with smoothBSpline, in place: per round OMPL's shortcutPath (passes bit 2), then smoothBSpline (bit 3), then
        reduceVertices (bit 0) and collapseCloseVertices (bit 1) -- arguments as for `shortcut_paths`, one wave per path,
        asynchronous, no read-back.  A smoothing step puts a vertex into the middle of every segment and pulls the old interior
        vertices towards their new neighbours, so rows that are no input rows appear and input rows change their active entries;
        `plen` can grow, never beyond max_path (a step that would need more rows ends the smoothing and counts as a capacity
        skip).  A vertex moves only if every segment that results has itself passed the motion check (DESIGN.md "K9 path
        simplification: smoothBSpline").  Paths with a non-zero status, fewer than 3 rows or more than max_path are not touched.
        With bit 3 clear the result is `shortcut_paths`'s.  checkAndRepair is not built (nothing is left for it to repair).
        Returns None, or with `want_info` an int64 [E, 10] tensor: motion checks, draws, rounds, accepted shortcut splices,
        capacity skips, largest vertex count reached, smoothing steps subdivided, vertices moved, idle midpoints dropped, state
        checks (0 for untouched paths)."""
        return self._k9_rows_launch(_lib.lib().mopa_smooth_paths_batch, 10, path, plen, status, seed, env_id_base, env_ids, seeds, passes, max_rounds,
                                    stream, want_info)

    def _k9_rows_launch(self, entry, info_cols, path, plen, status, seed, env_id_base, env_ids, seeds, passes, max_rounds, stream, want_info):
        """argument checks and launch shared by `simplify_paths`, `shortcut_paths` and `smooth_paths`; max_rounds=None: the entry
        point takes no such argument (`simplify_paths`)"""
        torch = _torch()
        if path.dtype != torch.float64 or not path.is_cuda or not path.is_contiguous() or path.dim() != 3 or path.shape[2] != self.nq:
            raise _lib.MopaError(f"path must be a contiguous float64 GPU tensor of shape [E, max_path, {self.nq}]")
        E, max_path = int(path.shape[0]), int(path.shape[1])
        for t, name in ((plen, "plen"), (status, "status")):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (E,)):
                raise _lib.MopaError(f"{name} must be a contiguous int32 GPU tensor of shape [E]")
        for t, name in ((env_ids, "env_ids"), (seeds, "seeds")):
            if t is not None and (t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (E,)):
                raise _lib.MopaError(f"{name} must be a contiguous int64 GPU tensor of shape [E]")
        info = None
        if want_info:
            if stream is not None:
                with torch.cuda.stream(stream):
                    info = torch.zeros(E, info_cols, dtype=torch.int64, device=path.device)
            else:
                info = torch.zeros(E, info_cols, dtype=torch.int64, device=path.device)
        _lib.check(entry(
            self.scene.handle, E, max_path, _ptr(path), _ptr(plen), _ptr(status) if status is not None else None,
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_base), _ptr(env_ids) if env_ids is not None else None,
            _ptr(seeds) if seeds is not None else None, int(passes), *(() if max_rounds is None else (int(max_rounds),)),
            _ptr(info) if info is not None else None, _stream_handle(stream)))
        return info

    def _k9_behind(self, path, plen, status, seed, env_id_base, env_ids, seeds, vertex_simplify, simplify_passes, path_shortcut, path_smooth,
                   stream):
        """the K9 launch the flags of `plan` / `plan_star` select, behind the planner's on the same stream with the same seed / ids /
        seeds; none when all flags are off"""
        name = k9_entry(vertex_simplify, path_shortcut, path_smooth)
        if name is not None:
            getattr(self, name)(path, plen, status, seed=seed, env_id_base=env_id_base, env_ids=env_ids, seeds=seeds,
                                passes=k9_passes(vertex_simplify, simplify_passes, path_shortcut, path_smooth), stream=stream)

    def plan_laddered(self, batches, max_iters: int = 2000, first_iters: int = 100, max_nodes: int = 1024, max_path: int = 256,
                      retry_streams=None, first_stream=None, max_workgroups_first: int = -1, retry_min: int = 1024, resume: bool = True,
                      retry_exclusive: bool = False, vertex_simplify: bool = False, simplify_passes: int = 3,
                      path_shortcut: bool = False, path_smooth: bool = False):
        """A stream of query batches through RRT-Connect with an iteration ladder.  `batches`: list of dicts with `start`,
        `goal` ([E, nq] tensors), `seed` and optionally `env_ids` / `seeds` as for `plan`.  Every batch first runs with
        `first_iters`; the queries that come back "no exact solution" (a few %: the ones that would have kept the whole
        launch waiting for their 2000 iterations) run again with `max_iters` -- pooled over batches until `retry_min` of them
        wait -- on other streams, next to the following batches' first launches.  A query's outcome depends on its endpoints and sample stream only and the budget merely
        ends the loop, so the second run continues where the first stopped (`resume`: from its trees and counters; False: it retraces
        the first iterations): each batch's (path, path_len, status, n_checks)
        are those of `plan(..., max_iters=max_iters)`, bit for bit.  Returns the list of those tuples (after all launches
        have finished).  One host read-back per batch (which queries go again).  The defaults of `first_iters` / `retry_min` are
        the ones that measured best over long streams of 4096-query batches on Push (tools/ladder_grid.py: 100 / 1024; they only
        schedule the work).  vertex_simplify / simplify_passes: as for `plan`, passed to every launch -- a query is solved by
        exactly one of them, which simplifies its rows.  path_shortcut, path_smooth: as for `plan`, likewise."""
        vs = dict(vertex_simplify=vertex_simplify, simplify_passes=simplify_passes, path_shortcut=path_shortcut)
        if path_smooth:          # (flag off: the launches get exactly the keywords they got before)
            vs["path_smooth"] = True
        torch = _torch()
        if first_iters <= 0 or first_iters >= max_iters:
            return [self.plan(b["start"], b["goal"], max_iters=max_iters, max_nodes=max_nodes, max_path=max_path, seed=b.get("seed", 0),
                              env_ids=b.get("env_ids"), seeds=b.get("seeds"), **vs) for b in batches]
        dev = batches[0]["start"].device
        main = torch.cuda.current_stream(dev)
        sa = first_stream if first_stream is not None else torch.cuda.Stream(device=dev)
        sbs = list(retry_streams) if retry_streams else [torch.cuda.Stream(device=dev) for _ in range(2)]
        sa.wait_stream(main)
        for st in sbs:
            st.wait_stream(main)
        out, pend, wait = [], [], []         # wait: unsolved queries of finished first launches, pooled into retry launches
        n_wait, n_retry = 0, 0

        def retry():
            nonlocal n_wait, n_retry, wait
            sb = sbs[n_retry % len(sbs)]
            n_retry += 1
            sb.wait_stream(sa)
            with torch.cuda.stream(sb):
                cat = lambda k: torch.cat([w[k] for w in wait]).contiguous()
                r2 = self.plan(cat("start"), cat("goal"), max_iters=max_iters, max_nodes=max_nodes, max_path=max_path, seed=0,
                               env_ids=cat("ids"), seeds=cat("seeds"), stream=sb, max_workgroups=0 if retry_exclusive else -1,
                               exclusive=retry_exclusive, resume=PlanState.cat([w["state"] for w in wait]) if resume else None, **vs)
            # the pooled slices were allocated on `sa` and are read by the cat on `sb`: tell the caching allocator, or the
            # next first launch on `sa` may be handed their blocks while `sb` still waits behind an earlier retry
            for w in wait:
                for k in ("start", "goal", "ids", "seeds", "rows"):
                    w[k].record_stream(sb)
                if resume:
                    for t in (w["state"].tree_q, w["state"].tree_p, w["state"].state):
                        t.record_stream(sb)
            pend.append(([(w["batch"], w["rows"]) for w in wait], r2, sb))
            wait, n_wait = [], 0

        for i, b in enumerate(batches):
            E = b["start"].shape[0]
            ids = b.get("env_ids")
            if ids is None:
                ids = torch.arange(E, device=dev, dtype=torch.int64)
            with torch.cuda.stream(sa):
                res = self.plan(b["start"], b["goal"], max_iters=first_iters, max_nodes=max_nodes, max_path=max_path, seed=b.get("seed", 0),
                                env_ids=ids, seeds=b.get("seeds"), stream=sa, max_workgroups=max_workgroups_first, keep_state=resume, **vs)
                kept = res[4] if resume else None
                res = res[:4]
                again = torch.nonzero(res[2] == _lib.PLAN_NO_EXACT).flatten()       # (waits for this launch: the one read-back)
                if len(again):
                    seeds = (b["seeds"][again] if b.get("seeds") is not None
                             else torch.full((len(again),), int(b.get("seed", 0)), dtype=torch.int64, device=dev))
                    wait.append(dict(start=b["start"][again], goal=b["goal"][again], ids=ids[again], seeds=seeds, batch=i, rows=again,
                                     state=kept.rows(again) if resume else None))
                    n_wait += len(again)
            out.append(list(res))
            if n_wait >= retry_min:
                retry()
        if n_wait:
            retry()
        for parts, r2, sb in pend:
            with torch.cuda.stream(sb):
                o = 0
                for bi, rows in parts:
                    for k in range(4):
                        out[bi][k][rows] = r2[k][o:o + len(rows)]
                    o += len(rows)
            main.wait_stream(sb)
        main.wait_stream(sa)
        for o in out:              # results live in blocks of `sa`'s pool (patched on the retry streams), consumed on `main`
            for t in o:
                t.record_stream(main)
                for sb in sbs:
                    t.record_stream(sb)
        return [tuple(o) for o in out]

    def pullback(self, cur, target, step_size: float, num_trials: int, stream=None):
        """The rollout's invalid-target back-off (rl/mopa_rollouts.py:133-143) for E envs in one launch.
        cur / target: [E, nq] float64 GPU tensors.  Returns (target' [E, nq], n_trials [E] int32, valid [E] uint8)."""
        torch = _torch()
        _check_f64(cur, "cur", self.nq)
        _check_f64(target, "target", self.nq)
        E = cur.shape[0]
        out = target.clone()
        trials = torch.zeros(E, dtype=torch.int32, device=cur.device)
        valid = torch.zeros(E, dtype=torch.uint8, device=cur.device)
        _lib.check(_lib.lib().mopa_pullback_batch(self.scene.handle, _ptr(cur), _ptr(out), E, float(step_size), int(num_trials),
                                                  _ptr(trials), _ptr(valid), _stream_handle(stream)))
        return out, trials, valid


def postprocess_paths(path, path_len, status, cur, n_arm: int, ac_scale: float, interpolate: bool, limits, is_valid, stream=None,
                      seam_mask: int = 0):
    """Planner rows -> executable trajectories on the device (C ABI `mopa_paths_*`): un-wrap by successive differences
    (reference motion_planners/sampling_based_planner.py:71-99; `path` [M, max_path, nq] is overwritten with the un-wrapped
    rows), then -- `interpolate` -- the reference's densification of steps longer than ac_scale (rl/sac_agent.py:205-233)
    with every interior state validated by `is_valid(rows [S, nq]) -> uint8/bool [S]`.

    limits: agent_planning.JointLimits (float32 state limits + margin).  Returns (traj [M, L, nq], length [M] int64 -- 0 for
    queries with status != 0 --, needs_fallback [M] bool: a long step of that query has an invalid interior state, the
    reference plans such a step with its fallback planners and the caller has to).  One small read-back (totals).
    seam_mask: bit c set = qpos coordinate c belongs to an unlimited joint (`non_limited_idx`): its steps across +-3.14 are taken
    the short way round (sampling_based_planner.py:79-97)."""
    torch = _torch()
    L = _lib.lib()
    M, max_path, nq = path.shape
    dev = path.device
    di = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _stream_handle(stream)
    seg = torch.empty(M, max_path, dtype=torch.int32, device=dev)
    n_walk = torch.empty(M, dtype=torch.int32, device=dev)
    out_len = torch.empty(M, dtype=torch.int32, device=dev)
    lim = [t.contiguous() for t in (limits.lo_state, limits.hi_state, limits.lo_shrunk, limits.hi_shrunk)]
    _lib.check(L.mopa_paths_unwrap_seam_batch(di, M, nq, int(n_arm), _ptr(path), max_path, _ptr(path_len), _ptr(status), _ptr(cur),
                                              float(ac_scale), int(bool(interpolate)), *[_ptr(t) for t in lim], _ptr(seg), _ptr(n_walk),
                                              _ptr(out_len), int(seam_mask), st))
    walk_off = torch.cumsum(n_walk.to(torch.int64), 0) - n_walk.to(torch.int64)
    tot_walk, rows = (int(x) for x in torch.stack([n_walk.sum(), out_len.max()]).cpu())
    rows = max(rows, 1)
    walk = walk_valid = None
    if tot_walk > 0:
        walk = torch.empty(tot_walk, nq, dtype=torch.float64, device=dev)
        _lib.check(L.mopa_paths_walk_batch(di, M, nq, int(n_arm), _ptr(path), max_path, _ptr(path_len), _ptr(out_len), float(ac_scale),
                                           *[_ptr(t) for t in lim], _ptr(seg), _ptr(walk_off), _ptr(walk), st))
        walk_valid = is_valid(walk).to(torch.uint8).contiguous()
    out = torch.zeros(M, rows, nq, dtype=torch.float64, device=dev)
    need = torch.zeros(M, dtype=torch.uint8, device=dev)
    _lib.check(L.mopa_paths_assemble_batch(di, M, nq, _ptr(path), max_path, _ptr(path_len), _ptr(out_len), _ptr(seg), _ptr(walk_off),
                                           _ptr(walk) if walk is not None else None, _ptr(walk_valid) if walk_valid is not None else None,
                                           _ptr(out), rows, _ptr(need), st))
    return out, out_len.to(torch.int64), need.bool()
