"""Helpers of the reuse_data relabelling tests (test_reuse_host.py, test_reuse_gpu.py): the library's counter RNG as an rng
object the host `reuse_transitions` can draw from, a synthetic per-waypoint record, and the host loop's draw / skip logic
with every draw's outcome named."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def mix64(z):
    """mopa_device.hpp mix64 (splitmix64 finaliser) in Python integers"""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def rng_key(seed, stream):
    return mix64((seed + GOLDEN_GAMMA * (stream + 1)) & M64)


def rng_uniform_k(key, counter):
    r = mix64((key + GOLDEN_GAMMA * (counter + 1)) & M64)
    return float(r >> 11) * 2.0 ** -53           # (r >> 11 < 2^53: exact)


def reuse_stream(env_total, global_env_id):
    """sample stream of an env's relabelling draws: behind the planners' e, E + e, 2E + e"""
    return 3 * int(env_total) + int(global_env_id)


class CounterDraw:
    """rng object over stream `stream` of seed `seed`: the k-th call of `randint(low, high)` takes the uniform of counter k and
    returns low + min(int(u * (high - low)), high - low - 1).  The host loop calls randint twice per draw (start, goal), so
    draw i uses counters 2i and 2i + 1."""

    def __init__(self, seed, stream):
        self.key = rng_key(int(seed) & M64, int(stream))
        self.calls = 0

    def randint(self, low, high):
        low, high = int(low), int(high)
        u = rng_uniform_k(self.key, self.calls)
        self.calls += 1
        return low + min(int(u * (high - low)), high - low - 1)


def counter_rng(seed, env_total, env_id_base=0):
    """callable env row -> CounterDraw, as `reuse_transitions(..., rng=...)` takes it"""
    return lambda e: CounterDraw(seed, reuse_stream(env_total, env_id_base + int(e)))


def synthetic_record(E, L, D, nq, seed, n_exec_max=12, scales=(0.02, 0.08, 0.35), n_exec_head=(0, 1, 3, 4)):
    """A record as `agent_step(..., record=True)` leaves it, as numpy arrays: random observations, running returns and done
    flags, waypoints that are a random walk per env whose step scale is one of `scales` (small: relabelled actions are no
    planner actions; large: they leave [-1, 1]), n_exec = `n_exec_head`, then n_exec_max, then uniform in 0 .. n_exec_max."""
    rng = np.random.default_rng(seed)
    n_exec = rng.integers(0, n_exec_max + 1, size=E).astype(np.int64)
    head = list(n_exec_head) + [n_exec_max]
    n_exec[:len(head)] = head[:E]
    scale = np.asarray(scales)[rng.integers(0, len(scales), size=E)]
    steps = rng.uniform(-1.0, 1.0, size=(E, L, nq)) * scale[:, None, None]
    return {"ob": rng.normal(size=(E, L, D)), "meta_rew": rng.normal(size=(E, L)),
            "done": (rng.uniform(size=(E, L)) < 0.2).astype(np.uint8),
            "waypoint": rng.uniform(-1.0, 1.0, size=(E, 1, nq)) + np.cumsum(steps, axis=1), "n_exec": n_exec}


def as_out(rec, dof, device="cpu", ac_type=None):
    """the dict `reuse_transitions` / `reuse_transitions_device` take, as torch tensors on `device`"""
    import torch
    out = {"record": {k: torch.tensor(v, device=device) for k, v in rec.items()},
           "ac": torch.zeros(len(rec["n_exec"]), dof, dtype=torch.float64, device=device)}
    if ac_type is not None:
        out["ac_type"] = torch.tensor(ac_type, dtype=torch.int64, device=device)
    return out


def classify_draws(rec, cfg, n_arm, rng, max_reuse_data, grip_qpos_idx=None):
    """the host loop of `reuse_transitions` with each draw's outcome counted: {"duplicate", "not_planner", "out_of_box",
    "kept"} (a draw that is both is counted as not_planner)"""
    from mopa_rl_amd.agent_planning import displacement_to_action
    wp, nexec = rec["waypoint"], rec["n_exec"]
    tally = {"duplicate": 0, "not_planner": 0, "out_of_box": 0, "kept": 0}
    for e in np.where(nexec > 3)[0]:
        draw = rng(int(e)) if callable(rng) else rng
        L = int(nexec[e])
        seen = set()
        for _ in range(min(L, max_reuse_data)):
            start = draw.randint(low=0, high=L - 1)
            goal = draw.randint(low=start + 1, high=L)
            assert 0 <= start < goal < L
            if (start, goal) in seen:
                tally["duplicate"] += 1
                continue
            seen.add((start, goal))
            ac = displacement_to_action(wp[e, goal, :n_arm] - wp[e, start, :n_arm], cfg.ac_scale, cfg.omega, cfg.action_range, cfg.ac_space_type)
            is_planner = bool(np.any(ac < -cfg.omega) or np.any(ac > cfg.omega))
            if grip_qpos_idx is not None:
                ac = np.concatenate([ac, [wp[e, goal, grip_qpos_idx] - wp[e, start, grip_qpos_idx]]])
            if not is_planner:
                tally["not_planner"] += 1
            elif not bool(np.all(ac >= -1.0) and np.all(ac <= 1.0)):
                tally["out_of_box"] += 1
            else:
                tally["kept"] += 1
    return tally
