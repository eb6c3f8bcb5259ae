"""`BatchPlanner` look-alike over the CPU oracle (test infrastructure shared by test_ref_py_agent.py and test_plan_jobs_host.py):
validity and RRT-Connect of the oracle behind the tensor signatures the batched host code calls."""
import types

import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class OracleBP:
    def __init__(self, orc, range_=None):
        self.orc, self.na, self.nq, self.range = orc, orc.na, orc.nq, range_
        self.scene = types.SimpleNamespace(active_idx=orc.active_idx)

    def is_valid(self, q_active, qpos_env, samples_per_env=None, **kw):
        import torch
        v, _ = self.orc.is_valid_batch(q_active.numpy(), qpos_env.numpy(), samples_per_env=samples_per_env, want_min_dist=False)
        return torch.from_numpy(v)

    def plan(self, start, goal, max_iters=2000, max_nodes=1024, max_path=256, seed=0, env_ids=None, seeds=None, **kw):
        """one `OracleScene.plan` per query, keyed like a launch of the library: (seeds[k], stream env_ids[k])"""
        import torch
        s, g = start.numpy(), goal.numpy()
        E = len(s)
        path, nchk = np.zeros((E, max_path, self.nq)), np.zeros(E, dtype=np.int64)
        plen, status = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        for k in range(E):
            status[k], p, nchk[k], _ = self.orc.plan(s[k], g[k], self.range, max_iters=max_iters, max_nodes=max_nodes, seed=int(seeds[k]),
                                                     env_id=int(env_ids[k]), max_path=max_path)
            path[k, :len(p)], plen[k] = p, len(p)
        return tuple(torch.from_numpy(x) for x in (path, plen, status, nchk))
