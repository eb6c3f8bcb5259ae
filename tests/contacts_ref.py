"""Expected contact reports, derived from the CPU oracle's per-pair distances (helpers of test_contacts_host / test_contacts_gpu)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 1.0e10


def load_census_tool():
    spec = importlib.util.spec_from_file_location("threshold_band_census", os.path.join(ROOT, "tools", "threshold_band_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ignored_mask(pi):
    """as tests/test_gpu_parity.py::test_pair_dist_bit_exact masks them: the HIP scene drops ignored pairs altogether"""
    m = pi.model
    ignored = set(pi.ignored_contacts)
    return np.array([(min(m.geom_mjid[a], m.geom_mjid[b]), max(m.geom_mjid[a], m.geom_mjid[b])) in ignored for a, b in m.pair_geom])


def full_state(pi, qa, row):
    q = np.array(row, dtype=np.float64, copy=True)
    q[pi.ref_joint_pos_indexes] = qa
    return q


def oracle_pair_dists(pi, orc, qa, rows, samples_per_env):
    """[N, npair] per-pair distances of the oracle, ignored pairs at FAR"""
    ign = ignored_mask(pi)
    out = np.empty((len(qa), len(pi.model.pair_geom)))
    for i in range(len(qa)):
        d = orc.pair_dist(full_state(pi, qa[i], rows[i // samples_per_env]))
        d[ign] = FAR
        out[i] = d
    return out


def report_from_dists(D, cutoff, K):
    """the contract of mopa_contacts_batch on a table of per-pair distances: count [N] int32, pair [N, K] int32, dist [N, K]"""
    N = len(D)
    count = np.zeros(N, dtype=np.int32)
    pair = np.full((N, K), -1, dtype=np.int32)
    dist = np.full((N, K), FAR)
    for i in range(N):
        hit = np.nonzero(D[i] <= cutoff)[0]
        count[i] = len(hit)
        k = min(K, len(hit))
        pair[i, :k] = hit[:k]
        dist[i, :k] = D[i, hit[:k]]
    return count, pair, dist
