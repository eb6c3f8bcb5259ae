"""Host reference of the contact-force readout (`BatchKinematicEnv.enable_contact_force`, C ABI `mopa_env_set_contact_force`).

A readout row is 8 doubles per contact of the last constraint solve of a launch: [pair, key, f0, f1, f2, f3, f4, f5], f = what
mj_contactForce returns in the contact frame.  Pyramidal cones with edge forces p (K8, K7 solvers 0 / 1):
    f0 = (p0 + p1) + (p2 + p3),  f1 = mu (p0 - p1),  f2 = mu (p2 - p3),  f3 = f4 = f5 = 0
Elliptic cones (K7 solver 2): the contact's `dim` solver forces, zero-padded.  Per env
    s_c   = ((((|f0| + |f1|) + |f2|) + |f3|) + |f4|) + |f5|
    force = (..((0.0 + s_0) + s_1)..)                                   in contact order
-- plain Python floats, no fused multiply-add, so a kernel that performs the same adds gives the same bits.

`PusherForceRef`: the K8 checker (tests/pusher_dyn_ref.py) with every forward pass asked for its constraint forces; the last pass of
`substeps(n)` -- the 4th RK4 stage of the last sub-step -- is what the constraint forces hold when the reference's
`_do_simulation` returns, hence the K8 reference of the readout.  PARITY UNPINNED against MuJoCo, like the checker itself."""
import numpy as np

from pusher_dyn_ref import PusherRef


def decode_pyramid(p, mu):
    """(f0, f1, f2) of one contact from its four pyramid edge forces, in the kernels' expression order"""
    f0 = (p[0] + p[1]) + (p[2] + p[3])
    f1 = mu * (p[0] - p[1])
    f2 = mu * (p[2] - p[3])
    return f0, f1, f2


def row_sum(f):
    """s_c of one row's six force entries"""
    return ((((abs(f[0]) + abs(f[1])) + abs(f[2])) + abs(f[3])) + abs(f[4])) + abs(f[5])


def force_of_rows(rows):
    """`contact_force` of one env from its rows [n, 8] (n = its contact count), in contact order"""
    force = 0.0
    for r in rows:
        force = force + row_sum([float(x) for x in r[2:8]])
    return force


def pyramid_rows(pairs, keys, edge_forces, mus):
    """rows [n, 8] of pyramidal contacts: pair / key per contact, edge_forces [n][4], mus [n]"""
    out = np.zeros((len(pairs), 8))
    for c in range(len(pairs)):
        f0, f1, f2 = decode_pyramid([float(x) for x in edge_forces[c]], float(mus[c]))
        out[c] = [float(pairs[c]), float(keys[c]), f0, f1, f2, 0.0, 0.0, 0.0]
    return out


class PusherForceRef(PusherRef):
    """PusherRef whose `forward` always computes the constraint forces and stashes (contacts, edge forces) of the pass"""

    def __init__(self, facts):
        super().__init__(facts)
        self.last = ([], [])

    def forward(self, q, v, ctrl, want=False):
        qacc, C, F = super().forward(q, v, ctrl, want=True)
        self.last = (C, F)
        return (qacc, C, F) if want else qacc

    def rows(self):
        """rows [n, 8] of the last forward pass: (pair, signed distance, f0, f1, f2, 0, 0, 0)"""
        C, F = self.last
        if not C:
            return np.zeros((0, 8))
        return pyramid_rows([c["pair"] for c in C], [c["dist"] for c in C], F, [c["mu"] for c in C])

    def readout(self, q, v, it, desired, prev, n):
        """n sub-steps of one env from (q [6], v [6], it [4]) -> (rows [count, 8], force) of the last constraint solve"""
        q, v, it = [float(x) for x in q], [float(x) for x in v], [float(x) for x in it]
        self.last = ([], [])
        self.substeps(q, v, it, [float(x) for x in desired], [float(x) for x in prev], n)
        rows = self.rows()
        return rows, force_of_rows(rows)
