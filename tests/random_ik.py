"""IK chains that are none of the shipped ones (helpers of test_random_ik_host / test_random_ik_gpu): random_scenes trees with a site
"tip" placed as test_env_tables_host.deep_site places it -- offset (0.03, -0.02, 0.05), rotated 0.4 rad about y, so every chain has
a site rotation -- and the list of movable joints handed to IK.  Built in memory."""
import copy
import functools
import types

import numpy as np

import random_scenes as RS
from random_scenes import JNT_FREE, JNT_HINGE, JNT_SLIDE, node

H, S, W = (JNT_HINGE,), (JNT_SLIDE,), ()
SITE_OFF = (0.03, -0.02, 0.05)
SITE_QUAT = (np.cos(0.2), 0.0, np.sin(0.2), 0.0)
E_GPU, E_HOST = 130, 40


def with_site(m, body):
    m2 = copy.copy(m)
    m2.site_names = ["tip"]
    m2.site_body = np.array([body], dtype=np.int32)
    m2.site_pos = np.array([SITE_OFF], dtype=np.float64)
    m2.site_quat = np.array([SITE_QUAT], dtype=np.float64)
    return m2


def _chain_case(name, seed, nodes, site_node, movable_nodes):
    """tree of `nodes` (no free body), the site on node `site_node`, the joints of `movable_nodes` movable, in that order"""
    m, pi = RS.build(name, seed, nodes, n_static=2, n_free=0)
    first = len(m.body_parent) - len(nodes)
    joints = [m.jnt_names[int(m.body_jntadr[first + k])] for k in movable_nodes]
    return types.SimpleNamespace(name=name, model=with_site(m, first + site_node), pi=pi, joints=joints)


def _line(kinds):
    return [node(k - 1, j) for k, j in enumerate(kinds)]


def eight():
    """8 one-joint bodies, slides at 2 and 5, all movable: row and column 7 of the 8 x 8 system are live"""
    kinds = [S if k in (2, 5) else H for k in range(8)]
    return _chain_case("eight", 301, _line(kinds), 7, range(8))


def nine_of_which_eight():
    """9 jointed and 2 jointless bodies in one chain (a jointless one in front: n_pre = 1, one inside); 8 joints movable, the hinge of
    node 4 fixed: the walk reads it from the qpos row"""
    kinds = [W, H, S, H, H, W, H, S, H, H, H]
    return _chain_case("nine_of_which_eight", 302, _line(kinds), 10, [1, 2, 3, 6, 7, 8, 9, 10])


def prefix():
    """two jointless bodies, then 4 joints: a jointless prefix off the Sawyer"""
    return _chain_case("prefix", 303, _line([W, W, H, H, S, H]), 5, [2, 3, 4, 5])


def one():
    """a single slide"""
    return _chain_case("one", 304, _line([S]), 0, [0])


def off_chain():
    """4 joints on the site's chain and 2 movable joints of another branch: their columns stay zero and keep the regulariser on the diagonal"""
    nodes = _line([H, H, S, H]) + [node(0, H), node(4, S)]
    return _chain_case("off_chain", 305, nodes, 3, [0, 4, 1, 2, 5, 3])


def none_on_chain():
    """the site on a body welded to a free body, 2 movable joints elsewhere: every column is zero, and the walk takes its free-joint branch"""
    rng = np.random.default_rng(306)
    M = RS._Model(rng, 0.25, 0.75)
    RS._statics(M, rng, 2)
    RS._tree(M, _line([H, S]))
    fb = M.body(0, (JNT_FREE,))
    M.geom(fb)
    wb = M.body(fb, ())
    M.geom(wb)
    m, pi = RS._finish(M, "none_on_chain", rng)
    joints = [m.jnt_names[j] for j in range(len(m.jnt_type)) if m.jnt_type[j] != JNT_FREE]
    assert len(joints) == 2
    return types.SimpleNamespace(name="none_on_chain", model=with_site(m, wb), pi=pi, joints=joints)


CHAINS = {f.__name__: f for f in (eight, nine_of_which_eight, prefix, one, off_chain, none_on_chain)}


@functools.lru_cache(maxsize=None)
def chain(name):
    return CHAINS[name]()


def joint_ids(c):
    return np.array([c.model.joint_name2id(j) for j in c.joints], dtype=np.int32)


def site_chain(c):
    """the bodies from the world to the site's body"""
    m, out = c.model, []
    b = int(m.site_body[0])
    while b > 0:
        out.append(b)
        b = int(m.body_parent[b])
    return out[::-1]


def rows(c, E, seed):
    """[E, nq] states: hinges and slides anywhere in their range (unlimited hinges in +-3.14), free bodies moved and turned"""
    m = c.model
    rng = np.random.default_rng([seed, 11])
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (E, 1))
    for j, t in enumerate(m.jnt_type):
        a = int(m.jnt_qposadr[j])
        if t == JNT_FREE:
            q[:, a:a + 3] += rng.uniform(-0.2, 0.2, (E, 3))
            quat = rng.normal(size=(E, 4))
            q[:, a + 3:a + 7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        else:
            lo, hi = (m.jnt_range[j] if m.jnt_limited[j] else (-3.14, 3.14))
            q[:, a] = rng.uniform(lo, hi, E)
    return q


def perturbed(c, q, seed):
    """the rows with the movable joints moved (hinges by N(0, 0.3), slides by N(0, 0.06)): their site poses are reachable targets"""
    m = c.model
    rng = np.random.default_rng([seed, 12])
    qt = q.copy()
    for j in joint_ids(c):
        qt[:, int(m.jnt_qposadr[j])] += rng.normal(0, 0.3 if m.jnt_type[j] == JNT_HINGE else 0.06, len(q))
    return qt


def far_targets(tgt, seed):
    """one target in three pushed 1.5 m away"""
    rng = np.random.default_rng([seed, 13])
    out = tgt.copy()
    out[::3] += rng.normal(0, 1.5, (len(out[::3]), 3))
    return out


def target_quats(quat, seed):
    """the perturbed poses' site quaternions, one in five replaced by an arbitrary one"""
    rng = np.random.default_rng([seed, 14])
    out = quat.copy()
    k = np.arange(2, len(out), 5)
    r = rng.normal(size=(len(k), 4))
    out[k] = r / np.linalg.norm(r, axis=1, keepdims=True)
    return out


def site_pose_ref(c, q):
    """(pos [3], mat [3, 3]) of the site by tests/dyn_ref.fk (scipy composition of the tree)"""
    import dyn_ref
    m = c.model
    P, R = dyn_ref.fk(m, q)
    b = int(m.site_body[0])
    return P[b] + R[b] @ m.site_pos[0], R[b] @ dyn_ref._rot(m.site_quat[0])
