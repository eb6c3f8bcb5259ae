"""Sequential checker of K8 (csrc/mopa_pusher_dyn.inc): the PusherObstacle-v0 dynamics written in the kernel's operation order,
one env at a time in plain Python floats (IEEE double, no fused multiply-add; sin / cos through the oracle library's orc_sincos),
so that its qpos / qvel / i_term agree with the GPU bit for bit.  Also: the K8 post-step (reward / obs) of one env through the
CPU oracle, and the contact list of one forward pass for the hand-built geometry tests."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O

NV, NARM, LS_EVALS = 6, 4, 50
MINVAL = 1e-15


def clampd(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def dmin(a, b):
    return a if a < b else b


def dmax(a, b):
    return a if a > b else b


def xform(p, lx, ly):
    x, y, c, s = p
    return x + (c * lx - s * ly), y + (s * lx + c * ly)


def impedance(par, dist):
    x = abs(dist - par[1]) / par[6]
    if x >= 1.0:
        y = 1.0
    elif x <= 0.5:
        y = 2.0 * (x * x)
    else:
        y = 1.0 - 2.0 * ((1.0 - x) * (1.0 - x))
    return par[4] + y * (par[5] - par[4])


def T(i, k):
    return i * (i + 1) // 2 + k


def ldl(A):
    for i in range(NV):
        for k in range(i + 1):
            acc = A[T(i, k)]
            for j in range(k):
                acc = acc - A[T(i, j)] * (A[T(k, j)] * A[T(j, j)])
            if k < i:
                A[T(i, k)] = acc / A[T(k, k)]
            else:
                A[T(i, i)] = acc


def ldl_solve(A, x):
    for i in range(NV):
        acc = x[i]
        for j in range(i):
            acc = acc - A[T(i, j)] * x[j]
        x[i] = acc
    for i in range(NV):
        x[i] = x[i] / A[T(i, i)]
    for i in range(NV - 1, -1, -1):
        acc = x[i]
        for j in range(i + 1, NV):
            acc = acc - A[T(j, i)] * x[j]
        x[i] = acc


class PusherRef:
    """f: dynamics.PusherDynFacts"""

    def __init__(self, f):
        self.f = f
        self.pairs = [[float(x) for x in r] for r in np.asarray(f.pairs)]
        g = lambda a: [float(x) for x in np.asarray(a).ravel()]
        self.rel, self.com = [g(r) for r in f.rel], [g(c) for c in f.com]
        self.mass, self.izz, self.arm, self.damp = g(f.mass), g(f.izz), g(f.armature), g(f.damping)
        self.lo, self.hi, self.limited = g(f.lo), g(f.hi), [int(x) for x in f.limited]
        self.gear, self.kv, self.clo, self.chi = g(f.gear), g(f.kv), g(f.ctrl_lo), g(f.ctrl_hi)
        self.lim_par = g(f.lim_par)
        self.dropped = 0

    # ---- kinematics
    def kinematics(self, q):
        f = self.f
        px, py, pc, ps, th = float(f.base[0]), float(f.base[1]), 1.0, 0.0, 0.0
        P = []
        for k in range(NARM):
            ox, oy = px, py
            if k > 0:
                ox, oy = xform((px, py, pc, ps), self.rel[k][0], self.rel[k][1])
            th = th + q[k]
            s, c = O.sincos(th)
            P.append((ox, oy, c, s))
            px, py, pc, ps = ox, oy, c, s
        P.append((float(f.box_org[0]) + (q[4] - float(f.box_ref[0])), float(f.box_org[1]) + (q[5] - float(f.box_ref[1])), 1.0, 0.0))
        return P

    @staticmethod
    def point_jac(P, b, x, y, nx, ny, sg, J):
        if b < 0:
            return
        if b == 4:
            J[4] = J[4] + sg * nx
            J[5] = J[5] + sg * ny
            return
        for j in range(NARM):
            if j <= b:
                rx, ry = x - P[j][0], y - P[j][1]
                J[j] = J[j] + sg * (rx * ny - ry * nx)

    def emit(self, C, P, ba, bb, pair, px, py, nx, ny, dist):
        if len(C) >= self.f.maxcon:
            self.dropped += 1
            return
        Jn, Jt = [0.0] * NV, [0.0] * NV
        tx, ty = -ny, nx
        self.point_jac(P, ba, px, py, nx, ny, 1.0, Jn)
        self.point_jac(P, bb, px, py, nx, ny, -1.0, Jn)
        self.point_jac(P, ba, px, py, tx, ty, 1.0, Jt)
        self.point_jac(P, bb, px, py, tx, ty, -1.0, Jt)
        C.append(dict(Jn=Jn, Jt=Jt, dist=dist, pair=pair, pos=(px, py), n=(nx, ny)))

    @staticmethod
    def seg_t(ax, ay, bx, by, x, y):
        dx, dy = bx - ax, by - ay
        L2 = dx * dx + dy * dy
        t = ((x - ax) * dx + (y - ay) * dy) / L2 if L2 > 0.0 else 0.0
        return 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)

    def collide(self, P):
        C = []
        for p, r in enumerate(self.pairs):
            cls, ba, bb = int(r[0]), int(r[1]), int(r[2])
            ga, gb = r[3:8], r[8:13]
            margin = r[14]
            pa = P[ba] if ba >= 0 else (0.0, 0.0, 1.0, 0.0)
            pb = P[bb] if bb >= 0 else (0.0, 0.0, 1.0, 0.0)
            if cls == 2:
                ax, ay = xform(pa, ga[0], ga[1])
                bx, by = xform(pb, gb[0], gb[1])
                ux, uy = ax - bx, ay - by
                ox, oy = (ga[2] + gb[2]) - abs(ux), (ga[3] + gb[3]) - abs(uy)
                dist = -(ox if ox < oy else oy)
                if not (ox > 0.0 and oy > 0.0) or not (dist < margin):
                    continue
                nx = ny = 0.0
                if ox <= oy:
                    nx = 1.0 if ux >= 0.0 else -1.0
                else:
                    ny = 1.0 if uy >= 0.0 else -1.0
                x0, x1 = dmax(ax - ga[2], bx - gb[2]), dmin(ax + ga[2], bx + gb[2])
                y0, y1 = dmax(ay - ga[3], by - gb[3]), dmin(ay + ga[3], by + gb[3])
                for (x, y) in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
                    self.emit(C, P, ba, bb, p, x, y, nx, ny, dist)
                continue
            a0x, a0y = xform(pa, ga[0], ga[1])
            a1x, a1y = xform(pa, ga[2], ga[3])
            ra = ga[4]
            cax, cay = 0.5 * (a0x + a1x), 0.5 * (a0y + a1y)
            dax, day = a1x - a0x, a1y - a0y
            rba = 0.5 * math.sqrt(dax * dax + day * day) + ra
            if cls == 1:
                b0x, b0y = xform(pb, gb[0], gb[1])
                b1x, b1y = xform(pb, gb[2], gb[3])
                rb = gb[4]
                cbx, cby = 0.5 * (b0x + b1x), 0.5 * (b0y + b1y)
                dbx, dby = b1x - b0x, b1y - b0y
                rbb = 0.5 * math.sqrt(dbx * dbx + dby * dby) + rb
                ccx, ccy, rr = cax - cbx, cay - cby, (rba + rbb) + margin
                if ccx * ccx + ccy * ccy > rr * rr:
                    continue
                have, best = False, 0.0
                X = Y = (0.0, 0.0)
                for k in range(4):
                    if k < 2:
                        xx, xy = (a0x, a0y) if k == 0 else (a1x, a1y)
                        t = self.seg_t(b0x, b0y, b1x, b1y, xx, xy)
                        yx, yy = b0x + t * dbx, b0y + t * dby
                    else:
                        yx, yy = (b0x, b0y) if k == 2 else (b1x, b1y)
                        t = self.seg_t(a0x, a0y, a1x, a1y, yx, yy)
                        xx, xy = a0x + t * dax, a0y + t * day
                    wx, wy = xx - yx, xy - yy
                    d2 = wx * wx + wy * wy
                    if not have or d2 < best:
                        have, best, X, Y = True, d2, (xx, xy), (yx, yy)
                d = math.sqrt(best)
                dist = (d - ra) - rb
                if not (dist < margin) or not (d > 0.0):
                    continue
                nx, ny = (X[0] - Y[0]) / d, (X[1] - Y[1]) / d
                off = ra + 0.5 * dist
                self.emit(C, P, ba, bb, p, X[0] - nx * off, X[1] - ny * off, nx, ny, dist)
                continue
            bx, by = xform(pb, gb[0], gb[1])
            hx, hy = gb[2], gb[3]
            ccx, ccy, rr = cax - bx, cay - by, (rba + math.sqrt(hx * hx + hy * hy)) + margin
            if ccx * ccx + ccy * ccy > rr * rr:
                continue
            cd, cp, cn = [0.0] * 6, [(0.0, 0.0)] * 6, [(0.0, 0.0)] * 6
            for k in range(2):
                ex, ey = (a0x, a0y) if k == 0 else (a1x, a1y)
                ux, uy = ex - bx, ey - by
                qx, qy = dmin(dmax(ux, -hx), hx), dmin(dmax(uy, -hy), hy)
                wx, wy = ux - qx, uy - qy
                d = math.sqrt(wx * wx + wy * wy)
                if d > 0.0:
                    nx, ny, dd = wx / d, wy / d, d
                else:
                    fx, fy = hx - abs(ux), hy - abs(uy)
                    if fx <= fy:
                        nx, ny, dd = (1.0 if ux >= 0.0 else -1.0), 0.0, -fx
                    else:
                        nx, ny, dd = 0.0, (1.0 if uy >= 0.0 else -1.0), -fy
                dist = dd - ra
                off = ra + 0.5 * dist
                cd[k], cp[k], cn[k] = dist, (ex - nx * off, ey - ny * off), (nx, ny)
            for k in range(4):
                kx, ky = bx + (hx if k & 1 else -hx), by + (hy if k & 2 else -hy)
                dx, dy = a1x - a0x, a1y - a0y
                L2 = dx * dx + dy * dy
                t = ((kx - a0x) * dx + (ky - a0y) * dy) / L2 if L2 > 0.0 else 0.0
                cd[2 + k] = 1.0
                if 0.0 < t < 1.0:
                    sx, sy = a0x + t * dx, a0y + t * dy
                    wx, wy = sx - kx, sy - ky
                    d = math.sqrt(wx * wx + wy * wy)
                    if d > 0.0:
                        nx, ny = wx / d, wy / d
                        dist = d - ra
                        off = ra + 0.5 * dist
                        cd[2 + k], cp[2 + k], cn[2 + k] = dist, (sx - nx * off, sy - ny * off), (nx, ny)
            i0 = i1 = -1
            for k in range(6):
                if cd[k] < margin:
                    if i0 < 0 or cd[k] < cd[i0]:
                        i1, i0 = i0, k
                    elif i1 < 0 or cd[k] < cd[i1]:
                        i1 = k
            for k in (i0, i1):
                if k >= 0:
                    self.emit(C, P, ba, bb, p, cp[k][0], cp[k][1], cn[k][0], cn[k][1], cd[k])
        return C

    # ---- one forward pass -> qacc (and, for tests, the contacts and their row forces)
    def forward(self, q, v, ctrl, want=False):
        P = self.kinematics(q)
        cx, cy = [0.0] * NARM, [0.0] * NARM
        for b in range(NARM):
            cx[b], cy[b] = xform(P[b], self.com[b][0], self.com[b][1])
        M = [0.0] * 21
        for j in range(NARM):
            for k in range(j + 1):
                acc = 0.0
                for b in range(NARM):
                    if b >= j:
                        rjx, rjy, rkx, rky = cx[b] - P[j][0], cy[b] - P[j][1], cx[b] - P[k][0], cy[b] - P[k][1]
                        acc = acc + (self.mass[b] * (rjx * rkx + rjy * rky) + self.izz[b])
                M[T(j, k)] = acc + self.arm[j] if j == k else acc
        bm = float(self.f.box_mass)
        M[14] = bm + self.arm[4]
        M[20] = bm + self.arm[5]
        W, aax, aay = [0.0] * NARM, [0.0] * NARM, [0.0] * NARM
        w = ax_ = ay_ = 0.0
        for k in range(NARM):
            if k > 0:
                w2 = W[k - 1] * W[k - 1]
                ax_ = ax_ - w2 * (P[k][0] - P[k - 1][0])
                ay_ = ay_ - w2 * (P[k][1] - P[k - 1][1])
            w = w + v[k]
            W[k], aax[k], aay[k] = w, ax_, ay_
        fr = [0.0] * NV
        for j in range(NARM):
            bias = 0.0
            for b in range(NARM):
                if b >= j:
                    w2 = W[b] * W[b]
                    acx, acy = aax[b] - w2 * (cx[b] - P[b][0]), aay[b] - w2 * (cy[b] - P[b][1])
                    rx, ry = cx[b] - P[j][0], cy[b] - P[j][1]
                    bias = bias + self.mass[b] * (rx * acy - ry * acx)
            cc = clampd(ctrl[j], self.clo[j], self.chi[j])
            act = self.gear[j] * (self.kv[j] * cc - self.kv[j] * self.gear[j] * v[j])
            fr[j] = (-(self.damp[j] * v[j]) - bias) + act
        fr[4] = -(self.damp[4] * v[4])
        fr[5] = -(self.damp[5] * v[5])
        L = list(M)
        ldl(L)
        a0 = list(fr)
        ldl_solve(L, a0)
        C = self.collide(P) if len(self.pairs) else []
        lside, laref, lD = [0.0] * NV, [0.0] * NV, [0.0] * NV
        any_ = len(C) > 0
        lp = self.lim_par
        for l in range(NV):
            if not self.limited[l]:
                continue
            dlo, dhi = q[l] - self.lo[l], self.hi[l] - q[l]
            dist = 0.0
            if dlo < 0.0:
                lside[l], dist = 1.0, dlo
            elif dhi < 0.0:
                lside[l], dist = -1.0, dhi
            if lside[l] != 0.0:
                any_ = True
                e = [0.0] * NV
                e[l] = 1.0
                ldl_solve(L, e)
                imp = impedance(lp, dist)
                Ri = ((1.0 - imp) / imp) * e[l]
                if Ri < MINVAL:
                    Ri = MINVAL
                laref[l] = -(lp[3] * (lside[l] * v[l])) - (lp[2] * imp) * (dist - lp[1])
                lD[l] = 1.0 / Ri
        qacc = list(a0)
        if not any_:
            return (qacc, C, []) if want else qacc
        for c in C:
            par = self.pairs[c["pair"]][13:20]
            bn, bt = list(c["Jn"]), list(c["Jt"])
            ldl_solve(L, bn)
            ldl_solve(L, bt)
            G0 = G1 = G3 = jvn = jvt = 0.0
            for i in range(NV):
                G0 = G0 + c["Jn"][i] * bn[i]
                G1 = G1 + c["Jn"][i] * bt[i]
                G3 = G3 + c["Jt"][i] * bt[i]
                jvn = jvn + c["Jn"][i] * v[i]
                jvt = jvt + c["Jt"][i] * v[i]
            mu = par[0]
            imp = impedance(par, c["dist"])
            kpos = (par[2] * imp) * (c["dist"] - par[1])
            c["mu"], c["D"], c["aref"] = mu, [0.0] * 4, [0.0] * 4
            for i in range(4):
                sm = mu if i == 0 else (-mu if i == 1 else 0.0)
                Aii = (G0 + (2.0 * sm) * G1) + (sm * sm) * G3
                Ri = ((1.0 - imp) / imp) * Aii
                if Ri < MINVAL:
                    Ri = MINVAL
                jv = jvn + sm * jvt
                c["D"][i] = 1.0 / Ri
                c["aref"][i] = -(par[3] * jv) - kpos

        def Mrow(i, k):
            return M[T(i, k)] if i >= k else M[T(k, i)]

        for _ in range(self.f.iterations):
            dq = [qacc[i] - a0[i] for i in range(NV)]
            Mg = [0.0] * NV
            for i in range(NV):
                acc = 0.0
                for k in range(NV):
                    acc = acc + Mrow(i, k) * dq[k]
                Mg[i] = acc
            gauss = 0.0
            for i in range(NV):
                gauss = gauss + dq[i] * Mg[i]
            gauss = 0.5 * gauss
            p0 = gauss
            g = list(Mg)
            H = list(M)
            for c in C:
                un = ut = 0.0
                for i in range(NV):
                    un = un + c["Jn"][i] * qacc[i]
                    ut = ut + c["Jt"][i] * qacc[i]
                for r in range(4):
                    sm = c["mu"] if r == 0 else (-c["mu"] if r == 1 else 0.0)
                    x = (un + sm * ut) - c["aref"][r]
                    if not (x < 0.0):
                        continue
                    D = c["D"][r]
                    p0 = p0 + (0.5 * D * x) * x
                    J = [c["Jn"][i] + sm * c["Jt"][i] for i in range(NV)]
                    for i in range(NV):
                        g[i] = g[i] + (D * x) * J[i]
                        for k in range(i + 1):
                            H[T(i, k)] = H[T(i, k)] + (D * J[i]) * J[k]
            for l in range(NV):
                if lD[l] > 0.0:
                    x = lside[l] * qacc[l] - laref[l]
                    if x < 0.0:
                        p0 = p0 + (0.5 * lD[l] * x) * x
                        g[l] = g[l] + (lD[l] * x) * lside[l]
                        H[T(l, l)] = H[T(l, l)] + lD[l]
            ldl(H)
            d = [-gi for gi in g]
            ldl_solve(H, d)
            Md = [0.0] * NV
            for i in range(NV):
                acc = 0.0
                for k in range(NV):
                    acc = acc + Mrow(i, k) * d[k]
                Md[i] = acc
            qa = qb = slope0 = 0.0
            for i in range(NV):
                qa = qa + d[i] * Md[i]
                qb = qb + d[i] * Mg[i]
                slope0 = slope0 + d[i] * g[i]
            alpha, lo, hi, pa = 1.0, 0.0, -1.0, p0
            exact = False
            for e in range(LS_EVALS):
                d1, d2 = alpha * qa + qb, qa
                pa = gauss + alpha * (qb + (0.5 * alpha) * qa)
                chg = False
                for c in C:
                    un = ut = dn = dt = 0.0
                    for i in range(NV):
                        un = un + c["Jn"][i] * qacc[i]
                        ut = ut + c["Jt"][i] * qacc[i]
                        dn = dn + c["Jn"][i] * d[i]
                        dt = dt + c["Jt"][i] * d[i]
                    for r in range(4):
                        sm = c["mu"] if r == 0 else (-c["mu"] if r == 1 else 0.0)
                        x, jd = (un + sm * ut) - c["aref"][r], dn + sm * dt
                        xr = x + alpha * jd
                        if (x < 0.0) != (xr < 0.0):
                            chg = True
                        if xr < 0.0:
                            D = c["D"][r]
                            d1 = d1 + (D * xr) * jd
                            d2 = d2 + (D * jd) * jd
                            pa = pa + (0.5 * D * xr) * xr
                for l in range(NV):
                    if lD[l] > 0.0:
                        x, jd = lside[l] * qacc[l] - laref[l], lside[l] * d[l]
                        xr = x + alpha * jd
                        if (x < 0.0) != (xr < 0.0):
                            chg = True
                        if xr < 0.0:
                            d1 = d1 + (lD[l] * xr) * jd
                            d2 = d2 + (lD[l] * jd) * jd
                            pa = pa + (0.5 * lD[l] * xr) * xr
                if abs(d1) <= 1e-9 * abs(slope0) or e == LS_EVALS - 1:
                    exact = e == 0 and not chg and abs(d1) <= 1e-9 * abs(slope0)
                    break
                if d1 < 0.0:
                    lo = alpha
                else:
                    hi = alpha
                an = alpha - d1 / d2
                if an <= lo or (hi >= 0.0 and an >= hi):
                    an = 0.5 * (lo + hi) if hi >= 0.0 else 2.0 * alpha
                alpha = an
            for i in range(NV):
                qacc[i] = qacc[i] + alpha * d[i]
            if (p0 - pa) * self.f.inv_scale < self.f.tolerance or exact:
                break
        if not want:
            return qacc
        forces = []
        for c in C:
            un = ut = 0.0
            for i in range(NV):
                un = un + c["Jn"][i] * qacc[i]
                ut = ut + c["Jt"][i] * qacc[i]
            fr4 = []
            for r in range(4):
                sm = c["mu"] if r == 0 else (-c["mu"] if r == 1 else 0.0)
                x = (un + sm * ut) - c["aref"][r]
                fr4.append(-(c["D"][r] * x) if x < 0.0 else 0.0)
            forces.append(fr4)
        return qacc, C, forces

    # ---- the env's PID (`_get_control`, env/base.py:200-209): ctrl, i_term updated in place
    def pid(self, q, v, it, desired, prev, tv0):
        f = self.f
        ctrl = [0.0] * NARM
        for j in range(NARM):
            pt = f.kp * (desired[j] - q[j])
            dt = f.kd * (tv0[j] - v[j])
            it[j] = f.alpha * it[j] + f.ki * (prev[j] - q[j])
            ctrl[j] = (pt + dt) + it[j]
        return ctrl

    # ---- one sub-step: PID, then RK4
    def substep(self, q, v, it, desired, prev, tv0):
        f = self.f
        ctrl = self.pid(q, v, it, desired, prev, tv0)
        A = ((0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 1.0))
        B = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)
        h = f.timestep
        Fv, Fa = [list(v)], [self.forward(q, v, ctrl)]
        for s in range(1, 4):
            qi, vi = [0.0] * NV, [0.0] * NV
            for i in range(NV):
                dv, da = Fv[0][i] * A[s - 1][0], Fa[0][i] * A[s - 1][0]
                for j in range(1, s):
                    dv = dv + Fv[j][i] * A[s - 1][j]
                    da = da + Fa[j][i] * A[s - 1][j]
                qi[i] = q[i] + h * dv
                vi[i] = v[i] + h * da
            Fv.append(vi)
            Fa.append(self.forward(qi, vi, ctrl))
        for i in range(NV):
            dv, da = Fv[0][i] * B[0], Fa[0][i] * B[0]
            for j in range(1, 4):
                dv = dv + Fv[j][i] * B[j]
                da = da + Fa[j][i] * B[j]
            q[i] = q[i] + h * dv
            v[i] = v[i] + h * da
        return ctrl

    def substeps(self, q, v, it, desired, prev, n):
        """n raw sub-steps of one env (lists, updated in place)"""
        f = self.f
        tv0 = [((desired[j] - prev[j]) / f.frame_dt) * 0.0 for j in range(NARM)]
        for _ in range(n):
            self.substep(q, v, it, desired, prev, tv0)

    def run_rows(self, qpos_row, qvel_row, iterm_row, desired, prev, n):
        """raw sub-steps on one env's rows (numpy in, numpy out)"""
        qadr = [int(a) for a in self.f.qadr]
        q = [float(qpos_row[a]) for a in qadr]
        v, it = [float(x) for x in qvel_row], [float(x) for x in iterm_row]
        self.substeps(q, v, it, [float(x) for x in desired], [float(x) for x in prev], n)
        row = np.array(qpos_row, dtype=np.float64).copy()
        for k, a in enumerate(qadr):
            row[a] = q[k]
        return row, np.array(v), np.array(it)


class PusherEnvRef:
    """E envs of the K8 env.step: the physics above, then K4 kind 3's reward / obs / bookkeeping through the CPU oracle (its
    step with the move flag clear leaves qpos alone and does exactly that half), with the carried velocities in the obs."""

    def __init__(self, env):
        self.ref = PusherRef(env.pdyn)
        self.scene = O.OracleScene(env.model, [], [], 0.0)
        self.oenv = O.OracleEnv(self.scene, env.facts, env.E, ac_scale=env.ac_scale, distance_threshold=env.distance_threshold,
                                 max_episode_steps=env.max_episode_steps)
        self.E = env.E

    def load(self, env):
        """copy the GPU env's state (qpos, qvel, i_term, prev_state, has_prev, ep_len)"""
        self.qpos = env.qpos.cpu().numpy().copy()
        self.qvel = env.qvel.cpu().numpy().copy()
        self.i_term = env.i_term.cpu().numpy().copy()
        self.prev = env.prev_state.cpu().numpy().copy()
        self.has_prev = env.has_prev.cpu().numpy().copy()
        self.ep_len = env.ep_len.cpu().numpy().copy()

    def step(self, action, is_planner, move_mask=None):
        E, qadr = self.E, [int(a) for a in self.ref.f.qadr]
        for e in range(E):
            flags = 1 if move_mask is None else int(move_mask[e])
            if flags & 2:
                continue
            use_prev = bool(is_planner) and bool(self.has_prev[e])
            pv = [float(self.prev[e, j]) if use_prev else float(self.qpos[e, qadr[j]]) for j in range(NARM)]
            des = [pv[j] + float(action[e, j]) for j in range(NARM)]
            self.has_prev[e] = 1
            self.prev[e] = des
            if flags & 1:
                row, v, it = self.ref.run_rows(self.qpos[e], self.qvel[e], self.i_term[e], des, pv, self.ref.f.nsub)
                self.qpos[e], self.qvel[e], self.i_term[e] = row, v, it
        # reward / obs / done through the oracle's kind 3 step with the move flag clear: qpos unchanged, bookkeeping as K4
        o = self.oenv
        o.qpos[:] = self.qpos
        o.prev_state[:] = self.prev
        o.has_prev[:] = 1
        o.ep_len[:] = self.ep_len
        zero = np.zeros((E, NARM))
        for e in range(E):
            if move_mask is not None and int(move_mask[e]) & 2:
                continue
            o._call(e, zero, 1, 0)
        self.qpos[:] = o.qpos
        self.ep_len[:] = o.ep_len
        obs = o.obs.copy()
        obs[:, 2 * NARM + 2:2 * NARM + 8] = self.qvel
        return obs, o.reward.copy(), o.done.copy(), o.success.copy()
