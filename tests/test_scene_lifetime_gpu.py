"""A scene that lives long: one Scene per env (Push: baked walk, LDS centres, pair drain; Lift: slab centres, mesh gate) takes a
script of calls of every entry point that shares its per-stream launch scratch -- the validity launches' self-resetting tile counter,
the reports' chunk counter, the motion buffers, the pose slab that grows from one region per wave to two -- in the order written, in
reverse, in one fixed interleaving, and in that interleaving on a second stream while the first run is in flight.  Every call has
fixed inputs and expected bytes computed once from the CPU references (the oracle, contacts_ref, proximity_ref, motion_report_ref),
which know nothing of call order: a call's output must not depend on the calls before it.  Last, a closed scene (its retired buffers
are freed there) is followed by a fresh one."""
import contextlib

import numpy as np
import pytest

import motion_report_ref as R
import proximity_ref as P
from contacts_ref import oracle_pair_dists, report_from_dists
from test_k1_counted_gpu import FILL_MD, FILL_VALID, LIFT, PUSH, SPE, Batch, _filled

pytestmark = pytest.mark.gpu

MOTION_FIELDS = ("valid", "n_states", "first_bad", "last_valid_t", "last_valid_q", "first_bad_q")

# the calls in the order written (what each one is: Life.__init__)
CALLS = ("valid_big_md", "valid_big", "valid_1_md", "valid_65", "counted_0_md", "counted_Tm1", "contacts_65", "contacts_big", "proximity_65",
         "motion_wave", "motion_expanded", "report_wave", "report_expanded")
# every small call (valid_1_md, valid_65, contacts_65, proximity_65, the count 0) directly behind a large call of another entry point;
# every validity call with depths (valid_1_md, valid_big_md, counted_0_md) directly behind a depth-less validity launch
INTERLEAVED = ("motion_expanded", "valid_1_md", "contacts_big", "valid_65", "valid_big", "contacts_65", "report_expanded", "proximity_65",
               "counted_Tm1", "valid_big_md", "motion_wave", "counted_0_md", "report_wave")


class Life:
    def __init__(self, env, oracle_mod, n_cu=None):
        """n_cu given: the expected bytes alone, for that many CUs, no device (the script's CPU-side facts can be checked without one)"""
        import torch
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner, _ptr, _stream_handle
        gpu = n_cu is None
        if gpu:
            n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        self.env = env
        self.b = b = Batch(env, n_cu, oracle_mod)
        pi, T, N = b.pi, b.T, b.N
        thr = pi.spec.contact_threshold
        self.sc = sc = self.new_scene() if gpu else None
        self.bp = bp = BatchPlanner(sc) if gpu else None
        assert not gpu or (sc.valid_kernel(N) == "k_is_valid_v5" and sc.valid_kernel(T - 1) == "k_is_valid" and sc.valid_kernel(65) == "k_is_valid")
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda() if gpu else None
        tq, tr = up(b.qa), up(b.rows)
        pre = {n: (tq[:n].contiguous(), tr[:(n + SPE - 1) // SPE].contiguous()) for n in (1, 65, N)} if gpu else None
        u64 = lambda a: np.ascontiguousarray(a).view(np.uint64)

        # ---- validity: the oracle's one run over the N states, every smaller batch a prefix ----
        # (outputs pre-filled: a launch that skips a state leaves the fill, whatever the memory held before)
        def valid(n, md):
            def fn(st):
                v, d = _filled(n, md)
                _lib.check(_lib.lib().mopa_is_valid_batch(sc.handle, _ptr(pre[n][0]), _ptr(pre[n][1]), n, SPE, _ptr(v), _ptr(d) if md else None, _stream_handle(st)))
                return (v, d) if md else (v,)
            return fn, ((b.ov[:n], u64(b.omd[:n]).view(np.int64)) if md else (b.ov[:n],))

        def counted(n, md):
            def fn(st):
                v, d = _filled(N, md)
                nd = torch.tensor([n], dtype=torch.int64, device="cuda")
                _lib.check(_lib.lib().mopa_is_valid_batch_counted(sc.handle, _ptr(tq), _ptr(tr), N, SPE, _ptr(v), _ptr(d) if md else None, _ptr(nd),
                                                                  _stream_handle(st)))
                return (v, d, nd) if md else (v, nd)          # (nd: kept alive until the launch has read it)
            wv = np.full(N, FILL_VALID, dtype=np.uint8)
            wv[:n] = b.ov[:n]
            wd = np.full(N, FILL_MD, dtype=np.uint64)
            wd[:n] = u64(b.omd[:n])
            cnt = np.array([n], dtype=np.int64)
            return fn, ((wv, wd.view(np.int64), cnt) if md else (wv, cnt))

        # ---- contact report at the threshold, proximity report: the oracle's pair distances / poses of the same states ----
        D = oracle_pair_dists(pi, b.orc, b.qa, b.rows, SPE)

        def contacts(n):
            return (lambda st: tuple(bp.contacts(*pre[n], samples_per_env=SPE, cutoff=thr, max_contacts=4, stream=st))), report_from_dists(D[:n], thr, 4)

        gpos, gmat = P.poses(pi, b.orc, b.qa[:65], b.rows, SPE)
        prox = P.select(P.pair_dists(pi, gpos, gmat, 0.01), 0.01, 3)

        # ---- motion: the 512 shared segments of motion_report_ref, tiled to one segment under / over the expansion threshold ----
        _, orc, qa, qb, row = R.shared_segments(env)
        rep = R.shared_report(env)
        blk = R.blockers(pi, orc, rep, row, 4, len(qa))
        trow = up(row)
        self.n_wave, self.n_exp = 16 * n_cu - 1, 16 * n_cu + 1
        assert not gpu or (sc.motion_kernel(self.n_wave) == "k_check_motion" and sc.motion_kernel(self.n_exp) == "k_motion_expand")
        seg = {}
        for n in (self.n_wave, self.n_exp):
            idx = np.resize(np.random.default_rng(3).permutation(512), n)
            seg[n] = (idx, up(qa[idx]), up(qb[idx]))

        def motion(n):
            idx, ta, tb = seg[n]
            return (lambda st: (bp.check_motion(ta, tb, trow, samples_per_env=n, stream=st),)), (rep["valid"][idx],)

        def report(n):
            idx, ta, tb = seg[n]

            def fn(st):
                r = bp.motion_report(ta, tb, trow, samples_per_env=n, max_contacts=4, stream=st)
                return tuple(getattr(r, k) for k in MOTION_FIELDS) + tuple(r.blockers)
            return fn, tuple(rep[k][idx] for k in MOTION_FIELDS) + tuple(x[idx] for x in blk)

        self.calls = {"valid_big_md": valid(N, True), "valid_big": valid(N, False), "valid_1_md": valid(1, True), "valid_65": valid(65, False),
                      "counted_0_md": counted(0, True), "counted_Tm1": counted(T - 1, False), "contacts_65": contacts(65), "contacts_big": contacts(N),
                      "proximity_65": ((lambda st: tuple(bp.proximity(*pre[65], samples_per_env=SPE, band=0.01, max_pairs=3, stream=st))), prox),
                      "motion_wave": motion(self.n_wave), "motion_expanded": motion(self.n_exp), "report_wave": report(self.n_wave),
                      "report_expanded": report(self.n_exp)}
        assert set(self.calls) == set(CALLS) == set(INTERLEAVED) and len(INTERLEAVED) == len(CALLS)
        if gpu:
            torch.cuda.synchronize()

    def new_scene(self):
        from mopa_rl_amd import _lib
        pi = self.b.pi
        return _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)

    def enqueue(self, order, stream=None):
        """the calls of `order` one behind the other on one stream, nothing read back: [(name, output tensors)]"""
        import torch
        out = []
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            for name in order:
                out.append((name, self.calls[name][0](stream)))
        return out

    def compare(self, outs, what):
        import torch
        torch.cuda.synchronize()
        host = [(name, [g.cpu().numpy() for g in got]) for name, got in outs]
        # the outputs go back to the allocator holding 0xA5 bytes, not results: a later call that is handed the same memory and skips
        # part of its work cannot pass on what an earlier, identical call left there
        for _, got in outs:
            for g in got:
                g.view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize()
        for pos, (name, got) in enumerate(host):
            want = self.calls[name][1]
            assert len(got) == len(want), (what, name)
            for k, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == w.dtype and g.shape == w.shape, (self.env, what, pos, name, k, g.dtype, w.dtype, g.shape, w.shape)
                assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (self.env, what, "call", pos, name, "output", k, "differs in",
                                                                           int((g.view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum()), "bytes",
                                                                           "behind", outs[pos - 1][0] if pos else None)


@pytest.fixture(scope="module", params=[PUSH, LIFT])
def life(request, oracle_mod):
    w = Life(request.param, oracle_mod)
    yield w
    w.sc.close()


def check_script(w):
    """CPU-side facts of the script: the batch's composition (as in test_k1_counted_gpu.py), reports that are not empty, motion
    segments of both verdicts, and the interleaving's two rules"""
    w.b.check_composition()
    for name in ("contacts_65", "contacts_big"):
        cnt = w.calls[name][1][0]
        assert 0 < (cnt > 0).sum() < len(cnt), name
    cl, cnt, _, _ = w.calls["proximity_65"][1]
    assert (cnt > 0).any() and (cl < 0.01).any()
    for name in ("motion_wave", "motion_expanded"):
        v = w.calls[name][1][0]
        assert 0 < int(v.sum()) < len(v), name
    assert (w.calls["report_expanded"][1][6] > 0).any()          # blockers reported
    small = {"valid_1_md", "valid_65", "contacts_65", "proximity_65", "counted_0_md"}
    large = {"valid_big_md", "valid_big", "counted_Tm1", "contacts_big", "motion_wave", "motion_expanded", "report_wave", "report_expanded"}
    entry = lambda n: n.split("_")[0]
    depthless_validity = {"valid_big", "valid_65", "counted_Tm1", "motion_wave", "motion_expanded"}
    for prev, cur in zip(INTERLEAVED, INTERLEAVED[1:]):
        if cur in small:
            assert prev in large and entry(prev) != entry(cur), (prev, cur)
        if cur.endswith("_md"):
            assert prev in depthless_validity, (prev, cur)
    assert INTERLEAVED[0] not in small and not INTERLEAVED[0].endswith("_md")


def test_the_script_covers_what_it_claims(life):
    check_script(life)


def test_in_the_order_written(life):
    life.compare(life.enqueue(CALLS), "order written")


def test_in_reverse(life):
    life.compare(life.enqueue(CALLS[::-1]), "reverse")


def test_interleaved(life):
    life.compare(life.enqueue(INTERLEAVED), "interleaved")


def test_interleaved_on_a_second_stream_with_the_first_in_flight(life):
    import torch
    torch.cuda.synchronize()
    first = life.enqueue(INTERLEAVED)
    second = life.enqueue(INTERLEAVED, torch.cuda.Stream())
    life.compare(first, "interleaved, first stream")
    life.compare(second, "interleaved, second stream")


def test_closed_scene_then_a_fresh_one(life):
    """(the last test of the module: it closes the module's scene, which frees every buffer the runs above retired)"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    w, b = life, life.b
    torch.cuda.synchronize()
    w.sc.close()
    sc = w.new_scene()
    tq, tr = torch.from_numpy(b.qa.copy()).cuda(), torch.from_numpy(b.rows.copy()).cuda()
    v, d = BatchPlanner(sc).is_valid(tq, tr, samples_per_env=SPE, want_min_dist=True)
    v0 = BatchPlanner(sc).is_valid(tq, tr, samples_per_env=SPE)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), b.ov) and np.array_equal(v0.cpu().numpy(), b.ov)
    assert d.cpu().numpy().view(np.uint64).tobytes() == b.omd.view(np.uint64).tobytes()
    sc.close()
