"""Where the wave slots of the baked K1 kernel stand empty: one launch of the bench batch (Push, 4096 envs x 256 states, verdict
only) on the timeline build of the library, in which every wave stamps the 100 MHz clock where its life changes phase
(mopa_valid_v5.inc: MOPA_V5_TIMELINE; the row's layout is there).

  bash tools/k1_knock.sh build          with K1_KNOCK_VARIANTS=timeline       (build container)
  MOPA_HIP_LIB=$PWD/mopa_rl_amd/csrc/libmopa_knock_timeline.so python tools/k1_wave_timeline.py      (GPU box)

The launch has one wave per wave slot (2 workgroups x 4 waves on every CU), so a wave's row is its slot's: the slot is empty from
the first wave's entry to its own, and from its exit to the last wave's.  Printed: distributions of start skew, staging time,
tiles and pulls per wave, the time of the last pull that got a tile, of the pull that found none, the final portal flush, the
exit; and the share of all slot-time (waves x span) each explains.  MOPA_K1_PAIR_TAIL_TILES applies as in any launch."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ROW = 64          # kTlRow
TICK_US = 0.01    # s_memrealtime: 100 MHz


def dist(name, x, unit="us"):
    x = np.asarray(x, dtype=np.float64)
    q = np.percentile(x, [0, 10, 50, 90, 99, 100])
    print(f"  {name:34s} min {q[0]:8.2f}  p10 {q[1]:8.2f}  p50 {q[2]:8.2f}  p90 {q[3]:8.2f}  p99 {q[4]:8.2f}  max {q[5]:8.2f}  mean {x.mean():8.2f} {unit}")


def main():
    import torch
    import bench
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs
    L = _lib.lib()
    if not hasattr(L, "mopa_k1_timeline_read"):
        raise SystemExit("this library is not a timeline build: set MOPA_HIP_LIB to libmopa_knock_timeline.so (tools/k1_knock.sh)")
    L.mopa_k1_timeline_read.restype = C.c_longlong
    L.mopa_k1_timeline_read.argtypes = [C.c_void_p, C.c_longlong]
    pi = planner_inputs(bench.ENV)
    dev = torch.device("cuda", 0)
    sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(sc)
    E, S = 4096, 256
    qa, rows = bench.make_inputs(torch, pi, E, S, seed=1234, device=dev)
    out = torch.empty(E * S, dtype=torch.uint8, device=dev)
    for _ in range(5):
        bp.is_valid(qa, rows, samples_per_env=S, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    bp.is_valid(qa, rows, samples_per_env=S, out=out)
    e1.record()
    torch.cuda.synchronize()
    cap = 1 << 14
    buf = np.zeros((cap, ROW), np.uint64)
    n = L.mopa_k1_timeline_read(buf.ctypes.data_as(C.c_void_p), cap)
    if n <= 0:
        raise SystemExit("no timeline rows: the batch did not take the lane-per-state kernel")
    r = buf[:n].astype(np.int64)
    t0 = r[:, 0].min()
    us = lambda col: (r[:, col] - t0) * TICK_US
    entry, staged, last_pull, fin_pull, flushed, exit_ = us(0), us(1), us(3), us(4), us(5), us(6)
    span = exit_.max()
    pulls, tiles, mpr_rows = r[:, 2], r[:, 8], r[:, 7]
    print(f"k_is_valid_v5 on {bench.ENV}, {E} envs x {S} states, verdict only; baked scene #{L.mopa_scene_k1_baked(sc.handle)}; "
          f"MOPA_K1_PAIR_TAIL_TILES={os.environ.get('MOPA_K1_PAIR_TAIL_TILES', '(default)')}")
    print(f"{n} waves; first entry to last exit {span:.2f} us; the launch between two events {e0.elapsed_time(e1) * 1e3:.2f} us "
          f"(this build stamps and stores: not the production kernel's time)")
    print("per wave, times from the first wave's entry:")
    dist("entry (start skew)", entry)
    dist("staging (entry -> staged)", staged - entry)
    dist("tiles", tiles, "")
    dist("pulls (the empty one included)", pulls, "")
    dist("last pull that got a tile", last_pull)
    dist("pull that found no tile", fin_pull)
    dist("last tile(s) (last pull -> empty pull)", fin_pull - last_pull)
    dist("final portal flush", flushed - fin_pull)
    dist("rows in the final flush", mpr_rows, "")
    dist("exit", exit_)
    dist("lifetime (entry -> exit)", exit_ - entry)
    life = (exit_ - entry).sum()
    slot = n * span
    print(f"slot-time = waves x span = {slot / 1e3:.1f} ms; waves resident {100 * life / slot:.1f} %, slots empty {100 * (1 - life / slot):.1f} %:")
    print(f"  before the wave's entry (start skew)            {100 * entry.sum() / slot:6.2f} %")
    print(f"  after the wave's exit (tail)                    {100 * (span - exit_).sum() / slot:6.2f} %")
    print("resident, but not on tiles:")
    print(f"  staging                                          {100 * (staged - entry).sum() / slot:6.2f} %")
    print(f"  final portal flush (partial batch)               {100 * (flushed - fin_pull).sum() / slot:6.2f} %")
    print(f"  flush end -> exit (counter release)              {100 * (exit_ - flushed).sum() / slot:6.2f} %")
    # the tail, split: what the spread of the waves' empty pulls explains, and what the flushes behind them add
    print("the tail, from the other end:")
    print(f"  empty pull -> last wave's empty pull             {100 * (fin_pull.max() - fin_pull).sum() / slot:6.2f} %")
    print(f"  last wave's empty pull -> last exit              {100 * (span - fin_pull.max()) / span:6.2f} %")
    # per XCD: the start skew is a dispatch order effect if it follows the XCD / the workgroup index
    xcc = (r[:, 9] >> 32) & 0xF
    print("per XCD (XCC_ID): waves, mean entry, mean exit, mean tiles")
    for x in np.unique(xcc):
        m = xcc == x
        print(f"  xcd {int(x)}: {int(m.sum()):5d} waves  entry {entry[m].mean():7.2f} us  exit {exit_[m].mean():7.2f} us  tiles {tiles[m].mean():5.2f}")
    wg = np.arange(n) // 4
    first, second = wg < wg.max() // 2 + 1, wg >= wg.max() // 2 + 1
    print(f"workgroups 0..{wg.max() // 2}: mean entry {entry[first].mean():.2f} us; the rest: {entry[second].mean():.2f} us")
    sc.close()


if __name__ == "__main__":
    main()
