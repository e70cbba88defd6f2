#!/usr/bin/env python3
"""Tuning: where and when the waves of dfl_tree_kernel run (a -DCCT_TREE_PROF build of the library, tools/debug/tree_prof.sh).

Every tree wave that has a block leaves a record: its hardware id (HW_ID and XCC_ID registers), s_memrealtime at entry and
exit (100 MHz), and its s_memtime delta (shader cycles).  This runs the bench workload as tools/prof_codec.py --what enc does,
reads the records of the last call and prints
  - tree waves per CU and per SIMD (histogram, maximum, mean),
  - the spread of the start times,
  - wave life against the number of tree waves on the same CU,
  - the in-kernel clock: delta s_memtime / delta s_memrealtime x 100 MHz (median over the waves).

    CCT_HIP_LIB=build_ab/libcompact_hip_tree_prof.so python tools/debug/tree_placement.py [--slices 256] [--tree-waves 0]
"""
import argparse
import collections
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "2023-compact-image-compression_amd")]

REC = np.dtype([("hw_id", "<u4"), ("xcc_id", "<u4"), ("slice", "<u4"), ("block", "<u4"),
                ("rt0", "<u8"), ("rt1", "<u8"), ("cycles", "<u8")])
CAP = 16384


def hist_line(counts):
    h = collections.Counter(counts)
    return " ".join(f"{k}:{h[k]}" for k in sorted(h))


def summarise(rec, out=sys.stdout):
    """rec: the records some wave wrote (rt1 != 0)."""
    # gfx9 HW_ID: wave 3:0, SIMD 5:4, pipe 7:6, CU 11:8, SH 12, SE 15:13.  XCC_ID: 3:0
    xcc = rec["xcc_id"] & 15
    simd = (rec["hw_id"] >> 4) & 3
    cu = (rec["hw_id"] >> 8) & 15
    sh = (rec["hw_id"] >> 12) & 1
    se = (rec["hw_id"] >> 13) & 7
    cu_key = (xcc.astype(np.int64) << 8) | ((rec["hw_id"].astype(np.int64) >> 8) & 255)  # (XCC, SE, SH, CU)
    simd_key = (cu_key << 2) | simd
    life_us = (rec["rt1"] - rec["rt0"]).astype(np.float64) / 100.0
    start_us = (rec["rt0"] - rec["rt0"].min()).astype(np.float64) / 100.0
    end_us = (rec["rt1"] - rec["rt0"].min()).astype(np.float64) / 100.0
    cus, per_cu_idx, per_cu = np.unique(cu_key, return_inverse=True, return_counts=True)
    _, per_simd = np.unique(simd_key, return_counts=True)
    _, per_xcc = np.unique(xcc, return_counts=True)
    p = lambda *a: print(*a, file=out)
    p(f"tree waves with a block: {len(rec)}   slices: {len(np.unique(rec['slice']))}   blocks per slice: "
      f"{hist_line(np.unique(rec['slice'], return_counts=True)[1])} (blocks:slices)")
    p(f"ids seen: XCC {sorted(set(xcc.tolist()))}  SE {sorted(set(se.tolist()))}  SH {sorted(set(sh.tolist()))}  "
      f"CU {sorted(set(cu.tolist()))}  SIMD {sorted(set(simd.tolist()))}")
    p(f"waves per XCC: {per_xcc.tolist()}")
    p(f"CUs that ran a tree wave: {len(cus)}   waves per CU: max {per_cu.max()}  mean {per_cu.mean():.2f}  min {per_cu.min()}")
    p(f"  histogram (waves:CUs)   {hist_line(per_cu)}")
    p(f"waves per SIMD: max {per_simd.max()}  mean {per_simd.mean():.2f}   histogram (waves:SIMDs)  {hist_line(per_simd)}")
    q = np.percentile(start_us, [50, 90, 99, 100])
    p(f"start after the first wave, us: median {q[0]:.2f}  p90 {q[1]:.2f}  p99 {q[2]:.2f}  last {q[3]:.2f}")
    stamped = (rec["slice"] == 0) & (rec["block"] == 0)  # this wave also prints its phase stamps: its end is not the kernel's
    p(f"first start to last end without the wave that prints its stamps: {end_us[~stamped].max():.1f} us")
    p(f"kernel, first start to last end: {end_us.max():.1f} us   wave life, us: mean {life_us.mean():.1f}  "
      f"median {np.median(life_us):.1f}  max {life_us.max():.1f}")
    # peak number of tree waves alive at once on a CU (by the time stamps), next to the plain count
    peak = np.zeros(len(cus), dtype=np.int64)
    for i in range(len(cus)):
        m = per_cu_idx == i
        ev = sorted([(t, 1) for t in rec["rt0"][m]] + [(t, -1) for t in rec["rt1"][m]], key=lambda e: (e[0], e[1]))
        c = 0
        for _, d in ev:
            c += d
            peak[i] = max(peak[i], c)
    p(f"peak tree waves alive at once on a CU: max {peak.max()}  mean {peak.mean():.2f}   histogram (waves:CUs)  {hist_line(peak)}")
    p("wave life against the tree waves on its CU (waves on the CU: waves, mean life us, max life us, last end us):")
    on_cu = per_cu[per_cu_idx]
    for k in sorted(set(on_cu.tolist())):
        m = on_cu == k
        p(f"  {k:3d}: {int(m.sum()):5d}  {life_us[m].mean():8.1f}  {life_us[m].max():8.1f}  {end_us[m].max():8.1f}")
    p("wave life against the tree waves on its SIMD (waves on the SIMD: waves, mean life us, max life us):")
    _, per_simd_idx = np.unique(simd_key, return_inverse=True)
    on_simd = per_simd[per_simd_idx]
    for k in sorted(set(on_simd.tolist())):
        m = on_simd == k
        p(f"  {k:3d}: {int(m.sum()):5d}  {life_us[m].mean():8.1f}  {life_us[m].max():8.1f}")
    # the same block index of every slice: what the block's own content does to a wave's life, whatever its place
    p("wave life against the block's index in its slice (block: waves, min / mean / max life us):")
    for b in sorted(set(rec["block"].tolist())):
        m = rec["block"] == b
        p(f"  {b:3d}: {int(m.sum()):5d}  {life_us[m].min():8.1f}  {life_us[m].mean():8.1f}  {life_us[m].max():8.1f}")
    clk = rec["cycles"].astype(np.float64) / np.maximum((rec["rt1"] - rec["rt0"]).astype(np.float64), 1.0) * 100.0
    p(f"in-kernel clock, MHz (s_memtime / s_memrealtime x 100): median {np.median(clk):.0f}  min {clk.min():.0f}  max {clk.max():.0f}")
    p(f"wave life, shader cycles: mean {rec['cycles'].mean():.0f}  max {rec['cycles'].max()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--tree-waves", type=int, default=None, help="option tree_waves of the library (0 automatic, 1, 16)")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from bench import make_batches
    import cct_hip
    from cct_hip import _ffi
    L = _ffi.lib()
    try:
        reset, read = L.cct_tree_prof_reset, L.cct_tree_prof_read
    except AttributeError:
        sys.exit("this library has no tree probe: build it with -DCCT_TREE_PROF (tools/debug/tree_prof.sh)")
    read.argtypes = [C.c_void_p, C.c_int]
    if args.tree_waves is not None:
        _ffi.check(L.cct_set_option(b"tree_waves", args.tree_waves))
    batch = make_batches(0, args.slices)[0]
    cfg = cct_hip.default_config()
    files = cct_hip.encode_batch(batch, cfg)
    for _ in range(args.reps):  # warm: graph captured, clocks up
        assert cct_hip.encode_batch(batch, cfg) == files
    if reset() != 0:
        sys.exit("cct_tree_prof_reset failed")
    assert cct_hip.encode_batch(batch, cfg) == files
    buf = np.zeros(CAP, dtype=REC)
    if read(buf.ctypes.data, CAP) != CAP:
        sys.exit("cct_tree_prof_read failed")
    rec = buf[buf["rt1"] != 0]
    if len(rec) == 0:
        sys.exit("no tree wave left a record")
    print(f"# tree placement, {args.slices} bench payloads, tree_waves option {args.tree_waves}")
    summarise(rec)


if __name__ == "__main__":
    main()
