"""What one CU streams as an AdamW rider of the grouped weight-gradient launch (vy_linear_wgrad_grouped_opt): rider-only
launches of 8, 40 and 256 workgroups -- one chunk each, one workgroup per CU -- over cold ranges of a large arena, beside
the plain vy_adamw_step launch over the same bytes.  ADAMW_RIDE_CU_BYTES_PER_US of vy_bwd.hip is set from the 40-workgroup
figure (HIP events around one launch: its launch latency is inside).
  python tools/bench_adamw_ride.py [--chunk 16384] [--reps 24]"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vyomai_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--chunk", type=int, default=16384, help="ADAMW_RIDE_CHUNK of vy_bwd.hip")
ap.add_argument("--reps", type=int, default=24)
a = ap.parse_args()
HY = (5e-5, 0.9, 0.999, 1e-8, 0.01, 3, 1.0)
for wgs in (8, 40, 256):
    n = wgs * a.chunk
    tot = n * (a.reps + 2)
    p, g = torch.randn(tot, device="cuda"), torch.randn(tot, device="cuda")
    m, v, pb = torch.zeros(tot, device="cuda"), torch.zeros(tot, device="cuda"), torch.zeros(tot, device="cuda", dtype=torch.bfloat16)
    res = {}
    for kind in ("ride", "plain"):
        ts = []
        for r in range(a.reps + 2):   # every launch its own range: nothing is warm in the caches
            s = slice(r * n, (r + 1) * n)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if kind == "ride":
                taken = ops.linear_wgrad_grouped([ops.AdamWRide(p[s], g[s], m[s], v[s], pb[s], *HY)])
                assert taken == [n]
            else:
                ops.adamw_step(p[s], g[s], m[s], v[s], pb[s], *HY)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = sorted(ts[2:])
        res[kind] = ts[len(ts) // 2]
    us = res["ride"]
    print(f"{wgs:4d} workgroups x {a.chunk} elements: ride {us:7.1f} us -> {a.chunk * 30 / us / 1e3:6.1f} GB/s per CU, "
          f"{n * 30 / us / 1e6:6.2f} TB/s in all   (plain vy_adamw_step over the same range: {res['plain']:7.1f} us)")
