"""What the riders of the vocabulary weight gradient cost (vy_linear_wgrad_riders): the launch at the benchmark's shape
(N = 50265, K = 768, M = 16384: 591 tiles, 79 of 256 CUs busy in the last round) alone, with zero riders, with
transposing riders and with both, each at several sizes, beside the plain fill / vy_transpose_batched launches over the
same bytes.  Printed per size: what rode (a size the launcher's budget cuts short is reported as taken), how much the
launch grew, and the marginal rate -- bytes ridden per microsecond of growth, per idle CU ("inf" when the launch did not
grow).  Under event timing the carrier's own spread (~100 us) is larger than what the riders add: DESIGN section 3 "Riders
in the vocabulary weight gradient" reads the growth off the step profile instead.
  python tools/bench_wgrad_riders.py [--reps 7] [--mb 128 256 512 652]"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vyomai_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--mb", type=int, nargs="+", default=[128, 256, 512, 652], help="bytes of rider traffic, in MB")
a = ap.parse_args()
dev = "cuda"
M, N, K = 16384, 50265, 768
IDLE = 256 - (197 * 3) % 256
ld = (N + 63) // 64 * 64
dy = (torch.randn(M, ld, device=dev) * 0.01).to(torch.bfloat16)[:, :N]
x = torch.randn(M, K, device=dev).to(torch.bfloat16)
dw = torch.zeros(N, K, device=dev)
db = torch.zeros(N, device=dev)
alpha = torch.ones(1, device=dev)


def timed(fn):
    ts = []
    for _ in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts = sorted(ts[2:])
    return ts[len(ts) // 2], ts[0], ts[-1]


base = timed(lambda: ops.linear_wgrad(dy, x, dw, db, True, alpha))
print(f"carrier alone: median {base[0]:.1f} us (min {base[1]:.1f}, max {base[2]:.1f}); {IDLE} CUs idle in the last round")
for mb in a.mb:
    nbytes = mb << 20
    # zero riders: write-only traffic
    z = torch.ones(nbytes // 4, device=dev)
    got = {}

    def ride_zero():
        got["z"] = ops.linear_wgrad_riders(dy, x, dw, db, True, alpha, zero=[z])[0][0]

    tz = timed(ride_zero)
    tf = timed(lambda: z.zero_())
    # transposing riders: read + write, 768-wide bf16 matrices as the decoder's weights (half the bytes read, half written)
    rows = nbytes // 2 // (768 * 2) // 64 * 64
    src = torch.randn(rows, 768, device=dev).to(torch.bfloat16)
    dst = torch.empty(768, rows, device=dev, dtype=torch.bfloat16)
    tb = ops.TransposeBatch([(src[i:i + 3072], dst[:, i:i + 3072]) for i in range(0, rows - 3071, 3072)])

    def ride_tr():
        got["t"] = ops.linear_wgrad_riders(dy, x, dw, db, True, alpha, transposes=tb)[1]

    tt = timed(ride_tr)
    tp = timed(tb.run)
    tbytes = got["t"] * 2 * 64 * 64 * 2
    for name, t, plain, rode in (("zero", tz, tf, got["z"] * 4), ("transpose", tt, tp, tbytes)):
        grow = t[0] - base[0]
        rate = rode / grow / IDLE if grow > 0 else float("inf")
        print(f"{mb:5d} MB {name:9s}: rode {rode / 2**20:7.1f} MB, launch {t[0]:7.1f} us (+{grow:6.1f}; min {t[1]:.1f}, max {t[2]:.1f}), "
              f"plain launch over the same bytes {plain[0]:6.1f} us -> {rate:8.0f} B/us per idle CU")
    del z, src, dst, tb
