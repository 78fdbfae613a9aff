"""dW and db of the bf16 weight-gradient calls, for comparing two builds of the library bit for bit (tools/ab_lib.sh,
VY_LIB_PATH; one fresh process per library):
  python tools/dump_wgrad.py OUT.npz          the bf16 shapes of tests.test_bwd_kernels_gpu.test_wgrad_exact, each through
                                              linear_wgrad (overwrite, accumulate, accumulate with alpha = 0.5) and the
                                              grouped entry point, and the six-item strided group of test_wgrad_grouped;
                                              on integer data ("int") and on random data ("rnd")
  python tools/dump_wgrad.py --compare A.npz B.npz [C.npz ...]
prints, per array and file, byte-identical or the largest difference from A in units of fp32 ulp.  The partial tiles of the
M-splits are added with float atomics in no fixed order, so an array's name says what may be asked of it:
  "exact."  integer data (exact in fp32 in any order), or random data with one addend per element, or two onto zeros
            (a + b = b + a): must be byte-identical -- the exit status says whether they all are;
  "pair."   random data, two addends onto a non-zero start ((c + a) + b is not always (c + b) + a);
  "sum."    random data, three or more addends."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda"
BF = torch.bfloat16


def cdiv(a, b):
    return (a + b - 1) // b


# the launchers' M-split arithmetic (vy_bwd.hip: wgrad_split and its two callers)
def m_splits(M, want):
    want = max(1, min(want, cdiv(M, 256)))
    return cdiv(M, cdiv(cdiv(M, want), 64) * 64)


def single_splits(M, N, K):
    big = N >= 8192 and M >= 4096
    tiles = cdiv(N, 256) * cdiv(K, 256) if big else cdiv(N, 128) * cdiv(K, 128)
    return m_splits(M, 256 // tiles if big else cdiv(384, tiles))


def group_splits(shapes):
    total = sum(cdiv(N, 256) * cdiv(K, 256) for M, N, K in shapes)
    return [m_splits(M, 256 // total) for M, N, K in shapes]


def tag(kind, addends, zero_start):
    if kind == "int" or addends == 1 or (addends == 2 and zero_start):
        return "exact."
    return "pair." if addends == 2 else "sum."


def dump(path):
    from tests import test_bwd_kernels_gpu as T
    from tests.test_kernels_gpu import ints, rnd
    from vyomai_amd import ops
    shapes = [c[1:] for c in T.test_wgrad_exact.pytestmark[0].args[1] if c[0] == BF]
    group = [(4096, 768, 768, True), (4096, 3072, 768, True), (4096, 768, 3072, False), (4100, 2304, 768, True),
             (1000, 520, 264, True), (300, 56, 8, False)]          # test_wgrad_grouped
    out = {}

    def make(kind, M, C, seed):
        return (ints(M, C, seed=seed, lo=-2, hi=2) if kind == "int" else rnd(M, C, seed=seed)).to(BF).to(DEV)

    def keep(name, dw, db):
        out[name + ".dW"] = dw.cpu().numpy()
        if db is not None:
            out[name + ".db"] = db.cpu().numpy()

    for kind in ("int", "rnd"):
        for M, N, K in shapes:
            ld = (N + 7) // 8 * 8
            dy_full = torch.zeros(M, ld, dtype=BF, device=DEV)
            dy_full[:, :N] = make(kind, M, N, 1)
            dy, x = dy_full[:, :N], make(kind, M, K, 2)
            alpha = torch.tensor([0.5], dtype=torch.float32, device=DEV)
            one, grp = single_splits(M, N, K), group_splits([(M, N, K)])[0]
            calls = (("overwrite", one, lambda dw, db: ops.linear_wgrad(dy, x, dw, db, accumulate=False)),
                     ("accumulate", one, lambda dw, db: ops.linear_wgrad(dy, x, dw, db, accumulate=True)),
                     ("alpha", one, lambda dw, db: ops.linear_wgrad(dy, x, dw, db, accumulate=True, alpha=alpha)),
                     ("grouped", grp, lambda dw, db: ops.linear_wgrad_grouped([(dy, x, dw, db)])))
            for call, addends, fn in calls:     # every call starts from 7.0, so that each stands alone
                dw = torch.full((N, K), 7.0, dtype=torch.float32, device=DEV)
                db = torch.full((N,), 7.0, dtype=torch.float32, device=DEV)
                fn(dw, db)
                keep(f"{tag(kind, addends, call == 'overwrite')}{kind}.{M}x{N}x{K}.{call}", dw, db)
        items = []
        for i, (M, N, K, bias) in enumerate(group):
            dy_full = make(kind, M, N + 8, 10 + i)              # row stride N + 8
            dw = torch.full((N, K), 3.0, dtype=torch.float32, device=DEV)
            db = torch.full((N,), 3.0, dtype=torch.float32, device=DEV) if bias else None
            items.append((dy_full[:, :N], make(kind, M, K, 30 + i), dw, db))
        ops.linear_wgrad_grouped(items)
        for i, ((dy, x, dw, db), addends) in enumerate(zip(items, group_splits([s[:3] for s in group]))):
            keep(f"{tag(kind, addends, False)}{kind}.group.{i}", dw, db)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays, {sum(k.startswith('exact.') for k in out)} of them order-independent")


def compare(paths):
    files = [np.load(p) for p in paths]
    a = files[0]
    bad = 0
    for p, f in zip(paths[1:], files[1:]):
        assert sorted(f.files) == sorted(a.files), "different cases"
        worst = {}
        for k in sorted(a.files):
            x, y = a[k], f[k]
            if x.tobytes() == y.tobytes():
                print(f"{p} vs {paths[0]}: {k}: byte-identical")
                continue
            ulp = float((np.abs(y.astype(np.float64) - x) / np.spacing(np.abs(x)).astype(np.float64)).max())
            print(f"{p} vs {paths[0]}: {k}: {int((x != y).sum())}/{x.size} differ, largest difference {ulp:.1f} ulp"
                  + ("  DIFFERENT" if k.startswith("exact.") else ""))
            cls = k.split(".")[0]
            worst[cls] = max(worst.get(cls, 0.0), ulp)
            bad += k.startswith("exact.")
        n = {c: sum(k.startswith(c + ".") for k in a.files) for c in ("exact", "pair", "sum")}
        print(f"{p} vs {paths[0]}: summary: " + "; ".join(
            f"{c}: {n[c]} arrays, " + (f"largest difference {worst[c]:.1f} ulp" if c in worst else "all byte-identical")
            for c in ("exact", "pair", "sum")))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
