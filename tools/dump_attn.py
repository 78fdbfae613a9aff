"""Outputs of the tuned attention kernels (attn_fwd_mfma_kernel<64|128>, attn_bwd_dq_kernel, attn_bwd_dkdv_kernel), for
comparing two builds of the library bit for bit (tools/ab_lib.sh, VY_LIB_PATH; one fresh process per library):
  python tools/dump_attn.py OUT.npz          the bf16 dh = 64 / 128 cases of tests.test_kernels_gpu.ATTN_CASES: out, lse;
                                             the dh = 64 cases of tests.test_bwd_kernels_gpu.BWD_CASES: out, lse, delta_ws
                                             and the whole packed dq/dk/dv buffer, once with ("rope.") and once without
                                             ("plain.") the fused rotary inverse
  python tools/dump_attn.py --compare A.npz B.npz [C.npz ...]
prints, per array and file, byte-identical or the first difference from A.  These kernels have no atomics and a fixed
summation order, so every array must be byte-identical -- the exit status says whether they all are."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda"


def dump(path):
    import torch
    from tests import test_bwd_kernels_gpu as TB
    from tests import test_kernels_gpu as TF
    from vyomai_amd import ops
    BF = torch.bfloat16
    rnd = TF.rnd
    out = {}

    def raw(t):
        t = t.detach().cpu().contiguous()
        return (t.view(torch.int16) if t.dtype == BF else t).numpy()

    def keypad_of(B, S, second):
        kp = torch.ones(B, S, dtype=torch.uint8)
        kp[0, S - S // 3:] = 0
        if B > 1:
            second(kp)
        return kp.to(DEV)

    for case in TF.ATTN_CASES:
        B, h, hk, L, S, dh, causal, start, use_kp, use_add = case
        if dh not in (64, 128):
            continue
        q, k, v = (rnd(B, n, T, dh, seed=s).to(BF).to(DEV) for n, T, s in ((h, L, 1), (hk, S, 2), (hk, S, 3)))
        kp = keypad_of(B, S, lambda m: m[1, : min(5, S - 1)].zero_()) if use_kp else None
        am = None
        if use_add:
            am = rnd(B, 1, L, S, seed=5)
            am[:, :, :, ::7] = torch.finfo(torch.float32).min
            am = am.to(DEV)
        lse = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
        o = ops.attention(q, k, v, causal=causal, start_pos=start, keypad=kp, addmask=am, lse=lse)
        name = "fwd." + ".".join(str(int(x)) for x in case)
        out[name + ".out"], out[name + ".lse"] = raw(o), raw(lse)
    cos, sin = ops.rope_tables(64, 1024, DEV)
    for case in TB.BWD_CASES:
        if len(case) > 8 and case[8] != 64:
            continue
        B, h, hk, L, S, causal, start, use_kp = case[:8]
        dh = 64
        q, k, v = (rnd(B, n, T, dh, seed=s).to(BF).to(DEV) for n, T, s in ((h, L, 1), (hk, S, 2), (hk, S, 3)))
        do = rnd(B, L, h * dh, seed=4).to(BF).to(DEV)
        kp = keypad_of(B, S, lambda m: m[1, S - 7:].zero_()) if use_kp else None
        lse = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
        o = ops.attention(q, k, v, causal=causal, start_pos=start, keypad=kp, lse=lse)
        name = "bwd." + ".".join(str(int(x)) for x in case[:8])
        out[name + ".out"], out[name + ".lse"] = raw(o), raw(lse)
        for tag, rope in (("plain.", {}), ("rope.", dict(cos=cos, sin=sin, rope_pos0=3))):
            W = (h + 2 * hk) * dh       # the packed layout the QKV dgrad consumes; 7.0 where no kernel writes
            packed = torch.full((B, max(L, S), W), 7.0, dtype=BF, device=DEV)
            dq = packed[:, :L, : h * dh].view(B, L, h, dh).permute(0, 2, 1, 3)
            dk = packed[:, :S, h * dh:(h + hk) * dh].view(B, S, hk, dh).permute(0, 2, 1, 3)
            dv = packed[:, :S, (h + hk) * dh:].view(B, S, hk, dh).permute(0, 2, 1, 3)
            delta = torch.zeros(B, h, L, dtype=torch.float32, device=DEV)
            ops.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, causal=causal, start_pos=start, keypad=kp, delta=delta, **rope)
            out[tag + name + ".packed"], out[tag + name + ".delta_ws"] = raw(packed), raw(delta)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays")


def compare(paths):
    files = [np.load(p) for p in paths]
    a = files[0]
    bad = 0
    for p, f in zip(paths[1:], files[1:]):
        if sorted(f.files) != sorted(a.files):
            print(f"{p} vs {paths[0]}: different cases")
            bad += 1
            continue
        for k in sorted(a.files):
            x, y = a[k], f[k]
            if x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes():
                print(f"{p} vs {paths[0]}: {k}: byte-identical")
                continue
            bad += 1
            if x.shape != y.shape or x.dtype != y.dtype:
                print(f"{p} vs {paths[0]}: {k}: DIFFERENT shape or type {x.shape} {x.dtype} / {y.shape} {y.dtype}")
                continue
            ne = x.view(np.uint8).reshape(x.size, -1) != y.view(np.uint8).reshape(y.size, -1)
            where = np.flatnonzero(ne.any(-1))
            i = np.unravel_index(where[0], x.shape)
            print(f"{p} vs {paths[0]}: {k}: DIFFERENT, {where.size}/{x.size} elements, first at {tuple(int(j) for j in i)}: "
                  f"{x[i]!r} / {y[i]!r}")
        print(f"{p} vs {paths[0]}: summary: {len(a.files)} arrays, " + ("all byte-identical" if not bad else f"{bad} DIFFERENT"))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
