"""Outputs of the six vocabulary-row calls (xent_fwd / xent_bwd_ / xent_fused_, logprob_fwd / logprob_bwd_ /
logprob_fused_) on the grids of tests.test_training_gpu.test_xent_kernels_vs_fp64 and
tests.test_dpo_gpu.test_logprob_kernels_vs_fp64, for comparing two builds of the library bit for bit (tools/ab_lib.sh,
VY_LIB_PATH; one fresh process per library):
  python tools/dump_head_rows.py OUT.npz          lse, logp, the whole buffer (pad columns included) of every case;
                                                  loss_sum of the one-row launches under "one.", of the others under "sum."
  python tools/dump_head_rows.py --compare A.npz B.npz [C.npz ...]
everything but "sum." must be byte-identical; "sum." (a float-atomic sum over rows, not order-fixed) is printed as the
largest difference from A in units of fp32 ulp, per file."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda"


def raw(t):
    t = t.detach().cpu().contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()


def dump(path):
    from tests.test_dpo_gpu import _kernel_case
    from tests.test_training_gpu import _xent_case
    from vyomai_amd import ops
    out = {}
    for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for V in (512, 1000, 1003, 32000, 50265, 65536, 70000):
            kinds = ("pair", "fused") if dtype == torch.bfloat16 and V <= 65536 else ("pair",)
            _, xbuf, xlab = _xent_case(V, dtype, seed=V % 97)
            _, lbuf, llab, w = _kernel_case(V, dtype, seed=V % 97)
            for oob in (None, 7):
                xl, ll = xlab.clone(), llab.clone()
                if oob is not None:
                    xl[oob] = ll[oob] = -1 if V % 2 else V
                for kind in kinds:
                    for rows, tag in ((slice(None), "sum."), (slice(0, 1), "one.")):
                        key = f"{dn}.{V}.{oob}.{kind}"
                        b = xbuf[rows].to(DEV).clone()
                        lab = xl[rows].to(DEV)
                        M = b.shape[0]
                        lse, acc = torch.full((M,), 9.0, device=DEV), torch.zeros(2, device=DEV)
                        gs, flag = torch.full((1,), 0.5, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
                        if kind == "fused":
                            acc[1] = float(((lab != -100) & (lab >= 0) & (lab < V)).sum())
                            ops.xent_fused_(b[:, :V], lab, -100, lse, acc[0:1], acc[1:2], gs, flag)
                        else:
                            ops.xent_fwd(b[:, :V], lab, -100, lse, acc[0:1], acc[1:2], flag)
                            ops.xent_bwd_(b[:, :V], lab, -100, lse, gs, acc[1:2])
                        out[tag + key] = raw(acc[0:1])
                        out[f"xent.{tag}{key}.lse"], out[f"xent.{tag}{key}.buf"] = raw(lse), raw(b)
                        out[f"xent.{tag}{key}.count_flag"] = np.array([acc[1].item(), flag.item()])
                    key = f"{dn}.{V}.{oob}.{kind}"
                    b, lab, wd = lbuf.to(DEV).clone(), ll.to(DEV), w.to(DEV)
                    lse, logp = torch.full((b.shape[0],), 9.0, device=DEV), torch.full((b.shape[0],), 9.0, device=DEV)
                    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
                    if kind == "fused":
                        ops.logprob_fused_(b[:, :V], lab, wd, lse, logp, flag)
                    else:
                        ops.logprob_fwd(b[:, :V], lab, wd, lse, logp, flag)
                        ops.logprob_bwd_(b[:, :V], lab, wd, lse)
                    out[f"logprob.{key}.lse"], out[f"logprob.{key}.logp"] = raw(lse), raw(logp)
                    out[f"logprob.{key}.buf"], out[f"logprob.{key}.flag"] = raw(b), np.array([flag.item()])
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays")


def compare(paths):
    files = [np.load(p) for p in paths]
    a = files[0]
    bad = 0
    for p, f in zip(paths[1:], files[1:]):
        assert sorted(f.files) == sorted(a.files), "different cases"
        exact = [k for k in a.files if not k.startswith("sum.")]
        diff = [k for k in exact if a[k].tobytes() != f[k].tobytes()]
        ulps = [abs(float(f[k][0]) - float(a[k][0])) / float(np.spacing(np.abs(a[k][0]))) for k in a.files if k.startswith("sum.")]
        print(f"{p} vs {paths[0]}: {len(exact) - len(diff)}/{len(exact)} arrays byte-identical; multi-row loss_sum: "
              f"largest difference {max(ulps):.1f} ulp, {sum(u == 0 for u in ulps)}/{len(ulps)} equal")
        for k in diff[:10]:
            print("  DIFFERENT:", k)
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    dump(sys.argv[1])
