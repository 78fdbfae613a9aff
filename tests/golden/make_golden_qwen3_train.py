"""Generate tests/golden/qwen3_train.npz by differentiating the REAL reference's Qwen3Model on the CPU.  The model lives
in a notebook cell (Examples/simple_vllm.ipynb of the reference checkout) and is plain torch through its prefill branch;
compute_logprobs / compute_dpo_loss_batch live in Examples/vyom-ai-llm-sft-dpo-training.ipynb.  Both are read and
executed at run time only (make_golden_qwen3.reference_classes, and the way make_golden_dpo.py fetches its functions);
only arrays are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qwen3_train.py <reference checkout>

flash_attn_varlen_func is a dense causal stand-in written here (differentiable, in the tensors' own dtype accumulating
in fp32), and the rows are packed at their TRUE lengths: right padding under a causal mask is the same computation at
the real positions, so the padded batch of cases_qwen3_train.train_batch must reproduce these numbers.

Keys (case = q | r | n | t):
  <case>.loss                       fp32 shifted next-token loss of the batch (fp64 scalar)
  <case>.d.<param>                  every parameter's gradient (sub_g), fp32 run
  <case>.train.loss, .train.w.<p>   TRAIN_STEPS steps of torch.optim.AdamW in fp32: losses and the TRAINED weights
  <case>.gap.loss, .gap.d.<param>   the reference's OWN bf16 model against its fp32 model: relative loss gap, rel_err
                                    of each gradient
  <case>.check.*                    the self-checks below, as measured
  q.dpo.*                           pi / ref log-probs, loss.<beta>, reward.*, d.<param> of the beta = 1 loss
The maker asserts that the reference alone is inside every bar of tests/test_qwen3_train_gpu.py: fp32 against fp64
gradients rel_err < 1e-4 and loss < 2e-5 relative, bf16 loss within 3e-2, bf16 gradients within 3e-2 or their own gap.
"""
import json
import os
import sys
import types

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import cases_qwen3_train as C  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)
BLOCK = 16
WANTED = ("compute_logprobs", "compute_dpo_loss", "compute_dpo_loss_batch")


def varlen_causal(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=True, **_):
    """flash_attn_varlen_func for self-attention over packed segments, differentiable: q (T, h, dh), k / v (T, hk, dh)
    -> (T, h, dh); scores and softmax in at least fp32, the output in q's dtype."""
    assert causal and torch.equal(cu_seqlens_q, cu_seqlens_k)
    h, hk = q.shape[1], k.shape[1]
    up = torch.float64 if q.dtype == torch.float64 else torch.float32
    outs = []
    cu = cu_seqlens_q.tolist()
    for a, b in zip(cu[:-1], cu[1:]):
        qs = q[a:b].to(up).transpose(0, 1)
        ks = k[a:b].to(up).transpose(0, 1).repeat_interleave(h // hk, dim=0)
        vs = v[a:b].to(up).transpose(0, 1).repeat_interleave(h // hk, dim=0)
        s = qs @ ks.transpose(1, 2) / (q.shape[-1] ** 0.5)
        s = s.masked_fill(torch.ones(b - a, b - a, dtype=torch.bool).triu(1), float("-inf"))
        outs.append((torch.softmax(s, dim=-1) @ vs).transpose(0, 1).to(q.dtype))
    return torch.cat(outs, dim=0)


def reference_classes(checkout):
    stand_in = types.ModuleType("flash_attn")
    stand_in.flash_attn_varlen_func = varlen_causal
    stand_in.flash_attn_with_kvcache = None          # the decode branch is never taken
    sys.modules["flash_attn"] = stand_in
    with open(os.path.join(checkout, "Examples", "simple_vllm.ipynb")) as f:
        nb = json.load(f)
    for cell in nb["cells"]:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and "class Qwen3Model" in src:
            ns = {"__name__": "simple_vllm_cell"}
            exec(compile(src, "simple_vllm.ipynb", "exec"), ns)
            return ns
    raise RuntimeError("no cell defines Qwen3Model")


def notebook_functions(checkout):
    ns = {"torch": torch}
    path = os.path.join(checkout, "Examples", "vyom-ai-llm-sft-dpo-training.ipynb")
    with open(path) as f:
        cells = json.load(f)["cells"]
    for cell in cells:
        src = "".join(cell["source"])
        if cell["cell_type"] == "code" and any(f"def {name}(" in src for name in WANTED):
            exec(compile(src, path, "exec"), ns)
    return tuple(ns[name] for name in WANTED)


def forward(m, rows):
    """The reference's packed prefill forward over whole sequences (a list of id lists), WITH grad -> logits (T, V)."""
    cfg = m.cfg_for_maker
    dt = m.tok_emb.weight.dtype
    lens = [len(r) for r in rows]
    cu = np.concatenate([[0], np.cumsum(lens)])
    pos = torch.cat([torch.arange(n) for n in lens])
    nblk = sum((n + BLOCK - 1) // BLOCK for n in lens)
    shape = (nblk, BLOCK, cfg["n_kv_groups"], cfg["head_dim"])
    kcs = [torch.zeros(shape, dtype=dt) for _ in range(cfg["n_layers"])]
    vcs = [torch.zeros(shape, dtype=dt) for _ in range(cfg["n_layers"])]
    slots, first = [], 0
    for n in lens:
        slots.append(first * BLOCK + torch.arange(n))
        first += (n + BLOCK - 1) // BLOCK
    metadata = {"is_decoding": False, "slot_mapping": torch.cat(slots), "block_size": BLOCK,
                "cu_seqlens": torch.tensor(cu, dtype=torch.int32), "max_seqlen": max(lens),
                "cos": m.cos_buf[pos].unsqueeze(1), "sin": m.sin_buf[pos].unsqueeze(1)}
    return m(torch.tensor([t for r in rows for t in r]), kcs, vcs, metadata), cu


def clm_loss(m, x, y):
    rows = [x[r, :n].tolist() for r, n in enumerate(C.LENGTHS)]
    lg, cu = forward(m, rows)
    lgs = torch.cat([lg[a:b][:-1] for a, b in zip(cu[:-1], cu[1:])])
    if lgs.dtype == torch.bfloat16:
        lgs = lgs.float()        # (the loss itself in fp32, as TiedLMHeadLossFn reduces it)
    tgt = torch.cat([torch.from_numpy(y[r, 1:n]) for r, n in enumerate(C.LENGTHS)])
    return F.cross_entropy(lgs, tgt, ignore_index=-100)


class Padded:
    """What compute_dpo_loss_batch calls: model(input_ids=ids).logits, (PAIRS, L, V) with zeros on the padding."""

    def __init__(self, m, batch):
        self.m, self.batch = m, batch

    def __call__(self, input_ids):
        key = "chosen" if torch.equal(input_ids, self.batch["chosen"]) else "rejected"
        assert torch.equal(input_ids, self.batch[key])
        lens = self.batch[key + "_len"].tolist()
        lg, cu = forward(self.m, [input_ids[i, :n].tolist() for i, n in enumerate(lens)])
        rows = [F.pad(lg[a:b], (0, 0, 0, C.L - (b - a))) for a, b in zip(cu[:-1], cu[1:])]
        return types.SimpleNamespace(logits=torch.stack(rows))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def named_grads(m):
    return {n: p.grad.detach().double().numpy().copy() for n, p in m.named_parameters()}


def build(ns, case, dtype):
    if dtype == torch.float64:
        m = C.build(ns["Qwen3Model"], case, torch.float32).double()
        m.cos_buf, m.sin_buf = m.cos_buf.double(), m.sin_buf.double()
    else:
        m = C.build(ns["Qwen3Model"], case, dtype)
    m.cfg_for_maker = C.cfg(case, dtype)
    return m


def loss_and_grads(ns, case, dtype, x, y):
    m = build(ns, case, dtype)
    loss = clm_loss(m, x, y)
    loss.backward()
    return float(loss.detach()), named_grads(m)


def main():
    checkout = sys.argv[1]
    ns = reference_classes(checkout)
    compute_logprobs, compute_dpo_loss, compute_dpo_loss_batch = notebook_functions(checkout)
    out = {}
    worst = {"f32.grad": 0.0, "f32.loss": 0.0, "bf16.loss": 0.0, "bf16.grad": 0.0}
    for case in C.CASES:
        x, _, y = C.train_batch(case)
        l64, g64 = loss_and_grads(ns, case, torch.float64, x, y)
        l32, g32 = loss_and_grads(ns, case, torch.float32, x, y)
        l16, g16 = loss_and_grads(ns, case, torch.bfloat16, x, y)
        e_g = max(rel_err(g32[n], g64[n]) for n in g32)
        e_l = abs(l32 - l64) / max(1.0, abs(l64))
        gap_l = abs(l16 - l32) / max(1.0, abs(l32))
        out[f"{case}.loss"] = np.float64(l32)
        out[f"{case}.gap.loss"] = np.float64(gap_l)
        for n in g32:
            out[f"{case}.d.{n}"] = C.sub_g(n, g32[n]).astype(np.float32).copy()
            out[f"{case}.gap.d.{n}"] = np.float64(rel_err(g16[n], g32[n]))
        gap_g = max(float(out[f"{case}.gap.d.{n}"]) for n in g32)
        out[f"{case}.check.f32_vs_f64.grad"] = np.float64(e_g)
        out[f"{case}.check.f32_vs_f64.loss"] = np.float64(e_l)
        print(f"{case}: loss {l32:.6f}  fp32 vs fp64: grads {e_g:.2e} loss {e_l:.2e}  bf16 vs fp32: loss {gap_l:.2e} "
              f"grads {gap_g:.2e}")
        assert e_g < 1e-4 and e_l < 2e-5 and gap_l < 3e-2, (e_g, e_l, gap_l)
        for k, v in (("f32.grad", e_g), ("f32.loss", e_l), ("bf16.loss", gap_l), ("bf16.grad", gap_g)):
            worst[k] = max(worst[k], v)
        # TRAIN_STEPS steps of AdamW in fp32
        m = build(ns, case, torch.float32).train()
        opt = torch.optim.AdamW(list(m.parameters()), lr=C.LR, weight_decay=C.WEIGHT_DECAY)
        losses = []
        for _ in range(C.TRAIN_STEPS):
            opt.zero_grad()
            loss = clm_loss(m, x, y)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        print(f"   training losses {losses}")
        out[f"{case}.train.loss"] = np.array(losses, dtype=np.float64)
        params = dict(m.named_parameters())
        for n in C.trained(case):
            out[f"{case}.train.w.{n}"] = C.sub_g(n, params[n].detach().numpy()).astype(np.float32).copy()
    for k, v in worst.items():
        out[f"check.worst.{k}"] = np.float64(v)
    print("worst over the cases:", worst)

    # DPO, case q, fp32
    case = C.DPO_CASE
    batch = {k: torch.from_numpy(v) for k, v in C.dpo_batch(case).items()}
    pol, frozen = C.build_policy(ns["Qwen3Model"], case, torch.float32), build(ns, case, torch.float32)
    pol.cfg_for_maker = C.cfg(case, torch.float32)
    P, Fz = Padded(pol, batch), Padded(frozen, batch)
    with torch.no_grad():
        for who, mod in (("pi", P), ("ref", Fz)):
            for k in ("chosen", "rejected"):
                out[f"{case}.dpo.{who}.{k}"] = compute_logprobs(mod(input_ids=batch[k]).logits, batch[k],
                                                                batch[k + "_mask"]).double().numpy().copy()
        for beta in C.BETAS:
            loss, rc, rr = compute_dpo_loss_batch(batch, P, Fz, beta)
            out[f"{case}.dpo.loss.{beta}"] = np.float64(loss.item())
            out[f"{case}.dpo.reward.chosen"], out[f"{case}.dpo.reward.rejected"] = np.float64(rc.item()), np.float64(rr.item())
    pol.zero_grad()
    compute_dpo_loss_batch(batch, P, Fz, C.GRAD_BETA)[0].backward()
    for n, g in named_grads(pol).items():
        out[f"{case}.dpo.d.{n}"] = C.sub_g(n, g).astype(np.float32).copy()
    z = (out[f"{case}.dpo.pi.chosen"] - out[f"{case}.dpo.pi.rejected"]) - \
        (out[f"{case}.dpo.ref.chosen"] - out[f"{case}.dpo.ref.rejected"])
    print(f"dpo {case}: DPO logits {z}  " + "  ".join(f"loss({b}) {float(out[f'{case}.dpo.loss.{b}']):.6f}" for b in C.BETAS))
    assert abs(float(out[f"{case}.dpo.loss.1.0"]) - np.log(2.0)) > 3e-2 and (z > 0).any() and (z < 0).any(), z

    path = os.path.join(HERE, "qwen3_train.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
