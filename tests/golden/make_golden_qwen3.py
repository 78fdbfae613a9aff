"""Generate tests/golden/qwen3.npz by running the REAL reference's Qwen3Model on the CPU.  The model lives in a notebook
cell (Examples/simple_vllm.ipynb of the reference checkout): the cell is read and executed at run time only, filled with
the deterministic recipe (cases_qwen3.py), and only inputs' outputs are stored (int / float arrays plus one string array
per case: the reference's state_dict keys).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_qwen3.py <reference checkout>

The cell imports flash_attn; a stand-in module written here supplies flash_attn_varlen_func as dense causal attention
per segment in fp32 math, so the reference's own Qwen3Model.forward runs in its prefill branch (is_decoding False): one
packed forward over whole sequences, K/V scattered into scratch pages that nothing reads.

Keys (case = q | r | n | t, see cases_qwen3.py):
  <case>.keys            state_dict keys of the reference model, sorted
  <case>.prompt.seed     the first seed of cases_qwen3.prompts whose greedy run has every top-2 margin above 4e-3 (100
                         times what the fp32 logits bar of the GPU test, 2e-5 of logits near 2, allows)
  <case>.prompt          (2, 8) prompt ids
  <case>.greedy          (2, 16) greedy ids: 16 full forwards over the growing sequences
  <case>.logits          (2, 16, vocab / 4) fp32 logits at the 16 positions that produced them (cases_qwen3.sub_v)
The maker asserts the margins and that the reference's own bf16 forward stays within rel_err 3e-2 of its fp32 logits at
the same positions: the bf16 bar of the GPU test is attainable by the reference alone.
"""
import json
import os
import sys
import types

os.environ["MKL_CBWR"] = "COMPATIBLE"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import cases_qwen3 as C  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)
BLOCK = 16
SEARCH_MARGIN = 4e-3


def varlen_causal(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=True, **_):
    """flash_attn_varlen_func for self-attention over packed segments: q (T, h, dh), k / v (T, hk, dh) -> (T, h, dh)."""
    assert causal and torch.equal(cu_seqlens_q, cu_seqlens_k)
    h, hk = q.shape[1], k.shape[1]
    out = torch.empty_like(q)
    cu = cu_seqlens_q.tolist()
    for a, b in zip(cu[:-1], cu[1:]):
        qs = q[a:b].float().transpose(0, 1)                                   # (h, n, dh)
        ks = k[a:b].float().transpose(0, 1).repeat_interleave(h // hk, dim=0)
        vs = v[a:b].float().transpose(0, 1).repeat_interleave(h // hk, dim=0)
        s = qs @ ks.transpose(1, 2) / (q.shape[-1] ** 0.5)
        s = s.masked_fill(torch.ones(b - a, b - a, dtype=torch.bool).triu(1), float("-inf"))
        out[a:b] = (torch.softmax(s, dim=-1) @ vs).transpose(0, 1).to(q.dtype)
    return out


def reference_classes(checkout):
    """Execute the notebook's first cell that defines Qwen3Model -> its namespace."""
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


def forward(m, rows):
    """The reference's packed prefill forward over whole sequences (a list of id lists) -> logits per sequence."""
    cfg = m.cfg_for_maker
    lens = [len(r) for r in rows]
    cu = np.concatenate([[0], np.cumsum(lens)])
    pos = torch.cat([torch.arange(n) for n in lens])
    nblk = sum((n + BLOCK - 1) // BLOCK for n in lens)
    shape = (nblk, BLOCK, cfg["n_kv_groups"], cfg["head_dim"])
    kcs = [torch.zeros(shape, dtype=cfg["dtype"]) for _ in range(cfg["n_layers"])]
    vcs = [torch.zeros(shape, dtype=cfg["dtype"]) for _ in range(cfg["n_layers"])]
    slots, first = [], 0
    for n in lens:
        slots.append(first * BLOCK + torch.arange(n))
        first += (n + BLOCK - 1) // BLOCK
    metadata = {"is_decoding": False, "slot_mapping": torch.cat(slots), "block_size": BLOCK,
                "cu_seqlens": torch.tensor(cu, dtype=torch.int32), "max_seqlen": max(lens),
                "cos": m.cos_buf[pos].unsqueeze(1), "sin": m.sin_buf[pos].unsqueeze(1)}
    with torch.no_grad():
        lg = m(torch.tensor([t for r in rows for t in r]), kcs, vcs, metadata)
    return [lg[a:b] for a, b in zip(cu[:-1], cu[1:])]


def greedy(m, prompt):
    rows, margin = [list(r) for r in prompt.tolist()], np.inf
    for _ in range(C.GREEDY_NEW):
        for r, lg in zip(rows, forward(m, rows)):
            top = lg[-1].float().topk(2).values
            margin = min(margin, float(top[0] - top[1]))
            r.append(int(lg[-1].argmax()))
    return rows, margin


def rel_err(got, want):
    got, want = got.float().numpy(), want.float().numpy()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


def build(ns, case, dtype):
    m = C.build(ns["Qwen3Model"], case, dtype)
    m.cfg_for_maker = C.cfg(case, dtype)
    return m


def main():
    ns = reference_classes(sys.argv[1])
    out = {}
    for case in C.CASES:
        m = build(ns, case, torch.float32)
        out[f"{case}.keys"] = np.array(sorted(m.state_dict().keys()))
        for seed in range(64):
            prompt = C.prompts(case, seed)
            rows, margin = greedy(m, prompt)
            if margin > SEARCH_MARGIN:
                break
        assert margin > 1e-3, margin
        # the logits that produced the 16 ids: positions PROMPT - 1 .. PROMPT + 14 of the finished sequences
        full = torch.stack([lg[C.PROMPT - 1:] for lg in forward(m, [r[:-1] for r in rows])])
        assert full.shape[1] == C.GREEDY_NEW
        assert torch.equal(full.argmax(-1), torch.tensor(rows)[:, C.PROMPT:])
        mb = build(ns, case, torch.bfloat16)
        fullb = torch.stack([lg[C.PROMPT - 1:] for lg in forward(mb, [r[:-1] for r in rows])])
        gap = rel_err(fullb, full)
        print(f"{case}: prompt seed {seed}, smallest top-2 margin {margin:.3e}, largest |logit| {float(full.abs().max()):.3f}, "
              f"reference bf16 vs fp32 logits {gap:.2e}")
        assert gap < 3e-2, gap
        out[f"{case}.prompt.seed"] = np.array([seed], dtype=np.int64)
        out[f"{case}.prompt"] = prompt
        out[f"{case}.greedy"] = np.array(rows, dtype=np.int64)[:, C.PROMPT:]
        out[f"{case}.logits"] = C.sub_v(full).numpy().astype(np.float32).copy()
    path = os.path.join(HERE, "qwen3.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
