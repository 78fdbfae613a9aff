"""What every model behind serving.ContinuousBatchEngine does the same way in a step of `forward_paged`: the attention
over the step's packed rows once a layer's K/V rows are in their pages, and the logits of the rows the engine samples
from.  The per-layer bodies (norms, the packed QKV projection, which rope-write op, the MLP) stay in the models."""
from __future__ import annotations

import torch

from .. import ops
from .attention import _shadow


def page_scales(kv_mgr, layer: int) -> dict:
    """The keywords the paged attention ops take for layer `layer` of an fp8 manager; none for an unquantised one."""
    if getattr(kv_mgr, "k_scale", None) is None:
        return {}
    return {"k_scale": kv_mgr.k_scale[layer], "v_scale": kv_mgr.v_scale[layer]}


def paged_step_attention(qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, metadata: dict, h: int, hk: int,
                         dh: int, **scales) -> torch.Tensor:
    """Attention of one layer over the step's packed rows qkv (T, (h + 2 hk) dh), rotated and already written to the
    pages kc / vc -> o (T, h dh).  vy_attn_paged_decode serves the rows with one query token; the prefill rows take ONE
    vy_attn_paged_prefill through the block tables (metadata["prefill_varlen"]: no gather, no loop, a segment may be a
    chunk in the middle of its prompt) or else causal vy_attn_fwd per sequence, straight on its slice of the packed
    buffer or with start_pos = prefix_len against its gathered pages when it starts from cached prefix blocks.
    scales: k_scale= / v_scale= of fp8 pages (page_scales), which only the two paged kernels read."""
    o = torch.empty((qkv.shape[0], h * dh), dtype=qkv.dtype, device=qkv.device)
    dec, pv = metadata["decode"], metadata.get("prefill_varlen")
    if dec is not None:
        ops.attention_paged_decode(qkv, kc, vc, dec["block_table"], dec["seqlens"], dec["max_seqlen"], h,
                                   q_rows=dec["rows"], out=o, **scales)
    if pv is not None:
        ops.attention_paged_prefill(qkv, kc, vc, pv["block_table"], pv["cu_q"], pv["ctx_lens"], pv["max_q"],
                                    pv["max_kv"], h, out=o, **scales)
    elif scales and metadata["prefill"]:
        raise ValueError("fp8 KV pages are read by the varlen prefill only (ContinuousBatchEngine(varlen_prefill=True))")
    for row0, rows, prefix_len, table in (() if pv is not None else metadata["prefill"]):
        seg = qkv[row0:row0 + rows]
        q4 = seg[:, :h * dh].view(rows, h, dh).permute(1, 0, 2).unsqueeze(0)
        if prefix_len:
            k3, v3 = ops.paged_gather(kc, vc, table, prefix_len + rows)
        else:
            k3 = seg[:, h * dh:(h + hk) * dh].view(rows, hk, dh).permute(1, 0, 2)
            v3 = seg[:, (h + hk) * dh:].view(rows, hk, dh).permute(1, 0, 2)
        ops.attention(q4, k3.unsqueeze(0), v3.unsqueeze(0), causal=True, start_pos=prefix_len,
                      out=o[row0:row0 + rows].unsqueeze(0))
    return o


def paged_step_logits(x: torch.Tensor, last_rows: torch.Tensor, norm, head_weight: torch.Tensor) -> torch.Tensor:
    """Logits (sequences, vocab) of rows `last_rows` of the step's hidden states x (T, d): the final norm and the head
    see one row per sequence whose rows reach its last token."""
    if last_rows.numel() == 0:    # every sequence of the step is a chunk short of its prompt's end
        return x.new_empty((0, head_weight.shape[0]))
    return ops.linear(norm(x.index_select(0, last_rows)), _shadow(head_weight, x.dtype))
