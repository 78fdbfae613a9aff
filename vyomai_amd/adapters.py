"""Per-request LoRA adapters for the serving engine: the weights of the reference's LoraLinear
(VyomAI/layers/adapters.py: linear(x) + alpha * F.linear(F.linear(x, lora_a), lora_b)) of many fine-tuned models, held
next to ONE copy of the base weights and added per row of a serving step (vy_lora_shrink / vy_lora_expand, the rule:
include/vyom_hip.h).  serving.ContinuousBatchEngine(..., adapters=store) and add_sequence(..., adapter="name") pick one
per request.  Serving only: nothing here trains, and DoRA (which renormalises the whole weight, so it is no additive
per-request delta) is refused.

Layout.  Per layer and projection group -- qkv, o, gate_up, down: the four GEMMs of forward_paged -- the store keeps
A (slots, parts * r_pad, K) and B (slots, N, r_pad) in the compute dtype, r_pad = max_rank rounded up to 32.  A packed
group stacks its parts' lora_a ([A_q; A_k; A_v], [A_gate; A_up]: one shrink serves the whole packed GEMM) and their
lora_b along N; a part's rank is padded with zeros to r_pad and a part that an adapter leaves alone is all zeros, so any
subset of the seven projections and any rank up to max_rank share the one launch pair.  alpha is fp32 (slots,)."""
from __future__ import annotations

import functools
import itertools
from typing import Dict, List, Optional, Tuple

import torch

# group -> its parts, per model family, by the reference's attribute names (the state_dict keys of a model whose
# linears were wrapped as in Examples/adapters.ipynb: <path of the wrapped nn.Linear>.lora_a / .lora_b)
_CAUSAL_LM = {"qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "o": ("self_attn.o_proj",),
              "gate_up": ("mlp.gate_proj", "mlp.up_proj"), "down": ("mlp.down_proj",)}
_QWEN3 = {"qkv": ("att.W_query", "att.W_key", "att.W_value"), "o": ("att.out_proj",), "gate_up": ("ff.fc1", "ff.fc2"),
          "down": ("ff.fc3",)}
GROUPS = ("qkv", "o", "gate_up", "down")


def _layers_of(model) -> Tuple[str, list, dict]:
    """-> (key prefix of layer l with {} for l, the layers, group -> part paths)."""
    if hasattr(model, "trf_blocks"):
        return "trf_blocks.{}.", list(model.trf_blocks), _QWEN3
    inner = getattr(model, "model", None)
    if inner is not None and hasattr(inner, "layers"):
        return "model.layers.{}.", list(inner.layers[: model.config.num_hidden_layers]), _CAUSAL_LM
    raise ValueError(f"LoraAdapters serves ModelForCausalLM and Qwen3Model, not {type(model).__name__}")


class LoraAdapters:
    """The adapter store of one model.  load(name, state_dict, alpha) -> slot; unload(name); slots / uid by name.
    device / dtype default to the model's parameters' device and its compute dtype; device="cpu" holds the same tensors
    for host-side work (the engine's planner needs only names, slots and uids)."""

    def __init__(self, model, max_adapters: int, max_rank: int = 32, device=None, dtype=None):
        if int(max_adapters) != max_adapters or max_adapters < 1:
            raise ValueError(f"max_adapters {max_adapters} must be a positive integer")
        if int(max_rank) != max_rank or max_rank < 1:
            raise ValueError(f"max_rank {max_rank} must be a positive integer")
        self.max_adapters, self.max_rank = int(max_adapters), int(max_rank)
        self.r_pad = (self.max_rank + 31) // 32 * 32
        prefix, layers, groups = _layers_of(model)
        p0 = next(model.parameters())
        if dtype is None:
            from .serving import _compute_dtype
            dtype = _compute_dtype(model)
        self.device, self.dtype = torch.device(p0.device if device is None else device), dtype
        # (layer, group) -> [(key path, first column, out, in)], and key path -> (layer, group, part)
        self.parts: Dict[Tuple[int, str], List[Tuple[str, int, int, int]]] = {}
        self.where: Dict[str, Tuple[int, str, int]] = {}
        self.A: List[Dict[str, torch.Tensor]] = []
        self.B: List[Dict[str, torch.Tensor]] = []
        self.boundaries: List[Dict[str, Tuple[int, ...]]] = []
        for l, layer in enumerate(layers):
            A, B, bounds = {}, {}, {}
            for g in GROUPS:
                col, rows = 0, []
                for k, path in enumerate(groups[g]):
                    lin = functools.reduce(getattr, path.split("."), layer)
                    out_f, in_f = lin.weight.shape
                    rows.append((prefix.format(l) + path, col, out_f, in_f))
                    self.where[prefix.format(l) + path] = (l, g, k)
                    col += out_f
                K = rows[0][3]
                name = f"{prefix.format(l)}{g}"
                if any(r[3] != K for r in rows) or K % 32 or any(r[2] % 16 for r in rows):
                    raise ValueError(f"{name}: in_features {K} must be a multiple of 32 and every out_features "
                                     f"{[r[2] for r in rows]} a multiple of 16 (vy_lora_shrink / vy_lora_expand)")
                self.parts[(l, g)] = rows
                A[g] = torch.zeros((self.max_adapters, len(rows) * self.r_pad, K), dtype=dtype, device=self.device)
                B[g] = torch.zeros((self.max_adapters, col, self.r_pad), dtype=dtype, device=self.device)
                bounds[g] = tuple(r[1] for r in rows[1:])
            self.A.append(A)
            self.B.append(B)
            self.boundaries.append(bounds)
        self.alpha = torch.zeros(self.max_adapters, dtype=torch.float32, device=self.device)
        self.slots: Dict[str, int] = {}          # name -> slot
        self.uid: Dict[str, int] = {}            # name -> the id of this load: a name loaded again is another adapter
        self.held: Dict[str, int] = {}           # name -> waiting or running requests that hold it
        self._uids = itertools.count(1)

    # ---- loading ---------------------------------------------------------------------------------------------
    def load(self, name: str, state_dict, alpha: float = 1.0) -> int:
        """The adapter of a state_dict with the reference's keys: `<linear>.lora_a` (rank, in) and `<linear>.lora_b`
        (out, rank).  The wrapped base weights (`.linear.weight`, `.linear.bias`) and every other key are ignored; the
        base model must be the one this store was built for.  lora_dropout is the identity at inference.  -> the slot.
        ValueError, naming the key: DoRA keys, a lora_a without lora_b (or the reverse), a key that names no known
        projection, a wrong shape, a rank above max_rank; also a name loaded twice and no free slot.  Nothing is
        written unless everything is valid."""
        if name in self.slots:
            raise ValueError(f"adapter {name!r} is already loaded (unload it first)")
        pairs: Dict[str, dict] = {}
        for key in state_dict:
            leaf = key.rsplit(".", 1)[-1]
            if leaf.startswith("dora_"):
                raise ValueError(f"{key}: DoRA renormalises the whole weight, so it is no additive per-request delta; only "
                                 "LoRA adapters can be served")
            if leaf in ("lora_a", "lora_b"):
                pairs.setdefault(key[: -len(leaf) - 1], {})[leaf] = key
        if not pairs:
            raise ValueError(f"adapter {name!r}: the state dict has no lora_a / lora_b keys")
        todo = []
        for path, found in pairs.items():
            for leaf, other in (("lora_a", "lora_b"), ("lora_b", "lora_a")):
                if other not in found:
                    raise ValueError(f"{found[leaf]} has no {path}.{other}")
            if path not in self.where:
                raise ValueError(f"{found['lora_a']} names no known projection (known: {sorted(self.where)[:7]} ...)")
            l, g, k = self.where[path]
            _, col, out_f, in_f = self.parts[(l, g)][k]
            a, b = torch.as_tensor(state_dict[found["lora_a"]]), torch.as_tensor(state_dict[found["lora_b"]])
            if a.dim() != 2 or a.shape[1] != in_f or a.shape[0] < 1:
                raise ValueError(f"{found['lora_a']} has shape {tuple(a.shape)}, expected (rank, {in_f})")
            rank = a.shape[0]
            if rank > self.max_rank:
                raise ValueError(f"{found['lora_a']} has rank {rank}, above max_rank {self.max_rank}")
            if tuple(b.shape) != (out_f, rank):
                raise ValueError(f"{found['lora_b']} has shape {tuple(b.shape)}, expected ({out_f}, {rank})")
            todo.append((l, g, k, col, out_f, rank, a, b))
        free = sorted(set(range(self.max_adapters)) - set(self.slots.values()))
        if not free:
            raise ValueError(f"adapter {name!r}: all {self.max_adapters} slots are taken")
        slot = free[0]
        self._clear(slot)
        with torch.no_grad():
            for l, g, k, col, out_f, rank, a, b in todo:
                r0 = k * self.r_pad
                self.A[l][g][slot, r0:r0 + rank] = a.detach().to(device=self.device, dtype=self.dtype)
                self.B[l][g][slot, col:col + out_f, :rank] = b.detach().to(device=self.device, dtype=self.dtype)
            self.alpha[slot] = float(alpha)
        self.slots[name], self.uid[name], self.held[name] = slot, next(self._uids), 0
        return slot

    def _clear(self, slot: int) -> None:
        with torch.no_grad():
            for A, B in zip(self.A, self.B):
                for g in GROUPS:
                    A[g][slot].zero_()
                    B[g][slot].zero_()
            self.alpha[slot] = 0.0

    def unload(self, name: str) -> None:
        """The slot becomes free.  ValueError for an unknown name and while a waiting or running request holds it."""
        if name not in self.slots:
            raise ValueError(f"adapter {name!r} is not loaded")
        if self.held[name]:
            raise ValueError(f"adapter {name!r} is held by {self.held[name]} waiting or running request(s)")
        del self.slots[name], self.uid[name], self.held[name]

    # ---- what the engine and the models call -----------------------------------------------------------------
    def acquire(self, name: str) -> None:
        if name not in self.slots:
            raise ValueError(f"adapter {name!r} is not loaded (loaded: {sorted(self.slots)})")
        self.held[name] += 1

    def release(self, name: str) -> None:
        self.held[name] -= 1

    def delta_(self, lora: dict, layer: int, group: str, y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """y += the adapters' delta of this layer's `group` GEMM over x, for the rows of lora["tiles"]."""
        from . import ops
        return ops.lora_delta_(y, x, self.A[layer][group], self.B[layer][group], self.alpha, lora["tiles"],
                               lora["n_tiles"], self.boundaries[layer][group], name=f"layer {layer} {group}")


def layer_delta(metadata: dict, layer: int):
    """-> f(group, y, x) that adds the step's LoRA delta behind one of the layer's GEMMs, or None in a step without
    adapted rows (metadata has no "lora": the forward launches exactly what it launches without a store)."""
    lora: Optional[dict] = metadata.get("lora")
    if lora is None:
        return None
    return functools.partial(lora["adapters"].delta_, lora, layer)
