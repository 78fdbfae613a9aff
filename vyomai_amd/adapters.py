"""Per-request LoRA adapters for the serving engine: the weights of the reference's LoraLinear
(VyomAI/layers/adapters.py: linear(x) + alpha * F.linear(F.linear(x, lora_a), lora_b)) of many fine-tuned models, held
next to ONE copy of the base weights and added per row of a serving step (vy_lora_shrink / vy_lora_expand, the rule:
include/vyom_hip.h).  serving.ContinuousBatchEngine(..., adapters=store) and add_sequence(..., adapter="name") pick one
per request.  DoRA (which renormalises the whole weight, so it is no additive per-request delta) is refused there: a
DoRA model is served merged.  The second half of this file is the training side: the reference's LoraLinear and
DoraLinear wrappers, add_lora / lora_state_dict / merge_lora / disable_lora and their DoRA counterparts for
ModelForCausalLM (the forward and backward of a wrapped layer: lora_train.py, dora_train.py); the LoRA functions also
take an EncoderModel or a module holding one (encoder_lora_train.py).

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
# the post-LN encoder block (EncoderModel.all_layer[l]; training only: encoder_lora_train.py).  The reference's names
# are BERT's -- attention.output.dense, intermediate.dense, output.dense -- and these are this package's for the same
# linears.
_ENCODER = {"qkv": ("attention.query", "attention.key", "attention.value"), "o": ("attention.out.dense",),
            "ffn1": ("feed_forward.intermediate",), "ffn2": ("feed_forward.out",)}
ENCODER_GROUPS = ("qkv", "o", "ffn1", "ffn2")


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


# ------------------------------------------------------------------------------------------------------------------
# Training through adapters: the reference's LoraLinear wrapper and what prepares a ModelForCausalLM for it.  The
# forward and backward of a wrapped layer are lora_train.py's (DecoderLayer picks them up from the wrapped modules).
# ------------------------------------------------------------------------------------------------------------------

MAX_TRAIN_RANK = 64      # vy_lora_wgrad: r_pad is 32 or 64
ALL_TARGETS = tuple(p for g in GROUPS for p in _CAUSAL_LM[g])
ENCODER_TARGETS = tuple(p for g in ENCODER_GROUPS for p in _ENCODER[g])
# Examples/adapters.ipynb wraps query, value, attention.output.dense, intermediate.dense and output.dense: key is off
NOTEBOOK_ENCODER_TARGETS = tuple(p for p in ENCODER_TARGETS if p != "attention.key")


class LoraLinear(torch.nn.Module):
    """linear(x) + alpha * (x @ lora_a.T) @ lora_b.T around an nn.Linear, with the reference's constructor, attribute
    and state_dict names (VyomAI/layers/adapters.py: `linear`, `lora_a` (rank, in) ~ N(0, 1 / rank), `lora_b`
    (out, rank) zero, `dropout`).  `weight` / `bias` forward to the wrapped linear, so the packed-QKV and gate/up
    machinery keeps reading the base weights; the low-rank term is added by the layer that owns the projection
    (DecoderLayer: lora_train.py).  Called on its own it runs under torch.no_grad() only."""

    def __init__(self, linear_layer, rank: int = 32, alpha=1, lora_dropout: float = 0.0) -> None:
        super().__init__()
        if not isinstance(linear_layer, torch.nn.Linear):
            raise ValueError(f"LoraLinear wraps an nn.Linear, not a {type(linear_layer).__name__} (wrapping twice?)")
        if lora_dropout:
            raise ValueError(f"lora_dropout {lora_dropout}: dropout on the adapter's output has no kernel here; use 0.0")
        if int(rank) != rank or not 1 <= rank <= MAX_TRAIN_RANK:
            raise ValueError(f"rank {rank} must be an integer from 1 to {MAX_TRAIN_RANK}")
        self.linear = linear_layer
        self.in_features, self.out_features = linear_layer.in_features, linear_layer.out_features
        if self.in_features % 32 or self.out_features % 16:
            raise ValueError(f"in_features {self.in_features} must be a multiple of 32 and out_features "
                             f"{self.out_features} a multiple of 16 (vy_lora_shrink / vy_lora_expand)")
        self.rank, self.alpha = int(rank), alpha
        w = linear_layer.weight
        self.lora_a = torch.nn.Parameter(torch.randn(self.rank, self.in_features, dtype=w.dtype, device=w.device)
                                         * self.rank ** -0.5)
        self.lora_b = torch.nn.Parameter(torch.zeros(self.out_features, self.rank, dtype=w.dtype, device=w.device))
        self.dropout = torch.nn.Dropout(lora_dropout)
        self._off = 0            # depth of disable_lora() contexts

    weight = property(lambda self: self.linear.weight)
    bias = property(lambda self: self.linear.bias)
    enabled = property(lambda self: self._off == 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from . import lora_train
        return lora_train.lora_linear_forward(self, x)

    def extra_repr(self) -> str:
        return f"rank={self.rank}, alpha={self.alpha}"


def _causal_lm(model, what: str):
    from .models.custom_transformer import ModelForCausalLM
    if not isinstance(model, ModelForCausalLM):
        raise ValueError(f"{what} prepares a ModelForCausalLM, not a {type(model).__name__}: only its pre-norm blocks "
                         "have a training path through adapters")
    return list(model.model.layers[: model.config.num_hidden_layers])


class _Family:
    """What add_lora and its companions need to know about a model: the key prefix of layer l ({} for l), the layers,
    group -> part paths, the groups in order and every target path."""

    def __init__(self, prefix, layers, table, groups):
        self.prefix, self.layers, self.table, self.groups = prefix, layers, table, groups
        self.targets = tuple(p for g in groups for p in table[g])
        self.encoder = table is _ENCODER
        self.default = NOTEBOOK_ENCODER_TARGETS if self.encoder else self.targets


def _family(model, what: str) -> _Family:
    """ModelForCausalLM; an EncoderModel, or a module that holds one as a direct child (EncoderForSequenceClassification
    .model, EncoderForMaskedLM.encoder).  Everything else is refused."""
    from .models.custom_transformer import ModelForCausalLM
    from .models.encoder import EncoderModel
    if isinstance(model, ModelForCausalLM):
        return _Family("model.layers.{}.", _causal_lm(model, what), _CAUSAL_LM, GROUPS)
    if isinstance(model, EncoderModel):
        return _Family("all_layer.{}.", list(model.all_layer), _ENCODER, ENCODER_GROUPS)
    if isinstance(model, torch.nn.Module):
        held = [(n, c) for n, c in model.named_children() if isinstance(c, EncoderModel)]
        if len(held) == 1:
            return _Family(held[0][0] + ".all_layer.{}.", list(held[0][1].all_layer), _ENCODER, ENCODER_GROUPS)
    raise ValueError(f"{what} prepares a ModelForCausalLM, not a {type(model).__name__}: only its pre-norm blocks and the "
                     "post-LN blocks of an EncoderModel (alone, or held by EncoderForSequenceClassification / "
                     "EncoderForMaskedLM) have a training path through adapters.  For a DecoderModel, a vision encoder or "
                     "an encoder-decoder, fold a trained update into the weights (W + alpha * lora_b @ lora_a) and run "
                     "the plain model")


def _wrapped(model, cls=None, what: str = "LoRA"):
    """-> [(owner module, attribute, key path, wrapper)] of every projection wrapped in a `cls` (LoraLinear), in layer
    order."""
    cls = LoraLinear if cls is None else cls
    fam = _family(model, what)
    out = []
    for l, layer in enumerate(fam.layers):
        for path in fam.targets:
            owner_path, _, attr = path.rpartition(".")
            owner = functools.reduce(getattr, owner_path.split("."), layer)
            m = getattr(owner, attr)
            if isinstance(m, cls):
                out.append((owner, attr, fam.prefix.format(l) + path, m))
    return out


def add_lora(model, rank: int = 32, alpha=1.0, targets=None):
    """Wrap the projections `targets` of every layer in a LoraLinear and freeze every parameter the model has at that
    moment, as Examples/adapters.ipynb does -> the model.  A ModelForCausalLM takes the paths of _CAUSAL_LM
    ("self_attn.q_proj", ..., "mlp.down_proj"; default: all seven); an EncoderModel -- or a module holding one:
    EncoderForSequenceClassification, EncoderForMaskedLM -- those of _ENCODER ("attention.query", "attention.key",
    "attention.value", "attention.out.dense", "feed_forward.intermediate", "feed_forward.out"; default: the notebook's
    five, key off).  Any non-empty subset.  What is created afterwards -- the notebook's classification head -- stays
    trainable; add_lora(classifier.model) keeps an existing head trainable.  ValueError: another model class, an unknown
    or empty target list, a model that is already wrapped."""
    fam = _family(model, "add_lora")
    layers = fam.layers
    targets = fam.default if targets is None else tuple(targets)
    unknown = [t for t in targets if t not in fam.targets]
    if unknown or not targets or len(set(targets)) != len(targets):
        raise ValueError(f"targets {list(targets)} must be a non-empty subset of {list(fam.targets)} without repeats")
    if _wrapped(model):
        raise ValueError("the model already carries LoRA adapters: merge_lora(model) first")
    if _wrapped(model, DoraLinear):
        raise ValueError("the model carries DoRA adapters, and a layer runs one kind: merge_dora(model) first")
    if int(rank) != rank or not 1 <= rank <= MAX_TRAIN_RANK:
        raise ValueError(f"rank {rank} must be an integer from 1 to {MAX_TRAIN_RANK}")
    for g in fam.groups:      # (everything is checked before anything is changed)
        shapes = [functools.reduce(getattr, p.split("."), layers[0]).weight.shape for p in fam.table[g]]
        if not any(p in targets for p in fam.table[g]):
            continue
        if sum(s[0] for s in shapes) % 32 or any(s[0] % 16 or s[1] % 32 for s in shapes):
            raise ValueError(f"the packed {g} projection has parts {[tuple(s) for s in shapes]}: in_features must be a "
                             "multiple of 32, every out_features of 16 and their sum of 32 (the adapter's backward "
                             "contracts over the packed width: vy_lora_shrink)")
    for p in model.parameters():
        p.requires_grad_(False)
    for layer in layers:
        for path in targets:
            owner_path, _, attr = path.rpartition(".")
            owner = functools.reduce(getattr, owner_path.split("."), layer)
            setattr(owner, attr, LoraLinear(getattr(owner, attr), rank=rank, alpha=alpha))
    return model


def lora_state_dict(model) -> Dict[str, torch.Tensor]:
    """Exactly the lora_a / lora_b entries of the wrapped model's state_dict (detached copies): what
    LoraAdapters.load(name, lora_state_dict(model), alpha) takes."""
    out = {}
    for _, _, key, m in _wrapped(model):
        out[key + ".lora_a"] = m.lora_a.detach().clone()
        out[key + ".lora_b"] = m.lora_b.detach().clone()
    return out


def merge_lora(model):
    """W += alpha * lora_b @ lora_a in fp32 into every wrapped linear, and the plain nn.Linear back in its place -> the
    model (the re-association of tests/golden/make_golden_lora.py's merged()).  requires_grad flags stay as they are."""
    with torch.no_grad():
        for owner, attr, _, m in _wrapped(model):
            w = m.linear.weight
            w += (float(m.alpha) * (m.lora_b.detach().float() @ m.lora_a.detach().float())).to(w.dtype)
            setattr(owner, attr, m.linear)
    return model


class disable_lora:
    """Context manager: inside it the wrapped model computes the base model (a DPO run scores its reference with the
    same weights).  Nests; restores on exceptions."""

    def __init__(self, model):
        self.mods = [m for *_, m in _wrapped(model)]

    def __enter__(self):
        for m in self.mods:
            m._off += 1
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m._off -= 1
        return False


# ------------------------------------------------------------------------------------------------------------------
# DoRA: the reference's DoraLinear re-parameterises the weight, W' = dora_m * D / ||D||_col with D = W + dora_a @ dora_b.
# All of its arithmetic is weight-sized: dora_train.py composes W' once per optimizer step (vy_dora_compose), runs the
# plain fused block on it and turns dL/dW' into the three small gradients (vy_dora_bwd).
# ------------------------------------------------------------------------------------------------------------------

MAX_DORA_RANK = 64       # vy_dora_compose / vy_dora_bwd


def _dora_shape_error(in_f: int, out_f: int) -> Optional[str]:
    if in_f % 8 or out_f % 8:
        return (f"in_features {in_f} and out_features {out_f} must be multiples of 8 (vy_dora_compose / vy_dora_bwd)")
    return None


class DoraLinear(torch.nn.Module):
    """F.linear(x, dora_m * D / ||D||_2 over dim 0, bias) with D = linear.weight + dora_a @ dora_b around an nn.Linear,
    with the reference's constructor, attribute and state_dict names (VyomAI/layers/adapters.py:50-75: `linear`,
    `dora_m` (1, in) = the column norms of the weight, `dora_a` (out, rank) ~ N(0, 1 / rank), `dora_b` (rank, in) zero).
    `weight` / `bias` forward to the wrapped linear; the layer that owns the projection composes the weight
    (DecoderLayer: dora_train.py).  Called on its own it runs under torch.no_grad() only."""

    def __init__(self, linear_layer, rank: int = 32) -> None:
        super().__init__()
        if not isinstance(linear_layer, torch.nn.Linear):
            raise ValueError(f"DoraLinear wraps an nn.Linear, not a {type(linear_layer).__name__} (wrapping twice?)")
        if int(rank) != rank or not 1 <= rank <= MAX_DORA_RANK:
            raise ValueError(f"rank {rank} must be an integer from 1 to {MAX_DORA_RANK}")
        self.linear = linear_layer
        self.in_features, self.out_features = linear_layer.in_features, linear_layer.out_features
        bad = _dora_shape_error(self.in_features, self.out_features)
        if bad:
            raise ValueError(bad)
        self.rank = int(rank)
        w = linear_layer.weight
        with torch.no_grad():
            self.dora_m = torch.nn.Parameter(w.detach().norm(p=2, dim=0, keepdim=True))
        self.dora_a = torch.nn.Parameter(torch.randn(self.out_features, self.rank, dtype=w.dtype, device=w.device)
                                         * self.rank ** -0.5)
        self.dora_b = torch.nn.Parameter(torch.zeros(self.rank, self.in_features, dtype=w.dtype, device=w.device))
        self._off = 0            # depth of disable_dora() contexts

    weight = property(lambda self: self.linear.weight)
    bias = property(lambda self: self.linear.bias)
    enabled = property(lambda self: self._off == 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from . import dora_train
        return dora_train.dora_linear_forward(self, x)

    def extra_repr(self) -> str:
        return f"rank={self.rank}"


def add_dora(model, rank: int = 32, targets=ALL_TARGETS):
    """Wrap the projections `targets` (paths of _CAUSAL_LM, any non-empty subset of the seven) of every layer of a
    ModelForCausalLM in a DoraLinear and freeze every other parameter, as Examples/adapters.ipynb does -> the model.
    ValueError, before anything is changed: another model class, an unknown or empty target list, a bad rank or
    shape, a model that already carries LoRA or DoRA wrappers."""
    layers = _causal_lm(model, "add_dora")
    targets = tuple(targets)
    unknown = [t for t in targets if t not in ALL_TARGETS]
    if unknown or not targets or len(set(targets)) != len(targets):
        raise ValueError(f"targets {list(targets)} must be a non-empty subset of {list(ALL_TARGETS)} without repeats")
    if _wrapped(model):
        raise ValueError("the model carries LoRA adapters, and a layer runs one kind: merge_lora(model) first")
    if _wrapped(model, DoraLinear):
        raise ValueError("the model already carries DoRA adapters: merge_dora(model) first")
    if int(rank) != rank or not 1 <= rank <= MAX_DORA_RANK:
        raise ValueError(f"rank {rank} must be an integer from 1 to {MAX_DORA_RANK}")
    for layer in layers:
        for path in targets:
            lin = functools.reduce(getattr, path.split("."), layer)
            if not isinstance(lin, torch.nn.Linear):
                raise ValueError(f"{path} is a {type(lin).__name__}, not an nn.Linear")
            bad = _dora_shape_error(lin.in_features, lin.out_features)
            if bad:
                raise ValueError(f"{path}: {bad}")
    for p in model.parameters():
        p.requires_grad_(False)
    for layer in layers:
        for path in targets:
            owner_name, attr = path.split(".")
            owner = getattr(layer, owner_name)
            setattr(owner, attr, DoraLinear(getattr(owner, attr), rank=rank))
    return model


def dora_state_dict(model) -> Dict[str, torch.Tensor]:
    """Exactly the dora_m / dora_a / dora_b entries of the wrapped model's state_dict (detached copies)."""
    out = {}
    for _, _, key, m in _wrapped(model, DoraLinear, "DoRA"):
        for leaf in ("dora_m", "dora_a", "dora_b"):
            out[f"{key}.{leaf}"] = getattr(m, leaf).detach().clone()
    return out


def merge_dora(model):
    """W <- dora_m * D / ||D||_col with D = W + dora_a @ dora_b, in fp32, into every wrapped linear, and the plain
    nn.Linear back in its place -> the model: what generate() and the serving engine run.  requires_grad flags stay as
    they are."""
    with torch.no_grad():
        for owner, attr, _, m in _wrapped(model, DoraLinear, "DoRA"):
            w = m.linear.weight
            d = w.detach().float() + m.dora_a.detach().float() @ m.dora_b.detach().float()
            w.copy_((m.dora_m.detach().float() * (d / d.norm(p=2, dim=0, keepdim=True))).to(w.dtype))
            setattr(owner, attr, m.linear)
    return model


class disable_dora:
    """Context manager: inside it the wrapped model computes the base model and nothing is composed (a DPO run scores
    its reference with the same weights).  Nests; restores on exceptions."""

    def __init__(self, model):
        self.mods = [m for *_, m in _wrapped(model, DoraLinear, "DoRA")]

    def __enter__(self):
        for m in self.mods:
            m._off += 1
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m._off -= 1
        return False
