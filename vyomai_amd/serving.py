"""Paged KV cache and continuous batching for ModelForCausalLM: the engine of the reference's
Examples/simple_vllm.ipynb (its prefix-caching version) under the notebook's class names -- RadixNode, SequenceState,
PagedKVManager, ContinuousBatchEngine -- serving this package's own model through vy_paged_rope_write,
vy_attn_paged_decode, vy_paged_gather and vy_attn_fwd, or vy_attn_paged_prefill in their place
(ModelForCausalLM.forward_paged; Qwen3Model.forward_paged serves the notebook's own network).  The notebook decodes
greedily; here every request may bring its own SamplingParams, drawn in one vy_sample_rows launch per step (below).

The bookkeeping (tokens, block tables, slot mappings, the radix tree, the queues) lives on the host: the manager and the
scheduler run without a GPU, and a step uploads its packed metadata once and reads the step's ids back once.  Only the
pages (PagedKVManager.k_cache / v_cache) live on `device`.

Where this departs from the notebook:

1. Mixed steps.  A step that holds prefilling AND decoding sequences is sent by the notebook through
   flash_attn_varlen_func on the step's own q / k / v, so its decoding rows attend to themselves only.  Here every token
   attends to its sequence's whole cached context (paged decode for the rows with one query token, vy_attn_fwd per
   prefilling sequence).  Steps whose sequences are all in one phase are the same in both.
2. A waiting request leaves nothing behind.  The notebook's get_prefix_blocks raises ref_count while the scheduler only
   peeks at the head of the waiting room, and again on every later step.  Here match_prefix has no side effects and
   acquire() counts the references when the request is admitted.
3. At least one prompt token is computed: at most (len(prompt) - 1) // block_size blocks are matched.  A fully cached
   prompt in the notebook has an empty query segment and no logits row.
4. Evicting a block drops its subtree: the registrations of all descendants go with it and their blocks move from the
   evictable queue to the free list (a holder of a child holds the whole chain, so every descendant has ref_count 0).
   The notebook leaves block_to_node entries that point into a detached parent.
5. Admission on the request's whole life.  A request enters when the blocks of prompt + max_gen_len (less the matched
   ones) fit into what is free or evictable beyond what the running sequences may still claim, so a sequence the engine
   admitted never meets "KV Cache full!" half way.  The notebook admits on the prompt's blocks alone and has no
   preemption to recover with.  The price: a request that stops early on eos had blocks reserved that it never used,
   which lowers concurrency when the cache is tight.

As in the notebook: only blocks complete at allocation time (prompt blocks) are registered; free() moves registered
blocks to the evictable queue and the others to the free list; eviction is oldest-first; RuntimeError("KV Cache full!")
when nothing is free or evictable.

Beyond the notebook, both off by default (the default engine's schedule, metadata and launches are as described above):

* varlen_prefill: the step's rows are ordered decoding sequences first, and all prefill rows go through ONE
  vy_attn_paged_prefill launch per layer (metadata["prefill_varlen"]: cu_q, ctx_lens, block tables, in the step's one
  int32 upload) -- the notebook's single flash_attn_varlen_func call, with every key read from the pages, so neither the
  per-sequence loop nor the gather after a prefix hit remains.
* max_step_tokens = N >= max_batch_size (chunked prefill, implies varlen_prefill): every decoding sequence takes its one
  token first, the rest of the budget goes to the prefilling sequences in admission order, min(prompt tokens left,
  budget left) each; one that gets nothing sits the step out.  A chunk that stops short of its prompt's end emits no
  token and has no logits row; the sequence stays is_prefill and SequenceState.num_computed counts what the pages hold.
  N >= max_batch_size guarantees progress (while a sequence prefills, at most max_batch_size - 1 decode).
  Invariant: a block is in the radix tree only if its rows are written by the end of the step that registered it -- so
  a prompt block is registered in the step whose chunk writes its last row (PagedKVManager.allocate(state, upto)), also
  one that an earlier chunk allocated and left part filled.

Sampling (add_sequence(..., sampling=SamplingParams(...)); None or temperature 0: greedy).  A step whose emitting
sequences are all greedy is the greedy step: torch.argmax and one .tolist().  Otherwise ONE vy_sample_rows launch draws
for every logits row (greedy rows ride along with inv_temperature 0) before the same single .tolist(): the token is
argmax over the kept columns of logit / temperature + Gumbel noise, a draw from softmax(logits / temperature) over the
set TopKProcessor / NucleusProcessor keep.  The noise of a row is keyed by (the request's seed, the position of the
token being drawn, column) and by nothing else, so what a request generates from given logits does not depend on the
batch around it, on its row, on prefix-cache hits or on how its prompt was chunked.  A sampled step makes no additional
copy in either direction.

What a step uploads: two tensors, one int64 and one int32, whatever the step holds (_StepUploads).  A planner appends
named lists to them -- per forward (_PackedRows) ids and slots to the int64 one, positions, decode rows / lengths / block
tables and cu_q / ctx_lens / block tables of the varlen segments to the int32 one; then the logits rows, and the
sampling parameters of a step that draws (top_k and the bit patterns of inv_temperature / top_p as int32, seed and
position as int64) -- and every tensor of the step's metadata is a view into one of the two.

Speculative decoding (ContinuousBatchEngine(..., draft_model=, draft_kv_mgr=, num_speculative_tokens=g); off by default,
and then the engine's schedule, metadata, uploads and launches are the ones above).  A step lets the drafter propose up
to g tokens for every decoding sequence and the target judge them all in ONE forward: the reference's
speculative_generate (speculative_decoding.py:86-245) for every sequence of the batch at once, with each request's own
SamplingParams, on the pages.  One step:

1. schedule, allocate, upload -- once: all g draft rounds and the verification are planned on the host in advance and
   ride in the step's two uploads; draft token ids stay on the device from round to round.  The decoding sequences
   come first, those with the most drafts in front (g_s = min(g, max_total_len - num_tokens - 1), the reference's
   corrected_gamma), so the sequences of round j are always the first n_j.  Under max_step_tokens a decoding
   sequence takes 1 + g_s rows of the budget.
2. draft round 0: one draft_model.forward_paged over the step's prompt chunks (the target's segments, no logits rows)
   and, per decoding sequence, a varlen segment of the tokens the drafter has not computed yet (1, or 2 after a round
   whose drafts were all accepted: draft_computed[sid] counts what its pages hold); one vy_sample_rows, counter =
   position.
3. draft rounds 1 .. g - 1: plain decode rows, one vy_sample_rows each; a sequence with g_s <= j sits round j out.
4. verify: one target forward_paged over the prompt chunks and, per decoding sequence, the varlen segment [last token,
   d_0 .. d_{g_s - 1}] with ctx_len = num_tokens - 1, all of its rows in last_rows; then ONE vy_spec_verify launch
   (accept / reject / resample, include/vyom_hip.h) in which prompts that finish prefilling ride along with n_draft = 0
   -- their row is vy_sample_rows' draw, so a step without drafts emits what the plain engine emits.
5. ONE device-to-host copy carries accept, alt and the draft tokens; the host finds the first rejection, appends the
   accepted drafts and alt, cuts at the first stop token among them (reference :210-214), and retires what finished.

Only the pages (and scales) of draft_kv_mgr are used, indexed by the target manager's block tables and slots; its own
free list and tree stay idle.  Invariant: both models write the same slots in the same step, so a block the prefix
cache hands out holds valid rows of both models, and eviction and reuse overwrite both.  Speculative rows land only at
positions >= prompt_len, in blocks that are never registered: a rejected draft never touches a shared block, its slot is
simply overwritten later, and g_s keeps every write inside the blocks admission reserved.  The reference's
skip_sample_adjustment is not carried over.

LoRA adapters (ContinuousBatchEngine(..., adapters=LoraAdapters(...)) and add_sequence(..., adapter="name"); needs
varlen_prefill; off by default).  Requests with different adapters, or none, share the ONE packed forward over the ONE
copy of the base weights: _PackedRows records, while it builds the segments, the tiles (row0, nrows <= 16, slot) of the
adapted rows -- consecutive rows of one request, cut every 16: a decoding row is one tile, a verification segment of
g + 1 rows one (or two), a prompt chunk of n rows ceil(n / 16) -- and puts them into the step's int32 upload;
metadata["lora"] = {"tiles", "n_tiles", "adapters"} then makes forward_paged add the delta behind each of a layer's four
GEMMs (vy_lora_shrink / vy_lora_expand, include/vyom_hip.h).  The tile count is known on the host and sizes the grid.
A step WITHOUT an adapted row uploads and launches exactly what it does in an engine without a store.  The drafter of
a speculative engine serves base weights (its forwards never carry tiles): the accept / reject rule is exact for any
drafter.  K/V depend on the adapter, so the prefix cache keys the FIRST block of a chain by (uid,) + tokens, uid the
id of that load of the adapter (a name loaded again with other weights is another adapter); requests without an adapter
use today's keys.  A request holds its adapter from add_sequence until it retires (LoraAdapters.unload refuses
meanwhile)."""
from __future__ import annotations

import itertools
import math
from collections import deque
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

_MASK64 = (1 << 64) - 1


class SamplingParams:
    """How one request draws its tokens.  temperature 0: greedy (top_k / top_p / seed unused).  top_k 0 and top_p 0 or 1:
    that filter is off; both are applied to the unscaled logits, top-k first, as the logits processors do.  seed: any
    int, used modulo 2^64; None lets add_sequence take one from rng.next_offset().  Fixed at construction."""

    def __init__(self, temperature: float = 0.0, top_k: int = 0, top_p: float = 0.0, seed: Optional[int] = None):
        temperature, top_p = float(temperature), float(top_p)
        if not math.isfinite(temperature) or temperature < 0.0:
            raise ValueError(f"temperature {temperature} must be finite and not negative")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError(f"top_k {top_k} must be a non-negative integer")
        if not 0.0 <= top_p <= 1.0:                      # (also rejects NaN)
            raise ValueError(f"top_p {top_p} must lie in [0, 1]")
        self.temperature, self.top_k, self.top_p = temperature, int(top_k), top_p
        self.seed = None if seed is None else int(seed) & _MASK64
        # how the parameters ride in a step's uploads, fixed here: top_k and the bit patterns of inv_temperature /
        # top_p as int32, the seed as the int64 that carries its 64 bits
        self.wire = (_f32_bits(self.inv_temperature), min(self.top_k, 0x7fffffff), _f32_bits(self.top_p),
                     _as_i64(self.seed or 0))

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0

    @property
    def inv_temperature(self) -> float:
        """What the kernel multiplies by: fp32(1 / temperature), 0 for a greedy request."""
        return 0.0 if self.greedy else float(np.float32(1.0 / self.temperature))

    def __repr__(self) -> str:
        return (f"SamplingParams(temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p}, "
                f"seed={self.seed})")


def _f32_bits(x: float) -> int:
    """The bit pattern of fp32(x) as an int32: how a float rides in the step's int32 upload."""
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def _as_i64(x: int) -> int:
    """A 64-bit pattern as the int64 that carries it."""
    return x - (1 << 64) if x >> 63 else x


class RadixNode:
    """One cached block: the block's id, its children keyed by their block_size token ids, the number of running
    sequences that hold it.  `parent` / `key` are the way back up (the notebook keeps them in block_to_node)."""

    def __init__(self, block_id: int, parent: Optional["RadixNode"] = None, key: Optional[tuple] = None):
        self.block_id = block_id
        self.children: Dict[tuple, "RadixNode"] = {}
        self.ref_count = 0
        self.parent, self.key = parent, key


class SequenceState:
    """Runtime state of one request: its tokens, the blocks that hold its keys (block_table) and the slot of every
    token (slot_mapping), all on the host.  `prefix_len` tokens were found in the prefix cache and are not computed."""

    def __init__(self, sid: int, prompt_ids: Sequence[int], max_gen_len: int, block_size: int, device="cpu",
                 matched_blocks: Optional[Sequence[int]] = None, salt=None):
        self.id, self.device, self.block_size = sid, torch.device(device), block_size
        self.salt = salt              # what keys the first block of its chain in the prefix cache (None: the tokens alone)
        matched_blocks = list(matched_blocks or [])
        self.prefix_len = len(matched_blocks) * block_size
        p_len = len(prompt_ids)
        if p_len == 0 or self.prefix_len >= p_len:
            raise ValueError("a sequence needs at least one prompt token to compute")
        self.prompt_len = p_len
        self.max_total_len = p_len + max_gen_len
        self.tokens = torch.zeros(self.max_total_len, dtype=torch.long)
        self.tokens[:p_len] = torch.as_tensor(list(prompt_ids), dtype=torch.long)
        self.num_tokens, self.is_prefill = p_len, True
        self.block_table = torch.zeros((self.max_total_len + block_size - 1) // block_size, dtype=torch.int32)
        self.block_count = len(matched_blocks)
        if matched_blocks:
            self.block_table[:self.block_count] = torch.as_tensor(matched_blocks, dtype=torch.int32)
        self.slot_mapping = torch.zeros(self.max_total_len, dtype=torch.long)
        # chunked prefill: num_computed prompt tokens are in the pages (from the prefix cache or from earlier chunks),
        # this step's chunk ends at chunk_end (None: at the end of the prompt), blocks [0, blocks_registered) have been
        # offered to the radix tree (or came from it)
        self.num_computed = self.prefix_len
        self.chunk_end: Optional[int] = None
        self.blocks_registered = len(matched_blocks)

    @property
    def query_start(self) -> int:
        """First token of this step's query rows: everything past what the pages already hold while prefilling (the
        cached prefix, and the chunks of earlier steps), then the last."""
        return self.num_computed if self.is_prefill else self.num_tokens - 1

    @property
    def query_end(self) -> int:
        """One past the last token of this step's query rows: the chunk's end while a prompt goes in chunks."""
        return self.chunk_end if self.is_prefill and self.chunk_end is not None else self.num_tokens

    def map_slots(self, a: int, b: int) -> None:
        """slot = block_table[i // block_size] * block_size + i % block_size for the tokens [a, b)."""
        idx = torch.arange(a, b)
        self.slot_mapping[idx] = self.block_table[idx // self.block_size].long() * self.block_size + idx % self.block_size

    def update_metadata(self) -> None:
        """The slots of the tokens this step computes."""
        self.map_slots(self.query_start, self.query_end)


class PagedKVManager:
    """The pages of every layer -- k_cache[i] / v_cache[i]: (max_blocks, block_size, num_key_value_heads, head_dim) on
    `device` -- and who owns them: a free list, a radix tree over complete prompt blocks, and the queue of registered
    blocks nobody holds (evictable, oldest first).  `config` is the model's Config (the notebook passes a dict).

    kv_cache_dtype="fp8" ("fp8_e4m3", torch.float8_e4m3fn): the pages hold OCP e4m3 codes, one byte an element, and
    k_scale[i] / v_scale[i] -- fp32 (max_blocks, block_size, num_key_value_heads) -- one scale per slot and KV head, at
    the block's own indices (the rule: include/vyom_hip.h).  Blocks, the tree, eviction and admission do not change.
    None: pages in `dtype`, k_scale / v_scale are None.  kv_bytes: what pages and scales hold."""

    def __init__(self, config, max_blocks: int, block_size: int, device="cpu", dtype=torch.float32,
                 kv_cache_dtype=None):
        if block_size < 8 or block_size > 256 or block_size & (block_size - 1):
            raise ValueError(f"block_size {block_size} must be a power of two from 8 to 256")
        if max_blocks < 1:
            raise ValueError(f"max_blocks {max_blocks} must be positive")
        self.config, self.max_blocks, self.block_size = config, max_blocks, block_size
        self.device, self.dtype = torch.device(device), dtype
        self.free_blocks = deque(range(max_blocks))
        self.evictable_blocks: deque = deque()
        self.radix_root = RadixNode(-1)
        self.block_to_node: Dict[int, RadixNode] = {}
        hk = config.num_key_value_heads
        dh = getattr(config, "head_dim", config.hidden_size // config.num_attention_heads)
        shape = (max_blocks, block_size, hk, dh)
        layers = range(config.num_hidden_layers)
        if kv_cache_dtype is None:
            self.kv_cache_dtype = None
            self.k_cache = [torch.zeros(shape, dtype=dtype, device=self.device) for _ in layers]
            self.v_cache = [torch.zeros(shape, dtype=dtype, device=self.device) for _ in layers]
            self.k_scale = self.v_scale = None
        elif kv_cache_dtype in ("fp8", "fp8_e4m3", torch.float8_e4m3fn):
            self.kv_cache_dtype = torch.float8_e4m3fn
            self.k_cache = [self._fp8_zeros(shape) for _ in layers]
            self.v_cache = [self._fp8_zeros(shape) for _ in layers]
            self.k_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=self.device) for _ in layers]
            self.v_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=self.device) for _ in layers]
        else:
            raise ValueError(f"kv_cache_dtype {kv_cache_dtype!r}: None, 'fp8', 'fp8_e4m3' or torch.float8_e4m3fn")

    def _fp8_zeros(self, shape) -> torch.Tensor:
        try:
            return torch.zeros(shape, dtype=torch.float8_e4m3fn, device=self.device)
        except (RuntimeError, TypeError):      # an allocator that refuses the dtype: the same bytes, viewed
            return torch.zeros(shape, dtype=torch.uint8, device=self.device).view(torch.float8_e4m3fn)

    @property
    def kv_bytes(self) -> int:
        """Bytes held by the pages of every layer, plus their scales."""
        held = self.k_cache + self.v_cache + (self.k_scale or []) + (self.v_scale or [])
        return sum(t.numel() * t.element_size() for t in held)

    def blocks_for(self, num_tokens: int) -> int:
        return (num_tokens + self.block_size - 1) // self.block_size

    # ---- prefix cache ----------------------------------------------------------------------------------------
    def match_prefix(self, token_ids: Sequence[int], salt=None) -> List[int]:
        """Block ids of the longest cached chain of whole blocks in front of token_ids, at most
        (len - 1) // block_size of them (one token is always left to compute).  No side effects.  salt (not None): the
        chains registered by sequences of that salt only -- the first block's key is (salt,) + tokens."""
        bs, node, out = self.block_size, self.radix_root, []
        for i in range((len(token_ids) - 1) // bs):
            key = tuple(int(t) for t in token_ids[i * bs:(i + 1) * bs])
            node = node.children.get(key if i or salt is None else (salt,) + key)
            if node is None:
                break
            out.append(node.block_id)
        return out

    def acquire(self, blocks: Sequence[int]) -> None:
        """A sequence starts to hold these registered blocks."""
        for b in blocks:
            node = self.block_to_node[b]
            if node.ref_count == 0:
                self.evictable_blocks.remove(b)
            node.ref_count += 1

    def get_prefix_blocks(self, token_ids: Sequence[int]) -> List[int]:
        """match_prefix + acquire: the notebook's call, for a caller that admits the request on the spot."""
        blocks = self.match_prefix(token_ids)
        self.acquire(blocks)
        return blocks

    def available(self, matched: Sequence[int] = ()) -> int:
        """Blocks allocate() could hand out if `matched` were acquired first."""
        held_back = sum(1 for b in matched if self.block_to_node[b].ref_count == 0)
        return len(self.free_blocks) + len(self.evictable_blocks) - held_back

    # ---- allocation ------------------------------------------------------------------------------------------
    def allocate(self, state: SequenceState, upto: Optional[int] = None) -> None:
        """Blocks for state.num_tokens tokens; a block whose tokens are all known now (a prompt block) is registered.
        upto (chunked prefill): blocks for the first `upto` tokens only, and only the prompt blocks that lie wholly in
        front of `upto` are registered -- also one that an earlier chunk allocated and left part filled.  The caller
        computes tokens [.., upto) in this step, so a block is in the tree only if its rows are written by the end of
        the step that registered it."""
        bs = self.block_size
        end = state.num_tokens if upto is None else upto
        whole = min(end, state.prompt_len) // bs           # prompt blocks complete once this step has run
        while state.blocks_registered < min(state.block_count, whole):
            i = state.blocks_registered
            self._register_block(state, i, int(state.block_table[i]))
            state.blocks_registered = i + 1
        while state.block_count < self.blocks_for(end):
            if not self.free_blocks:
                if not self.evictable_blocks:
                    raise RuntimeError("KV Cache full!")
                self._evict(self.evictable_blocks.popleft())
            new_block = self.free_blocks.popleft()
            i = state.block_count
            state.block_table[i] = new_block
            if i < whole:
                self._register_block(state, i, new_block)
                state.blocks_registered = i + 1
            state.block_count += 1

    def _register_block(self, state: SequenceState, i: int, block_id: int) -> None:
        """Block i of the sequence becomes a child of block i - 1's node, held once."""
        if i and int(state.block_table[i - 1]) not in self.block_to_node:
            return                       # the parent lost its registration: this block stays private
        parent = self.block_to_node[int(state.block_table[i - 1])] if i else self.radix_root
        key = tuple(state.tokens[i * self.block_size:(i + 1) * self.block_size].tolist())
        if i == 0 and state.salt is not None:
            key = (state.salt,) + key
        if key in parent.children:
            return                       # the same tokens were registered by a concurrent sequence: stays private
        node = RadixNode(block_id, parent, key)
        node.ref_count = 1
        parent.children[key] = node
        self.block_to_node[block_id] = node

    def _evict(self, block_id: int) -> None:
        """The block leaves the tree and becomes free; so does every block below it."""
        node = self.block_to_node[block_id]
        del node.parent.children[node.key]
        stack = [node]
        while stack:
            n = stack.pop()
            assert n.ref_count == 0, "a held block below an evicted one"
            del self.block_to_node[n.block_id]
            if n is not node:
                self.evictable_blocks.remove(n.block_id)
            self.free_blocks.append(n.block_id)
            stack.extend(n.children.values())
            n.children = {}

    def free(self, state: SequenceState) -> None:
        """The sequence lets go of its blocks: registered ones become evictable with their last holder, others free."""
        for i in range(state.block_count):
            b = int(state.block_table[i])
            node = self.block_to_node.get(b)
            if node is not None:
                node.ref_count -= 1
                if node.ref_count == 0:
                    self.evictable_blocks.append(b)
            else:
                self.free_blocks.append(b)
        state.block_count = 0


def _compute_dtype(model) -> torch.dtype:
    """The dtype of the model's packed QKV rows: compute_dtype where a model keeps fp32 masters, else its parameters'."""
    inner = getattr(model, "model", model)
    return getattr(inner, "compute_dtype", None) or next(model.parameters()).dtype


class _StepUploads:
    """The step's two host-to-device copies (module docstring): named lists are collected for one int64 and one int32
    buffer, in the order they are put, and upload() builds and moves each buffer once and splits it -> {name: the
    entry's view of the device tensor}, in the dtype it was put in (the _f32_bits() patterns of a float entry:
    .view(torch.float32)).  An entry without values is an empty view; a name that was never put is not in the dict."""

    def __init__(self):
        self._l64, self._l32 = {}, {}

    def put64(self, name: str, values) -> None:
        assert name not in self._l64 and name not in self._l32, f"{name} is already in the step's uploads"
        self._l64[name] = values

    def put32(self, name: str, values) -> None:
        assert name not in self._l64 and name not in self._l32, f"{name} is already in the step's uploads"
        self._l32[name] = values

    def upload(self, device) -> Dict[str, torch.Tensor]:
        views = {}
        for entries, dtype in ((self._l64, torch.long), (self._l32, torch.int32)):
            buf = torch.tensor(list(itertools.chain.from_iterable(entries.values())), dtype=dtype).to(device)
            views.update(zip(entries, buf.split([len(values) for values in entries.values()])))
        return views


def _put_sampling(up: _StepUploads, params: List[SamplingParams]) -> None:
    """One entry per row of SamplingParams.wire: inv_temperature, top_k and top_p in the int32 upload, the seed in the
    int64 one (a greedy row: inv_temperature 0)."""
    up.put32("inv_temperature", [sp.wire[0] for sp in params])
    up.put32("top_k", [sp.wire[1] for sp in params])
    up.put32("top_p", [sp.wire[2] for sp in params])
    up.put64("seed", [sp.wire[3] for sp in params])


def _sampling_views(at: Dict[str, torch.Tensor], n: Optional[int] = None, **more) -> dict:
    """What _put_sampling uploaded (n: the first n rows of it), as vy_sample_rows / vy_spec_verify take it; `more`: the
    caller's own per-row entries (counter: the position of the token being drawn)."""
    views = {"inv_temperature": at["inv_temperature"].view(torch.float32), "top_k": at["top_k"],
             "top_p": at["top_p"].view(torch.float32), "seed": at["seed"]}
    if n is not None:
        views = {name: view[:n] for name, view in views.items()}
    return {**views, **more}


def _metadata(positions, slot_mapping, last_rows, max_position: int, prefill=(), decode=None, prefill_varlen=None) -> dict:
    """The dict forward_paged and layers/paged.py read.  last_rows: the rows that get logits; prefill: the default
    engine's per-sequence list; decode / prefill_varlen: what the paged decode launch and the ONE varlen prefill
    launch read, None / no such key when the forward has no such rows."""
    md = {"positions": positions, "slot_mapping": slot_mapping, "last_rows": last_rows, "max_position": max_position,
          "prefill": list(prefill), "decode": decode}
    if prefill_varlen is not None:
        md["prefill_varlen"] = prefill_varlen
    return md


def _padded_tables(states: List[SequenceState]):
    """-> (width, {sid: the sequence's block table padded with zeros to width})."""
    width = max(s.block_table.numel() for s in states)
    return width, {s.id: s.block_table[:s.block_count].tolist() + [0] * (width - s.block_count) for s in states}


class _PackedRows:
    """One packed forward, built segment by segment in row order: ids, positions and slots of every row, the rows that
    get logits (the last n_last of a segment), and per kind of segment what its attention launch reads.  decode(s): the
    one query row of a decoding sequence, for vy_attn_paged_decode.  varlen(s, a, b, n_last): tokens [a, b) as a segment
    of the ONE vy_attn_paged_prefill launch (cu_q counts rows of the packed buffer, ctx_len = a).  per_sequence(s, a, b,
    n_last): the default engine's prefill (first row, rows, prefix_len, its block table after a prefix hit).
    put() appends all of it to the step's uploads under `prefix`, metadata() builds the dict from the views.
    lora = (the LoraAdapters store, {sid: adapter slot}): the rows of those sequences are recorded as tiles
    (row0, nrows <= 16, slot), cut every 16 rows; put() uploads them only if there are any, and only then has the
    metadata a "lora" entry."""

    def __init__(self, width: int, tables: Dict[int, List[int]], prefix: str = "", lora=None):
        self.width, self.tables, self.prefix = width, tables, prefix
        self.adapters, self.slot_of = lora if lora is not None else (None, {})
        self.tiles: List[int] = []
        self.ids, self.pos, self.slots, self.last = [], [], [], []
        self.dec_rows, self.dec_lens, self.dec_tables, self.prefill = [], [], [], []
        self.seg_rows, self.ctx, self.seg_tables, self.max_q, self.max_kv = [], [], [], 0, 0

    def _rows(self, s: SequenceState, a: int, b: int, n_last: int) -> int:
        row0 = len(self.ids)
        self.ids += s.tokens[a:b].tolist()
        self.pos += range(a, b)
        self.slots += s.slot_mapping[a:b].tolist()
        self.last += range(row0 + b - a - n_last, row0 + b - a)
        slot = self.slot_of.get(s.id)
        if slot is not None:
            for r in range(row0, row0 + b - a, 16):
                self.tiles += (r, min(16, row0 + b - a - r), slot)
        return row0

    def decode(self, s: SequenceState) -> None:
        assert not self.ctx, "decoding sequences come first"
        self.dec_rows.append(self._rows(s, s.num_tokens - 1, s.num_tokens, 1))
        self.dec_lens.append(s.num_tokens)
        self.dec_tables += self.tables[s.id]

    def varlen(self, s: SequenceState, a: int, b: int, n_last: int) -> None:
        self.seg_rows.append(self._rows(s, a, b, n_last))
        self.ctx.append(a)
        self.seg_tables += self.tables[s.id]
        self.max_q, self.max_kv = max(self.max_q, b - a), max(self.max_kv, b)

    def per_sequence(self, s: SequenceState, a: int, b: int, n_last: int) -> None:
        self.prefill.append((self._rows(s, a, b, n_last), b - a, a, self.tables[s.id][:s.block_count] if a else None))

    def put(self, up: _StepUploads) -> None:
        p = self.prefix
        for name, values in (("ids", self.ids), ("slots", self.slots), ("last", self.last)):
            up.put64(p + name, values)
        for name, values in (("pos", self.pos), ("dec_rows", self.dec_rows), ("dec_lens", self.dec_lens),
                             ("dec_tables", self.dec_tables)):
            up.put32(p + name, values)
        for k, (_, _, _, table) in enumerate(self.prefill):
            if table is not None:
                up.put32(f"{p}prefill{k}", table)
        if self.ctx or not self.ids:             # (a draft round 0 without rows still has its cu_q = [0])
            up.put32(p + "cu", self.seg_rows + [len(self.ids)])      # the varlen segments end the forward
            up.put32(p + "ctx", self.ctx)
            up.put32(p + "tab", self.seg_tables)
        if self.tiles:
            up.put32(p + "tiles", self.tiles)

    def metadata(self, at: Dict[str, torch.Tensor], max_position: int) -> dict:
        """at: what upload() returned."""
        p, decode, varlen = self.prefix, None, None
        if self.dec_rows:
            decode = {"rows": at[p + "dec_rows"], "seqlens": at[p + "dec_lens"], "max_seqlen": max(self.dec_lens),
                      "block_table": at[p + "dec_tables"].view(len(self.dec_rows), self.width)}
        if self.ctx:
            varlen = {"cu_q": at[p + "cu"], "ctx_lens": at[p + "ctx"], "max_q": self.max_q, "max_kv": self.max_kv,
                      "block_table": at[p + "tab"].view(len(self.ctx), self.width)}
        prefill = [(row0, n, prefix_len, None if table is None else at[f"{p}prefill{k}"])
                   for k, (row0, n, prefix_len, table) in enumerate(self.prefill)]
        md = _metadata(at[p + "pos"], at[p + "slots"], at[p + "last"], max_position, prefill, decode, varlen)
        if self.tiles:
            md["lora"] = {"tiles": at[p + "tiles"].view(-1, 3), "n_tiles": len(self.tiles) // 3, "adapters": self.adapters}
        return md


class ContinuousBatchEngine:
    """add_sequence() queues a request; step() admits what fits, runs ONE packed forward over every running sequence
    (all unseen prompt tokens of the newly admitted ones, one token of the others), appends to each the token its
    SamplingParams draw (greedy by default; `sampling[sid]` holds the resolved parameters while the request lives) and
    returns the sequences that finished in this step as {sid: token list}.  Stop tokens: `eos_token_ids` (default: the
    model config's eos_token_id); the notebook hard-codes Qwen's two ids.

    max_step_tokens / varlen_prefill: chunked prefill and the one varlen prefill launch (module docstring); with both at
    None the engine prefills a prompt in one step, one attention launch per prefilling sequence.

    draft_model / draft_kv_mgr / num_speculative_tokens: speculative decoding (module docstring).  drafts_proposed /
    drafts_accepted count over the engine's life.

    adapters: a LoraAdapters store (module docstring); add_sequence(..., adapter="name") then serves that request with
    the adapter's weights, `adapter[sid]` holds the name while the request lives.

    prompt_tokens_computed[sid]: prompt tokens that went through the model so far (the rest came from the prefix cache).
    record_logits=True keeps every step's last-row logits per sequence in `logits[sid]` (fp32, host): a debug aid.  In a
    speculative engine that is one row per emitted token, the target row that decided it, and `rounds[sid]` holds per
    round {position0, draft_tokens, draft_rows, target_rows, accepted, emitted}."""

    def __init__(self, model, kv_mgr: PagedKVManager, max_batch_size: int = 8, eos_token_ids=None,
                 record_logits: bool = False, max_step_tokens: Optional[int] = None,
                 varlen_prefill: Optional[bool] = None, draft_model=None, draft_kv_mgr: Optional[PagedKVManager] = None,
                 num_speculative_tokens: int = 0, adapters=None):
        if varlen_prefill is None:
            varlen_prefill = max_step_tokens is not None
        if max_step_tokens is not None:
            if not varlen_prefill:
                raise ValueError("max_step_tokens needs varlen_prefill: a chunk attends to pages of its own prompt")
            if max_step_tokens < max_batch_size:
                raise ValueError(f"max_step_tokens {max_step_tokens} must be at least max_batch_size {max_batch_size}: "
                                 "every decoding sequence takes a token and a prefilling one must still progress")
        self.max_step_tokens, self.varlen_prefill = max_step_tokens, bool(varlen_prefill)
        if getattr(kv_mgr, "k_scale", None) is not None:
            if not varlen_prefill:
                raise ValueError("fp8 KV pages need varlen_prefill=True: the per-sequence prefill attends to the "
                                 "step's own unquantised rows and gathers bf16 pages")
            computes = kv_mgr.dtype if model is None else _compute_dtype(model)
            if computes != torch.bfloat16 or kv_mgr.dtype != torch.bfloat16:
                raise ValueError(f"fp8 KV pages serve a model that computes in bfloat16: the model computes in "
                                 f"{computes}, the manager was built for {kv_mgr.dtype}")
        if adapters is not None and not varlen_prefill:
            raise ValueError("adapters= needs varlen_prefill=True: the tiles of the adapted rows are recorded by the "
                             "planner of the one varlen prefill launch, the per-sequence prefill loop stays as it is")
        self.adapters = adapters
        self.adapter: Dict[int, str] = {}            # the requests that carry an adapter -> its name
        self.speculative = draft_model is not None or draft_kv_mgr is not None or num_speculative_tokens != 0
        if self.speculative:
            self._check_drafter(model, kv_mgr, draft_model, draft_kv_mgr, num_speculative_tokens, max_batch_size)
            if draft_model is not None:
                draft_model.eval()
        self.draft_model, self.draft_kv_mgr, self.num_speculative_tokens = draft_model, draft_kv_mgr, num_speculative_tokens
        self.draft_computed: Dict[int, int] = {}     # tokens of a decoding sequence the drafter's pages hold
        self.drafts_proposed = self.drafts_accepted = 0
        self.rounds: Dict[int, List[dict]] = {}
        self.model, self.kv_mgr = model, kv_mgr
        if model is not None:
            model.eval()
        self.max_batch = max_batch_size
        self.device = kv_mgr.device
        if eos_token_ids is None:
            eos = getattr(kv_mgr.config, "eos_token_id", None)
            eos_token_ids = [] if eos is None else eos
        self.eos_token_ids = set(eos_token_ids) if isinstance(eos_token_ids, (list, tuple, set)) else {int(eos_token_ids)}
        self.active: Dict[int, SequenceState] = {}
        self.waiting_room: deque = deque()
        self.id_gen = itertools.count()
        self.prompt_tokens_computed: Dict[int, int] = {}
        self.record_logits = record_logits
        self.logits: Dict[int, List[torch.Tensor]] = {}
        self.sampling: Dict[int, SamplingParams] = {}

    def _check_drafter(self, model, kv_mgr, draft_model, draft_kv_mgr, g, max_batch_size) -> None:
        if not self.varlen_prefill:
            raise ValueError("speculative decoding needs varlen_prefill=True: a verification segment of g + 1 rows "
                             "attends to its sequence's pages through vy_attn_paged_prefill")
        if draft_kv_mgr is None or (model is None) != (draft_model is None):
            raise ValueError("speculative decoding needs draft_model and draft_kv_mgr, the drafter's own pages")
        if int(g) != g or not 1 <= g <= 16:
            raise ValueError(f"num_speculative_tokens {g} must be an integer from 1 to 16")
        tv, dv = getattr(kv_mgr.config, "vocab_size", None), getattr(draft_kv_mgr.config, "vocab_size", None)
        if tv != dv:
            raise ValueError(f"drafter and target need one vocabulary: the drafter has {dv} entries, the target {tv}")
        if (draft_kv_mgr.max_blocks, draft_kv_mgr.block_size) != (kv_mgr.max_blocks, kv_mgr.block_size):
            raise ValueError(f"draft_kv_mgr holds {draft_kv_mgr.max_blocks} blocks of {draft_kv_mgr.block_size}, the target's "
                             f"manager {kv_mgr.max_blocks} of {kv_mgr.block_size}: the drafter's pages are indexed by the "
                             "target's block tables")
        if draft_kv_mgr.device != kv_mgr.device:
            raise ValueError(f"draft_kv_mgr is on {draft_kv_mgr.device}, the target's manager on {kv_mgr.device}")
        computes = kv_mgr.dtype if draft_model is None else _compute_dtype(draft_model)
        if draft_kv_mgr.dtype != computes:
            raise ValueError(f"draft_kv_mgr was built for {draft_kv_mgr.dtype}, the drafter computes in {computes}")
        if model is not None and _compute_dtype(model) != computes:
            raise ValueError(f"the drafter computes in {computes}, the target in {_compute_dtype(model)}: vy_spec_verify "
                             "compares logits of one dtype")
        if getattr(draft_kv_mgr, "k_scale", None) is not None and computes != torch.bfloat16:
            raise ValueError(f"fp8 KV pages serve a drafter that computes in bfloat16, not {computes}")
        if self.max_step_tokens is not None and self.max_step_tokens < max_batch_size * (g + 1):
            raise ValueError(f"max_step_tokens {self.max_step_tokens} must be at least max_batch_size * "
                             f"(num_speculative_tokens + 1) = {max_batch_size * (g + 1)}: a decoding sequence takes "
                             "1 + g rows of the budget and a prefilling one must still progress")

    def add_sequence(self, prompt_ids: Sequence[int], max_gen_len: int = 128,
                     sampling: Optional[SamplingParams] = None, adapter: Optional[str] = None) -> int:
        """sampling=None: greedy.  A sampled request without a seed gets one here from the package's random stream
        (rng.next_offset(): torch.manual_seed / rng.manual_seed govern it, every call a different one).
        adapter: the name of a loaded adapter of the engine's store (None: the base weights); the request holds it
        until it retires."""
        prompt_ids = [int(t) for t in prompt_ids]
        if not prompt_ids or max_gen_len < 1:
            raise ValueError("a request needs a prompt and max_gen_len >= 1")
        if self.kv_mgr.blocks_for(len(prompt_ids) + max_gen_len) > self.kv_mgr.max_blocks:
            raise ValueError(f"{len(prompt_ids)} + {max_gen_len} tokens do not fit into {self.kv_mgr.max_blocks} blocks "
                             f"of {self.kv_mgr.block_size}")
        if adapter is not None:
            if self.adapters is None:
                raise ValueError(f"adapter {adapter!r}: the engine was built without adapters=")
            if adapter not in self.adapters.slots:
                raise ValueError(f"adapter {adapter!r} is not loaded (loaded: {sorted(self.adapters.slots)})")
        if sampling is None:
            sampling = SamplingParams()
        elif not isinstance(sampling, SamplingParams):
            raise ValueError(f"sampling must be a SamplingParams or None, got {type(sampling).__name__}")
        elif not sampling.greedy and sampling.seed is None:
            from . import rng
            base, offset = rng.next_offset()
            # an odd multiplier is a bijection modulo 2^64: different offsets of one base seed never collide
            sampling = SamplingParams(sampling.temperature, sampling.top_k, sampling.top_p,
                                      (base + 0x9E3779B97F4A7C15 * offset) & _MASK64)
        sid = next(self.id_gen)
        self.sampling[sid] = sampling
        salt = None
        if adapter is not None:
            self.adapters.acquire(adapter)
            self.adapter[sid] = adapter
            salt = self.adapters.uid[adapter]        # K/V depend on the adapter: cached blocks are shared within one only
        self.waiting_room.append({"sid": sid, "prompt_ids": prompt_ids, "max_gen_len": max_gen_len, "salt": salt})
        return sid

    def _try_schedule_waiting(self) -> None:
        """Admit from the head of the waiting room while the batch has room and the head's whole life fits."""
        mgr = self.kv_mgr
        while self.waiting_room and len(self.active) < self.max_batch:
            req = self.waiting_room[0]
            matched = mgr.match_prefix(req["prompt_ids"], req["salt"])
            need = mgr.blocks_for(len(req["prompt_ids"]) + req["max_gen_len"]) - len(matched)
            claimed = sum(s.block_table.numel() - s.block_count for s in self.active.values())
            if need > mgr.available(matched) - claimed:
                break
            self.waiting_room.popleft()
            mgr.acquire(matched)
            self.active[req["sid"]] = SequenceState(req["sid"], req["prompt_ids"], req["max_gen_len"], mgr.block_size,
                                                    self.device, matched_blocks=matched, salt=req["salt"])

    def _schedule_prompts(self, decode_rows: int) -> List[SequenceState]:
        """The prefilling sequences that run in this step, in admission order, their chunk_end set.  Under
        max_step_tokens the decoding sequences took decode_rows of the budget; each prompt gets min(prompt tokens left,
        budget left) and one that gets nothing sits the step out."""
        budget = math.inf if self.max_step_tokens is None else self.max_step_tokens - decode_rows
        run = []
        for s in self.active.values():
            n = min(s.prompt_len - s.num_computed, budget) if s.is_prefill else 0
            if n > 0:
                budget -= n
                s.chunk_end = s.num_computed + n
                run.append(s)
        return run

    def _lora_rows(self, states: List[SequenceState]):
        """What _PackedRows needs to record the tiles of the step's adapted rows; None in an engine without a store."""
        if self.adapters is None:
            return None
        return self.adapters, {s.id: self.adapters.slots[self.adapter[s.id]] for s in states if s.id in self.adapter}

    def _allocate(self, s: SequenceState) -> None:
        """Blocks and slots of the tokens this step computes of its sequence."""
        self.kv_mgr.allocate(s, s.query_end)
        s.update_metadata()
        if s.is_prefill:
            self.prompt_tokens_computed[s.id] = s.query_end - s.prefix_len

    def _plan_step(self):
        """-> (states, metadata, input_ids) of the next step, its blocks allocated and its metadata uploaded; None when
        nothing runs.  Everything a step does before the model (no GPU work but the two uploads).  states, in the order
        of their rows: every running sequence in admission order, a prefilling one with all its unseen prompt tokens
        through its own attention launch (metadata["prefill"]); varlen_prefill: the decoding sequences first, then the
        prompts _schedule_prompts() lets run, as segments of ONE launch (metadata["prefill_varlen"]).  last_rows has one
        row per sequence whose query rows reach its last token; if one of those sequences samples, metadata["sampling"]
        holds one entry per last row, else the step uploads no sampling entries and has no such key."""
        self._try_schedule_waiting()
        if not self.active:
            return None
        states = list(self.active.values())
        if self.varlen_prefill:
            dec = [s for s in states if not s.is_prefill]
            states = dec + self._schedule_prompts(len(dec))
        for s in states:
            self._allocate(s)
        rows = _PackedRows(*_padded_tables(states), lora=self._lora_rows(states))
        for s in states:
            a, b = s.query_start, s.query_end
            if not s.is_prefill:
                rows.decode(s)
            elif self.varlen_prefill:
                rows.varlen(s, a, b, int(b == s.num_tokens))
            else:
                rows.per_sequence(s, a, b, int(b == s.num_tokens))
        drawn = [s for s in states if s.query_end == s.num_tokens]
        params = [self.sampling[s.id] for s in drawn]
        sampled = any(not sp.greedy for sp in params)
        up = _StepUploads()
        rows.put(up)
        if sampled:
            _put_sampling(up, params)
            up.put64("counter", [s.num_tokens for s in drawn])
        at = up.upload(self.device)
        metadata = rows.metadata(at, max(s.num_tokens for s in states))
        if sampled:
            metadata["sampling"] = _sampling_views(at, counter=at["counter"])
        return states, metadata, at["ids"]

    def step(self) -> Dict[int, List[int]]:
        if self.speculative:
            return self._spec_step()
        plan = self._plan_step()
        if plan is None:
            return {}
        states, metadata, input_ids = plan
        logits = self.model.forward_paged(input_ids, metadata["positions"], metadata, self.kv_mgr)
        sp = metadata.get("sampling")
        if sp is None:
            picked = torch.argmax(logits, dim=-1)
        else:
            from . import ops
            picked = ops.sample_rows(logits, sp["inv_temperature"], sp["top_k"], sp["top_p"], sp["seed"], sp["counter"])
        next_tokens = picked.tolist()                                # the step's one device-to-host copy
        if self.record_logits:
            host = logits.float().cpu()
            for i, s in enumerate(s for s in states if s.query_end == s.num_tokens):
                self.logits.setdefault(s.id, []).append(host[i])
        return self._finish_step(states, next_tokens)

    @staticmethod
    def _end_step(states: List[SequenceState]) -> None:
        """The step's rows are in the pages: what it computed counts, and the next step cuts its own chunks."""
        for s in states:
            s.num_computed, s.chunk_end = s.query_end, None

    def _retire(self, s: SequenceState, finished: Dict[int, List[int]]) -> None:
        """A sequence that met a stop token or its length leaves: its tokens go to `finished`, its blocks back."""
        finished[s.id] = s.tokens[:s.num_tokens].tolist()
        self.kv_mgr.free(s)
        del self.active[s.id]
        del self.sampling[s.id]
        if s.id in self.adapter:
            self.adapters.release(self.adapter.pop(s.id))
        self.draft_computed.pop(s.id, None)

    def _finish_step(self, states: List[SequenceState], next_tokens: List[int]) -> Dict[int, List[int]]:
        """Append next_tokens (one per sequence whose query rows reached its last token, in row order) and retire what
        finished: everything a step does after the model, on the host."""
        emitting = [s for s in states if s.query_end == s.num_tokens]   # (a chunk short of its prompt's end: no token)
        self._end_step(states)
        finished = {}
        for s, token_id in zip(emitting, next_tokens):
            s.is_prefill = False
            s.tokens[s.num_tokens] = token_id
            s.num_tokens += 1
            if token_id in self.eos_token_ids or s.num_tokens >= s.max_total_len:
                self._retire(s, finished)
        return finished

    # ---- speculative decoding (module docstring) -------------------------------------------------------------
    def _plan_spec_step(self):
        """-> the plan of one speculative step, its blocks allocated and its metadata uploaded (two uploads, as a
        plain step); None when nothing runs.  Keys: states (row order: decoding sequences, most drafts first, then the
        prompt chunks), emitting (the sequences vy_spec_verify judges, in its order) with n_draft / t_row0 per entry,
        verify = (metadata, input_ids) of the target forward, draft = per round (metadata, input_ids or None, n, sampling)
        -- round j >= 1 reads its ids from round j - 1's draws -- scatter = (rows of the verify ids, flat indices into
        the (g, S) draft tokens) and sampling = the per-sequence arguments of vy_spec_verify."""
        self._try_schedule_waiting()
        if not self.active:
            return None
        G = self.num_speculative_tokens
        dec = [s for s in self.active.values() if not s.is_prefill]
        g_of = {s.id: max(0, min(G, s.max_total_len - s.num_tokens - 1)) for s in dec}
        dec.sort(key=lambda s: -g_of[s.id])
        prompts = self._schedule_prompts(sum(1 + g for g in g_of.values()))
        states = dec + prompts
        seen = {}                     # first token of a decoding sequence that the drafter has not computed yet
        for s in dec:
            seen[s.id] = min(self.draft_computed.get(s.id, s.num_tokens - 1), s.num_tokens - 1)
            self.kv_mgr.allocate(s, s.num_tokens + g_of[s.id])
            s.map_slots(seen[s.id], s.num_tokens + g_of[s.id])
        for s in prompts:
            self._allocate(s)
        # the verification: [last token, d_0 .. d_{g - 1}] per decoding sequence (the drafts are scattered in on the
        # device), every row with logits; draft round 0: what the drafter has not computed yet of every sequence that
        # drafts, its last row with logits; both: the prompt chunks, the target's with a logits row where a prompt ends
        width, tables = _padded_tables(states)
        # (the drafter serves base weights: only the target's forward carries the tiles of adapted rows)
        v, r0 = _PackedRows(width, tables, "v_", lora=self._lora_rows(states)), _PackedRows(width, tables, "r0_")
        for s in dec:
            v.varlen(s, s.num_tokens - 1, s.num_tokens + g_of[s.id], g_of[s.id] + 1)
            if g_of[s.id]:
                r0.varlen(s, seen[s.id], s.num_tokens, 1)
        for s in prompts:
            v.varlen(s, s.query_start, s.query_end, int(s.query_end == s.num_tokens))
            r0.varlen(s, s.query_start, s.query_end, 0)
        emitting = dec + [s for s in prompts if s.query_end == s.num_tokens]
        S, n_dec, cu = len(emitting), len(dec), v.seg_rows + [len(v.ids)]
        # the decoding sequences lead the verification, so the first logits row of sequence k is its first row, cu[k]
        n_draft = [g_of[s.id] for s in dec] + [0] * (S - n_dec)
        t_row0 = cu[:n_dec] + list(range(cu[n_dec], cu[n_dec] + S - n_dec))
        v_dst = [row for k in range(n_dec) for row in range(cu[k] + 1, cu[k + 1])]
        v_src = [i * S + k for k in range(n_dec) for i in range(n_draft[k])]
        n_of = [sum(1 for g in n_draft[:n_dec] if g > j) for j in range(G)]    # the sequences of round j: the first n_of[j]
        later = [(j, n_of[j]) for j in range(1, G) if n_of[j]]
        up = _StepUploads()
        v.put(up)
        up.put64("v_dst", v_dst)
        up.put64("v_src", v_src)
        r0.put(up)
        up.put32("rows", list(range(n_dec)))
        up.put32("t_row0", t_row0)
        up.put32("n_draft", n_draft)
        _put_sampling(up, [self.sampling[s.id] for s in emitting])
        up.put64("position0", [s.num_tokens for s in emitting])
        up.put64("rows64", list(range(n_dec)))
        for j, n in [(0, n_of[0])] + later:         # round j draws the token at num_tokens + j, reads position num_tokens - 1 + j
            up.put64(f"counter{j}", [s.num_tokens + j for s in dec[:n]])
            if j:
                up.put64(f"slots{j}", [int(s.slot_mapping[s.num_tokens - 1 + j]) for s in dec[:n]])
                up.put32(f"pos{j}", [s.num_tokens - 1 + j for s in dec[:n]])
                up.put32(f"lens{j}", [s.num_tokens + j for s in dec[:n]])
        at = up.upload(self.device)
        draft = []
        if r0.ids:
            draft.append((r0.metadata(at, r0.max_kv), at["r0_ids"], n_of[0],
                          _sampling_views(at, n_of[0], counter=at["counter0"])))
        dec_tab = at["v_tab"].view(len(v.ctx), width)      # the decoding sequences' tables lead the verification's
        for j, n in later:
            longest = max(s.num_tokens + j for s in dec[:n])
            md = _metadata(at[f"pos{j}"], at[f"slots{j}"], at["rows64"][:n], longest,
                           decode={"rows": at["rows"][:n], "seqlens": at[f"lens{j}"], "block_table": dec_tab[:n],
                                   "max_seqlen": longest})
            draft.append((md, None, n, _sampling_views(at, n, counter=at[f"counter{j}"])))
        return {"states": states, "emitting": emitting, "n_draft": n_draft, "t_row0": t_row0, "S": S,
                "verify": (v.metadata(at, v.max_kv), at["v_ids"]), "draft": draft, "scatter": (at["v_dst"], at["v_src"]),
                "sampling": _sampling_views(at, t_row0=at["t_row0"], n_draft=at["n_draft"], position0=at["position0"])}

    def _spec_step(self) -> Dict[int, List[int]]:
        plan = self._plan_spec_step()
        if plan is None:
            return {}
        from . import ops
        G, S = self.num_speculative_tokens, plan["S"]
        dtok = torch.zeros((G, max(S, 1)), dtype=torch.long, device=self.device)
        dlog = None
        for j, (md, ids, n, sp) in enumerate(plan["draft"]):
            rows = self.draft_model.forward_paged(dtok[j - 1, :n] if ids is None else ids, md["positions"], md,
                                                  self.draft_kv_mgr)
            if n:
                if dlog is None:
                    dlog = rows.new_empty((G, S, rows.shape[1]))
                dlog[j, :n] = rows
                dtok[j, :n] = ops.sample_rows(rows, sp["inv_temperature"], sp["top_k"], sp["top_p"], sp["seed"],
                                              sp["counter"])
        md, ids = plan["verify"]
        dst, src = plan["scatter"]
        if dst.numel():
            ids[dst] = dtok.view(-1)[src]
        target_rows = self.model.forward_paged(ids, md["positions"], md, self.kv_mgr)
        if not S:                                       # prompt chunks only: nothing to judge
            return self._finish_spec_step(plan, [], [], [])
        if dlog is None:                                # no sequence drafts in this step: the rows are never read
            dlog = target_rows.new_empty((G, S, target_rows.shape[1]))
        sp = plan["sampling"]
        accept, alt = ops.spec_verify(target_rows, dlog, dtok, sp["t_row0"], sp["n_draft"], sp["inv_temperature"],
                                      sp["top_k"], sp["top_p"], sp["seed"], sp["position0"])
        host = torch.cat([accept.view(-1).long(), alt.view(-1), dtok.view(-1)]).tolist()   # the step's one device-to-host copy
        n = S * (G + 1)
        accept = [host[k * (G + 1):(k + 1) * (G + 1)] for k in range(S)]
        alt = [host[n + k * (G + 1):n + (k + 1) * (G + 1)] for k in range(S)]
        drafts = [host[2 * n + i * S:2 * n + (i + 1) * S] for i in range(G)]
        recorded = (target_rows.float().cpu(), dlog.float().cpu()) if self.record_logits else None
        return self._finish_spec_step(plan, accept, alt, drafts, recorded)

    def _finish_spec_step(self, plan, accept, alt, drafts, recorded=None) -> Dict[int, List[int]]:
        """What a speculative step does after vy_spec_verify, on the host.  accept / alt: one list of g + 1 entries per
        judged sequence, drafts: one list of S tokens per draft index.  Per sequence: the drafts before the first
        rejection, then alt of that row; cut after the first stop token and at max_total_len; retire what finished."""
        self._end_step(plan["states"])
        finished = {}
        for k, s in enumerate(plan["emitting"]):
            g, n = plan["n_draft"][k], s.num_tokens
            mine = [int(drafts[i][k]) for i in range(g)]
            a = 0
            while a < g and accept[k][a]:
                a += 1
            emitted = (mine[:a] + [int(alt[k][a])])[:s.max_total_len - n]
            for c, token_id in enumerate(emitted):
                if token_id in self.eos_token_ids:
                    emitted = emitted[:c + 1]
                    break
            self.drafts_proposed += g
            self.drafts_accepted += a
            if s.is_prefill or g:                       # what the drafter's pages hold of the tokens that stay
                self.draft_computed[s.id] = n if s.is_prefill else n + min(a, g - 1)
            s.is_prefill = False
            s.tokens[n:n + len(emitted)] = torch.as_tensor(emitted, dtype=torch.long)
            s.num_tokens = n + len(emitted)
            if recorded is not None:
                r0 = plan["t_row0"][k]
                self.logits.setdefault(s.id, []).extend(recorded[0][r0 + c] for c in range(len(emitted)))
                self.rounds.setdefault(s.id, []).append({
                    "position0": n, "draft_tokens": mine, "draft_rows": recorded[1][:g, k].clone(),
                    "target_rows": recorded[0][r0:r0 + g + 1].clone(), "accepted": a, "emitted": list(emitted)})
            if emitted[-1] in self.eos_token_ids or s.num_tokens >= s.max_total_len:
                self._retire(s, finished)
        return finished


    def run(self) -> Dict[int, List[int]]:
        """step() until nothing is running or waiting -> every finished sequence."""
        done = {}
        while self.active or self.waiting_room:
            done.update(self.step())
        return done
