"""torch.autograd.Function wrappers whose forward AND backward are HIP kernel launches.

PyTorch supplies the tape only.  Parameters stay fp32 (master weights); activations and the
weights the kernels read are bf16 copies (``_shadow``), refreshed by the fused AdamW kernel when
the FlatTrainer owns the parameters.

Gradient delivery has two modes per parameter:
  * direct   -- ``param.grad`` is a preallocated fp32 view into the trainer's flat gradient arena
               (``param._vy_direct``): wgrad kernels accumulate straight into it (no temporaries,
               contiguous buckets for the RCCL reducer) and autograd receives ``None``;
  * returned -- otherwise a fresh fp32 gradient is computed and handed back to autograd.
"""
from __future__ import annotations

import os

import weakref
from typing import NamedTuple, Optional

import torch

from . import _lib, lazy_zero, ops
from ._lib import ACT_GELU_ERF, ACT_NONE, VyomHipError
from .autograd import gated_mlp
from .layers.attention import _shadow
from .layers.mask import AttnMask
from .layers.positional_embeddings import resolve_freqs

BF16 = torch.bfloat16


# bumped by FlatTrainer.step(): its AdamW kernel rewrites weights without touching tensor versions
WEIGHT_EPOCH = [0]


class _WtRegistry:
    """Every W^T the dgrad GEMMs read.  The first backward transposes each matrix as it meets it; from
    then on ONE vy_transpose_batched launch per weight epoch refreshes all that were used in the
    previous epoch (the per-matrix launches are latency-bound: ~8 us each, 50 per step).  Owners are
    held weakly: a model that is dropped, or no longer trained, falls out of the batch."""

    def __init__(self) -> None:
        self.entries = []      # [weakref(owner), key_fn, src_fn, dst_view, last_used_epoch]
        self.batches = {}
        self.epoch_done = -1

    def register(self, owner, key_fn, src_fn, dst):
        e = [weakref.ref(owner), key_fn, src_fn, dst, WEIGHT_EPOCH[0]]
        self.entries.append(e)
        return e

    def refresh(self, hand_off=None):
        """Re-transpose the recently used matrices for the current WEIGHT_EPOCH (once per epoch).
        hand_off: a dtype whose batch is built and accounted for as usual but RETURNED instead of run -- the caller runs
        it before anything reads a W^T (the vocabulary weight gradient carries it as rider workgroups)."""
        ep = WEIGHT_EPOCH[0]
        if self.epoch_done == ep:
            return None
        handed = None
        self.epoch_done = ep
        self.entries = [e for e in self.entries if e[0]() is not None]
        live = [e for e in self.entries if e[4] >= ep - 1 and getattr(e[0](), "_vy_wt_key", None) != e[1](e[0]())]
        if not live:
            return None
        pairs = [(e[2](e[0]()), e[3]) for e in live]
        # one launch per dtype (a bf16 model and an fp32 one trained in the same process share this registry)
        for dt in sorted({s_.dtype for s_, _ in pairs}, key=str):
            sub = [(s_, d_) for s_, d_ in pairs if s_.dtype == dt]
            keys = [(s_.data_ptr(), d_.data_ptr()) for s_, d_ in sub]
            batch = self.batches.get(dt)
            if batch is None or batch.keys != keys:
                batch = self.batches[dt] = ops.TransposeBatch(sub)
            if dt == hand_off:
                handed = batch
            else:
                batch.run()
        for e in live:
            e[0]()._vy_wt_key = e[1](e[0]())
        return handed


_WT = _WtRegistry()


def _wt_cached(owner, key_fn, src_fn) -> torch.Tensor:
    """Shared body of _wt / _wt_packed: owner carries _vy_wt_key / _vy_wt_view / _vy_wt_entry.
    key_fn / src_fn take the owner as their argument (the registry must not keep it alive)."""
    view = getattr(owner, "_vy_wt_view", None)
    key = key_fn(owner)
    entry = getattr(owner, "_vy_wt_entry", None)
    if entry is not None:
        entry[4] = WEIGHT_EPOCH[0]
    if view is not None and getattr(owner, "_vy_wt_key", None) == key:
        return view
    src = src_fn(owner)
    if view is not None and view.dtype == src.dtype and view.device == src.device:
        _WT.refresh()   # weights changed: all recently used matrices in one launch
        if owner._vy_wt_key != key:
            ops.transpose(src, view)   # not in the batch (first use after a pause, or an in-place edit)
            owner._vy_wt_key = key
        return view
    N, K = src.shape
    ld = _row_stride(N)
    view = torch.zeros((K, ld), dtype=src.dtype, device=src.device)[:, :N]  # pad columns stay zero
    ops.transpose(src, view)
    owner._vy_wt_view, owner._vy_wt_key = view, key
    owner._vy_wt_entry = _WT.register(owner, key_fn, src_fn, view)
    return view


_ROW_GRANULE = int(os.environ.get("VY_ROW_GRANULE", "64"))   # (8: the layout of rounds 1-2, for A/B runs)


def _row_stride(n: int) -> int:
    """Row stride (elements) of a matrix with n columns that a GEMM reads as an operand: whole 128-byte lines per row
    (64 bf16), so that no row starts in the middle of a line.  With the 16-byte granule of rounds 1-2 the 50265-wide logits had a
    100,544-byte stride: every second row of the dgrad / wgrad operand began 64 bytes into a line and each 128-byte piece an
    LDS-DMA instruction fetches came from two lines."""
    g = _ROW_GRANULE
    return (n + g - 1) // g * g


def _wt(param: torch.Tensor, dtype) -> torch.Tensor:
    """W^T ([K, N], row stride padded to 8) of a 2-D parameter in `dtype`, cached per version."""
    return _wt_cached(param, lambda p: (p._version, WEIGHT_EPOCH[0], dtype), lambda p: _shadow(p, dtype))


def _direct(p: Optional[torch.Tensor]) -> bool:
    return p is not None and getattr(p, "_vy_direct", False) and p.grad is not None


def _notify(*params) -> None:
    for p in params:
        if p is not None:
            cb = getattr(p, "_vy_ready", None)
            if cb is not None:
                cb(p)


class _WgradGroup:
    """Weight gradients that accumulate straight into the gradient arena do not have to be launched where
    autograd reaches them: the projections of a layer are small wgrad problems (9-36 tiles of 256 x 256),
    and one at a time each needs M-splits -- fp32 atomic traffic -- to fill the chip.  They are collected
    here and go out as ONE launch per ~layer (vy_linear_wgrad_grouped); the parameters are reported ready
    (DDP buckets, per-bucket AdamW) when that launch has been enqueued.  Whatever is still pending when
    the backward pass ends is flushed by an autograd-engine callback.
    The column sums of a LayerNorm backward (dgamma, dbeta: two small launches of their own per LayerNorm) ride in the
    same launch, on the CUs its tiles leave idle (add_colsum); a group may hold nothing else."""

    TILES = int(os.environ.get("VY_WGRAD_GROUP_TILES", "100"))   # flush once this many 256 x 256 output tiles are pending (one post-LN layer: 108)

    def __init__(self):
        self.items, self.colsums, self.tiles, self.armed = [], [], 0, False
        # AdamW ranges waiting for a seat in a launch (add_ride): [ops.AdamWRide, owner]
        self.rides = []

    def add_ride(self, ride, owner) -> None:
        """ride: an ops.AdamWRide whose gradients are final and were written by launches already enqueued.  It is stepped
        by spare workgroups of the next grouped launches that hold a weight gradient, as far as the launcher's budget
        goes -- never by the launch that is being flushed when it is queued: a rider's only ordering against the kernels
        that write its gradients is the stream's kernel boundary.  owner.rode(ranges, bytes) hears what went; whatever is
        still here when backward returns is the owner's to step (take_rides)."""
        self.rides.append([ride, owner])

    def take_rides(self, owner) -> list:
        mine = [r for r, o in self.rides if o is owner]
        self.rides = [e for e in self.rides if e[1] is not owner]
        return mine

    def wants(self, dy, w, alpha) -> bool:
        if alpha is not None or not _GROUP_WGRADS:
            return False
        N, K = w.shape
        return dy.numel() // N >= _GROUP_MIN_ROWS and N < 8192 and N * K >= 512 * 512 and K % 8 == 0

    def add(self, dy, x, w, b) -> None:
        self.add_tensors(dy, x, w.grad, None if b is None else b.grad, [p for p in (w, b) if p is not None])

    def add_tensors(self, dy, x, dw, db, members) -> None:
        """dw / db: the fp32 gradient tensors the launch accumulates into (views of the arena); members: the
        parameters to report ready once it has been enqueued (a packed projection has several)."""
        self.items.append((dy, x, dw, db, members))
        # autograd's own post-accumulate hook fires for these parameters as soon as this backward function
        # returns -- the reducer must not take that for "gradient written" (training.BucketReducer._hook)
        for p in members:
            p._vy_deferred = True
        self.tiles += -(-dw.shape[0] // 256) * -(-dw.shape[1] // 256)
        self._arm()
        if self.tiles >= self.TILES or len(self.items) == 8:
            self.flush()

    def add_colsum(self, ws, dgamma, dbeta, members) -> None:
        """ws: the slab ops.layernorm_bwd_partial left; dgamma / dbeta: the fp32 gradients its column sums are added to."""
        self.colsums.append((ws, dgamma, dbeta, members))
        for p in members:
            p._vy_deferred = True
        self._arm()
        if len(self.colsums) == 8:
            self.flush()

    def _arm(self) -> None:
        if not self.armed:
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)
            self.armed = True

    def flush(self) -> None:
        items, colsums, self.items, self.colsums, self.tiles = self.items, self.colsums, [], [], 0
        if not items and not colsums:
            return
        # the AdamW ranges queued before this flush ride along (what the notifications below queue waits for the next one)
        k = 0   # (the leading ones that share their hyper-parameters: one launch carries one set)
        while items and k < min(8, len(self.rides)) and self.rides[k][0][5:] == self.rides[0][0][5:]:
            k += 1
        rides, self.rides = self.rides[:k], self.rides[k:]
        taken = ops.linear_wgrad_grouped([(dy, x, dw, db) for dy, x, dw, db, _ in items] +
                                         [ops.ColSum(ws, dg, db, True, torch.bfloat16) for ws, dg, db, _ in colsums] +
                                         [r for r, _ in rides])
        if rides:
            left = []
            for (r, owner), got in zip(rides, taken):
                if got:
                    owner.rode(1, got * (30 if r.p_bf16 is not None else 28))
                if got < r.p.numel():   # over budget: the rest keeps its place in the queue
                    left.append([r._replace(p=r.p[got:], g=r.g[got:], m=r.m[got:], v=r.v[got:],
                                            p_bf16=None if r.p_bf16 is None else r.p_bf16[got:]), owner])
            self.rides = left + self.rides
        for *_, members in items + colsums:
            for p in members:
                p._vy_deferred = False
            _notify(*members)

    def _end_of_backward(self) -> None:
        self.armed = False
        self.flush()

    def discard(self) -> None:
        for *_, members in self.items + self.colsums:
            for p in members:
                p._vy_deferred = False
        self.items, self.colsums, self.tiles, self.armed = [], [], 0, False
        self.rides = []


_GROUP_WGRADS = os.environ.get("VY_WGRAD_GROUP", "1") != "0"
_DEFER_RESIDUALS = os.environ.get("VY_DEFER_RESIDUALS", "1") != "0"
_GROUP_MIN_ROWS = int(os.environ.get("VY_WGRAD_GROUP_ROWS", "2048"))   # measured on configs[3] (2112 decoder rows): -6 %
_GROUP_QKV = os.environ.get("VY_WGRAD_GROUP_QKV", "1") != "0"              # the packed QKV gradient joins the group
_GROUP_LN_COLSUMS = os.environ.get("VY_LN_COLSUM_GROUP", "1") != "0"          # LayerNorm dgamma / dbeta sums join it too
_wgrad_group = _WgradGroup()


class _WgradRiders:
    """The vocabulary weight gradient (N >= 8192, M >= 4096: the one 256 x 256 launch that is not grouped) runs 2.3 rounds
    of tiles on the benchmark model and leaves 177 CUs idle for a tile time.  When it is the first launch of backward it
    carries, as rider workgroups (ops.linear_wgrad_riders), the two passes over memory that depend on nothing backward
    produces: the W^T refresh of the weight epoch and the zeroing of the gradient arena (lazy_zero).  What the launcher's
    budget does not take follows in plain launches right behind it.
    on: VY_WGRAD_RIDERS (default on), overridden per backward by FlatTrainer(wgrad_riders=); stats: the running
    trainer's per-step counters."""

    def __init__(self):
        self.on = os.environ.get("VY_WGRAD_RIDERS", "1") != "0"
        self.stats = None

    def carries(self, dy, w, b) -> bool:
        """Will _wgrad(dy, ., w, b) be the direct 256 x 256 bf16 launch?"""
        return (self.on and dy.dtype == BF16 and dy.is_cuda and _direct(w) and (b is None or _direct(b))
                and w.shape[0] >= 8192 and dy.numel() // dy.shape[-1] >= 4096 and w.shape[1] % 8 == 0)

    def launch(self, dy, x, w, b, alpha, claim) -> None:
        """The accumulating weight gradient of (w, b) with whatever may ride.  The transposes read the weights' shadows
        and write the W^T copies, the zero ranges are arena gradients of OTHER parameters: none of them is dy, x, w.grad
        or b.grad (the launcher checks the zero ranges itself)."""
        zero = lazy_zero.take(claim) or []
        batch = _WT.refresh(hand_off=dy.dtype)
        dw, db = w.grad, None if b is None else b.grad
        if not zero and batch is None:
            ops.linear_wgrad(dy, x, dw, db, accumulate=True, alpha=alpha)
            return
        try:
            took, tiles = ops.linear_wgrad_riders(dy, x, dw, db, True, alpha, zero=zero[:8], transposes=batch)
        except BaseException:   # the refresh is already accounted for and the claim is spent: do both before giving up
            if batch is not None:
                batch.run()
            for z in zero:
                z.zero_()
            raise
        took += [0] * (len(zero) - len(took))
        if batch is not None:
            batch.run(first=tiles)
        for z, n in zip(zero, took):
            if n < z.numel():
                z[n:].zero_()
        st = self.stats if claim is None or claim.stats is None else claim.stats
        if st is not None:
            st["zero_rode_bytes"] += 4 * sum(took)
            st["zero_plain_bytes"] += 4 * sum(z.numel() - n for z, n in zip(zero, took))
            if batch is not None:
                st["wt_rode_tiles"] += tiles
                st["wt_plain_tiles"] += batch.total - tiles


_wgrad_riders = _WgradRiders()


def _wgrad(dy, x, w: torch.Tensor, b: Optional[torch.Tensor], alpha: Optional[torch.Tensor] = None, zero_claim=None):
    """-> (dw, db) to return to autograd (None when accumulated in place).  zero_claim: LMHeadLossFn's claim on the
    arena's pending zeroing (only the launch that _wgrad_riders.carries was true for is given one)."""
    if _direct(w) and (b is None or _direct(b)):
        if _wgrad_group.wants(dy, w, alpha):
            _wgrad_group.add(dy, x, w, b)
            return None, None
        if _wgrad_riders.carries(dy, w, b):
            _wgrad_riders.launch(dy, x, w, b, alpha, zero_claim)
        else:
            ops.linear_wgrad(dy, x, w.grad, None if b is None else b.grad, accumulate=True, alpha=alpha)
        _notify(w, b)
        return None, None
    dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
    db = torch.empty(b.shape, dtype=torch.float32, device=w.device) if b is not None else None
    ops.linear_wgrad(dy, x, dw, db, accumulate=False, alpha=alpha)
    return dw.to(w.dtype), (db.to(b.dtype) if b is not None else None)


def _ln_bwd(dy, x, ln_w, ln_b, mean, rstd):
    dt = x.dtype
    if _direct(ln_w) and _direct(ln_b):
        if (_GROUP_LN_COLSUMS and _GROUP_WGRADS and dt == torch.bfloat16
                and x.numel() // x.shape[-1] >= _GROUP_MIN_ROWS):
            dx, ws = ops.layernorm_bwd_partial(dy, x, _shadow(ln_w, dt), mean, rstd)
            _wgrad_group.add_colsum(ws, ln_w.grad, ln_b.grad, [ln_w, ln_b])
            return dx, None, None
        dx = ops.layernorm_bwd(dy, x, _shadow(ln_w, dt), mean, rstd, ln_w.grad, ln_b.grad, accumulate=True)
        _notify(ln_w, ln_b)
        return dx, None, None
    dg = torch.empty(ln_w.shape, dtype=torch.float32, device=x.device)
    db = torch.empty(ln_b.shape, dtype=torch.float32, device=x.device)
    dx = ops.layernorm_bwd(dy, x, _shadow(ln_w, dt), mean, rstd, dg, db, accumulate=False)
    return dx, dg.to(ln_w.dtype), db.to(ln_b.dtype)


def _defer_list(t: torch.Tensor):
    """The list a layer attached to its input tensor (`_vy_defer`): backward functions that produce a
    residual-path gradient for that tensor append it there instead of returning it, and the
    self-attention backward -- which autograd necessarily runs after them -- adds them in its dgrad
    epilogue.  None when the layer did not opt in."""
    return getattr(t, "_vy_defer", None) if t is not None else None


def defer_residual_grads(x: torch.Tensor) -> None:
    """Called by a post-LN transformer layer on its input (training only): see _defer_list."""
    if torch.is_grad_enabled() and x.requires_grad and _DEFER_RESIDUALS:
        x._vy_defer = []


def _require_bf16(x: torch.Tensor) -> None:
    """The training kernels run in bf16 (the measured path: MFMA GEMMs, flash attention) and in fp32 (the parity
    path: plain-FMA kernels, gradients checked against the reference's autograd at 1e-4)."""
    if x.dtype != BF16 and x.dtype != torch.float32:
        raise VyomHipError("training kernels take bf16 or fp32 activations (fp32 master weights), not %s" % x.dtype)


# id(table) -> [forwards recorded, backwards run]: a table that several embeddings share (ELECTRA's generator and
# discriminator, Examples/electra-pretraining.ipynb cell 32) receives one scatter per use, in an order autograd does
# not fix, and is final -- reported to the reducer -- only after the last of them.  The count only decides how EARLY
# the table reports: a table that has been scattered into and is still waiting when the backward pass ends (a forward
# whose graph was dropped, a backward through one of the two uses) is reported then, by an autograd-engine callback.
_EMB_USES = {}
_EMB_WAITING = {}   # id(table) -> table: scattered into during this backward pass, not reported yet


def reset_embedding_uses() -> None:
    """Forget forwards whose backward never ran (FlatTrainer.zero_grad)."""
    _EMB_USES.clear()
    _EMB_WAITING.clear()


def _embedding_end_of_backward() -> None:
    waiting = list(_EMB_WAITING.values())
    _EMB_WAITING.clear()
    for w in waiting:
        _EMB_USES.pop(id(w), None)
        _notify(w)


class EmbeddingFn(torch.autograd.Function):
    """hidden = table[ids] read from the compute-dtype shadow of the fp32 table; the gradient rows are
    accumulated straight into the flat fp32 gradient arena (nn.Embedding: models/decoder.py:287)."""

    @staticmethod
    def forward(ctx, ids, weight, padding_idx, dtype):
        ctx.save_for_backward(ids)
        ctx.weight, ctx.padding_idx = weight, padding_idx
        if _direct(weight):
            _EMB_USES.setdefault(id(weight), [0, 0])[0] += 1
        return ops.embedding(_shadow(weight, dtype), ids)

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        w = ctx.weight
        if _direct(w):
            ops.embedding_bwd_(dout.contiguous(), ids, w.grad, ctx.padding_idx)
            uses = _EMB_USES.get(id(w))
            if uses is not None:
                uses[1] += 1
                if uses[1] < uses[0]:   # another scatter into this table may still come
                    _EMB_WAITING[id(w)] = w
                    torch.autograd.Variable._execution_engine.queue_callback(_embedding_end_of_backward)
                    return None, None, None, None
                del _EMB_USES[id(w)]
                _EMB_WAITING.pop(id(w), None)
            _notify(w)
            return None, None, None, None
        dw = torch.zeros(w.shape, dtype=torch.float32, device=w.device)
        ops.embedding_bwd_(dout.contiguous(), ids, dw, ctx.padding_idx)
        return None, dw.to(w.dtype), None, None


class PatchifyFn(torch.autograd.Function):
    """tokens = patches W^T + b with W the stride == kernel Conv2d weight (d, C, p, p) viewed (d, C*p*p): the
    ViT patch embedding (reference models/vision_encoder.py:83-88, 114).  Backward is the weight / bias
    gradient only -- the pixels are data."""

    @staticmethod
    def forward(ctx, patches, w, b):
        _require_bf16(patches)
        dt = patches.dtype
        ctx.save_for_backward(patches)
        ctx.params = (w, b)
        return ops.linear(patches, _shadow(w, dt).reshape(w.shape[0], -1), _shadow(b, dt))

    @staticmethod
    def backward(ctx, dy):
        (patches,) = ctx.saved_tensors
        w, b = ctx.params
        dy = dy.contiguous()
        N = w.shape[0]
        if _direct(w) and (b is None or _direct(b)):
            ops.linear_wgrad(dy, patches, w.grad.view(N, -1), None if b is None else b.grad, accumulate=True)
            _notify(w, b)
            return None, None, None
        dw = torch.empty((N, w.numel() // N), dtype=torch.float32, device=w.device)
        db = torch.empty(b.shape, dtype=torch.float32, device=w.device) if b is not None else None
        ops.linear_wgrad(dy, patches, dw, db, accumulate=False)
        return None, dw.view(w.shape).to(w.dtype), (db.to(b.dtype) if b is not None else None)


class LinearResidualLayerNormFn(torch.autograd.Function):
    """y = LN(x W^T + b + residual).  AttentionSelfOutput (reference layers/attention.py:69-72)."""

    @staticmethod
    def forward(ctx, x, residual, w, b, ln_w, ln_b, eps, drop=None):
        _require_bf16(x)
        dt = x.dtype
        s = ops.linear(x, _shadow(w, dt), _shadow(b, dt), residual=residual, dropout=drop)
        y, mean, rstd = ops.layernorm(s, _shadow(ln_w, dt), _shadow(ln_b, dt), eps, save_stats=True)
        ctx.save_for_backward(x, s, mean, rstd)
        ctx.params = (w, b, ln_w, ln_b)
        ctx.defer = _defer_list(residual)
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, dy):
        x, s, mean, rstd = ctx.saved_tensors
        w, b, ln_w, ln_b = ctx.params
        dy = dy.contiguous()
        ds, dg, dbt = _ln_bwd(dy, s, ln_w, ln_b, mean, rstd)
        # dropout sits between the projection and the residual add: the projection's gradient is ds under
        # the forward's mask (regenerated from (seed, offset)), the residual's is ds itself
        dz = ops.dropout(ds, *ctx.drop) if ctx.drop is not None else ds
        dx = ops.linear_dgrad(dz, _wt(w, x.dtype))
        dw, db = _wgrad(dz, x, w, b)
        if ctx.defer is not None:      # the residual gradient rides to the QKV dgrad epilogue
            ctx.defer.append(ds)
            ds = None
        return dx, ds, dw, db, dg, dbt, None, None


class FfnBlockFn(torch.autograd.Function):
    """y = LN(act(x W1^T + b1) W2^T + b2 + residual).  FeedForward (reference layers/ffn.py:32-40)."""

    @staticmethod
    def forward(ctx, x, residual, w1, b1, w2, b2, ln_w, ln_b, eps, act, drop=None):
        _require_bf16(x)
        dt = x.dtype
        pre = torch.empty((*x.shape[:-1], w1.shape[0]), dtype=dt, device=x.device)
        hmid = torch.empty_like(pre)
        # `pre` holds act'(x W1^T + b1), not the pre-activation: the backward multiplies by it directly
        ops.linear(x, _shadow(w1, dt), _shadow(b1, dt), act=act | _lib.ACT_SAVE_DERIV, pre_out=pre, out=hmid)
        s = ops.linear(hmid, _shadow(w2, dt), _shadow(b2, dt), residual=residual, dropout=drop)
        ctx.drop = drop
        y, mean, rstd = ops.layernorm(s, _shadow(ln_w, dt), _shadow(ln_b, dt), eps, save_stats=True)
        ctx.save_for_backward(x, pre, hmid, s, mean, rstd)
        ctx.params = (w1, b1, w2, b2, ln_w, ln_b)
        ctx.act = act
        ctx.defer = _defer_list(residual) if residual is not x else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pre, hmid, s, mean, rstd = ctx.saved_tensors
        w1, b1, w2, b2, ln_w, ln_b = ctx.params
        dt = x.dtype
        dy = dy.contiguous()
        ds, dg, dbt = _ln_bwd(dy, s, ln_w, ln_b, mean, rstd)
        dz = ops.dropout(ds, *ctx.drop) if ctx.drop is not None else ds   # the forward's mask (see above)
        dpre = ops.linear_dgrad(dz, _wt(w2, dt), pre=pre, act=ctx.act | _lib.ACT_SAVE_DERIV)  # (dz W2) * act'(pre), act' saved
        dw2, db2 = _wgrad(dz, hmid, w2, b2)
        dx = ops.linear_dgrad(dpre, _wt(w1, dt))
        dw1, db1 = _wgrad(dpre, x, w1, b1)
        if ctx.defer is not None:
            ctx.defer.append(ds)
            ds = None
        return dx, ds, dw1, db1, dw2, db2, dg, dbt, None, None, None


class _AttnArgs(NamedTuple):
    """What the attention kernels take from the mask descriptor and the RoPE slice."""
    causal: bool
    keypad: Optional[torch.Tensor]
    start_pos: int
    cos: Optional[torch.Tensor]
    sin: Optional[torch.Tensor]
    pos0: int


def _attn_args(attention_mask, freqs, S: int, device) -> _AttnArgs:
    """S: the number of keys the kernels see; a wider key-padding row is trimmed to it."""
    if attention_mask is not None and not isinstance(attention_mask, AttnMask):
        raise VyomHipError("training needs a mask descriptor (AttnMask): dense additive masks have no "
                           "backward kernel")
    cos, sin, pos0 = resolve_freqs(freqs, device)
    if attention_mask is None:
        return _AttnArgs(False, None, 0, cos, sin, pos0)
    kp = attention_mask.keypad
    if kp is not None and kp.shape[1] != S:
        kp = kp[:, :S].contiguous()
    return _AttnArgs(attention_mask.causal, kp, attention_mask.start_pos, cos, sin, pos0)


def _heads(x2: torch.Tensor, heads: int, dh: int) -> torch.Tensor:
    B, L, _ = x2.shape
    return x2.view(B, L, heads, dh).permute(0, 2, 1, 3)


def _qkv_heads(packed: torch.Tensor, h: int, hk: int, dh: int):
    """The q / k / v head views (B, heads, L, dh) of packed (B, L, >= (h + 2 hk) dh) rows laid out [q | k | v], 'b l (h d)'."""
    return (_heads(packed[:, :, : h * dh], h, dh), _heads(packed[:, :, h * dh:(h + hk) * dh], hk, dh),
            _heads(packed[:, :, (h + hk) * dh:(h + 2 * hk) * dh], hk, dh))


def _project_qkv(n, mod, am: _AttnArgs, qk=None, delta=None, w=None):
    """The packed q / k / v projection of n (B, L, d) with RoPE -> (q, k, v as (B, heads, L, dh), qkv).  `mod` packs
    q/k/v as the _SelfAttentionBase modules do.  Three ways, each with its own launches and rounding:
      * neither: vy_qkv_rope_fwd writes the rotated q, k and v into three buffers; qkv is None;
      * qk = (q_scale, k_scale, eps), Qwen3's qk_norm: the plain bias-free GEMM keeps the RAW rows in qkv,
        vy_qknorm_rope_fwd writes the normalised, rotated q and k beside them, and v is a strided view of those rows;
      * delta = f(group, y, x), LoRA: the plain GEMM, the adapter's delta behind it -- before RoPE -- and ops.rope_ on the
        q and k views of qkv; all three are views.
    w: a packed weight to use in place of the module's own shadow (DoRA's composed one: dora_train.py)."""
    B, L, _ = n.shape
    h, hk, dh = mod.num_attention_heads, mod.num_key_value_heads, mod.head_dim
    dt, dev = n.dtype, n.device
    sw, sb = mod._packed_shadow(dt)
    if w is not None:
        sw = w
    if delta is not None:
        qkv = torch.empty((B, L, (h + 2 * hk) * dh), dtype=dt, device=dev)
        ops.linear(n, sw, sb, out=qkv)
        delta("qkv", qkv, n)
        q, k, v = _qkv_heads(qkv, h, hk, dh)
        if am.cos is not None:       # (an encoder with absolute or sinusoidal positions has no rotation)
            ops.rope_(q, am.cos, am.sin, am.pos0)
            ops.rope_(k, am.cos, am.sin, am.pos0)
        return q, k, v, qkv
    q = torch.empty((B, h, L, dh), dtype=dt, device=dev)
    k = torch.empty((B, hk, L, dh), dtype=dt, device=dev)
    if qk is not None:
        q_scale, k_scale, qk_eps = qk
        qkv = ops.linear(n, sw)       # (B, L, W): W is a multiple of 8, so the rows are dense
        ops.qknorm_rope(qkv, h, hk, dh, _shadow(q_scale, torch.float32), _shadow(k_scale, torch.float32), qk_eps, am.cos,
                        am.sin, am.pos0, q, k)
        return q, k, _qkv_heads(qkv, h, hk, dh)[2], qkv
    v = torch.empty_like(k)
    ops.qkv_rope(n, sw, sb, h, hk, dh, am.cos, am.sin, am.pos0, q, k, v)
    return q, k, v, None


def _attend(q, k, v, am: _AttnArgs):
    """-> (o (B, L, h dh), lse)."""
    B, h, L, _ = q.shape
    lse = torch.empty((B, h, L), dtype=torch.float32, device=q.device)
    return ops.attention(q, k, v, causal=am.causal, start_pos=am.start_pos, keypad=am.keypad, lse=lse), lse


def _attention_bwd(q, k, v, o, do, lse, am: _AttnArgs) -> torch.Tensor:
    """-> the packed gradient (B, L, (h + 2 hk) dh), [dq | dk | dv] as the packed projection lays its columns out.
    RoPE is orthogonal: its backward (the inverse rotation of dq, dk) runs in the epilogues."""
    B, h, L, dh = q.shape
    hk = k.shape[1]
    packed = torch.empty((B, L, (h + 2 * hk) * dh), dtype=o.dtype, device=o.device)
    dq, dk, dv = _qkv_heads(packed, h, hk, dh)
    ops.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, causal=am.causal, start_pos=am.start_pos, keypad=am.keypad,
                      cos=am.cos, sin=am.sin, rope_pos0=am.pos0)
    return packed


class SelfAttentionFn(torch.autograd.Function):
    """o = merge_heads(softmax(rope(q) rope(k)^T / sqrt(dh) + mask) v) with q,k,v = x W^T + b.
    Inputs after `mod` are the projection parameters in module order (q,k,v weights then biases,
    or the fused qkv weight and bias)."""

    @staticmethod
    def forward(ctx, x, mod, attention_mask, freqs, start_pos, *params):
        _require_bf16(x)
        am = _attn_args(attention_mask, freqs, x.shape[1], x.device)
        q, k, v, _ = _project_qkv(x, mod, am)
        o, lse = _attend(q, k, v, am)
        ctx.save_for_backward(x, q, k, v, o, lse)
        ctx.meta = (mod, am, params)
        ctx.defer = _defer_list(x)
        return o

    @staticmethod
    def backward(ctx, do):
        x, q, k, v, o, lse = ctx.saved_tensors
        mod, am, params = ctx.meta
        dt = x.dtype
        packed = _attention_bwd(q, k, v, o, do.contiguous(), lse, am)
        w, b = mod._packed()
        # the layer input's other gradient contributions (residual paths of this layer's out-projection
        # and feed-forward, deferred by their backward) are added in this GEMM's epilogue
        adds = ctx.defer if ctx.defer is not None else []
        extra = None
        for t in adds[2:]:
            extra = t if extra is None else extra + t
        a1 = adds[0] if len(adds) > 0 else None
        a2 = adds[1] if len(adds) > 1 else None
        if extra is not None:
            a2 = a2 + extra
        dx = ops.linear_dgrad(packed, _wt_packed(mod, w, dt), add_to=a1, add_to2=a2)
        if ctx.defer is not None:
            ctx.defer.clear()
        grads = _packed_wgrad(mod, packed, x, w, b, params)
        return (dx, None, None, None, None, *grads)


class CrossAttentionFn(torch.autograd.Function):
    """o = merge_heads(softmax(q k^T / sqrt(dh) + key-padding mask) v), q = x Wq^T + bq,
    k/v = enc Wk/v^T + b: the encoder-decoder attention of the seq2seq decoder layer
    (reference layers/attention.py:410-474, 512-573).  Gradients flow to the decoder state, to the
    ENCODER output and to the three projections."""

    @staticmethod
    def forward(ctx, x, enc, mod, enc_mask, wq, bq, wk, bk, wv, bv):
        _require_bf16(x)
        B, L, _ = x.shape
        h, hk, dh = mod.num_attention_heads, mod.num_key_value_heads, mod.head_dim
        dt, dev = x.dtype, x.device
        am = _attn_args(enc_mask, None, enc.shape[1], dev)
        if am.causal:
            raise VyomHipError("cross-attention takes a key-padding mask, not a causal one")
        q2 = ops.linear(x, _shadow(wq, dt), _shadow(bq, dt))
        k2 = ops.linear(enc, _shadow(wk, dt), _shadow(bk, dt))
        v2 = ops.linear(enc, _shadow(wv, dt), _shadow(bv, dt))
        lse = torch.empty((B, h, L), dtype=torch.float32, device=dev)
        o = ops.attention(_heads(q2, h, dh), _heads(k2, hk, dh), _heads(v2, hk, dh), causal=False, keypad=am.keypad,
                          lse=lse)
        ctx.save_for_backward(x, enc, q2, k2, v2, o, lse)
        ctx.meta = (mod, am.keypad, (wq, bq, wk, bk, wv, bv))
        return o

    @staticmethod
    def backward(ctx, do):
        x, enc, q2, k2, v2, o, lse = ctx.saved_tensors
        mod, kp, (wq, bq, wk, bk, wv, bv) = ctx.meta
        h, hk, dh = mod.num_attention_heads, mod.num_key_value_heads, mod.head_dim
        dt = x.dtype
        do = do.contiguous()
        dq2, dk2, dv2 = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(v2)
        ops.attention_bwd(_heads(q2, h, dh), _heads(k2, hk, dh), _heads(v2, hk, dh), o, do, lse,
                          _heads(dq2, h, dh), _heads(dk2, hk, dh), _heads(dv2, hk, dh), causal=False, keypad=kp)
        dx = ops.linear_dgrad(dq2, _wt(wq, dt))
        denc = ops.linear_dgrad(dk2, _wt(wk, dt))
        denc = ops.linear_dgrad(dv2, _wt(wv, dt), add_to=denc)
        dwq, dbq = _wgrad(dq2, x, wq, bq)
        dwk, dbk = _wgrad(dk2, enc, wk, bk)
        dwv, dbv = _wgrad(dv2, enc, wv, bv)
        return dx, denc, None, None, dwq, dbq, dwk, dbk, dwv, dbv


def _wt_packed(mod, w, dtype):
    """W^T of the packed projection: keyed on the versions of the member parameters."""
    return _wt_cached(mod, lambda m: tuple(p._version for p in m._params()) + (WEIGHT_EPOCH[0], dtype),
                      lambda m: m._packed_shadow(dtype)[0])


def _packed_wgrad(mod, dy, x, w, b, params):
    members = mod._params()
    nw = 1 if mod._fused_qkv else 3
    ws, bs = members[:nw], members[nw:]
    if all(_direct(p) for p in members):
        # the trainer lays the member gradients out adjacently, mirroring the packed weights
        g0 = ws[0].grad
        N = sum(p.shape[0] for p in ws)
        dw = torch.as_strided(g0, (N, g0.shape[1]), (g0.stride(0), 1))
        ok = all(p.grad.data_ptr() == g0.data_ptr() + off * g0.shape[1] * 4
                 for p, off in zip(ws, _offsets(ws)))
        db = None
        if bs:
            db0 = bs[0].grad
            db = torch.as_strided(db0, (N,), (1,))
            ok = ok and all(p.grad.data_ptr() == db0.data_ptr() + off * 4 for p, off in zip(bs, _offsets(bs)))
        if ok:
            dy2 = dy.view(-1, dy.shape[-1])
            if _GROUP_WGRADS and _GROUP_QKV and dy2.shape[0] >= _GROUP_MIN_ROWS and N * dw.shape[1] >= 512 * 512 and dw.shape[1] % 8 == 0:
                # with the layer's other weight gradients in one grouped launch (27 of its 108 tiles: on its own
                # this launch ran at 670 TFLOP/s, the group at 850)
                _wgrad_group.add_tensors(dy2, x.view(-1, x.shape[-1]), dw, db, list(members))
            else:
                ops.linear_wgrad(dy, x, dw, db, accumulate=True)
                _notify(*members)
            return [None] * len(params)
    N, K = w.shape
    dw = torch.empty((N, K), dtype=torch.float32, device=w.device)
    db = torch.empty((N,), dtype=torch.float32, device=w.device) if b is not None else None
    ops.linear_wgrad(dy, x, dw, db, accumulate=False)
    out, off = [], 0
    for p in ws:
        out.append(dw[off:off + p.shape[0]].to(p.dtype))
        off += p.shape[0]
    off = 0
    for p in bs:
        out.append(db[off:off + p.shape[0]].to(p.dtype))
        off += p.shape[0]
    return out


def _offsets(ps):
    offs, o = [], 0
    for p in ps:
        offs.append(o)
        o += p.shape[0]
    return offs


# ------------------------------------------------------------------------------------------
# Vocabulary heads: the pieces the six Functions below (and the no-grad scoring path) share
# ------------------------------------------------------------------------------------------


def _head_transform(hidden, wd, bd, ln_w, ln_b, eps):
    """n = LN(gelu(h Wd^T + bd)) -> (pre, g, n, mean, rstd), all kept for _head_transform_backward."""
    dt = hidden.dtype
    pre = torch.empty_like(hidden)
    g = torch.empty_like(hidden)
    ops.linear(hidden, _shadow(wd, dt), _shadow(bd, dt), act=ACT_GELU_ERF, pre_out=pre, out=g)
    n, mean, rstd = ops.layernorm(g, _shadow(ln_w, dt), _shadow(ln_b, dt), eps, save_stats=True)
    return pre, g, n, mean, rstd


def _head_transform_backward(dn, hidden, pre, g, mean, rstd, wd, bd, ln_w, ln_b):
    """-> (dh, dwd, dbd, dgamma, dbeta) from dn = d loss / d n."""
    dg, dgam, dbet = _ln_bwd(dn, g, ln_w, ln_b, mean, rstd)
    dpre = ops.act_bwd(dg, pre, ACT_GELU_ERF)
    dh = ops.linear_dgrad(dpre, _wt(wd, hidden.dtype))
    dwd, dbd = _wgrad(dpre, hidden, wd, bd)
    return dh, dwd, dbd, dgam, dbet


def _vocab_logits(n, w, bias, zero_pad=True):
    """logits = n W^T (+ bias) over all B * L rows into a fresh buffer with a padded row stride -> (buf [M, ld],
    logits = buf[:, :V]).  zero_pad: the pad columns are zeroed (only they: the GEMM writes the rest), as the backward
    GEMMs need that contract over the padded width; a reader that stops at V does not."""
    dt = n.dtype
    V = w.shape[0]
    ld = _row_stride(V)
    buf = torch.empty((n.numel() // n.shape[-1], ld), dtype=dt, device=n.device)
    if zero_pad and ld != V:
        buf[:, V:].zero_()
    logits = buf[:, :V]
    ops.linear(n.view(buf.shape[0], -1), _shadow(w, dt), None if bias is None else _shadow(bias, dt), out=logits)
    return buf, logits


def _rehome(x, ld, dtype, reuse=False):
    """x [..., V] in a buffer [..., ld] of `dtype` whose pad columns are zero (ld: a padded row stride, so the rows are
    16-byte aligned and GEMMs can contract over the padded width).  reuse: an x that already sits in such a buffer is
    taken as it is, and only its pad columns are zeroed; otherwise it is copied."""
    V = x.shape[-1]
    if reuse and x.stride(-1) == 1 and x.stride(-2) == ld and x.dtype == dtype:
        buf = torch.as_strided(x, (*x.shape[:-1], ld), x.stride())
        if ld != V:
            buf[..., V:].zero_()
        return buf
    buf = torch.zeros((*x.shape[:-1], ld), dtype=dtype, device=x.device)
    buf[..., :V] = x
    return buf


def _shifted_labels(labels, ignore_index, dev):
    """Position t is scored against token t + 1, the last one against nothing: labels[:, 1:] and one ignore_index per
    sequence, flat [B * L] on dev."""
    shifted = torch.full(labels.shape, ignore_index, dtype=torch.long, device=dev)
    shifted[:, :-1] = labels[:, 1:]
    return shifted.view(-1)


def _xent_forward(logits, shifted, ignore_index, err_flag=None, in_place=True, sample=None):
    """Mean cross-entropy of the live rows -> (loss, lse, acc = [loss_sum, count], fused).  in_place: the logits may
    be overwritten, and where one kernel can do it (vy_xent_fused: bf16, V <= 65536) they then hold the UNIT gradient
    (d loss / d logits for an upstream gradient of 1; backward scales by the actual one, by linearity); otherwise
    vy_xent_fwd only reads them.  sample = (sampled int64 [M], inv_temperature, seed, offset): the same kernels also
    draw a replacement token per live row (vy_xent_sample_*)."""
    V = logits.shape[1]
    dev = logits.device
    lse = torch.empty(logits.shape[0], dtype=torch.float32, device=dev)
    acc = torch.zeros(2, dtype=torch.float32, device=dev)
    fused = in_place and V <= 65536 and logits.dtype == BF16
    if fused:
        # rows with an out-of-range label contribute neither loss nor gradient -- the kernel raises err_flag for
        # them -- so they must not count in the mean either, exactly as on the two-pass path
        acc[1] = ((shifted != ignore_index) & (shifted >= 0) & (shifted < V)).sum()
        if sample is None:
            ops.xent_fused_(logits, shifted, ignore_index, lse, acc[0:1], acc[1:2], _one(dev), err_flag)
        else:
            ops.xent_sample_fused_(logits, shifted, ignore_index, lse, acc[0:1], acc[1:2], _one(dev), *sample, err_flag)
    elif sample is None:
        ops.xent_fwd(logits, shifted, ignore_index, lse, acc[0:1], acc[1:2], err_flag)
    else:
        ops.xent_sample_fwd(logits, shifted, ignore_index, lse, acc[0:1], acc[1:2], *sample, err_flag)
    return acc[0] / acc[1].clamp_min(1.0), lse, acc, fused


def _xent_backward(logits, shifted, ignore_index, lse, acc, fused, gout):
    """logits <- d loss / d logits, up to the factor returned: the upstream gradient as a device scalar where the
    logits already hold the unit gradient (fused), None after vy_xent_bwd has written the scaled one."""
    gs = gout.detach().to(torch.float32).reshape(1).contiguous()
    if fused:
        return gs
    ops.xent_bwd_(logits, shifted, ignore_index, lse, gs, acc[1:2])
    return None


class LMHeadFn(torch.autograd.Function):
    """logits = LN(gelu(h Wd^T + bd)) Wv^T + bias (reference models/decoder.py:267-275).  The logits
    row stride is padded to 8 and the pad columns are zero, so the backward GEMMs can contract
    over the padded width."""

    @staticmethod
    def forward(ctx, hidden, wd, bd, ln_w, ln_b, wv, bias, eps):
        _require_bf16(hidden)
        dt = hidden.dtype
        pre, g, n, mean, rstd = _head_transform(hidden, wd, bd, ln_w, ln_b, eps)
        V = wv.shape[0]
        ld = _row_stride(V)
        buf = torch.zeros((*hidden.shape[:-1], ld), dtype=dt, device=hidden.device)
        logits = buf[..., :V]
        ops.linear(n, _shadow(wv, dt), _shadow(bias, dt), out=logits)
        ctx.save_for_backward(hidden, pre, g, n, mean, rstd)
        ctx.params = (wd, bd, ln_w, ln_b, wv, bias)
        ctx.ld = ld
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        hidden, pre, g, n, mean, rstd = ctx.saved_tensors
        wd, bd, ln_w, ln_b, wv, bias = ctx.params
        dt = hidden.dtype
        # the contraction of the dgrad GEMM runs over the PADDED vocabulary width: a gradient that autograd hands
        # back in the padded logits buffer is used where it is
        buf = _rehome(dlogits, ctx.ld, dt, reuse=True)
        dn = ops.linear_dgrad(buf, _wt_padded(wv, dt, ctx.ld))
        dwv, dbias = _wgrad(buf[..., :wv.shape[0]], n, wv, bias)
        return (*_head_transform_backward(dn, hidden, pre, g, mean, rstd, wd, bd, ln_w, ln_b), dwv, dbias, None)


class LMHeadLossFn(torch.autograd.Function):
    """Shifted causal-LM loss fused with the LM head: mean cross-entropy of logits[:, :-1] against
    labels[:, 1:] with ignore_index (Examples/vyom-ai-decoder_clm.ipynb cell 29).  The logits
    ([M, V] bf16, padded row stride) are produced by the vocabulary GEMM, then reduced AND
    overwritten IN PLACE by their unit gradient in one pass (vy_xent_fused; vy_xent_fwd + vy_xent_bwd
    beyond 65536 columns) -- they are never copied, up-cast or re-materialised (SURVEY.md section 8f
    item 1).  Backward multiplies by the upstream gradient through the GEMMs (a device scalar)."""

    @staticmethod
    def forward(ctx, hidden, labels, ignore_index, wd, bd, ln_w, ln_b, wv, bias, eps, err_flag=None, shift=True,
                sample=None):
        """shift=False: position t is scored against label t (the masked-LM loss).  sample = (inv_temperature, seed,
        offset): also returns one sampled token per position, -1 where the label is ignored (not differentiable)."""
        _require_bf16(hidden)
        pre, g, n, mean, rstd = _head_transform(hidden, wd, bd, ln_w, ln_b, eps)
        buf, logits = _vocab_logits(n, wv, bias)
        dev = hidden.device
        shifted = _shifted_labels(labels, ignore_index, dev) if shift else labels.to(dev).reshape(-1).contiguous()
        sampled = None
        if sample is not None:
            sampled = torch.empty(shifted.shape, dtype=torch.long, device=dev)
            sample = (sampled, *sample)
        loss, lse, acc, fused = _xent_forward(logits, shifted, ignore_index, err_flag, sample=sample)
        ctx.save_for_backward(hidden, pre, g, n, mean, rstd, buf, shifted, lse, acc)
        ctx.params = (wd, bd, ln_w, ln_b, wv, bias)
        ctx.ignore = ignore_index
        ctx.fused = fused
        # the arena's pending zeroing rides in this node's first backward launch, if the trainer finds this node at the
        # root of the loss (lazy_zero); wv / bias are marked so that train_step() clears THEIR gradients at once
        ctx.zero_claim = None
        if _wgrad_riders.carries(logits, wv, bias):
            wv._vy_carrier = True
            if bias is not None:
                bias._vy_carrier = True
            ctx.zero_claim = lazy_zero.PENDING.claim_for(wv.grad, None if bias is None else bias.grad)
        if sampled is None:
            return loss
        sampled = sampled.view(labels.shape)
        ctx.mark_non_differentiable(sampled)
        return loss, sampled

    @staticmethod
    def backward(ctx, gout, *_):
        hidden, pre, g, n, mean, rstd, buf, shifted, lse, acc = ctx.saved_tensors
        wd, bd, ln_w, ln_b, wv, bias = ctx.params
        dt = hidden.dtype
        logits = buf[:, :wv.shape[0]]
        alpha = _xent_backward(logits, shifted, ctx.ignore, lse, acc, ctx.fused, gout)
        # the weight gradient FIRST when it carries riders (_WgradRiders): both GEMMs only read buf and n, that launch does
        # the W^T refresh the dgrad reads, and its parameters' bucket is final one launch earlier.  Any other launch keeps
        # its place behind the dgrad
        first = _wgrad_riders.carries(logits, wv, bias)
        if first:
            dwv, dbias = _wgrad(logits, n.view(buf.shape[0], -1), wv, bias, alpha=alpha, zero_claim=ctx.zero_claim)
        # contract over the padded vocabulary width (pad columns of both operands are zero)
        dn = ops.linear_dgrad(buf, _wt_padded(wv, dt, buf.shape[1]))
        if alpha is not None:
            dn = dn * alpha.to(dt)
        if not first:
            dwv, dbias = _wgrad(logits, n.view(buf.shape[0], -1), wv, bias, alpha=alpha)
        dh, dwd, dbd, dgam, dbet = _head_transform_backward(dn.view(g.shape), hidden, pre, g, mean, rstd, wd, bd, ln_w, ln_b)
        return dh, None, None, dwd, dbd, dgam, dbet, dwv, dbias, None, None, None, None


class BceHeadLossFn(torch.autograd.Function):
    """ELECTRA's discriminator head and loss: mean over the live (non-pad) tokens of
    binary_cross_entropy_with_logits(h . w + b, target) (Examples/electra-pretraining.ipynb cells 21, 27) without an
    N = 1 GEMM: vy_bce_head_fwd / vy_bce_head_bwd read h once each.  -> (loss, z fp32)."""

    @staticmethod
    def forward(ctx, hidden, w, b, target, live):
        _require_bf16(hidden)
        dt = hidden.dtype
        dev = hidden.device
        live8 = live.reshape(-1).to(torch.uint8).contiguous()
        tgt = target.reshape(-1).to(torch.float32).contiguous()
        acc = torch.zeros(2, dtype=torch.float32, device=dev)
        acc[1] = live8.sum()
        ws = _shadow(w, dt).reshape(-1)
        z = ops.bce_head_fwd(hidden, ws, _shadow(b, dt), tgt, live8, acc[0:1])
        ctx.save_for_backward(hidden, z, tgt, live8, acc)
        ctx.params = (w, b)
        ctx.mark_non_differentiable(z)
        return acc[0] / acc[1].clamp_min(1.0), z

    @staticmethod
    def backward(ctx, gout, _gz):
        hidden, z, tgt, live8, acc = ctx.saved_tensors
        w, b = ctx.params
        gs = gout.detach().to(torch.float32).reshape(1).contiguous()
        ws = _shadow(w, hidden.dtype).reshape(-1)
        if _direct(w) and _direct(b):
            dh = ops.bce_head_bwd(hidden, ws, z.view(-1), tgt, live8, gs, acc[1:2], w.grad.view(-1), b.grad, True)
            _notify(w, b)
            return dh, None, None, None, None
        dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
        db = torch.empty(b.shape, dtype=torch.float32, device=w.device)
        dh = ops.bce_head_bwd(hidden, ws, z.view(-1), tgt, live8, gs, acc[1:2], dw.view(-1), db, False)
        return dh, dw.to(w.dtype), db.to(b.dtype), None, None


class BceHeadLogitsFn(torch.autograd.Function):
    """z = h . w + b alone (Discriminator.forward, the notebook's own loop: logits, then ElectraLoss, then backward).
    The backward is vy_bce_head_bwd fed the upstream gradient: its dz is (sigmoid(z) - y) * gscale / count, which
    with z = -inf (sigmoid exactly 0), y = -gz and gscale = count = 1 is gz bit for bit.  -> z fp32 [M]."""

    @staticmethod
    def forward(ctx, hidden, w, b):
        _require_bf16(hidden)
        ctx.save_for_backward(hidden)
        ctx.params = (w, b)
        return ops.bce_head_fwd(hidden, _shadow(w, hidden.dtype).reshape(-1), _shadow(b, hidden.dtype))

    @staticmethod
    def backward(ctx, gz):
        (hidden,) = ctx.saved_tensors
        w, b = ctx.params
        dev = hidden.device
        y = (-gz).to(torch.float32).reshape(-1).contiguous()
        z = torch.full_like(y, float("-inf"))
        live8 = torch.ones(y.shape, dtype=torch.uint8, device=dev)
        ws = _shadow(w, hidden.dtype).reshape(-1)
        if _direct(w) and _direct(b):
            dh = ops.bce_head_bwd(hidden, ws, z, y, live8, _one(dev), _one(dev), w.grad.view(-1), b.grad, True)
            _notify(w, b)
            return dh, None, None
        dw = torch.empty(w.shape, dtype=torch.float32, device=dev)
        db = torch.empty(b.shape, dtype=torch.float32, device=dev)
        dh = ops.bce_head_bwd(hidden, ws, z, y, live8, _one(dev), _one(dev), dw.view(-1), db, False)
        return dh, dw.to(w.dtype), db.to(b.dtype)


def _cls_head_backward(hidden, w, b, dlogits, gs):
    """-> (dh, dw, db) of the classification head to return to autograd (None where accumulated in place)."""
    ws = _shadow(w, hidden.dtype)
    if not w.requires_grad and (b is None or not b.requires_grad):     # a frozen head: only dh is read
        scratch = torch.empty(w.shape, dtype=torch.float32, device=w.device)
        return ops.cls_head_bwd(hidden, ws, dlogits, gs, scratch, None, False), None, None
    if _direct(w) and (b is None or _direct(b)):
        dh = ops.cls_head_bwd(hidden, ws, dlogits, gs, w.grad, None if b is None else b.grad, True)
        _notify(w, b)
        return dh, None, None
    dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
    db = None if b is None else torch.empty(b.shape, dtype=torch.float32, device=w.device)
    dh = ops.cls_head_bwd(hidden, ws, dlogits, gs, dw, db, False)
    return dh, dw.to(w.dtype), None if b is None else db.to(b.dtype)


class ClsHeadLossFn(torch.autograd.Function):
    """The sequence-classification head and its loss: mean CrossEntropyLoss of hidden[:, 0, :] @ W^T + b against the
    labels (Examples/adapters.ipynb and vyom-ai-classification.ipynb, ClinicModel) in vy_cls_head_fwd / vy_cls_head_bwd:
    no gather of the first rows, no (B, L, d) zero-fill pass, no atomics.  -> the loss (fp32 scalar)."""

    @staticmethod
    def forward(ctx, hidden, labels, w, b, err_flag):
        _require_bf16(hidden)
        dt = hidden.dtype
        hidden = hidden.contiguous()
        dlogits, _, loss = ops.cls_head_fwd(hidden, _shadow(w, dt), _shadow(b, dt), labels.reshape(-1).contiguous(),
                                            err_flag)
        ctx.save_for_backward(hidden, dlogits)
        ctx.params = (w, b)
        return loss

    @staticmethod
    def backward(ctx, gout):
        hidden, dlogits = ctx.saved_tensors
        w, b = ctx.params
        gs = gout.detach().to(torch.float32).reshape(1).contiguous()
        dh, dw, db = _cls_head_backward(hidden, w, b, dlogits, gs)
        return dh, None, dw, db, None


class ClsHeadLogitsFn(torch.autograd.Function):
    """logits (B, C) fp32 alone (ClinicModel.forward; the notebook's loop takes its own loss of them)."""

    @staticmethod
    def forward(ctx, hidden, w, b):
        _require_bf16(hidden)
        hidden = hidden.contiguous()
        ctx.save_for_backward(hidden)
        ctx.params = (w, b)
        return ops.cls_head_fwd(hidden, _shadow(w, hidden.dtype), _shadow(b, hidden.dtype))

    @staticmethod
    def backward(ctx, gz):
        (hidden,) = ctx.saved_tensors
        w, b = ctx.params
        dh, dw, db = _cls_head_backward(hidden, w, b, gz.to(torch.float32).contiguous(), None)
        return dh, dw, db


_ONES = {}


def _one(dev) -> torch.Tensor:
    t = _ONES.get(dev)
    if t is None:
        t = _ONES[dev] = torch.ones(1, dtype=torch.float32, device=dev)
    return t


def _wt_padded(param, dtype, ld):
    """[K, ld] zero-padded W^T (full padded width, for contractions over the padded vocabulary)."""
    wt = _wt(param, dtype)
    full = torch.as_strided(wt, (wt.shape[0], ld), (wt.stride(0), 1))
    assert wt.stride(0) == ld
    return full


# ------------------------------------------------------------------------------------------
# Pre-norm residual blocks of the RMSNorm + gated-MLP decoder (reference models/custom_transformer.py)
# ------------------------------------------------------------------------------------------


def _rms_bwd(dy, x, w, eps, add_to=None):
    """-> (dx + add_to, dw to return to autograd or None when accumulated in place): RMSNorm with w_offset = 0."""
    dt = x.dtype
    if not w.requires_grad:   # a frozen weight (LoRA fine-tuning): no gradient is returned, nothing is written to .grad
        scratch = torch.empty(w.shape, dtype=torch.float32, device=x.device)
        return ops.rmsnorm_bwd(dy, x, _shadow(w, dt), eps, 0.0, scratch, False, add_to=add_to), None
    if _direct(w):
        dx = ops.rmsnorm_bwd(dy, x, _shadow(w, dt), eps, 0.0, w.grad, True, add_to=add_to)
        _notify(w)
        return dx, None
    dw = torch.empty(w.shape, dtype=torch.float32, device=x.device)
    dx = ops.rmsnorm_bwd(dy, x, _shadow(w, dt), eps, 0.0, dw, False, add_to=add_to)
    return dx, dw.to(w.dtype)


def _override(weights, group: str, transposed: bool = False):
    """The matrix a block body reads for `group` in place of the module's own shadow (or of its transposed copy), or None.
    weights: None, or an object with w (group -> matrix in the compute dtype) and wt(group) (dora_train.py)."""
    if weights is None or group not in weights.w:
        return None
    return weights.wt(group) if transposed else weights.w[group]


def prenorm_attention_forward(x, mod, attention_mask, freqs, ln_w, eps, wo, qk=None, delta=None, weights=None):
    """y = x + attn(project(RMSNorm(x))) Wo^T: the attention half of a pre-norm block (the reference's DecoderLayer,
    models/custom_transformer.py:268-282) -> (y, (n, q, k, v, qkv, o, lse), am).  `mod`, qk and delta: see _project_qkv,
    the only step that differs between the plain, the qk_norm and the LoRA block; delta is also called behind the
    out-projection, as delta("o", y, o).  weights: see _override (groups "qkv" and "o"); absent, nothing changes."""
    dt = x.dtype
    am = _attn_args(attention_mask, freqs, x.shape[1], x.device)
    n = ops.rmsnorm(x, _shadow(ln_w, dt), eps, 0.0)
    q, k, v, qkv = _project_qkv(n, mod, am, qk, delta, _override(weights, "qkv"))
    o, lse = _attend(q, k, v, am)
    wo_c = _override(weights, "o")
    y = ops.linear(o, _shadow(wo, dt) if wo_c is None else wo_c, None, residual=x)
    if delta is not None:
        delta("o", y, o)
    return y, (n, q, k, v, qkv, o, lse), am


def prenorm_attention_backward(dy, x, n, o, lse, am, mod, ln_w, eps, wo, params=(), q=None, k=None, v=None, qkv=None,
                               qk=None, adapters=None, need_dx=True, weights=None):
    """Backward of prenorm_attention_forward -> (dx, dln_w, dwo, dq_scale, dk_scale, the gradients of `params`, the
    projection's parameters in _params() order), each None where nothing is returned to autograd.  q / k / v that the
    forward left as views of qkv are passed as None and read there.  adapters: None trains the base weights (_wgrad,
    _packed_wgrad); a dict group -> f(dy, x, dx) freezes them and runs the adapter backward of the groups it names
    (lora_train.py), and then need_dx=False skips the packed dgrad and the RMSNorm backward nobody reads.  The residual
    branch's gradient is added in the RMSNorm backward's store (vy_rmsnorm_bwd add_to).  weights: as in the forward; the
    dgrads read its transposed copies."""
    h, hk, dh = mod.num_attention_heads, mod.num_key_value_heads, mod.head_dim
    dt = x.dtype
    dy = dy.contiguous()
    wot = _override(weights, "o", True)
    do = ops.linear_dgrad(dy, _wt(wo, dt) if wot is None else wot)
    dwo = None
    if adapters is None:
        dwo, _ = _wgrad(dy, o, wo, None)
    elif "o" in adapters:
        adapters["o"](dy, o, do)
    if qkv is not None:
        views = _qkv_heads(qkv, h, hk, dh)
        q, k, v = (t if t is not None else view for t, view in zip((q, k, v), views))
    packed = _attention_bwd(q, k, v, o, do, lse, am)
    dqs = dks = None
    if qk is not None:    # the dq | dk columns become the gradient of the raw projection, in place, before both readers
        dqs, dks = _qk_scale_bwd(packed, qkv, h, hk, dh, *qk)
    w, b = mod._packed()
    wt = _override(weights, "qkv", True) if need_dx else None
    dn = ops.linear_dgrad(packed, _wt_packed(mod, w, dt) if wt is None else wt) if need_dx else None
    grads = ()
    if adapters is None:
        grads = _packed_wgrad(mod, packed, n, w, b, params)
    elif "qkv" in adapters:
        adapters["qkv"](packed, n, dn)
    dx = dlnw = None
    if need_dx:
        dx, dlnw = _rms_bwd(dn, x, ln_w, eps, add_to=dy)
    return dx, dlnw, dwo, dqs, dks, grads


class PreNormAttentionFn(torch.autograd.Function):
    """prenorm_attention_forward / _backward with the fused QKV + RoPE projection (biased q/k/v or bias-free, bias-free
    o_proj).  `mod` carries `o_proj`; inputs after `wo` are its q/k/v parameters in _params() order."""

    @staticmethod
    def forward(ctx, x, mod, attention_mask, freqs, ln_w, eps, wo, *params):
        _require_bf16(x)
        y, (n, q, k, v, _, o, lse), am = prenorm_attention_forward(x, mod, attention_mask, freqs, ln_w, eps, wo)
        ctx.save_for_backward(x, n, q, k, v, o, lse)
        ctx.meta = (mod, am, ln_w, eps, wo, params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, n, q, k, v, o, lse = ctx.saved_tensors
        mod, am, ln_w, eps, wo, params = ctx.meta
        dx, dlnw, dwo, _, _, grads = prenorm_attention_backward(dy, x, n, o, lse, am, mod, ln_w, eps, wo, params,
                                                                q=q, k=k, v=v)
        return (dx, None, None, None, dlnw, None, dwo, *grads)


def _qk_scale_bwd(packed, qkv, h, hk, dh, q_scale, k_scale, eps):
    """vy_qknorm_bwd on the packed [dq | dk | dv] buffer, in place -> the two scale gradients to return to autograd.  The
    three ways of _rms_bwd, per scale: accumulated into the arena gradient and reported (None), returned as a tensor, or
    -- a frozen scale -- neither written nor returned."""
    qs, ks = _shadow(q_scale, torch.float32), _shadow(k_scale, torch.float32)
    if _direct(q_scale) and _direct(k_scale) and q_scale.requires_grad and k_scale.requires_grad:
        ops.qknorm_bwd_(packed, qkv, h, hk, dh, qs, ks, eps, q_scale.grad, k_scale.grad, True)
        _notify(q_scale, k_scale)
        return None, None
    dq = torch.empty((dh,), dtype=torch.float32, device=qkv.device)
    dk = torch.empty((dh,), dtype=torch.float32, device=qkv.device)
    ops.qknorm_bwd_(packed, qkv, h, hk, dh, qs, ks, eps, dq, dk, False)
    out = []
    for p, g in ((q_scale, dq), (k_scale, dk)):
        if not p.requires_grad:
            out.append(None)
        elif _direct(p):
            p.grad.add_(g)
            _notify(p)
            out.append(None)
        else:
            out.append(g.to(p.dtype))
    return out[0], out[1]


class PreNormQkNormAttentionFn(torch.autograd.Function):
    """PreNormAttentionFn for a block whose q and k heads pass a per-head RMSNorm between the projection and the rotation
    (Qwen3's qk_norm; Examples/simple_vllm.ipynb, GroupedQueryAttention.forward).  The backward is PreNormAttentionFn's
    with one launch added, vy_qknorm_bwd.  Inputs after `k_scale` are the projection weights in _params() order."""

    @staticmethod
    def forward(ctx, x, mod, attention_mask, freqs, ln_w, eps, wo, q_scale, k_scale, qk_eps, *params):
        _require_bf16(x)
        qk = (q_scale, k_scale, qk_eps)
        y, (n, q, k, _, qkv, o, lse), am = prenorm_attention_forward(x, mod, attention_mask, freqs, ln_w, eps, wo, qk=qk)
        ctx.save_for_backward(x, n, qkv, q, k, o, lse)
        ctx.meta = (mod, am, ln_w, eps, wo, qk, params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, n, qkv, q, k, o, lse = ctx.saved_tensors
        mod, am, ln_w, eps, wo, qk, params = ctx.meta
        dx, dlnw, dwo, dqs, dks, grads = prenorm_attention_backward(dy, x, n, o, lse, am, mod, ln_w, eps, wo, params,
                                                                    q=q, k=k, qkv=qkv, qk=qk)
        return (dx, None, None, None, dlnw, None, dwo, dqs, dks, None, *grads)


def _wt_gate_up(mlp, dtype):
    """W^T of the packed [gate; up] projection of a gated MLP module (gate_proj / up_proj / _packed_gate_up)."""
    return _wt_cached(mlp, lambda m: (m.gate_proj.weight._version, m.up_proj.weight._version, WEIGHT_EPOCH[0], dtype),
                      lambda m: m._packed_gate_up(dtype))


def _gate_up_wgrad(dgu, n, wg, wu):
    """Weight gradients of the packed [gate; up] GEMM, to the two parameters (as _packed_wgrad does for q/k/v)."""
    I, K = wg.shape
    if _direct(wg) and _direct(wu) and wu.grad.data_ptr() == wg.grad.data_ptr() + I * K * 4 \
            and wu.grad.untyped_storage().data_ptr() == wg.grad.untyped_storage().data_ptr():
        # the trainer lays the two gradients out adjacently: one GEMM writes both
        dw = torch.as_strided(wg.grad, (2 * I, K), (K, 1))
        d2, n2 = dgu.view(-1, 2 * I), n.view(-1, K)
        if _GROUP_WGRADS and d2.shape[0] >= _GROUP_MIN_ROWS and 2 * I < 8192 and 2 * I * K >= 512 * 512 and K % 8 == 0:
            _wgrad_group.add_tensors(d2, n2, dw, None, [wg, wu])
        else:
            ops.linear_wgrad(d2, n2, dw, None, accumulate=True)
            _notify(wg, wu)
        return None, None
    dw = torch.empty((2 * I, K), dtype=torch.float32, device=wg.device)
    ops.linear_wgrad(dgu, n, dw, None, accumulate=False)
    outs = []
    for p, part in ((wg, dw[:I]), (wu, dw[I:])):
        if _direct(p):
            p.grad.add_(part)
            _notify(p)
            outs.append(None)
        else:
            outs.append(part.to(p.dtype))
    return outs[0], outs[1]


def prenorm_gated_mlp_forward(x, mlp, ln_w, eps, act, wd, delta=None, weights=None):
    """y = x + (act(n Wg^T) * n Wu^T) Wd^T with n = RMSNorm(x): the MLP half of a pre-norm block (the reference's
    DecoderLayer, models/custom_transformer.py:76-89, 285-288) -> (y, n, gate_up).  delta: see autograd.gated_mlp.
    weights: see _override (groups "gate_up" and "down")."""
    n = ops.rmsnorm(x, _shadow(ln_w, x.dtype), eps, 0.0)
    wd_c = _override(weights, "down")
    y, gu = gated_mlp(n, mlp, act, _shadow(wd, x.dtype) if wd_c is None else wd_c, residual=x, delta=delta,
                      gate_up=_override(weights, "gate_up"))
    return y, n, gu


def prenorm_gated_mlp_backward(dy, x, n, gu, mlp, ln_w, eps, act, wg, wu, wd, adapters=None, weights=None):
    """Backward of prenorm_gated_mlp_forward -> (dx, dln_w, dwg, dwu, dwd).  The gated product is recomputed from gate_up
    (one streaming pass) for whoever reads it: the down projection's weight gradient or its adapter's.  adapters: as in
    prenorm_attention_backward, groups "gate_up" and "down"; weights: as in the forward."""
    dt = x.dtype
    dy = dy.contiguous()
    wdt = _override(weights, "down", True)
    da = ops.linear_dgrad(dy, _wt(wd, dt) if wdt is None else wdt)
    dwg = dwu = dwd = None
    if adapters is None:
        dwd, _ = _wgrad(dy, ops.gated_act(gu, act), wd, None)
    elif "down" in adapters:
        adapters["down"](dy, ops.gated_act(gu, act), da)
    dgu = ops.gated_act_bwd(da, gu, act)
    wgut = _override(weights, "gate_up", True)
    dn = ops.linear_dgrad(dgu, _wt_gate_up(mlp, dt) if wgut is None else wgut)
    if adapters is None:
        dwg, dwu = _gate_up_wgrad(dgu, n, wg, wu)
    elif "gate_up" in adapters:
        adapters["gate_up"](dgu, n, dn)
    dx, dlnw = _rms_bwd(dn, x, ln_w, eps, add_to=dy)
    return dx, dlnw, dwg, dwu, dwd


class PreNormGatedMlpFn(torch.autograd.Function):
    """prenorm_gated_mlp_forward / _backward over the three base weights: one packed [gate; up] GEMM; gate_up and n are
    saved, the gated product is not."""

    @staticmethod
    def forward(ctx, x, mlp, ln_w, eps, act, wg, wu, wd):
        _require_bf16(x)
        y, n, gu = prenorm_gated_mlp_forward(x, mlp, ln_w, eps, act, wd)
        ctx.save_for_backward(x, n, gu)
        ctx.meta = (mlp, ln_w, eps, act, wg, wu, wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, n, gu = ctx.saved_tensors
        dx, dlnw, dwg, dwu, dwd = prenorm_gated_mlp_backward(dy, x, n, gu, *ctx.meta)
        return dx, None, dlnw, None, None, dwg, dwu, dwd


class RMSNormFn(torch.autograd.Function):
    """y = x * rsqrt(mean x^2 + eps) * w (reference models/custom_transformer.py:227-241) on its own: the final norm of
    the trunk when the hidden state itself is asked for."""

    @staticmethod
    def forward(ctx, x, w, eps):
        _require_bf16(x)
        ctx.save_for_backward(x)
        ctx.meta = (w, eps)
        return ops.rmsnorm(x, _shadow(w, x.dtype), eps, 0.0)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        w, eps = ctx.meta
        dx, dw = _rms_bwd(dy.contiguous(), x, w, eps)
        return dx, dw, None


def _tied_head_backward(buf, V, n, table, table_pending, alpha, row_scale=None):
    """Shared backward of the tied vocabulary projection logits = n E^T: buf ([M, ld], pad columns zero) holds
    d loss / d logits (to be scaled by the device scalar alpha when given, and row m by row_scale[m] -- fp32 [M] --
    when given) -> (dn, dE to return to autograd or None).  The row scale never touches buf: dn = s (.) (buf E)
    scales [M, d] rows afterwards, dE = buf^T (s (.) n) scales the rows of n beforehand.
    The embedding table receives the vocabulary weight gradient here and, when it also embedded the input ids of
    this graph (`table_pending`), the embedding scatter later in the same backward: both ACCUMULATE into the one arena
    gradient (zeroed by zero_grad), this one first, and the table is reported ready by the last of them only -- its
    bucket must not be reduced or stepped between the two."""
    dt = n.dtype
    dn = ops.linear_dgrad(buf, _wt_padded(table, dt, buf.shape[1]))
    if alpha is not None:
        dn = dn * alpha.to(dt)
    logits = buf[:, :V]
    n2 = n.view(buf.shape[0], -1)
    if row_scale is not None:
        rs = row_scale.view(-1, 1)
        dn = (dn * rs).to(dt)      # (the products are taken in fp32 and rounded once)
    if not table.requires_grad:    # a frozen table (LoRA fine-tuning): the V x d weight gradient has no reader
        return dn.view(n.shape), None
    if row_scale is not None:
        n2 = (n2 * rs).to(dt)
    if _direct(table):
        ops.linear_wgrad(logits, n2, table.grad, None, accumulate=True, alpha=alpha)
        if not table_pending:
            _notify(table)
        return dn.view(n.shape), None
    dtab = torch.empty(table.shape, dtype=torch.float32, device=table.device)
    ops.linear_wgrad(logits, n2, dtab, None, accumulate=False, alpha=alpha)
    return dn.view(n.shape), dtab.to(table.dtype)


class TiedLMHeadFn(torch.autograd.Function):
    """logits = n E^T with E the embedding table and no bias (reference models/custom_transformer.py:612-613, 662).
    The logits row stride is padded and the pad columns are zero, as in LMHeadFn."""

    @staticmethod
    def forward(ctx, n, table, table_pending):
        _require_bf16(n)
        dt = n.dtype
        V = table.shape[0]
        ld = _row_stride(V)
        buf = torch.zeros((*n.shape[:-1], ld), dtype=dt, device=n.device)
        logits = buf[..., :V]
        ops.linear(n, _shadow(table, dt), None, out=logits)
        ctx.save_for_backward(n)
        ctx.meta = (table, table_pending, ld)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        (n,) = ctx.saved_tensors
        table, table_pending, ld = ctx.meta
        V = table.shape[0]
        buf = _rehome(dlogits.reshape(-1, V), ld, n.dtype)
        dn, dtab = _tied_head_backward(buf, V, n, table, table_pending, None)
        return dn, dtab, None


class ShiftedXentFn(torch.autograd.Function):
    """mean CE(logits[:, :-1], labels[:, 1:]) with ignore_index over MATERIALISED logits (the reference's
    ModelForCausalLM.forward with labels, models/custom_transformer.py:664-672): vy_xent_fwd for the loss, vy_xent_bwd
    on a copy for the gradient.  The fused path that never keeps the logits is TiedLMHeadLossFn."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        _require_bf16(logits)
        B, L, V = logits.shape
        if logits.stride(-1) != 1 or logits.stride(1) % 8 or logits.stride(0) != L * logits.stride(1):
            logits = _rehome(logits, _row_stride(V), logits.dtype)[..., :V]   # rows 16-byte aligned
        l2 = torch.as_strided(logits, (B * L, V), (logits.stride(1), 1), logits.storage_offset())
        shifted = _shifted_labels(labels, ignore_index, logits.device)
        loss, lse, acc, _ = _xent_forward(l2, shifted, ignore_index, in_place=False)
        ctx.save_for_backward(l2, shifted, lse, acc)
        ctx.meta = (ignore_index, (B, L, V))
        return loss

    @staticmethod
    def backward(ctx, gout):
        l2, shifted, lse, acc = ctx.saved_tensors
        ignore_index, shape = ctx.meta
        ld = l2.stride(0)
        buf = torch.empty((l2.shape[0], ld), dtype=l2.dtype, device=l2.device)
        d2 = buf[:, :l2.shape[1]]
        d2.copy_(l2)
        _xent_backward(d2, shifted, ignore_index, lse, acc, False, gout)
        return torch.as_strided(buf, shape, (shape[1] * ld, ld, 1)), None, None


class TiedLMHeadLossFn(torch.autograd.Function):
    """loss = shifted CE(RMSNorm(h) E^T) with E the embedding table: no bias, no transform.  LMHeadLossFn's structure:
    padded row stride, the logits reduced and overwritten in place by their unit gradient (vy_xent_fused: bf16,
    V <= 65536; the two-pass pair otherwise), ignore_index -100."""

    @staticmethod
    def forward(ctx, hidden, labels, ignore_index, ln_w, eps, table, table_pending, err_flag=None):
        _require_bf16(hidden)
        n = ops.rmsnorm(hidden, _shadow(ln_w, hidden.dtype), eps, 0.0)
        buf, logits = _vocab_logits(n, table, None)
        shifted = _shifted_labels(labels, ignore_index, hidden.device)
        loss, lse, acc, fused = _xent_forward(logits, shifted, ignore_index, err_flag)
        ctx.save_for_backward(hidden, n, buf, shifted, lse, acc)
        ctx.meta = (ln_w, eps, table, table_pending, ignore_index, fused)
        return loss

    @staticmethod
    def backward(ctx, gout):
        hidden, n, buf, shifted, lse, acc = ctx.saved_tensors
        ln_w, eps, table, table_pending, ignore_index, fused = ctx.meta
        V = table.shape[0]
        alpha = _xent_backward(buf[:, :V], shifted, ignore_index, lse, acc, fused, gout)
        dn, dtab = _tied_head_backward(buf, V, n, table, table_pending, alpha)
        dh, dlnw = _rms_bwd(dn, hidden, ln_w, eps)
        return dh, None, None, dlnw, None, dtab, None, None


def logprob_rows(input_ids, selection_mask):
    """Row operands of the per-sequence average log-probability (the notebook's compute_logprobs: labels and mask are
    both shifted by one) -> (labels [B*L] int64, w [B, L] fp32): position t is scored against input_ids[t + 1] with
    weight mask[t + 1] / sum(mask[1:]); the last position has weight 0, and so has every position of a sequence whose
    mask is empty (its score is 0, not 0 / 0)."""
    B, L = input_ids.shape
    labels = torch.zeros((B, L), dtype=torch.long, device=input_ids.device)
    labels[:, :-1] = input_ids[:, 1:]
    m = selection_mask.to(device=input_ids.device, dtype=torch.float32)
    w = torch.zeros((B, L), dtype=torch.float32, device=input_ids.device)
    w[:, :-1] = m[:, 1:]
    total = w.sum(-1, keepdim=True)
    w = torch.where(total > 0, w / total.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(w))
    return labels.view(-1), w


def tied_head_logprobs(hidden, labels, w, ln_w, eps, table, err_flag=None, in_place=False):
    """seq_logp[b] = sum_t w[b, t] log softmax(RMSNorm(h) E^T)[b, t, label[b, t]] -> (seq_logp fp32 [B], what
    TiedLMHeadLogprobFn saves).  in_place=False scores only (no-grad): the logits are read by vy_logprob_fwd and freed
    on return, and their pad columns, which that kernel never reads, are not zeroed.  in_place=True leaves in the
    logits u = w (.) (onehot - softmax) for the backward GEMMs: in one pass where vy_logprob_fused applies (bf16,
    V <= 65536), by vy_logprob_bwd in the backward otherwise."""
    dev = hidden.device
    n = ops.rmsnorm(hidden, _shadow(ln_w, hidden.dtype), eps, 0.0)
    buf, logits = _vocab_logits(n, table, None, zero_pad=in_place)
    wrow = w.reshape(-1)
    lse = torch.empty(buf.shape[0], dtype=torch.float32, device=dev)
    logp = torch.empty(buf.shape[0], dtype=torch.float32, device=dev)
    fused = in_place and table.shape[0] <= 65536 and hidden.dtype == BF16
    if fused:
        ops.logprob_fused_(logits, labels, wrow, lse, logp, err_flag)
    else:
        ops.logprob_fwd(logits, labels, wrow, lse, logp, err_flag)
    # one fixed-order reduction per sequence (no atomics, the same bits every run)
    return (logp.view(w.shape) * w).sum(-1), (n, buf, wrow, lse, fused)


class TiedLMHeadLogprobFn(torch.autograd.Function):
    """tied_head_logprobs with a backward: the per-sequence average log-probability of direct preference optimisation
    (Examples/vyom-ai-llm-sft-dpo-training.ipynb: compute_logprobs over model(input_ids).logits).  TiedLMHeadLossFn's
    structure: padded row stride, the logits reduced and overwritten in place by u.  The upstream gradient is
    one number per SEQUENCE and is known only after every sequence has been scored, so it cannot be baked into u:
    the backward applies it as a per-row scale around the two GEMMs and never passes over the logits again."""

    @staticmethod
    def forward(ctx, hidden, labels, w, ln_w, eps, table, table_pending, err_flag=None):
        _require_bf16(hidden)
        seq, (n, buf, wrow, lse, fused) = tied_head_logprobs(hidden, labels, w, ln_w, eps, table, err_flag, in_place=True)
        ctx.save_for_backward(hidden, n, buf, labels, wrow, lse)
        ctx.meta = (ln_w, eps, table, table_pending, fused, w.shape)
        return seq

    @staticmethod
    def backward(ctx, gseq):
        hidden, n, buf, labels, wrow, lse = ctx.saved_tensors
        ln_w, eps, table, table_pending, fused, (B, L) = ctx.meta
        V = table.shape[0]
        if not fused:
            ops.logprob_bwd_(buf[:, :V], labels, wrow, lse)   # logits <- u
        g_row = gseq.detach().to(torch.float32).reshape(B, 1).expand(B, L).reshape(-1)
        dn, dtab = _tied_head_backward(buf, V, n, table, table_pending, None, row_scale=g_row)
        dh, dlnw = _rms_bwd(dn, hidden, ln_w, eps)
        return dh, None, None, dlnw, None, dtab, None, None
