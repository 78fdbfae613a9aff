"""Tensor-level wrappers over the C ABI (include/vyom_hip.h).

PyTorch is used for device memory and the current HIP stream only; every computation below is a
call into libvyom_hip.so.  All functions require CUDA (ROCm) tensors and raise otherwise -- there
is no CPU or eager fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import call, dtype_code

Tensor = torch.Tensor


# ------------------------------------------------------------------------------------------
# Two lanes: the training forward as two batch halves on two HIP streams.
#
# Every kernel of the block forward is row-separable (GEMM rows, LayerNorm rows, attention batches), so the
# first B0 sequences can run through the whole stack on the current stream while the remaining ones run through
# it on a side stream, both writing into the SAME full-batch tensors (which is all the full-batch backward needs).
# What it buys on MI355X: a K = 768 GEMM launch is a k-loop bound by what the CUs take in from L2 followed by an
# epilogue in which all 256 workgroups store at once (HBM-bound, matrix pipe idle) -- a third of the launch.  Two
# independent half-size launch chains drift apart, so one chain's epilogue / LayerNorm / attention softmax runs
# under the other's MFMA loop.
#
# Ordering rules (correct by construction):
#   * lane 1 waits, before each of its launches, for everything the host has enqueued on the main stream so far
#     EXCEPT lane 0's launch of the same op (event recorded first): torch ops on the main stream (mask bytes,
#     casts) are visible to it; it can lag behind lane 0 but never run ahead of the host's program order;
#   * any op that is not lane-aware, and the end of the region, makes the main stream wait for lane 1 first;
#   * the region is entered only where every tensor produced inside is kept until after the join (training
#     forward: saved for backward), so the caching allocator -- which sees main-stream use only -- never hands a
#     block that lane 1 still touches to someone else.
# ------------------------------------------------------------------------------------------


class _Lanes:
    active = False
    side: Optional[torch.cuda.Stream] = None
    fork_ev: Optional[torch.cuda.Event] = None
    join_ev: Optional[torch.cuda.Event] = None
    B = L = B0 = 0
    dirty = False        # lane 1 has work the main stream has not waited for yet
    keep: list = []      # every tensor a split launch touched: alive until the join, whatever the caller does with it
    streams = {}


class lanes:
    """with ops.lanes(B, L, enabled): ... -- see the block comment above.  No-op when not enabled or B < 2."""

    def __init__(self, B: int, L: int, enabled: bool = True):
        self.on = bool(enabled) and B >= 2 and not _Lanes.active and torch.cuda.is_available()
        self.B, self.L = B, L

    def __enter__(self):
        if self.on:
            dev = torch.cuda.current_device()
            st = _Lanes.streams.get(dev)
            if st is None:
                st = _Lanes.streams[dev] = (torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event())
            _Lanes.side, _Lanes.fork_ev, _Lanes.join_ev = st
            _Lanes.B, _Lanes.L, _Lanes.B0 = self.B, self.L, self.B // 2
            _Lanes.active, _Lanes.dirty, _Lanes.keep = True, False, []
            call("vy_set_concurrent_chains", 2)   # (grids are sized on the host, in program order with the launches)
        return self

    def __exit__(self, *exc):
        if self.on:
            _lanes_join()
            _Lanes.active = False
            call("vy_set_concurrent_chains", 1)
            if _Lanes.keep:
                # the allocator may reuse these blocks for main-stream work from here on: that work is ordered behind
                # the join just enqueued
                _Lanes.keep = []
        return False


def _lanes_join() -> None:
    if _Lanes.active and _Lanes.dirty:
        _Lanes.join_ev.record(_Lanes.side)
        torch.cuda.current_stream().wait_event(_Lanes.join_ev)
        _Lanes.dirty = False


def _lane_plan(rows: Optional[int] = None, batches: Optional[int] = None, keep=()):
    """-> [(first, count, stream)] over rows (of a (B*L, .) view) or batches: one entry when the op runs whole, two
    when it is split over the lanes."""
    main = torch.cuda.current_stream()
    if _Lanes.active:
        if rows is not None and rows == _Lanes.B * _Lanes.L:
            cut, n = _Lanes.B0 * _Lanes.L, rows
        elif batches is not None and batches == _Lanes.B:
            cut, n = _Lanes.B0, batches
        else:
            cut = None
        if cut is not None:
            _Lanes.fork_ev.record(main)
            _Lanes.side.wait_event(_Lanes.fork_ev)
            _Lanes.dirty = True
            if keep:
                _Lanes.keep.extend(t for t in keep if t is not None)
            return [(0, cut, main.cuda_stream), (cut, n - cut, _Lanes.side.cuda_stream)]
        _lanes_join()
    n = rows if rows is not None else batches
    return [(0, n, main.cuda_stream)]


def _stream() -> int:
    """The stream of an op that always runs whole (inside a lane region: after the main stream has joined lane 1)."""
    _lanes_join()
    return torch.cuda.current_stream().cuda_stream


_WS = {}
_WS_BYTES = 64 << 20


def _stream_ws() -> Tensor:
    """The current stream's scratch buffer (vy_workspace_set: one per stream, registered once; the library never
    allocates device memory).  Launches on one stream are ordered, so everything on it can share the buffer."""
    st = torch.cuda.current_stream()
    key = (st.device_index, st.cuda_stream)
    if key not in _WS:
        buf = torch.empty(_WS_BYTES, dtype=torch.uint8, device=torch.device("cuda", st.device_index))
        call("vy_workspace_set", st.cuda_stream, buf.data_ptr(), _WS_BYTES)
        _WS[key] = buf
    return _WS[key]


def _mid_ws(rows: int) -> None:
    """Mid-size GEMMs (32 < rows <= 4096) split K over workgroups and need scratch for their fp32 partial tiles."""
    if rows <= 32 or rows > 4096 or _Lanes.active:
        return
    _stream_ws()


def _at(t: Optional[Tensor], first: int):
    """data pointer of t[first:] (None stays None)."""
    if t is None:
        return None
    return t.data_ptr() + first * t.stride(0) * t.element_size()


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _need_gpu(*ts: Optional[Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VyomHipError(
                "vyomai_amd ops run on MI355X only: got a CPU tensor (no CPU fallback exists; "
                "move the module and its inputs to 'cuda')"
            )


def _rows(x: Tensor) -> Tensor:
    """View (..., K) as (M, K) without copying when the rows are uniformly strided."""
    if x.dim() == 2:
        return x if x.stride(1) == 1 else x.contiguous()
    if x.stride(-1) != 1:
        x = x.contiguous()
    try:
        return x.view(-1, x.shape[-1])
    except RuntimeError:
        return x.reshape(-1, x.shape[-1])


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, act: int = _lib.ACT_NONE,
           residual: Optional[Tensor] = None, pre_out: Optional[Tensor] = None,
           out: Optional[Tensor] = None, dropout: Optional[Tuple[float, int, int]] = None) -> Tensor:
    """act(x @ w.T + bias) + residual   (vy_linear_fwd).
    dropout = (p, seed, offset): dropout(x @ w.T + bias) / (1 - p) + residual  (vy_linear_dropout_fwd)."""
    _need_gpu(x, w, bias, residual)
    x2 = _rows(x)
    M, K = x2.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.stride(1) == 1
    r2 = _rows(residual) if residual is not None else None
    if out is None:
        # row stride padded to 8 elements so every row is 16-byte aligned (N = vocab is odd)
        ldy = (N + 7) // 8 * 8
        buf = torch.empty((M, ldy), dtype=x.dtype, device=x.device)
        y2 = buf[:, :N]
        ret = buf.view(*x.shape[:-1], ldy)[..., :N]
    else:
        y2 = _rows(out)
        ret = out
    p2 = _rows(pre_out) if pre_out is not None else None
    if p2 is not None:
        assert p2.stride(0) == y2.stride(0)
    if dropout is not None and dropout[0] > 0.0:
        # (the mask is a function of the global row index: this launch is never split over the lanes)
        assert act == _lib.ACT_NONE and p2 is None
        _mid_ws(M)
        call("vy_linear_dropout_fwd", x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), _ptr(bias),
             _ptr(r2), r2.stride(0) if r2 is not None else 0, y2.data_ptr(), y2.stride(0), M, N, K,
             float(dropout[0]), int(dropout[1]), int(dropout[2]), dtype_code(x.dtype), _stream())
        return ret
    _mid_ws(M)
    whole = _Lanes.active and (x2.data_ptr() != x.data_ptr() or (r2 is not None and r2.data_ptr() != residual.data_ptr()))
    for m0, m, st in ([(0, M, _stream())] if whole else _lane_plan(rows=M, keep=(x2, r2, y2, p2, w, bias))):
        call("vy_linear_fwd", _at(x2, m0), x2.stride(0), w.data_ptr(), w.stride(0), _ptr(bias),
             _at(r2, m0), r2.stride(0) if r2 is not None else 0, _at(y2, m0), y2.stride(0), _at(p2, m0),
             m, N, K, act, dtype_code(x.dtype), st)
    return ret


def qkv_rope(x: Tensor, w_packed: Tensor, b_packed: Optional[Tensor], h: int, hk: int, dh: int,
             cos: Optional[Tensor], sin: Optional[Tensor], pos0: int,
             q: Tensor, k: Tensor, v: Tensor) -> None:
    """Fused projection + RoPE + head split; q/k/v are (B, heads, L, dh) *views* that are written
    in place (k/v may be slices of a static KV cache).  (vy_qkv_rope_fwd)"""
    _need_gpu(x, w_packed, q, k, v)
    B, L, K = x.shape
    x2 = _rows(x)
    for t in (q, k, v):
        assert t.stride(3) == 1
    _mid_ws(B * L)
    whole = _Lanes.active and (x2.data_ptr() != x.data_ptr() or L != _Lanes.L)
    for b0, nb, st in ([(0, B, _stream())] if whole else _lane_plan(batches=B, keep=(x2, q, k, v, w_packed, b_packed))):
        call("vy_qkv_rope_fwd", _at(x2, b0 * L), x2.stride(0), w_packed.data_ptr(), w_packed.stride(0),
             _ptr(b_packed), _ptr(cos), _ptr(sin), pos0,
             _at(q, b0), q.stride(0), q.stride(1), q.stride(2),
             _at(k, b0), k.stride(0), k.stride(1), k.stride(2),
             _at(v, b0), v.stride(0), v.stride(1), v.stride(2),
             nb, L, K, h, hk, dh, dtype_code(x.dtype), st)


def attention(q: Tensor, k: Tensor, v: Tensor, *, causal: bool = False, start_pos: int = 0,
              keypad: Optional[Tensor] = None, addmask: Optional[Tensor] = None,
              scale: Optional[float] = None, lse: Optional[Tensor] = None,
              out: Optional[Tensor] = None) -> Tensor:
    """q (B,h,L,dh), k/v (B,hk,S,dh) -> (B, L, h*dh).  (vy_attn_fwd)"""
    _need_gpu(q, k, v, keypad, addmask)
    B, h, L, dh = q.shape
    hk, S = k.shape[1], k.shape[2]
    if out is None:
        out = torch.empty((B, L, h * dh), dtype=q.dtype, device=q.device)
    kind = 0
    if causal:
        kind |= _lib.MASK_CAUSAL
    if keypad is not None:
        assert keypad.dtype == torch.uint8 and keypad.shape == (B, S) and keypad.stride(1) == 1
        kind |= _lib.MASK_KEYPAD
    am_sb = am_sl = 0
    if addmask is not None:
        assert addmask.dtype == torch.float32 and addmask.dim() == 4 and addmask.stride(3) == 1
        assert addmask.shape[3] == S
        kind |= _lib.MASK_ADDITIVE
        am_sb = addmask.stride(0) if addmask.shape[0] > 1 else 0
        am_sl = addmask.stride(2) if addmask.shape[2] > 1 else 0
    if scale is None:
        scale = 1.0 / math.sqrt(dh)
    if lse is not None:
        assert lse.is_contiguous() and lse.shape == (B, h, L)
    whole = addmask is not None or (_Lanes.active and L != _Lanes.L)
    for b0, nb, st in ([(0, B, _stream())] if whole else _lane_plan(batches=B, keep=(q, k, v, out, lse, keypad))):
        call("vy_attn_fwd", _at(q, b0), q.stride(0), q.stride(1), q.stride(2),
             _at(k, b0), k.stride(0), k.stride(1), k.stride(2),
             _at(v, b0), v.stride(0), v.stride(1), v.stride(2),
             _at(out, b0), out.stride(0), out.stride(1), _at(lse, b0), kind, start_pos,
             _at(keypad, b0), keypad.stride(0) if keypad is not None else 0,
             _ptr(addmask), am_sb, am_sl, nb, h, hk, L, S, dh, float(scale), dtype_code(q.dtype), st)
    return out


def attention_decode(q: Tensor, k: Tensor, v: Tensor, S: int, scale: Optional[float] = None) -> Tensor:
    """q (B,h,1,dh) against cache k/v (B,hk,>=S,dh): attends keys [0,S).  (vy_attn_decode)"""
    _need_gpu(q, k, v)
    B, h, _, dh = q.shape
    hk = k.shape[1]
    out = torch.empty((B, 1, h * dh), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(dh)
    call("vy_attn_decode", q.data_ptr(), q.stride(0), q.stride(1),
         k.data_ptr(), k.stride(0), k.stride(1), k.stride(2),
         v.data_ptr(), v.stride(0), v.stride(1), v.stride(2),
         out.data_ptr(), out.stride(0), B, h, hk, S, dh, float(scale), dtype_code(q.dtype), _stream())
    return out


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float,
              save_stats: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    _need_gpu(x, gamma, beta)
    x2 = _rows(x)
    M, N = x2.shape
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    whole = _Lanes.active and x2.data_ptr() != x.data_ptr()
    for m0, m, st in ([(0, M, _stream())] if whole else _lane_plan(rows=M, keep=(x2, y, mean, rstd, gamma, beta))):
        call("vy_layernorm_fwd", _at(x2, m0), x2.stride(0), gamma.data_ptr(), beta.data_ptr(),
             _at(y, m0), y.stride(0), _at(mean, m0), _at(rstd, m0), m, N, float(eps), dtype_code(x.dtype), st)
    return y.view(x.shape), mean, rstd


def rope_(x: Tensor, cos: Tensor, sin: Tensor, pos0: int = 0, inverse: bool = False) -> Tensor:
    """In-place rotary embedding on (B, heads, L, dh).  (vy_rope_fwd)"""
    _need_gpu(x, cos, sin)
    B, heads, L, dh = x.shape
    assert x.stride(3) == 1
    call("vy_rope_fwd", x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), cos.data_ptr(),
         sin.data_ptr(), pos0, B, heads, L, dh, 1 if inverse else 0, dtype_code(x.dtype), _stream())
    return x


def rope_tables(head_dim: int, max_pos: int, device) -> Tuple[Tensor, Tensor]:
    """fp32 cos/sin of the reference's angle table (VyomAI/layers/positional_embeddings.py:
    127-137, 173-175), half width (the reference concatenates the angles with themselves).
    Evaluated on the host in fp32 exactly like the reference, then uploaded once."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, head_dim, 2).float() / head_dim))
    t = torch.arange(max_pos).type_as(inv_freq)
    ang = torch.einsum("i,j->ij", t, inv_freq)
    return ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)


# ------------------------------------------------------------------------------------------
# backward / training entry points
# ------------------------------------------------------------------------------------------


def linear_dgrad(dy: Tensor, wt: Tensor, pre: Optional[Tensor] = None, act: int = _lib.ACT_NONE,
                 add_to: Optional[Tensor] = None, out: Optional[Tensor] = None,
                 add_to2: Optional[Tensor] = None) -> Tensor:
    """dX = (dY @ W) * act'(pre) + add_to + add_to2, with W^T given ([K, N] row-major).  (vy_linear_dgrad)"""
    _need_gpu(dy, wt, pre, add_to, add_to2)
    if add_to is None and add_to2 is not None:
        add_to, add_to2 = add_to2, None
    d2 = _rows(dy)
    M, N = d2.shape
    K = wt.shape[0]
    assert wt.shape[1] == N and wt.stride(1) == 1
    if out is None:
        out = torch.empty((*dy.shape[:-1], K), dtype=dy.dtype, device=dy.device)
    o2 = _rows(out)
    p2 = _rows(pre) if pre is not None else None
    a2 = _rows(add_to) if add_to is not None else None
    b2 = _rows(add_to2) if add_to2 is not None else None
    _mid_ws(M)
    call("vy_linear_dgrad", d2.data_ptr(), d2.stride(0), wt.data_ptr(), wt.stride(0), _ptr(p2),
         p2.stride(0) if p2 is not None else 0, act, _ptr(a2), a2.stride(0) if a2 is not None else 0,
         _ptr(b2), b2.stride(0) if b2 is not None else 0,
         o2.data_ptr(), o2.stride(0), M, N, K, dtype_code(dy.dtype), _stream())
    return out


def linear_wgrad(dy: Tensor, x: Tensor, dw: Tensor, db: Optional[Tensor], accumulate: bool,
                 alpha: Optional[Tensor] = None) -> None:
    """dw (fp32 [N,K]) (+)= alpha * dy^T @ x ; db (fp32 [N]) (+)= alpha * colsum(dy).  (vy_linear_wgrad)
    alpha: optional fp32 device scalar (read by the kernel, no host sync)."""
    _need_gpu(dy, x, dw, db, alpha)
    assert alpha is None or (alpha.dtype == torch.float32 and alpha.numel() == 1)
    d2, x2 = _rows(dy), _rows(x)
    M, N = d2.shape
    K = x2.shape[1]
    assert dw.dtype == torch.float32 and dw.shape == (N, K) and dw.stride(1) == 1
    call("vy_linear_wgrad", d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0), dw.data_ptr(),
         dw.stride(0), _ptr(db), 1.0 if accumulate else 0.0, _ptr(alpha), M, N, K, dtype_code(dy.dtype), _stream())


def linear_wgrad_riders(dy: Tensor, x: Tensor, dw: Tensor, db: Optional[Tensor], accumulate: bool,
                        alpha: Optional[Tensor] = None, zero=(), transposes: Optional["TransposeBatch"] = None):
    """linear_wgrad with data movement riding on the CUs its last round of tiles leaves idle (vy_linear_wgrad_riders).
    zero: up to 8 contiguous fp32 tensors to clear; transposes: a TransposeBatch none of whose destinations is dy, x,
    dw or db.  -> ([elements of each zero range that were cleared], tiles of the batch that were transposed): the
    launcher takes what its budget allows (nothing outside the 256 x 256 bf16 launch), the rest is the caller's."""
    _need_gpu(dy, x, dw, db, alpha, *zero)
    assert alpha is None or (alpha.dtype == torch.float32 and alpha.numel() == 1)
    d2, x2 = _rows(dy), _rows(x)
    M, N = d2.shape
    K = x2.shape[1]
    assert dw.dtype == torch.float32 and dw.shape == (N, K) and dw.stride(1) == 1
    assert len(zero) <= 8 and all(z.dtype == torch.float32 and z.is_contiguous() for z in zero)
    import ctypes as C
    zd = (_lib.VyZeroRideDesc * max(1, len(zero)))()
    for i, z in enumerate(zero):
        zd[i] = _lib.VyZeroRideDesc(z.data_ptr(), z.numel(), 0)
    took = C.c_int32(0)
    tb = transposes
    call("vy_linear_wgrad_riders", d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0), dw.data_ptr(),
         dw.stride(0), _ptr(db), 1.0 if accumulate else 0.0, _ptr(alpha), M, N, K, dtype_code(dy.dtype),
         C.cast(zd, C.c_void_p) if zero else None, len(zero), tb.table.data_ptr() if tb else None, tb.n if tb else 0,
         tb.total if tb else 0, dtype_code(tb.dtype) if tb else 0, C.byref(took), _stream())
    return [int(zd[i].taken) for i in range(len(zero))], int(took.value)


class ColSum(NamedTuple):
    """An entry of linear_wgrad_grouped's list that is no weight gradient: the column sums of the slab `ws` that
    layernorm_bwd_partial returned, written (accumulate: added) to the fp32 [N] tensors dgamma / dbeta.  dtype: the
    LayerNorm's storage type (it names the path when the list holds nothing else)."""
    ws: Tensor
    dgamma: Tensor
    dbeta: Tensor
    accumulate: bool
    dtype: torch.dtype


class AdamWRide(NamedTuple):
    """An entry of linear_wgrad_grouped's list that is an optimizer update: adamw_step(p, g, m, v, p_bf16, ...) over a
    flat range, done by spare workgroups of the same launch as far as the launcher's budget goes.  The range must not
    depend on the launch (its gradients were written by earlier launches).  Every AdamWRide of a list carries the same
    hyper-parameters."""
    p: Tensor
    g: Tensor
    m: Tensor
    v: Tensor
    p_bf16: Optional[Tensor]
    lr: float
    beta1: float
    beta2: float
    eps: float
    weight_decay: float
    step: int
    grad_scale: float = 1.0


def linear_wgrad_grouped(items):
    """items: up to 8 tuples (dy, x, dw, db|None): dw += dy^T @ x, db += colsum(dy), ONE launch
    (vy_linear_wgrad_grouped).  The tensors must stay alive until the launch has been enqueued (they do:
    the caller holds them).
    The list may also hold up to 8 ColSum entries, summed in the same launch (vy_linear_wgrad_grouped_cs), and
    then need not hold a weight gradient at all.
    It may also hold up to 8 AdamWRide entries (vy_linear_wgrad_grouped_opt); then the return value is the list of how
    many leading elements of each the launch stepped (the launcher's budget decides), otherwise None."""
    import ctypes as C
    rides = [it for it in items if isinstance(it, AdamWRide)]
    colsums = [it for it in items if isinstance(it, ColSum)]
    items = [it for it in items if not isinstance(it, (ColSum, AdamWRide))]
    n, ncs, nopt = len(items), len(colsums), len(rides)
    assert n <= 8 and ncs <= 8 and nopt <= 8 and n + ncs + nopt >= 1
    arr = (_lib.VyWgradDesc * max(n, 1))()
    dt = None
    for i, (dy, x, dw, db) in enumerate(items):
        _need_gpu(dy, x, dw, db)
        d2, x2 = _rows(dy), _rows(x)
        M, N = d2.shape
        K = x2.shape[1]
        assert x2.shape[0] == M and dw.dtype == torch.float32 and dw.shape == (N, K) and dw.stride(1) == 1
        assert db is None or (db.dtype == torch.float32 and db.numel() == N)
        assert dt is None or dt == dy.dtype
        dt = dy.dtype
        a = arr[i]
        a.dy, a.lddy, a.x, a.ldx = d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0)
        a.dw, a.lddw, a.db = dw.data_ptr(), dw.stride(0), _ptr(db)
        a.M, a.N, a.K = M, N, K
    if not ncs and not nopt:
        call("vy_linear_wgrad_grouped", C.cast(arr, C.c_void_p), n, dtype_code(dt), _stream())
        return None
    cs = (_lib.VyColsumDesc * max(ncs, 1))()
    for i, (ws, dgamma, dbeta, accumulate, cdt) in enumerate(colsums):
        _need_gpu(ws, dgamma, dbeta)
        dt = cdt if dt is None else dt
        N = dgamma.numel()
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() % (2 * N) == 0
        assert dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32 and dbeta.numel() == N
        assert dgamma.is_contiguous() and dbeta.is_contiguous()
        c = cs[i]
        c.ws, c.W, c.N = ws.data_ptr(), ws.numel() // (2 * N), N
        c.out0, c.out1, c.acc = dgamma.data_ptr(), dbeta.data_ptr(), 1 if accumulate else 0
    if not nopt:
        call("vy_linear_wgrad_grouped_cs", C.cast(arr, C.c_void_p) if n else None, n, C.cast(cs, C.c_void_p), ncs,
             dtype_code(dt), _stream())
        return None
    opt = (_lib.VyAdamwRideDesc * nopt)()
    hyper = None
    for i, r in enumerate(rides):
        _need_gpu(r.p, r.g, r.m, r.v, r.p_bf16)
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == r.p.numel() for t in (r.p, r.g, r.m, r.v))
        assert r.p_bf16 is None or (r.p_bf16.dtype == torch.bfloat16 and r.p_bf16.is_contiguous() and r.p_bf16.numel() == r.p.numel())
        assert hyper is None or hyper == tuple(r[5:]), "the AdamWRide entries of one launch share their hyper-parameters"
        hyper = tuple(r[5:])
        o = opt[i]
        o.p, o.g, o.m, o.v, o.p_bf16, o.n = r.p.data_ptr(), r.g.data_ptr(), r.m.data_ptr(), r.v.data_ptr(), _ptr(r.p_bf16), r.p.numel()
    lr, beta1, beta2, eps, weight_decay, step, grad_scale = hyper
    hy = _lib.VyAdamwHyper(lr, beta1, beta2, eps, weight_decay, grad_scale, step)
    # (a launch of riders alone runs on the bf16 path: the one with spare workgroups)
    call("vy_linear_wgrad_grouped_opt", C.cast(arr, C.c_void_p) if n else None, n, C.cast(cs, C.c_void_p) if ncs else None, ncs,
         C.cast(opt, C.c_void_p), nopt, C.byref(hy), dtype_code(torch.bfloat16 if dt is None else dt), _stream())
    return [int(o.taken) for o in opt]


def layernorm_bwd_partial(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor):
    """-> (dx, ws): layernorm_bwd without dgamma / dbeta; their per-block partials stay in ws (fp32, [2 * ws_rows * N])
    for a ColSum entry of linear_wgrad_grouped to sum.  (vy_layernorm_bwd_partial)"""
    _need_gpu(dy, x, gamma, mean, rstd)
    d2, x2 = _rows(dy), _rows(x)
    M, N = x2.shape
    dx = torch.empty((M, N), dtype=x.dtype, device=x.device)
    W = _lib.load().vy_layernorm_bwd_ws_rows(M)
    ws = torch.empty((2 * W * N,), dtype=torch.float32, device=x.device)
    call("vy_layernorm_bwd_partial", d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0), gamma.data_ptr(),
         mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dx.stride(0), ws.data_ptr(), M, N, dtype_code(x.dtype), _stream())
    return dx.view(x.shape), ws


def layernorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, dgamma: Tensor,
                  dbeta: Tensor, accumulate: bool) -> Tensor:
    _need_gpu(dy, x, gamma, mean, rstd, dgamma, dbeta)
    d2, x2 = _rows(dy), _rows(x)
    M, N = x2.shape
    dx = torch.empty((M, N), dtype=x.dtype, device=x.device)
    W = _lib.load().vy_layernorm_bwd_ws_rows(M)
    ws = torch.empty((2 * W * N,), dtype=torch.float32, device=x.device)
    call("vy_layernorm_bwd", d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0), gamma.data_ptr(),
         mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dx.stride(0), dgamma.data_ptr(), dbeta.data_ptr(),
         1.0 if accumulate else 0.0, ws.data_ptr(), M, N, dtype_code(x.dtype), _stream())
    return dx.view(x.shape)


def attention_bwd(q, k, v, out, dout, lse, dq, dk, dv, *, causal: bool, start_pos: int = 0,
                  keypad: Optional[Tensor] = None, scale: Optional[float] = None,
                  cos: Optional[Tensor] = None, sin: Optional[Tensor] = None, rope_pos0: int = 0,
                  delta: Optional[Tensor] = None) -> None:
    """Flash attention backward; dq/dk/dv are (B, heads, L|S, dh) views written in place.  delta: optional (B, h, L)
    fp32 workspace the dQ kernel leaves rowsum(dO * O) in (negated on the bf16 path) -- allocated here when None."""
    _need_gpu(q, k, v, out, dout, lse, dq, dk, dv, keypad)
    B, h, L, dh = q.shape
    hk, S = k.shape[1], k.shape[2]
    kind = (_lib.MASK_CAUSAL if causal else 0) | (_lib.MASK_KEYPAD if keypad is not None else 0)
    if scale is None:
        scale = 1.0 / math.sqrt(dh)
    assert out.stride() == dout.stride() and out.stride(2) == 1
    if delta is None:
        delta = torch.empty((B, h, L), dtype=torch.float32, device=q.device)
    assert delta.dtype == torch.float32 and delta.is_contiguous() and delta.shape == (B, h, L)
    call("vy_attn_bwd", q.data_ptr(), q.stride(0), q.stride(1), q.stride(2),
         k.data_ptr(), k.stride(0), k.stride(1), k.stride(2),
         v.data_ptr(), v.stride(0), v.stride(1), v.stride(2),
         out.data_ptr(), dout.data_ptr(), out.stride(0), out.stride(1), lse.data_ptr(), delta.data_ptr(),
         dq.data_ptr(), dq.stride(0), dq.stride(1), dq.stride(2),
         dk.data_ptr(), dk.stride(0), dk.stride(1), dk.stride(2),
         dv.data_ptr(), dv.stride(0), dv.stride(1), dv.stride(2),
         kind, start_pos, _ptr(keypad), keypad.stride(0) if keypad is not None else 0,
         _ptr(cos), _ptr(sin), rope_pos0,
         B, h, hk, L, S, dh, float(scale), dtype_code(q.dtype), _stream())


def adamw_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Optional[Tensor], lr: float,
               beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
               grad_scale: float = 1.0, scale_dev: Optional[Tensor] = None, gate: Optional[Tensor] = None) -> None:
    """scale_dev: optional fp32 device scalar multiplied into grad_scale by the kernel (clip coefficient).
    gate: optional fp32 device scalar; when it is 0 the launch changes nothing (vy_adamw_step_gated)."""
    _need_gpu(p, g, m, v, p_bf16, scale_dev, gate)
    assert scale_dev is None or (scale_dev.dtype == torch.float32 and scale_dev.numel() == 1)
    if gate is None:
        call("vy_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(p_bf16), p.numel(),
             lr, beta1, beta2, eps, weight_decay, step, grad_scale, _ptr(scale_dev), _stream())
    else:
        assert gate.dtype == torch.float32 and gate.numel() == 1
        call("vy_adamw_step_gated", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(p_bf16), p.numel(),
             lr, beta1, beta2, eps, weight_decay, step, grad_scale, _ptr(scale_dev), gate.data_ptr(), _stream())


def sumsq(x: Tensor) -> Tensor:
    """sum(x^2) of a contiguous fp32 tensor as a device scalar (vy_sumsq; deterministic)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(1024, dtype=torch.float32, device=x.device)
    call("vy_sumsq", x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), _stream())
    return out[0]


def dropout(x: Tensor, p: float, seed: int, offset: int, out: Optional[Tensor] = None) -> Tensor:
    """x * keep(seed, offset, row, column) / (1 - p) over the (rows, last dim) view of x (vy_dropout): the
    mask vy_linear_dropout_fwd applied in its epilogue for the same (seed, offset)."""
    _need_gpu(x, out)
    x2 = _rows(x)
    if out is None:
        out = torch.empty_like(x2)
        ret = out.view(x.shape)
    else:
        ret = out
    o2 = _rows(out)
    call("vy_dropout", x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), x2.shape[0], x2.shape[1],
         float(p), int(seed), int(offset), dtype_code(x.dtype), _stream())
    return ret


def transpose(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    _need_gpu(x)
    R, C = x.shape
    if out is None:
        out = torch.empty((C, R), dtype=x.dtype, device=x.device)
    call("vy_transpose", x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), R, C, dtype_code(x.dtype), _stream())
    return out


class TransposeBatch:
    """Descriptor table for vy_transpose_batched: many (src [R,C] -> dst [C,R]) pairs, one launch."""

    def __init__(self, pairs) -> None:
        import ctypes as C
        import numpy as np

        class Desc(C.Structure):
            _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("ldin", C.c_int64), ("ldout", C.c_int64),
                        ("R", C.c_int32), ("C", C.c_int32), ("tile0", C.c_int32), ("tiles_c", C.c_int32)]
        assert C.sizeof(Desc) == 48
        arr = (Desc * len(pairs))()
        tile0 = 0
        self.dtype = pairs[0][0].dtype
        for i, (src, dst) in enumerate(pairs):
            _need_gpu(src, dst)
            R, Cc = src.shape
            assert dst.shape == (Cc, R) and src.stride(1) == 1 and dst.stride(1) == 1 and src.dtype == self.dtype
            tc = (Cc + 63) // 64
            arr[i] = Desc(src.data_ptr(), dst.data_ptr(), src.stride(0), dst.stride(0), R, Cc, tile0, tc)
            tile0 += tc * ((R + 63) // 64)
        self.n, self.total = len(pairs), tile0
        self.keys = [(s_.data_ptr(), d_.data_ptr()) for s_, d_ in pairs]
        host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
        self.table = host.to(pairs[0][0].device)

    def run(self, first: int = 0) -> None:
        """first: the leading tiles that are already done (by riders of ops.linear_wgrad_riders)."""
        if first == 0:
            call("vy_transpose_batched", self.table.data_ptr(), self.n, self.total, dtype_code(self.dtype), _stream())
        elif first < self.total:
            call("vy_transpose_batched_range", self.table.data_ptr(), self.n, first, self.total - first,
                 dtype_code(self.dtype), _stream())


def cast(src: Tensor, dst: Tensor) -> Tensor:
    _need_gpu(src, dst)
    call("vy_cast", src.data_ptr(), dst.data_ptr(), src.numel(), dtype_code(src.dtype), dtype_code(dst.dtype), _stream())
    return dst


def act_bwd(dy: Tensor, pre: Tensor, act: int) -> Tensor:
    """dy * act'(pre).  (vy_act_bwd)"""
    _need_gpu(dy, pre)
    d2, p2 = _rows(dy), _rows(pre)
    M, N = p2.shape
    out = torch.empty((M, N), dtype=dy.dtype, device=dy.device)
    call("vy_act_bwd", d2.data_ptr(), d2.stride(0), p2.data_ptr(), p2.stride(0), out.data_ptr(), out.stride(0),
         M, N, act, dtype_code(dy.dtype), _stream())
    return out.view(pre.shape)


def _row_args(logits2d: Tensor, labels: Tensor, *rows: Tensor, scalars=()) -> None:
    """Operand check of the six xent / logprob calls, whose kernels index by row: labels int64 (M,), every other
    per-row operand fp32 (M,), all contiguous; the device scalars fp32 with one element."""
    M = logits2d.shape[0]
    assert labels.dtype == torch.long and labels.numel() == M and labels.is_contiguous()
    for t in rows:
        assert t.dtype == torch.float32 and t.numel() == M and t.is_contiguous()
    for t in scalars:
        assert t.dtype == torch.float32 and t.numel() == 1


def xent_fwd(logits2d: Tensor, labels: Tensor, ignore_index: int, lse: Tensor, loss_sum: Tensor, count: Tensor,
             err_flag: Optional[Tensor] = None) -> None:
    """logits2d: (M, V) view with 16-byte aligned, padded rows; labels int64 (M,).  err_flag: device int32,
    set to 1 when a label is neither ignore_index nor in [0, V) (such rows count as ignored)."""
    _need_gpu(logits2d, labels, lse, loss_sum, count, err_flag)
    _row_args(logits2d, labels, lse, scalars=(loss_sum, count))
    M, V = logits2d.shape
    call("vy_xent_fwd", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), ignore_index, lse.data_ptr(),
         loss_sum.data_ptr(), count.data_ptr(), M, V, _ptr(err_flag), dtype_code(logits2d.dtype), _stream())


def xent_bwd_(logits2d: Tensor, labels: Tensor, ignore_index: int, lse: Tensor, gscale: Tensor, count: Tensor) -> None:
    """Overwrite logits with d loss / d logits (in place)."""
    _need_gpu(logits2d, labels, lse, gscale, count)
    _row_args(logits2d, labels, lse, scalars=(gscale, count))
    M, V = logits2d.shape
    call("vy_xent_bwd", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), ignore_index, lse.data_ptr(),
         gscale.data_ptr(), count.data_ptr(), M, V, dtype_code(logits2d.dtype), _stream())


def xent_fused_(logits2d: Tensor, labels: Tensor, ignore_index: int, lse: Tensor, loss_sum: Tensor,
                count: Tensor, gscale: Tensor, err_flag: Optional[Tensor] = None) -> None:
    """One pass: lse / loss_sum as xent_fwd, then logits <- d loss / d logits in place (vy_xent_fused).
    count (#rows with label != ignore) is an input here."""
    _need_gpu(logits2d, labels, lse, loss_sum, count, gscale, err_flag)
    _row_args(logits2d, labels, lse, scalars=(loss_sum, count, gscale))
    M, V = logits2d.shape
    call("vy_xent_fused", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), ignore_index, lse.data_ptr(),
         loss_sum.data_ptr(), count.data_ptr(), gscale.data_ptr(), M, V, _ptr(err_flag), dtype_code(logits2d.dtype),
         _stream())


def xent_sample_fwd(logits2d: Tensor, labels: Tensor, ignore_index: int, lse: Tensor, loss_sum: Tensor, count: Tensor,
                    sampled: Tensor, inv_temperature: float, seed: int, offset: int,
                    err_flag: Optional[Tensor] = None) -> None:
    """xent_fwd that also draws sampled[m] = argmax_v(logits[m, v] * inv_temperature + gumbel(m, v)) on every live row
    (-1 on skipped rows); sampled int64 (M,) (vy_xent_sample_fwd)."""
    _need_gpu(logits2d, labels, lse, loss_sum, count, sampled, err_flag)
    _row_args(logits2d, labels, lse, scalars=(loss_sum, count))
    M, V = logits2d.shape
    assert sampled.dtype == torch.long and sampled.numel() == M and sampled.is_contiguous()
    call("vy_xent_sample_fwd", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), ignore_index, lse.data_ptr(),
         loss_sum.data_ptr(), count.data_ptr(), sampled.data_ptr(), float(inv_temperature), int(seed), int(offset), M, V,
         _ptr(err_flag), dtype_code(logits2d.dtype), _stream())


def xent_sample_fused_(logits2d: Tensor, labels: Tensor, ignore_index: int, lse: Tensor, loss_sum: Tensor, count: Tensor,
                       gscale: Tensor, sampled: Tensor, inv_temperature: float, seed: int, offset: int,
                       err_flag: Optional[Tensor] = None) -> None:
    """xent_fused_ that also draws `sampled` as xent_sample_fwd does, from the row it holds in registers
    (vy_xent_sample_fused)."""
    _need_gpu(logits2d, labels, lse, loss_sum, count, gscale, sampled, err_flag)
    _row_args(logits2d, labels, lse, scalars=(loss_sum, count, gscale))
    M, V = logits2d.shape
    assert sampled.dtype == torch.long and sampled.numel() == M and sampled.is_contiguous()
    call("vy_xent_sample_fused", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), ignore_index,
         lse.data_ptr(), loss_sum.data_ptr(), count.data_ptr(), gscale.data_ptr(), sampled.data_ptr(),
         float(inv_temperature), int(seed), int(offset), M, V, _ptr(err_flag), dtype_code(logits2d.dtype), _stream())


def gumbel_noise(M: int, V: int, seed: int, offset: int, device) -> Tensor:
    """The (M, V) fp32 noise the two calls above add for the same (seed, offset) (vy_gumbel_noise; for tests)."""
    out = torch.empty((M, V), dtype=torch.float32, device=device)
    _need_gpu(out)
    call("vy_gumbel_noise", out.data_ptr(), out.stride(0), M, V, int(seed), int(offset), _stream())
    return out


def _bce_args(h2: Tensor, w: Tensor, M: int, *rows: Tensor, scalars=()) -> None:
    assert w.dtype == h2.dtype and w.numel() == h2.shape[1] and w.is_contiguous()
    for t in rows:
        assert t.numel() == M and t.is_contiguous()
    for t in scalars:
        assert t.dtype == torch.float32 and t.numel() == 1


def bce_head_fwd(h: Tensor, w: Tensor, b: Optional[Tensor], target: Optional[Tensor] = None,
                 live: Optional[Tensor] = None, loss_sum: Optional[Tensor] = None) -> Tensor:
    """z = h . w + b per row, fp32, shape h.shape[:-1]; with target (fp32 0 / 1) and live (uint8) the BCE-with-logits
    of the live rows is added to the device scalar loss_sum (vy_bce_head_fwd)."""
    _need_gpu(h, w, b, target, live, loss_sum)
    h2 = _rows(h)
    M, d = h2.shape
    z = torch.empty(h.shape[:-1], dtype=torch.float32, device=h.device)
    _bce_args(h2, w, M)
    if target is not None:
        _bce_args(h2, w, M, target, live, scalars=(loss_sum,))
        assert target.dtype == torch.float32 and live.dtype == torch.uint8
    assert b is None or (b.dtype == h.dtype and b.numel() == 1)
    call("vy_bce_head_fwd", h2.data_ptr(), h2.stride(0), w.data_ptr(), _ptr(b), z.data_ptr(), _ptr(target), _ptr(live),
         _ptr(loss_sum), M, d, dtype_code(h.dtype), _stream())
    return z


def bce_head_bwd(h: Tensor, w: Tensor, z: Tensor, target: Tensor, live: Tensor, gscale: Tensor, count: Tensor,
                 dw: Tensor, db: Tensor, accumulate: bool) -> Tensor:
    """-> dh (h's shape and dtype); dw [d] / db [1] fp32 written or (accumulate) added to (vy_bce_head_bwd)."""
    _need_gpu(h, w, z, target, live, gscale, count, dw, db)
    h2 = _rows(h)
    M, d = h2.shape
    _bce_args(h2, w, M, z, target, live, scalars=(gscale, count, db))
    assert z.dtype == torch.float32 and target.dtype == torch.float32 and live.dtype == torch.uint8
    assert dw.dtype == torch.float32 and dw.numel() == d and dw.is_contiguous()
    dh = torch.empty((M, d), dtype=h.dtype, device=h.device)
    call("vy_bce_head_bwd", h2.data_ptr(), h2.stride(0), w.data_ptr(), z.data_ptr(), target.data_ptr(), live.data_ptr(),
         gscale.data_ptr(), count.data_ptr(), dh.data_ptr(), dh.stride(0), dw.data_ptr(), db.data_ptr(),
         1 if accumulate else 0, M, d, dtype_code(h.dtype), _stream())
    return dh.view(h.shape)


def mlm_mask(ids: Tensor, special_ids: Tensor, fraction: float, mask_id: int, vocab: int, ignore_index: int,
             seed: int, offset: int) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (masked_ids, labels, masked bool) of ids' shape (vy_mlm_mask).  special_ids: int64 device list, may be
    empty."""
    _need_gpu(ids, special_ids)
    assert ids.dtype == torch.long and special_ids.dtype == torch.long and special_ids.is_contiguous()
    idc = ids.contiguous()
    out = torch.empty_like(idc)
    labels = torch.empty_like(idc)
    masked = torch.empty(idc.shape, dtype=torch.uint8, device=ids.device)
    ns = special_ids.numel()
    call("vy_mlm_mask", idc.data_ptr(), idc.numel(), special_ids.data_ptr() if ns else None, ns, float(fraction),
         int(mask_id), int(vocab), int(ignore_index), int(seed), int(offset), out.data_ptr(), labels.data_ptr(),
         masked.data_ptr(), _stream())
    return out, labels, masked.view(torch.bool)


def embedding(table: Tensor, ids: Tensor, err_flag: Optional[Tensor] = None) -> Tensor:
    """out[..., :] = table[ids[...], :]  (vy_embedding_fwd).  table: (V, d) bf16/fp32; ids int64."""
    _need_gpu(table, ids, err_flag)
    assert ids.dtype == torch.long and table.dim() == 2 and table.stride(1) == 1
    idc = ids.contiguous()
    V, d = table.shape
    out = torch.empty((*ids.shape, d), dtype=table.dtype, device=table.device)
    call("vy_embedding_fwd", table.data_ptr(), table.stride(0), idc.data_ptr(), out.data_ptr(), d, idc.numel(), d, V,
         _ptr(err_flag), dtype_code(table.dtype), _stream())
    return out


def greedy_step_(logits: Tensor, tokens: Tensor, cur_pos: int, text_mask: Optional[Tensor], eos_ids: Tensor,
                 eos_reached: Tensor, not_done: Optional[Tensor] = None) -> None:
    """One generated position of the greedy loop (vy_greedy_step): tokens[:, cur_pos] <- forced prompt token or
    argmax(logits); eos_reached |= new EOS; not_done (one int32) += rows still running."""
    _need_gpu(logits, tokens, text_mask, eos_ids, eos_reached, not_done)
    assert logits.dim() == 2 and logits.stride(1) == 1 and tokens.dtype == torch.long and tokens.stride(1) == 1
    assert eos_reached.dtype in (torch.bool, torch.uint8) and eos_reached.is_contiguous()
    assert eos_ids.dtype == torch.long and eos_ids.is_contiguous()
    B, V = logits.shape
    assert tokens.shape[0] == B and eos_reached.numel() == B and 0 <= cur_pos < tokens.shape[1]
    if text_mask is not None:
        assert text_mask.dtype in (torch.bool, torch.uint8) and text_mask.stride(1) == 1 and text_mask.shape == tokens.shape
    if not_done is not None:
        assert not_done.dtype == torch.int32 and not_done.numel() == 1
    call("vy_greedy_step", logits.data_ptr(), logits.stride(0), B, V, dtype_code(logits.dtype), tokens.data_ptr(),
         tokens.stride(0), int(cur_pos), _ptr(text_mask), 0 if text_mask is None else text_mask.stride(0),
         eos_ids.data_ptr(), eos_ids.numel(), eos_reached.data_ptr(), _ptr(not_done), _stream())


def sampling_probs(logits: Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0) -> Tensor:
    """fp32 softmax(mask(logits) / temperature) over the last dimension (vy_sampling_probs):
    top_k > 0 and 0 < top_p < 1 mask as TopKProcessor / NucleusProcessor of the reference do."""
    _need_gpu(logits)
    V = logits.shape[-1]
    l2 = logits.reshape(-1, V)
    if l2.stride(1) != 1:
        l2 = l2.contiguous()
    probs = torch.empty((l2.shape[0], V), dtype=torch.float32, device=logits.device)
    if l2.shape[0] == 0:   # no rows (the last round of speculative decoding verifies zero drafts)
        return probs.view(*logits.shape)
    call("vy_sampling_probs", l2.data_ptr(), l2.stride(0), l2.shape[0], V, dtype_code(l2.dtype), float(temperature),
         int(top_k), float(top_p), probs.data_ptr(), probs.stride(0), _stream())
    return probs.view(*logits.shape)


def sample_rows(logits2d: Tensor, inv_temperature: Tensor, top_k: Tensor, top_p: Tensor, seed: Tensor,
                counter: Tensor) -> Tensor:
    """One token per row of logits2d (R, V), every row with its own parameters, in one launch (vy_sample_rows):
    inv_temperature[r] == 0 -> the arg-max; otherwise argmax over the columns vy_sampling_probs keeps for top_k[r] /
    top_p[r] of logit * inv_temperature[r] + gumbel_noise(1, V, seed[r], counter[r])[0].  inv_temperature / top_p fp32,
    top_k int32, seed / counter int64 (a seed is the 64-bit pattern), each (R,) on the logits' device -> int64 (R,).
    inv_temperature must be >= 0 and not NaN; the caller checks (the values are on the device)."""
    if logits2d.dim() != 2 or logits2d.shape[0] < 1 or logits2d.shape[1] < 1 or logits2d.stride(1) != 1:
        raise ValueError(f"sample_rows: logits must be (R, V) with unit column stride, got {tuple(logits2d.shape)} "
                         f"strides {logits2d.stride()}")
    if logits2d.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"sample_rows: logits must be float32 or bfloat16, got {logits2d.dtype}")
    R, V = logits2d.shape
    if logits2d.stride(0) < V:
        raise ValueError(f"sample_rows: row stride {logits2d.stride(0)} is below V = {V}")
    for name, t, dt in (("inv_temperature", inv_temperature, torch.float32), ("top_k", top_k, torch.int32),
                        ("top_p", top_p, torch.float32), ("seed", seed, torch.long), ("counter", counter, torch.long)):
        if not isinstance(t, Tensor) or t.dtype != dt or t.dim() != 1 or t.numel() != R or t.stride(0) != 1:
            raise ValueError(f"sample_rows: {name} must be a contiguous {dt} tensor of {R} elements")
        if t.device != logits2d.device:
            raise ValueError(f"sample_rows: {name} is on {t.device}, the logits on {logits2d.device}")
    _need_gpu(logits2d)
    tokens = torch.empty(R, dtype=torch.long, device=logits2d.device)
    call("vy_sample_rows", logits2d.data_ptr(), logits2d.stride(0), R, V, dtype_code(logits2d.dtype),
         inv_temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), seed.data_ptr(), counter.data_ptr(),
         tokens.data_ptr(), _stream())
    return tokens


def spec_verify(target_logits: Tensor, draft_logits: Tensor, draft_tokens: Tensor, t_row0: Tensor, n_draft: Tensor,
                inv_temperature: Tensor, top_k: Tensor, top_p: Tensor, seed: Tensor, position0: Tensor):
    """The accept / reject / resample rule of speculative decoding for every drafted token of a step, in one launch
    (vy_spec_verify; the rule: include/vyom_hip.h) -> (accept int32 (S, gamma + 1), alt int64 (S, gamma + 1)).
    target_logits (rows, V): sequence s owns rows t_row0[s] .. t_row0[s] + n_draft[s].  draft_logits (gamma, S, V) of
    the same dtype, unit column stride; draft_tokens (gamma, S) int64, contiguous.  t_row0 / n_draft / top_k int32,
    inv_temperature / top_p fp32, seed / position0 int64, each (S,) on the logits' device.  n_draft[s] in [0, gamma]
    and inv_temperature >= 0 are the caller's duty (the values are on the device); a sequence whose rows would leave
    target_logits is not read and gets accept 0, alt -1."""
    if target_logits.dim() != 2 or target_logits.shape[0] < 1 or target_logits.shape[1] < 1 or target_logits.stride(1) != 1:
        raise ValueError(f"spec_verify: target logits must be (rows, V) with unit column stride, got "
                         f"{tuple(target_logits.shape)} strides {target_logits.stride()}")
    if target_logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"spec_verify: logits must be float32 or bfloat16, got {target_logits.dtype}")
    Rt, V = target_logits.shape
    if target_logits.stride(0) < V:
        raise ValueError(f"spec_verify: target row stride {target_logits.stride(0)} is below V = {V}")
    if not isinstance(draft_logits, Tensor) or draft_logits.dim() != 3 or draft_logits.shape[2] != V or \
            not 1 <= draft_logits.shape[0] <= 16 or draft_logits.shape[1] < 1 or draft_logits.stride(2) != 1 or \
            draft_logits.stride(1) < V or draft_logits.stride(0) < 0:
        raise ValueError(f"spec_verify: draft logits must be (gamma, S, {V}) with 1 <= gamma <= 16, unit column stride and "
                         f"a row stride of at least V, got {tuple(getattr(draft_logits, 'shape', ()))}")
    if draft_logits.dtype != target_logits.dtype:
        raise ValueError(f"spec_verify: draft logits are {draft_logits.dtype}, target logits {target_logits.dtype}")
    gamma, S = draft_logits.shape[:2]
    if not isinstance(draft_tokens, Tensor) or draft_tokens.dtype != torch.long or tuple(draft_tokens.shape) != (gamma, S) \
            or not draft_tokens.is_contiguous():
        raise ValueError(f"spec_verify: draft_tokens must be a contiguous int64 tensor of shape ({gamma}, {S})")
    per_seq = (("t_row0", t_row0, torch.int32), ("n_draft", n_draft, torch.int32),
               ("inv_temperature", inv_temperature, torch.float32), ("top_k", top_k, torch.int32),
               ("top_p", top_p, torch.float32), ("seed", seed, torch.long), ("position0", position0, torch.long))
    for name, t, dt in per_seq:
        if not isinstance(t, Tensor) or t.dtype != dt or t.dim() != 1 or t.numel() != S or t.stride(0) != 1:
            raise ValueError(f"spec_verify: {name} must be a contiguous {dt} tensor of {S} elements")
    for name, t in (("draft_logits", draft_logits), ("draft_tokens", draft_tokens)) + tuple(x[:2] for x in per_seq):
        if t.device != target_logits.device:
            raise ValueError(f"spec_verify: {name} is on {t.device}, the target logits on {target_logits.device}")
    _need_gpu(target_logits)
    accept = torch.empty((S, gamma + 1), dtype=torch.int32, device=target_logits.device)
    alt = torch.empty((S, gamma + 1), dtype=torch.long, device=target_logits.device)
    call("vy_spec_verify", target_logits.data_ptr(), target_logits.stride(0), Rt, draft_logits.data_ptr(),
         draft_logits.stride(0), draft_logits.stride(1), S, gamma, V, dtype_code(target_logits.dtype),
         draft_tokens.data_ptr(), t_row0.data_ptr(), n_draft.data_ptr(), inv_temperature.data_ptr(), top_k.data_ptr(),
         top_p.data_ptr(), seed.data_ptr(), position0.data_ptr(), accept.data_ptr(), alt.data_ptr(), _stream())
    return accept, alt


def lora_delta_(y: Tensor, x: Tensor, A: Tensor, B: Tensor, alpha: Tensor, tiles: Tensor, n_tiles: int,
                boundaries: Sequence[int] = (), name: str = "projection") -> Tensor:
    """y[t] += alpha[s] * (x[t] @ A[s].T) @ B[s].T in place for the rows of the tiles, s the tile's adapter slot
    (vy_lora_shrink, then vy_lora_expand; the rule: include/vyom_hip.h) -> y.  y (T, N) is the output of the
    projection's own GEMM over x (T, K) (its row stride may be padded), A (slots, parts * r_pad, K) and
    B (slots, N, r_pad) the stacked adapters of the projection's parts, which start at column 0 and at `boundaries` (at
    most two), alpha fp32 (slots,), tiles the int32 (n_tiles, 3) device view of (row0, nrows <= 16, slot).  n_tiles is
    the host's count: it sizes the grid and 0 launches nothing.  `name`: the projection, for the messages."""
    n_tiles = int(n_tiles)
    if n_tiles == 0:
        return y
    for what, t in (("y", y), ("x", x), ("A", A), ("B", B), ("alpha", alpha), ("tiles", tiles)):
        if not isinstance(t, Tensor):
            raise ValueError(f"lora_delta_ ({name}): {what} must be a tensor")
    if y.dtype not in (torch.float32, torch.bfloat16) or not (x.dtype == A.dtype == B.dtype == y.dtype):
        raise ValueError(f"lora_delta_ ({name}): y, x, A and B must share float32 or bfloat16, got {y.dtype}, {x.dtype}, "
                         f"{A.dtype}, {B.dtype}")
    if y.dim() != 2 or x.dim() != 2 or x.shape[0] != y.shape[0] or y.stride(1) != 1 or x.stride(1) != 1:
        raise ValueError(f"lora_delta_ ({name}): y (T, N) and x (T, K) must be 2-D over the same rows with unit column "
                         f"stride, got {tuple(y.shape)} strides {y.stride()} and {tuple(x.shape)} strides {x.stride()}")
    (T, N), K = y.shape, x.shape[1]
    bounds = [int(b) for b in boundaries]
    if len(bounds) > 2 or any(b % 16 for b in bounds) or bounds != sorted(set(bounds)) or (bounds and not 0 < bounds[0]) \
            or (bounds and bounds[-1] >= N):
        raise ValueError(f"lora_delta_ ({name}): boundaries {bounds} must be at most two increasing multiples of 16 "
                         f"inside (0, {N})")
    if T < 1 or K % 32 or N % 16 or K < 32 or N < 16:
        raise ValueError(f"lora_delta_ ({name}): K = {K} must be a multiple of 32 and N = {N} (every part's width) a "
                         "multiple of 16")
    parts = 1 + len(bounds)
    if A.dim() != 3 or B.dim() != 3 or not A.is_contiguous() or not B.is_contiguous() or A.shape[0] != B.shape[0] \
            or A.shape[2] != K or B.shape[1] != N or B.shape[2] % 32 or A.shape[1] != parts * B.shape[2] or A.shape[0] < 1:
        raise ValueError(f"lora_delta_ ({name}): A must be a contiguous (slots, {parts} * r_pad, {K}) and B a contiguous "
                         f"(slots, {N}, r_pad) tensor with r_pad a multiple of 32, got {tuple(A.shape)} and {tuple(B.shape)}")
    slots, _, r_pad = B.shape
    if alpha.dtype != torch.float32 or alpha.dim() != 1 or alpha.numel() != slots or alpha.stride(0) != 1:
        raise ValueError(f"lora_delta_ ({name}): alpha must be a contiguous float32 tensor of {slots} elements")
    if tiles.dtype != torch.int32 or tiles.numel() != 3 * n_tiles or not tiles.is_contiguous() or n_tiles < 0:
        raise ValueError(f"lora_delta_ ({name}): tiles must be a contiguous int32 tensor of {n_tiles} x 3 elements, got "
                         f"{tiles.dtype} {tuple(tiles.shape)}")
    es = y.element_size()
    if y.stride(0) < N or y.stride(0) % 4 or y.data_ptr() % (4 * es) or x.stride(0) < K or (x.stride(0) * es) % 16 \
            or x.data_ptr() % 16:
        raise ValueError(f"lora_delta_ ({name}): rows of x must be 16-byte aligned and rows of y aligned to four "
                         f"elements (row strides {x.stride(0)}, {y.stride(0)})")
    for what, t in (("x", x), ("A", A), ("B", B), ("alpha", alpha), ("tiles", tiles)):
        if t.device != y.device:
            raise ValueError(f"lora_delta_ ({name}): {what} is on {t.device}, y on {y.device}")
    _need_gpu(y)
    R = parts * r_pad
    u = torch.empty((T, R), dtype=y.dtype, device=y.device)
    st, code = _stream(), dtype_code(y.dtype)
    call("vy_lora_shrink", x.data_ptr(), x.stride(0), A.data_ptr(), tiles.data_ptr(), n_tiles, u.data_ptr(), R, T, K, R,
         slots, code, st)
    call("vy_lora_expand", y.data_ptr(), y.stride(0), u.data_ptr(), R, B.data_ptr(), alpha.data_ptr(), tiles.data_ptr(),
         n_tiles, T, N, r_pad, slots, *(bounds + [N, N])[:2], code, st)
    return y


def _lora_rows(fn: str, name: str, dtype=None, **mats: Tensor):
    """Shared host checks of the LoRA training entries: 2-D tensors of one float32 / bfloat16 dtype on one device over
    the same rows, unit column stride, 16-byte aligned rows -> (rows, dtype)."""
    first = next(iter(mats.values()))
    for what, t in mats.items():
        if not isinstance(t, Tensor):
            raise ValueError(f"{fn} ({name}): {what} must be a tensor")
    dtype = first.dtype if dtype is None else dtype
    if dtype not in (torch.float32, torch.bfloat16) or any(t.dtype != dtype for t in mats.values()):
        raise ValueError(f"{fn} ({name}): {', '.join(mats)} must share float32 or bfloat16, got "
                         f"{[str(t.dtype) for t in mats.values()]}")
    for what, t in mats.items():
        if t.dim() != 2 or t.shape[0] != first.shape[0] or t.shape[0] < 1 or t.stride(1) != 1:
            raise ValueError(f"{fn} ({name}): {what} must be 2-D over the same {first.shape[0]} rows with unit column "
                             f"stride, got {tuple(t.shape)} strides {t.stride()}")
        if (t.stride(0) * t.element_size()) % 16 or t.data_ptr() % 16 or t.stride(0) < t.shape[1]:
            raise ValueError(f"{fn} ({name}): rows of {what} must be 16-byte aligned (row stride {t.stride(0)})")
        if t.device != first.device:
            raise ValueError(f"{fn} ({name}): {what} is on {t.device}, {next(iter(mats))} on {first.device}")
    return first.shape[0], dtype


def _lora_bounds(fn: str, name: str, boundaries: Sequence[int], N: int):
    bounds = [int(b) for b in boundaries]
    if len(bounds) > 2 or any(b % 16 for b in bounds) or bounds != sorted(set(bounds)) or (bounds and not 0 < bounds[0]) \
            or (bounds and bounds[-1] >= N) or N % 16 or N < 16:
        raise ValueError(f"{fn} ({name}): boundaries {bounds} must be at most two increasing multiples of 16 inside "
                         f"(0, {N}), and N a multiple of 16: every part's width is a multiple of 16")
    return bounds


def _lora_tiles(fn: str, name: str, tiles: Tensor, n_tiles: int, like: Tensor) -> None:
    if not isinstance(tiles, Tensor) or tiles.dtype != torch.int32 or tiles.numel() != 3 * n_tiles \
            or not tiles.is_contiguous() or n_tiles < 1 or tiles.device != like.device:
        raise ValueError(f"{fn} ({name}): tiles must be a contiguous int32 tensor of {n_tiles} x 3 elements on {like.device}")


def lora_delta_keep_u_(y: Tensor, x: Tensor, A: Tensor, B: Tensor, alpha: Tensor, tiles: Tensor, n_tiles: int,
                       boundaries: Sequence[int] = (), name: str = "projection") -> Tensor:
    """lora_delta_ for training: y += alpha * (x @ A[0].T) @ B[0].T in place through the same launch pair and the same
    operand layout (A (1, parts * r_pad, K), B (1, N, r_pad), alpha fp32 (1,), one slot) -> u (T, parts * r_pad), the
    shrink's output in the storage dtype, which the backward keeps (vy_lora_wgrad's u).  The tiles must cover every
    row: a row outside them would leave its u unwritten."""
    fn = "lora_delta_keep_u_"
    n_tiles = int(n_tiles)
    T, dt = _lora_rows(fn, name, y=y, x=x)
    (_, N), K = y.shape, x.shape[1]
    bounds = _lora_bounds(fn, name, boundaries, N)
    parts = 1 + len(bounds)
    if K % 32 or K < 32:
        raise ValueError(f"{fn} ({name}): K = {K} must be a multiple of 32")
    for what, t in (("A", A), ("B", B)):
        if not isinstance(t, Tensor) or t.dim() != 3 or t.shape[0] != 1 or not t.is_contiguous() or t.dtype != dt \
                or t.device != y.device:
            raise ValueError(f"{fn} ({name}): {what} must be a contiguous (1, rows, columns) {dt} tensor on {y.device}")
    r_pad = B.shape[2]
    if r_pad not in (32, 64) or tuple(B.shape) != (1, N, r_pad) or tuple(A.shape) != (1, parts * r_pad, K):
        raise ValueError(f"{fn} ({name}): A must be (1, {parts} * r_pad, {K}) and B (1, {N}, r_pad) with r_pad 32 or 64, "
                         f"got {tuple(A.shape)} and {tuple(B.shape)}")
    if not isinstance(alpha, Tensor) or alpha.dtype != torch.float32 or alpha.numel() != 1 or alpha.device != y.device:
        raise ValueError(f"{fn} ({name}): alpha must be a float32 tensor of one element on {y.device}")
    _lora_tiles(fn, name, tiles, n_tiles, y)
    _need_gpu(y)
    R = parts * r_pad
    u = torch.empty((T, R), dtype=dt, device=y.device)
    st, code = _stream(), dtype_code(dt)
    call("vy_lora_shrink", x.data_ptr(), x.stride(0), A.data_ptr(), tiles.data_ptr(), n_tiles, u.data_ptr(), R, T, K, R,
         1, code, st)
    call("vy_lora_expand", y.data_ptr(), y.stride(0), u.data_ptr(), R, B.data_ptr(), alpha.data_ptr(), tiles.data_ptr(),
         n_tiles, T, N, r_pad, 1, *(bounds + [N, N])[:2], code, st)
    return u


def lora_shrink(x: Tensor, A: Tensor, tiles: Tensor, n_tiles: int, name: str = "projection") -> Tensor:
    """u (T, R) = x @ A[0].T over the tiles (vy_lora_shrink, one slot): the first half of lora_delta_keep_u_, for a
    caller that hands u to lora_expand_epi_.  x (T, K), A (1, R, K) contiguous, K and R multiples of 32."""
    fn = "lora_shrink"
    n_tiles = int(n_tiles)
    T, dt = _lora_rows(fn, name, x=x)
    K = x.shape[1]
    if not isinstance(A, Tensor) or A.dim() != 3 or A.shape[0] != 1 or not A.is_contiguous() or A.dtype != dt \
            or A.device != x.device or A.shape[2] != K or A.shape[1] % 32 or A.shape[1] < 32 or K % 32 or K < 32:
        raise ValueError(f"{fn} ({name}): A must be a contiguous (1, R, {K}) {dt} tensor on {x.device} with R and K "
                         f"multiples of 32, got {tuple(getattr(A, 'shape', ()))}")
    _lora_tiles(fn, name, tiles, n_tiles, x)
    _need_gpu(x)
    R = A.shape[1]
    u = torch.empty((T, R), dtype=dt, device=x.device)
    call("vy_lora_shrink", x.data_ptr(), x.stride(0), A.data_ptr(), tiles.data_ptr(), n_tiles, u.data_ptr(), R, T, K, R,
         1, dtype_code(dt), _stream())
    return u


def lora_expand_epi_(z: Tensor, u: Tensor, B: Tensor, alpha: Tensor, tiles: Tensor, n_tiles: int,
                     boundaries: Sequence[int] = (), *, act: Optional[int] = None, pre: Optional[Tensor] = None,
                     residual: Optional[Tensor] = None, dropout=None, mul: Optional[Tensor] = None,
                     out: Optional[Tensor] = None, name: str = "projection") -> Tensor:
    """The expand half of the adapter's delta with the epilogue of the GEMM it follows (vy_lora_expand_epi; the rule:
    include/vyom_hip.h) -> out.  z (T, N): the base GEMM's output with its bias; u (T, parts * r_pad): lora_shrink's
    output; B (1, N, r_pad), alpha fp32 (1,), one slot; v = z + alpha * u @ B.T in fp32, never rounded, then one of
      act=<a vy_act but ACT_NONE>, pre=(T, N):  out = act(v), pre <- act'(v)      (what linear_dgrad(pre=) takes)
      residual=(T, N), dropout=None | (p, seed, offset):  out = dropout(v) + residual, the mask of ops.dropout
      mul=(T, N):  out = v * mul   (the backward behind an adapted GEMM: z the base dgrad, u = lora_dgrad_'s t, B the
                                    transposed stacked A as (1, K, R), mul the saved act')
    r_pad is 32 or 64 (mul=: any multiple of 32 up to 192, no boundaries).  out defaults to z (in place); given, it must
    not overlap pre, residual or mul.  The tiles must cover every row."""
    fn = "lora_expand_epi_"
    n_tiles = int(n_tiles)
    if (act is not None) + (residual is not None) + (mul is not None) != 1:
        raise ValueError(f"{fn} ({name}): give exactly one of act= (with pre=), residual= (with dropout=) and mul=")
    out = z if out is None else out
    mats = dict(z=z, u=u, out=out)
    if act is not None:
        if int(act) not in range(_lib.ACT_GELU_ERF, _lib.ACT_LEAKY_RELU + 1):
            raise ValueError(f"{fn} ({name}): act = {act} must be an activation code other than ACT_NONE (without flags)")
        if pre is None or dropout is not None:
            raise ValueError(f"{fn} ({name}): act= writes act'(v) to pre= and takes no dropout")
        mats["pre"] = pre
        mode = _lib.LORA_EPI_ACT
    else:
        if pre is not None or (mul is not None and dropout is not None):
            raise ValueError(f"{fn} ({name}): pre= belongs to act=, dropout= to residual=")
        if mul is not None:
            mats["mul"], mode = mul, _lib.LORA_EPI_MUL
        else:
            mats["residual"], mode = residual, _lib.LORA_EPI_DROP_RES
    T, dt = _lora_rows(fn, name, **mats)
    N = z.shape[1]
    bounds = _lora_bounds(fn, name, boundaries, N)
    parts = 1 + len(bounds)
    for what, t in mats.items():
        if what != "u" and t.shape[1] != N:
            raise ValueError(f"{fn} ({name}): {what} must be (T, {N}), got {tuple(t.shape)}")
    ranks = range(32, 193, 32) if mul is not None else (32, 64)
    if not isinstance(B, Tensor) or B.dim() != 3 or B.shape[0] != 1 or not B.is_contiguous() or B.dtype != dt \
            or B.device != z.device or B.shape[1] != N or B.shape[2] not in ranks or (mul is not None and bounds):
        raise ValueError(f"{fn} ({name}): B must be a contiguous (1, {N}, r_pad) {dt} tensor on {z.device} with r_pad in "
                         f"{list(ranks)} (mul=: no boundaries), got {tuple(getattr(B, 'shape', ()))}")
    r_pad = B.shape[2]
    if u.shape[1] != parts * r_pad:
        raise ValueError(f"{fn} ({name}): u must be (T, {parts} * {r_pad}), got {tuple(u.shape)}")
    if not isinstance(alpha, Tensor) or alpha.dtype != torch.float32 or alpha.numel() != 1 or alpha.device != z.device:
        raise ValueError(f"{fn} ({name}): alpha must be a float32 tensor of one element on {z.device}")
    _lora_tiles(fn, name, tiles, n_tiles, z)
    for what in ("pre", "residual", "mul"):
        t = mats.get(what)
        if t is not None and t.data_ptr() == out.data_ptr():
            raise ValueError(f"{fn} ({name}): {what} must not be the output buffer")
    p, seed, offset = (0.0, 0, 0) if dropout is None else dropout
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"{fn} ({name}): dropout p = {p} must lie in [0, 1)")
    _need_gpu(z)
    side = pre if act is not None else mul
    call("vy_lora_expand_epi", z.data_ptr(), z.stride(0), out.data_ptr(), out.stride(0), _ptr(side),
         0 if side is None else side.stride(0), _ptr(residual), 0 if residual is None else residual.stride(0),
         u.data_ptr(), u.stride(0), B.data_ptr(), alpha.data_ptr(), tiles.data_ptr(), n_tiles, T, N, r_pad, 1,
         *(bounds + [N, N])[:2], mode, int(act or 0), float(p), int(seed), int(offset), dtype_code(dt), _stream())
    return out


def cls_head_fwd(hidden: Tensor, w: Tensor, bias: Optional[Tensor], labels: Optional[Tensor] = None,
                 err_flag: Optional[Tensor] = None):
    """The classification head over row 0 of every sequence (vy_cls_head_fwd): hidden (B, L, d) contiguous, w (C, d),
    bias (C) in hidden's dtype -> logits fp32 (B, C); with labels (int64, B) -> (dlogits fp32 (B, C) = (softmax -
    onehot) / count in the logits' place, lse fp32 (B), loss fp32 scalar tensor)."""
    _need_gpu(hidden, w, bias, labels, err_flag)
    if hidden.dim() != 3 or not hidden.is_contiguous() or w.dim() != 2 or not w.is_contiguous() \
            or w.shape[1] != hidden.shape[2] or w.dtype != hidden.dtype or hidden.shape[2] % 8:
        raise ValueError(f"cls_head_fwd: hidden must be a contiguous (B, L, d) tensor with d a multiple of 8 and w a "
                         f"contiguous (C, d) tensor of its dtype, got {tuple(hidden.shape)} {hidden.dtype} and "
                         f"{tuple(w.shape)} {w.dtype}")
    B, L, d = hidden.shape
    C = w.shape[0]
    if bias is not None and (bias.dtype != w.dtype or bias.numel() != C or not bias.is_contiguous()):
        raise ValueError(f"cls_head_fwd: bias must be a contiguous ({C},) tensor of w's dtype")
    logits = torch.empty((B, C), dtype=torch.float32, device=hidden.device)
    lse = loss = None
    if labels is not None:
        if labels.dtype != torch.int64 or labels.numel() != B or not labels.is_contiguous():
            raise ValueError(f"cls_head_fwd: labels must be a contiguous int64 tensor of {B} elements")
        if err_flag is not None and (err_flag.dtype != torch.int32 or err_flag.numel() != 1):
            raise ValueError("cls_head_fwd: err_flag must be an int32 tensor of one element")
        lse = torch.empty(B, dtype=torch.float32, device=hidden.device)
        loss = torch.empty((), dtype=torch.float32, device=hidden.device)
    call("vy_cls_head_fwd", hidden.data_ptr(), L * d, w.data_ptr(), _ptr(bias), logits.data_ptr(), _ptr(labels), _ptr(lse),
         _ptr(loss), _ptr(err_flag), B, C, d, dtype_code(hidden.dtype), _stream())
    return logits if labels is None else (logits, lse, loss)


def cls_head_bwd(hidden: Tensor, w: Tensor, dlogits: Tensor, gscale: Optional[Tensor], dw: Tensor,
                 db: Optional[Tensor], accumulate: bool) -> Tensor:
    """-> dh (hidden's shape and dtype): row 0 of every sequence = gscale * dlogits @ w, every other row zero; dw (C, d) /
    db (C) fp32 written or (accumulate) added to (vy_cls_head_bwd).  Deterministic."""
    _need_gpu(hidden, w, dlogits, gscale, dw, db)
    B, L, d = hidden.shape
    C = w.shape[0]
    if not hidden.is_contiguous() or not w.is_contiguous() or w.dtype != hidden.dtype or tuple(w.shape) != (C, d):
        raise ValueError("cls_head_bwd: hidden (B, L, d) and w (C, d) must be contiguous and share a dtype")
    if dlogits.dtype != torch.float32 or tuple(dlogits.shape) != (B, C) or not dlogits.is_contiguous():
        raise ValueError(f"cls_head_bwd: dlogits must be a contiguous float32 ({B}, {C}) tensor")
    if gscale is not None and (gscale.dtype != torch.float32 or gscale.numel() != 1):
        raise ValueError("cls_head_bwd: gscale must be a float32 tensor of one element")
    if dw.dtype != torch.float32 or tuple(dw.shape) != (C, d) or not dw.is_contiguous() \
            or (db is not None and (db.dtype != torch.float32 or db.numel() != C or not db.is_contiguous())):
        raise ValueError(f"cls_head_bwd: dw must be a contiguous float32 ({C}, {d}) tensor and db one of {C} elements")
    dh = torch.empty_like(hidden)
    call("vy_cls_head_bwd", hidden.data_ptr(), L * d, w.data_ptr(), dlogits.data_ptr(), _ptr(gscale), dh.data_ptr(),
         dw.data_ptr(), _ptr(db), 1 if accumulate else 0, B, L, C, d, dtype_code(hidden.dtype), _stream())
    return dh


def lora_dgrad_(dx: Optional[Tensor], dy: Tensor, Bt: Tensor, At: Tensor, alpha: Tensor, tiles: Tensor, n_tiles: int,
                name: str = "projection") -> Tensor:
    """The adapter's two data-gradient products of one GEMM group -> t (M, R) = dy @ B per part, and, when dx is given,
    dx += alpha * t @ A in place (what dx held -- the base dgrad, an add_to -- is kept).  dy (M, N); Bt (R, N) the
    block-diagonal transposed B (row p * r_pad + j holds column j of B_p in part p's columns, zeros elsewhere), so ONE
    vy_lora_shrink over dy serves every part; At (K, R) the transposed stacked A, vy_lora_expand's `B` with
    r_pad := R and no boundaries.  N and R multiples of 32 (the shrink contracts over N), K of 16."""
    fn = "lora_dgrad_"
    n_tiles = int(n_tiles)
    M, dt = _lora_rows(fn, name, dy=dy) if dx is None else _lora_rows(fn, name, dy=dy, dx=dx)
    N = dy.shape[1]
    for what, t in (("Bt", Bt), ("At", At)):
        if not isinstance(t, Tensor) or t.dim() != 2 or not t.is_contiguous() or t.dtype != dt or t.device != dy.device:
            raise ValueError(f"{fn} ({name}): {what} must be a contiguous 2-D {dt} tensor on {dy.device}")
    R, K = Bt.shape[0], At.shape[0]
    if N % 32 or R % 32 or not 32 <= R <= 192 or K % 16 or Bt.shape[1] != N or At.shape[1] != R \
            or (dx is not None and dx.shape[1] != K):
        raise ValueError(f"{fn} ({name}): dy (M, N = {N}) needs Bt (R, N) and At (K, R) with N and R multiples of 32, "
                         f"R <= 192, K of 16 and dx (M, K); got Bt {tuple(Bt.shape)}, At {tuple(At.shape)}, dx "
                         f"{None if dx is None else tuple(dx.shape)}")
    if not isinstance(alpha, Tensor) or alpha.dtype != torch.float32 or alpha.numel() != 1 or alpha.device != dy.device:
        raise ValueError(f"{fn} ({name}): alpha must be a float32 tensor of one element on {dy.device}")
    _lora_tiles(fn, name, tiles, n_tiles, dy)
    _need_gpu(dy)
    t = torch.empty((M, R), dtype=dt, device=dy.device)
    st, code = _stream(), dtype_code(dt)
    call("vy_lora_shrink", dy.data_ptr(), dy.stride(0), Bt.data_ptr(), tiles.data_ptr(), n_tiles, t.data_ptr(), R, M, N, R,
         1, code, st)
    if dx is not None:
        call("vy_lora_expand", dx.data_ptr(), dx.stride(0), t.data_ptr(), R, At.data_ptr(), alpha.data_ptr(),
             tiles.data_ptr(), n_tiles, M, K, R, 1, K, K, code, st)
    return t


def lora_wgrad_chunk_rows(M: int, N: int, K: int) -> int:
    """Rows of M per chunk of vy_lora_wgrad (the shapes alone decide; cdiv(M, rows) chunks, the last one ragged)."""
    return int(_lib.load().vy_lora_wgrad_chunk_rows(int(M), int(N), int(K)))


def lora_wgrad(dy: Tensor, u: Tensor, x: Tensor, t: Tensor, dA: Sequence[Optional[Tensor]],
               dB: Sequence[Optional[Tensor]], boundaries: Sequence[int], r_pad: int, alpha: float, accumulate: bool,
               name: str = "projection") -> None:
    """Both low-rank weight gradients of one GEMM group in one launch pair (vy_lora_wgrad; the rule: include/vyom_hip.h):
    dB[p] (out_p, rank_p) (+)= alpha * dy[:, part p].T @ u[:, p * r_pad : + rank_p] and
    dA[p] (rank_p, K) (+)= alpha * t[:, p * r_pad : + rank_p].T @ x, fp32 contiguous, one pair per part of the packed
    projection; a part without an adapter has None for both.  Deterministic: two calls give the same bits."""
    fn = "lora_wgrad"
    M, dt = _lora_rows(fn, name, dy=dy, u=u, x=x, t=t)
    N, K = dy.shape[1], x.shape[1]
    bounds = _lora_bounds(fn, name, boundaries, N)
    parts = 1 + len(bounds)
    if K % 32 or K < 32:
        raise ValueError(f"{fn} ({name}): K = {K} must be a multiple of 32")
    if r_pad not in (32, 64) or u.shape[1] != parts * r_pad or t.shape[1] != parts * r_pad:
        raise ValueError(f"{fn} ({name}): r_pad {r_pad} must be 32 or 64 and u, t (M, {parts} * r_pad), got "
                         f"{tuple(u.shape)} and {tuple(t.shape)}")
    if len(dA) != parts or len(dB) != parts or all(a is None for a in dA):
        raise ValueError(f"{fn} ({name}): dA and dB need one entry per part ({parts}), at least one of them a tensor")
    cols = [0] + bounds + [N]
    ptrs_a, ptrs_b, ranks = [None] * 3, [None] * 3, [0] * 3
    for p, (a, b) in enumerate(zip(dA, dB)):
        if (a is None) != (b is None):
            raise ValueError(f"{fn} ({name}): part {p} has one of dA / dB only")
        if a is None:
            continue
        out_p = cols[p + 1] - cols[p]
        rank = a.shape[0] if isinstance(a, Tensor) and a.dim() == 2 else -1
        if not 1 <= rank <= r_pad:
            raise ValueError(f"{fn} ({name}): rank {rank} of part {p} is outside [1, r_pad = {r_pad}]")
        for what, g, shape in (("dA", a, (rank, K)), ("dB", b, (out_p, rank))):
            if not isinstance(g, Tensor) or g.dtype != torch.float32 or tuple(g.shape) != shape or not g.is_contiguous() \
                    or g.device != dy.device:
                raise ValueError(f"{fn} ({name}): {what}[{p}] must be a contiguous float32 {shape} tensor on {dy.device}, "
                                 f"got {getattr(g, 'dtype', None)} {tuple(getattr(g, 'shape', ()))}")
        ptrs_a[p], ptrs_b[p], ranks[p] = a.data_ptr(), b.data_ptr(), rank
    _need_gpu(dy)
    st = _stream()
    _stream_ws()
    call("vy_lora_wgrad", dy.data_ptr(), dy.stride(0), u.data_ptr(), u.stride(0), x.data_ptr(), x.stride(0), t.data_ptr(),
         t.stride(0), *ptrs_a, *ptrs_b, *ranks, M, N, K, int(r_pad), *(bounds + [N, N])[:2], float(alpha),
         1 if accumulate else 0, dtype_code(dt), st)


class DoraProblem(NamedTuple):
    """One projection of dora_compose / dora_bwd's table (vy_dora_desc; the rule: include/vyom_hip.h).  w: (out, in)
    float32 or bfloat16 with unit column stride; a (out, r), b (r, in), m (in) and c (in): contiguous float32.
    dora_compose writes c and wp -- (out, in) in the compute dtype, any row stride: a part of a packed projection passes
    its row block of the packed buffer.  dora_bwd reads c and g (out, in) float32 and writes dm, da, db, contiguous
    float32 of m's, a's and b's shapes."""
    w: Tensor
    a: Tensor
    b: Tensor
    m: Tensor
    c: Tensor
    wp: Optional[Tensor] = None
    g: Optional[Tensor] = None
    dm: Optional[Tensor] = None
    da: Optional[Tensor] = None
    db: Optional[Tensor] = None


def _dora_table(fn: str, problems: Sequence[DoraProblem], bwd: bool):
    import ctypes as C
    problems = list(problems)
    if not 1 <= len(problems) <= 8:
        raise ValueError(f"{fn}: a table holds 1 to 8 problems, got {len(problems)}")
    arr = (_lib.VyDoraDesc * len(problems))()
    dev = problems[0].w.device if isinstance(problems[0].w, Tensor) else None
    for i, p in enumerate(problems):
        w = p.w
        if not isinstance(w, Tensor) or w.dim() != 2 or w.dtype not in (torch.float32, torch.bfloat16) or w.stride(1) != 1:
            raise ValueError(f"{fn}: problem {i}: w must be a float32 or bfloat16 (out, in) matrix with unit column stride")
        _need_gpu(w)
        out_f, in_f = w.shape
        r = p.a.shape[1] if isinstance(p.a, Tensor) and p.a.dim() == 2 else -1
        if in_f % 8 or out_f % 8 or not 1 <= r <= 64:
            raise ValueError(f"{fn}: problem {i}: in {in_f} and out {out_f} must be multiples of 8 and the rank {r} lie in "
                             "1..64")
        small = [("a", p.a, (out_f, r)), ("b", p.b, (r, in_f)), ("m", p.m, (in_f,)), ("c", p.c, (in_f,))]
        if bwd:
            small += [("dm", p.dm, (in_f,)), ("da", p.da, (out_f, r)), ("db", p.db, (r, in_f))]
        for what, t, shape in small:
            # (a vector may come as the reference's (1, in) parameter)
            if not isinstance(t, Tensor) or t.dtype != torch.float32 or t.numel() != math.prod(shape) \
                    or (len(shape) > 1 and tuple(t.shape) != shape) or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{fn}: problem {i}: {what} must be a contiguous float32 {shape} tensor on {dev}, got "
                                 f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}")
        big, what = (p.g, "g") if bwd else (p.wp, "wp")
        if not isinstance(big, Tensor) or tuple(big.shape) != (out_f, in_f) or big.stride(1) != 1 or big.stride(0) < in_f \
                or big.device != dev or (bwd and big.dtype != torch.float32):
            raise ValueError(f"{fn}: problem {i}: {what} must be an (out, in) = {(out_f, in_f)} matrix on {dev} with unit "
                             f"column stride{' in float32' if bwd else ''}")
        d = arr[i]
        d.w, d.ldw, d.w_dtype = w.data_ptr(), w.stride(0), dtype_code(w.dtype)
        d.a, d.b, d.m, d.c = p.a.data_ptr(), p.b.data_ptr(), p.m.data_ptr(), p.c.data_ptr()
        d.out, d.in_, d.r = out_f, in_f, r
        if bwd:
            d.g, d.ldg = big.data_ptr(), big.stride(0)
            d.dm, d.da, d.db = p.dm.data_ptr(), p.da.data_ptr(), p.db.data_ptr()
        else:
            d.wp, d.ldwp = big.data_ptr(), big.stride(0)
    return C.cast(arr, C.c_void_p), len(problems), arr


def dora_compose(problems: Sequence[DoraProblem]) -> None:
    """W' = dora_m * D / c with D = w + a @ b and c = the column norms of D (written too), for up to 8 projections in one
    launch (vy_dora_compose).  Every wp of a table has the same dtype, float32 or bfloat16."""
    fn = "dora_compose"
    table, n, keep = _dora_table(fn, problems, False)
    dts = {p.wp.dtype for p in problems}
    if len(dts) != 1:
        raise ValueError(f"{fn}: the wp of one table share a dtype, got {sorted(map(str, dts))}")
    call("vy_dora_compose", table, n, dtype_code(dts.pop()), _stream())


def dora_bwd(problems: Sequence[DoraProblem], accumulate: bool) -> None:
    """dm, da, db (+)= the gradients of dora_m, dora_a, dora_b given g = dL/dW' in float32, for up to 8 projections in
    one launch pair (vy_dora_bwd); D is recomputed, c is what dora_compose left.  Deterministic: two calls give the same
    bits."""
    table, n, keep = _dora_table("dora_bwd", problems, True)
    st = _stream()
    _stream_ws()
    call("vy_dora_bwd", table, n, 1 if accumulate else 0, st)


def embedding_bwd_(dout: Tensor, ids: Tensor, dw: Tensor, padding_idx: Optional[int]) -> None:
    """dw[ids[m], :] += dout[m, :] in fp32, skipping padding_idx  (vy_embedding_bwd)."""
    _need_gpu(dout, ids, dw)
    d2 = _rows(dout)
    idc = ids.contiguous()
    assert dw.dtype == torch.float32 and dw.stride(1) == 1 and idc.numel() == d2.shape[0]
    call("vy_embedding_bwd", d2.data_ptr(), d2.stride(0), idc.data_ptr(), dw.data_ptr(), dw.stride(0),
         -1 if padding_idx is None else int(padding_idx), d2.shape[0], d2.shape[1], dw.shape[0],
         dtype_code(dout.dtype), _stream())


def logprob_fwd(logits2d: Tensor, labels: Tensor, weight: Tensor, lse: Tensor, logp: Tensor,
                err_flag: Optional[Tensor] = None) -> None:
    """lse[m] = logsumexp(row m), logp[m] = logits[m, label] - lse[m] for rows with weight != 0 (vy_logprob_fwd);
    logits2d: (M, V) view with 16-byte aligned, padded rows, read only; labels int64 (M,), weight / lse / logp fp32 (M,)."""
    _need_gpu(logits2d, labels, weight, lse, logp, err_flag)
    _row_args(logits2d, labels, weight, lse, logp)
    M, V = logits2d.shape
    call("vy_logprob_fwd", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), weight.data_ptr(), lse.data_ptr(),
         logp.data_ptr(), M, V, _ptr(err_flag), dtype_code(logits2d.dtype), _stream())


def logprob_bwd_(logits2d: Tensor, labels: Tensor, weight: Tensor, lse: Tensor) -> None:
    """logits <- weight * (onehot(label) - softmax) in place from the saved lse (vy_logprob_bwd)."""
    _need_gpu(logits2d, labels, weight, lse)
    _row_args(logits2d, labels, weight, lse)
    M, V = logits2d.shape
    call("vy_logprob_bwd", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), weight.data_ptr(), lse.data_ptr(),
         M, V, dtype_code(logits2d.dtype), _stream())


def logprob_fused_(logits2d: Tensor, labels: Tensor, weight: Tensor, lse: Tensor, logp: Tensor,
                   err_flag: Optional[Tensor] = None) -> None:
    """One pass: lse / logp as logprob_fwd, then the row overwritten as by logprob_bwd_ (vy_logprob_fused)."""
    _need_gpu(logits2d, labels, weight, lse, logp, err_flag)
    _row_args(logits2d, labels, weight, lse, logp)
    M, V = logits2d.shape
    call("vy_logprob_fused", logits2d.data_ptr(), logits2d.stride(0), labels.data_ptr(), weight.data_ptr(),
         lse.data_ptr(), logp.data_ptr(), M, V, _ptr(err_flag), dtype_code(logits2d.dtype), _stream())


def rmsnorm(x: Tensor, w: Tensor, eps: float, w_offset: float = 1.0) -> Tensor:
    """x * rsqrt(mean x^2 + eps) * (w_offset + w)  (vy_rmsnorm_fwd; Gemma: w_offset = 1)."""
    _need_gpu(x, w)
    x2 = _rows(x)
    M, N = x2.shape
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    call("vy_rmsnorm_fwd", x2.data_ptr(), x2.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0), M, N, float(eps),
         float(w_offset), dtype_code(x.dtype), _stream())
    return y.view(x.shape)


def gated_act(gate_up: Tensor, act: int) -> Tensor:
    """act(gate_up[..., :I]) * gate_up[..., I:]  (vy_gated_act_fwd)."""
    _need_gpu(gate_up)
    g2 = _rows(gate_up)
    M, two_i = g2.shape
    I = two_i // 2
    out = torch.empty((M, I), dtype=gate_up.dtype, device=gate_up.device)
    call("vy_gated_act_fwd", g2.data_ptr(), g2.stride(0), out.data_ptr(), out.stride(0), M, I, act,
         dtype_code(gate_up.dtype), _stream())
    return out.view(*gate_up.shape[:-1], I)


def rmsnorm_bwd(dy: Tensor, x: Tensor, w: Tensor, eps: float, w_offset: float, dw: Tensor, accumulate: bool,
                add_to: Optional[Tensor] = None) -> Tensor:
    """dx = d/dx [x * rsqrt(mean x^2 + eps) * (w_offset + w)] . dy + add_to; dw (fp32 [N]) (+)= the weight gradient
    (vy_rmsnorm_bwd: no saved statistics, deterministic dw)."""
    _need_gpu(dy, x, w, dw, add_to)
    d2, x2 = _rows(dy), _rows(x)
    a2 = _rows(add_to) if add_to is not None else None
    M, N = x2.shape
    assert dw.dtype == torch.float32 and dw.numel() == N and dw.is_contiguous()
    dx = torch.empty((M, N), dtype=x.dtype, device=x.device)
    ws = torch.empty((_lib.load().vy_layernorm_bwd_ws_rows(M) * N,), dtype=torch.float32, device=x.device)
    call("vy_rmsnorm_bwd", d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0), w.data_ptr(), _ptr(a2),
         a2.stride(0) if a2 is not None else 0, dx.data_ptr(), dx.stride(0), dw.data_ptr(), 1.0 if accumulate else 0.0,
         ws.data_ptr(), M, N, float(eps), float(w_offset), dtype_code(x.dtype), _stream())
    return dx.view(x.shape)


def gated_act_bwd(d_act: Tensor, gate_up: Tensor, act: int) -> Tensor:
    """[d_act * up * act'(gate) | d_act * act(gate)] in gate_up's layout  (vy_gated_act_bwd)."""
    _need_gpu(d_act, gate_up)
    d2, g2 = _rows(d_act), _rows(gate_up)
    M, two_i = g2.shape
    I = two_i // 2
    assert d2.shape == (M, I)
    out = torch.empty((M, two_i), dtype=gate_up.dtype, device=gate_up.device)
    call("vy_gated_act_bwd", d2.data_ptr(), d2.stride(0), g2.data_ptr(), g2.stride(0), out.data_ptr(), out.stride(0),
         M, I, act, dtype_code(gate_up.dtype), _stream())
    return out.view(gate_up.shape)


def _qk_scales(dh: int, *scales: Tensor) -> None:
    for s in scales:
        assert s.dtype == torch.float32 and s.is_contiguous() and s.shape == (dh,)


def qknorm_rope(qkv: Tensor, h: int, hk: int, dh: int, q_scale: Tensor, k_scale: Tensor, eps: float, cos: Tensor,
                sin: Tensor, pos0: int, q: Tensor, k: Tensor) -> None:
    """qkv (B, L, >= (h + 2 hk) dh), the packed rows of the bias-free QKV GEMM, left as they are: every q head becomes
    rope(x * rsqrt(mean x^2 + eps) * q_scale) in q (B, h, L, dh), every k head the same with k_scale in k (B, hk, L, dh)
    -- views written in place; scales fp32 (dh,), fp32 cos / sin tables, row pos0 + l; fp32 from the load to the one
    store.  (vy_qknorm_rope_fwd)"""
    _need_gpu(qkv, q_scale, k_scale, cos, sin, q, k)
    B, L = qkv.shape[0], qkv.shape[1]
    assert qkv.dim() == 3 and qkv.stride(2) == 1 and qkv.stride(0) == L * qkv.stride(1) and qkv.shape[2] >= (h + 2 * hk) * dh
    assert q.shape == (B, h, L, dh) and k.shape == (B, hk, L, dh) and q.stride(3) == 1 and k.stride(3) == 1
    assert q.dtype == qkv.dtype and k.dtype == qkv.dtype
    assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape[1] == dh // 2 and sin.shape == cos.shape
    _qk_scales(dh, q_scale, k_scale)
    call("vy_qknorm_rope_fwd", qkv.data_ptr(), qkv.stride(1), cos.data_ptr(), sin.data_ptr(), cos.shape[0], int(pos0),
         q_scale.data_ptr(), k_scale.data_ptr(), float(eps), q.data_ptr(), q.stride(0), q.stride(1), q.stride(2),
         k.data_ptr(), k.stride(0), k.stride(1), k.stride(2), B, L, h, hk, dh, dtype_code(qkv.dtype), _stream())


def qknorm_bwd_(dqkv: Tensor, qkv: Tensor, h: int, hk: int, dh: int, q_scale: Tensor, k_scale: Tensor, eps: float,
                dq_scale: Tensor, dk_scale: Tensor, accumulate: bool) -> Tensor:
    """dqkv (..., >= (h + 2 hk) dh), layout [dq | dk | dv] with dq / dk the gradients of the NORMALISED heads: its q and k
    columns are overwritten in place by the gradient of the raw projection qkv (the saved rows qknorm_rope read); the dv
    columns keep their bits.  dq_scale / dk_scale (fp32 (dh,)) (+)= the scale gradients, deterministic.
    (vy_qknorm_bwd: no saved statistics)"""
    _need_gpu(dqkv, qkv, q_scale, k_scale, dq_scale, dk_scale)
    d2, x2 = dqkv.view(-1, dqkv.shape[-1]), qkv.view(-1, qkv.shape[-1])
    T = x2.shape[0]
    assert d2.shape[0] == T and d2.stride(1) == 1 and x2.stride(1) == 1 and d2.dtype == x2.dtype
    _qk_scales(dh, q_scale, k_scale, dq_scale, dk_scale)
    ws = torch.empty((_lib.load().vy_qknorm_bwd_ws_floats(T, h, hk, dh),), dtype=torch.float32, device=qkv.device)
    call("vy_qknorm_bwd", d2.data_ptr(), d2.stride(0), x2.data_ptr(), x2.stride(0), q_scale.data_ptr(), k_scale.data_ptr(),
         float(eps), dq_scale.data_ptr(), dk_scale.data_ptr(), 1.0 if accumulate else 0.0, ws.data_ptr(), T, h, hk, dh,
         dtype_code(qkv.dtype), _stream())
    return dqkv


# ------------------------------------------------------------------------------------------
# paged KV cache (vy_paged.hip)
# ------------------------------------------------------------------------------------------


def _is_fp8_pages(t: Tensor) -> bool:
    return t.dtype == torch.float8_e4m3fn


def _check_pages(k_cache: Tensor, v_cache: Tensor, dtype, k_scale: Optional[Tensor] = None,
                 v_scale: Optional[Tensor] = None) -> Tuple[int, int, int, int]:
    """(max_blocks, block_size, hk, dh) of one layer's pages; the shape rules of include/vyom_hip.h as ValueErrors.
    fp8 (torch.float8_e4m3fn) pages come with their fp32 (max_blocks, block_size, hk) scales and a bf16 step; pages of
    the step's dtype come without scales."""
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("k_cache / v_cache must be contiguous (max_blocks, block_size, hk, dh) tensors of one shape")
    nb, bs, hk, dh = k_cache.shape
    if bs < 8 or bs > 256 or bs & (bs - 1):
        raise ValueError(f"block_size {bs} must be a power of two from 8 to 256")
    if dh % 8 or dh > 256:
        raise ValueError(f"head_dim {dh} must be a multiple of 8 up to 256")
    if _is_fp8_pages(k_cache) or _is_fp8_pages(v_cache):
        if k_cache.dtype != v_cache.dtype or dtype != torch.bfloat16:
            raise ValueError(f"fp8 pages serve a bfloat16 step with fp8 k and v pages, got {k_cache.dtype} / "
                             f"{v_cache.dtype} pages and a {dtype} step")
        if k_scale is None or v_scale is None:
            raise ValueError("fp8 pages need k_scale= and v_scale=")
        for sc in (k_scale, v_scale):
            if sc.dtype != torch.float32 or sc.shape != (nb, bs, hk) or not sc.is_contiguous():
                raise ValueError(f"k_scale / v_scale must be contiguous float32 {(nb, bs, hk)} tensors")
        return nb, bs, hk, dh
    if k_scale is not None or v_scale is not None:
        raise ValueError(f"k_scale / v_scale belong to fp8 pages, these pages are {k_cache.dtype}")
    if k_cache.dtype != dtype or v_cache.dtype != dtype:
        raise ValueError(f"pages are {k_cache.dtype}, the step computes in {dtype}")
    return nb, bs, hk, dh


def paged_rope_write_(qkv: Tensor, positions: Tensor, slot_mapping: Tensor, cos: Tensor, sin: Tensor, h: int,
                      k_cache: Tensor, v_cache: Tensor, *, k_scale: Optional[Tensor] = None,
                      v_scale: Optional[Tensor] = None) -> Tensor:
    """qkv (T, (h + 2 hk) dh), the packed projection of a step's tokens: q and k heads of token t rotated in place with
    row positions[t] (int32) of the fp32 cos / sin tables, the rotated k and the v stored into slot slot_mapping[t]
    (int64; negative: nothing is stored) of the pages.  (vy_paged_rope_write)
    fp8 pages (k_scale= / v_scale=, fp32 (max_blocks, block_size, hk)): the same in-place rows, every k / v head stored
    as e4m3 codes and one scale -- the rule of include/vyom_hip.h.  (vy_paged_rope_write_fp8)"""
    nb, bs, hk, dh = _check_pages(k_cache, v_cache, qkv.dtype, k_scale, v_scale)
    _need_gpu(qkv, positions, slot_mapping, cos, sin, k_cache, v_cache, k_scale, v_scale)
    T = qkv.shape[0]
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[1] == (h + 2 * hk) * dh
    assert positions.dtype == torch.int32 and positions.is_contiguous() and positions.numel() == T
    assert slot_mapping.dtype == torch.long and slot_mapping.is_contiguous() and slot_mapping.numel() == T
    assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape[1] == dh // 2 and sin.shape == cos.shape
    if k_scale is not None:
        call("vy_paged_rope_write_fp8", qkv.data_ptr(), qkv.stride(0), positions.data_ptr(), slot_mapping.data_ptr(),
             cos.data_ptr(), sin.data_ptr(), cos.shape[0], None, None, 0.0, k_cache.data_ptr(), v_cache.data_ptr(),
             k_scale.data_ptr(), v_scale.data_ptr(), nb, bs, T, h, hk, dh, dtype_code(qkv.dtype), _stream())
        return qkv
    call("vy_paged_rope_write", qkv.data_ptr(), qkv.stride(0), positions.data_ptr(), slot_mapping.data_ptr(),
         cos.data_ptr(), sin.data_ptr(), cos.shape[0], k_cache.data_ptr(), v_cache.data_ptr(), nb, bs, T, h, hk, dh,
         dtype_code(qkv.dtype), _stream())
    return qkv


def paged_qknorm_rope_write_(qkv: Tensor, positions: Tensor, slot_mapping: Tensor, cos: Tensor, sin: Tensor,
                             q_scale: Tensor, k_scale: Tensor, eps: float, h: int, k_cache: Tensor,
                             v_cache: Tensor, *, k_page_scale: Optional[Tensor] = None,
                             v_page_scale: Optional[Tensor] = None) -> Tensor:
    """paged_rope_write_ with Qwen3's qk_norm in the same launch: every q head becomes x * rsqrt(mean x^2 + eps) *
    q_scale, every k head the same with k_scale (fp32 (dh,), shared by all heads), and the normalised head is what is
    rotated, stored in place and (k) stored into its slot; fp32 from the load to the one store.  v heads are only
    stored into their slots.  (vy_paged_qknorm_rope_write)
    fp8 pages: their scales come as k_page_scale= / v_page_scale= (k_scale is the norm weight here), otherwise as
    paged_rope_write_.  (vy_paged_rope_write_fp8)"""
    nb, bs, hk, dh = _check_pages(k_cache, v_cache, qkv.dtype, k_page_scale, v_page_scale)
    _need_gpu(qkv, positions, slot_mapping, cos, sin, q_scale, k_scale, k_cache, v_cache, k_page_scale, v_page_scale)
    T = qkv.shape[0]
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[1] == (h + 2 * hk) * dh
    assert positions.dtype == torch.int32 and positions.is_contiguous() and positions.numel() == T
    assert slot_mapping.dtype == torch.long and slot_mapping.is_contiguous() and slot_mapping.numel() == T
    assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape[1] == dh // 2 and sin.shape == cos.shape
    for s in (q_scale, k_scale):
        assert s.dtype == torch.float32 and s.is_contiguous() and s.shape == (dh,)
    if k_page_scale is not None:
        call("vy_paged_rope_write_fp8", qkv.data_ptr(), qkv.stride(0), positions.data_ptr(), slot_mapping.data_ptr(),
             cos.data_ptr(), sin.data_ptr(), cos.shape[0], q_scale.data_ptr(), k_scale.data_ptr(), float(eps),
             k_cache.data_ptr(), v_cache.data_ptr(), k_page_scale.data_ptr(), v_page_scale.data_ptr(), nb, bs, T, h, hk,
             dh, dtype_code(qkv.dtype), _stream())
        return qkv
    call("vy_paged_qknorm_rope_write", qkv.data_ptr(), qkv.stride(0), positions.data_ptr(), slot_mapping.data_ptr(),
         cos.data_ptr(), sin.data_ptr(), cos.shape[0], q_scale.data_ptr(), k_scale.data_ptr(), float(eps),
         k_cache.data_ptr(), v_cache.data_ptr(), nb, bs, T, h, hk, dh, dtype_code(qkv.dtype), _stream())
    return qkv


def attention_paged_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, block_table: Tensor, seqlens: Tensor,
                           max_seqlen: int, h: int, *, q_rows: Optional[Tensor] = None, out: Optional[Tensor] = None,
                           n_split: int = 0, scale: Optional[float] = None, k_scale: Optional[Tensor] = None,
                           v_scale: Optional[Tensor] = None) -> Tensor:
    """One query token per sequence against its pages.  q (rows, >= h dh): sequence b's heads sit at row q_rows[b]
    (int32; None: row b); block_table int32 (B, n), seqlens int32 (B,), keys [0, seqlens[b]) are attended.  out
    (rows, h dh) is written at the same rows and returned.  n_split: workgroups per context (0: chosen by the library).
    (vy_attn_paged_decode)  fp8 pages: k_scale= / v_scale=, the keys are read as code * scale.
    (vy_attn_paged_decode_fp8)"""
    nb, bs, hk, dh = _check_pages(k_cache, v_cache, q.dtype, k_scale, v_scale)
    _need_gpu(q, k_cache, v_cache, block_table, seqlens, q_rows, out, k_scale, v_scale)
    B = seqlens.numel()
    assert q.dim() == 2 and q.stride(1) == 1 and q.shape[1] >= h * dh
    assert block_table.dtype == torch.int32 and block_table.dim() == 2 and block_table.stride(1) == 1 \
        and block_table.shape[0] == B
    assert seqlens.dtype == torch.int32 and seqlens.is_contiguous()
    assert max_seqlen <= block_table.shape[1] * bs
    if q_rows is not None:
        assert q_rows.dtype == torch.int32 and q_rows.is_contiguous() and q_rows.numel() == B
    if out is None:
        out = torch.empty((q.shape[0], h * dh), dtype=q.dtype, device=q.device)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[1] == h * dh and out.dtype == q.dtype
    if scale is None:
        scale = 1.0 / math.sqrt(dh)
    code = dtype_code(q.dtype)
    fp8 = k_scale is not None
    ws_bytes = _lib.load().vy_attn_paged_decode_fp8_ws_bytes if fp8 else _lib.load().vy_attn_paged_decode_ws_bytes
    need = ws_bytes(B, h, hk, dh, int(max_seqlen), int(n_split), code)
    ws = None
    if need:      # split-KV partials: the stream's GEMM workspace (an automatic split that would not fit runs unsplit)
        if need <= _WS_BYTES:
            ws = _stream_ws()
        elif n_split:
            raise ValueError(f"n_split {n_split} needs {need} bytes of workspace, the stream's buffer has {_WS_BYTES}")
    if fp8:
        call("vy_attn_paged_decode_fp8", q.data_ptr(), q.stride(0), _ptr(q_rows), k_cache.data_ptr(), v_cache.data_ptr(),
             k_scale.data_ptr(), v_scale.data_ptr(), nb, bs, block_table.data_ptr(), block_table.stride(0),
             seqlens.data_ptr(), int(max_seqlen), out.data_ptr(), out.stride(0), B, h, hk, dh, float(scale), int(n_split),
             _ptr(ws), 0 if ws is None else ws.numel(), code, _stream())
        return out
    call("vy_attn_paged_decode", q.data_ptr(), q.stride(0), _ptr(q_rows), k_cache.data_ptr(), v_cache.data_ptr(), nb, bs,
         block_table.data_ptr(), block_table.stride(0), seqlens.data_ptr(), int(max_seqlen), out.data_ptr(),
         out.stride(0), B, h, hk, dh, float(scale), int(n_split), _ptr(ws), 0 if ws is None else ws.numel(), code,
         _stream())
    return out


def attention_paged_prefill(q: Tensor, k_cache: Tensor, v_cache: Tensor, block_table: Tensor, cu_q: Tensor,
                            ctx_lens: Tensor, max_q: int, max_kv: int, h: int, *, out: Optional[Tensor] = None,
                            scale: Optional[float] = None, k_scale: Optional[Tensor] = None,
                            v_scale: Optional[Tensor] = None) -> Tensor:
    """Causal attention of packed query segments against the pages, one launch for all of them.  q (rows, >= h dh): rows
    cu_q[s] .. cu_q[s+1] - 1 (int32, n + 1 entries) are sequence s, row i of it sits at position ctx_lens[s] + i (int32,
    (n,)) and attends to keys [0, ctx_lens[s] + i] read through block_table[s] (int32, (n, width)); the step's own K/V
    rows are already in the pages.  max_q >= every segment length, max_kv >= every ctx + length (host values).  out
    (rows, h dh) is written at the segments' rows and returned.  (vy_attn_paged_prefill)  fp8 pages: k_scale= /
    v_scale=, a key row enters as bf16(code * scale).  (vy_attn_paged_prefill_fp8)"""
    nb, bs, hk, dh = _check_pages(k_cache, v_cache, q.dtype, k_scale, v_scale)
    _need_gpu(q, k_cache, v_cache, block_table, cu_q, ctx_lens, out, k_scale, v_scale)
    n = ctx_lens.numel()
    assert q.dim() == 2 and q.stride(1) == 1 and q.shape[1] >= h * dh
    assert block_table.dtype == torch.int32 and block_table.dim() == 2 and block_table.stride(1) == 1 \
        and block_table.shape[0] == n
    assert cu_q.dtype == torch.int32 and cu_q.is_contiguous() and cu_q.numel() == n + 1
    assert ctx_lens.dtype == torch.int32 and ctx_lens.is_contiguous()
    assert 0 <= max_q <= q.shape[0] and max_kv <= block_table.shape[1] * bs
    if out is None:
        out = torch.empty((q.shape[0], h * dh), dtype=q.dtype, device=q.device)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[1] == h * dh and out.dtype == q.dtype \
        and out.shape[0] >= q.shape[0]
    if scale is None:
        scale = 1.0 / math.sqrt(dh)
    if k_scale is not None:
        call("vy_attn_paged_prefill_fp8", q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(),
             k_scale.data_ptr(), v_scale.data_ptr(), nb, bs, block_table.data_ptr(), block_table.stride(0),
             cu_q.data_ptr(), ctx_lens.data_ptr(), n, int(max_q), int(max_kv), out.data_ptr(), out.stride(0), h, hk, dh,
             float(scale), dtype_code(q.dtype), _stream())
        return out
    call("vy_attn_paged_prefill", q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), nb, bs,
         block_table.data_ptr(), block_table.stride(0), cu_q.data_ptr(), ctx_lens.data_ptr(), n, int(max_q), int(max_kv),
         out.data_ptr(), out.stride(0), h, hk, dh, float(scale), dtype_code(q.dtype), _stream())
    return out


def paged_gather(k_cache: Tensor, v_cache: Tensor, block_table: Tensor, S: int) -> Tuple[Tensor, Tensor]:
    """Keys [0, S) of one sequence (block_table: its int32 entries) from the pages -> contiguous k, v (hk, S, dh).
    (vy_paged_gather)"""
    nb, bs, hk, dh = _check_pages(k_cache, v_cache, k_cache.dtype)
    _need_gpu(k_cache, v_cache, block_table)
    assert block_table.dtype == torch.int32 and block_table.dim() == 1 and block_table.is_contiguous()
    assert 0 < S <= block_table.numel() * bs
    k = torch.empty((hk, S, dh), dtype=k_cache.dtype, device=k_cache.device)
    v = torch.empty_like(k)
    call("vy_paged_gather", k_cache.data_ptr(), v_cache.data_ptr(), nb, bs, block_table.data_ptr(), block_table.numel(),
         S, k.data_ptr(), v.data_ptr(), hk, dh, dtype_code(k_cache.dtype), _stream())
    return k, v
