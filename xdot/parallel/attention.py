"""Sequence-parallel fused ("flash") attention — the MI355X fast path of the module.

The reference materialises the (B, H, T/N, T) score block per rank and runs six chunked
distributed products per fwd+bwd (2x nt, 2x all, 2x tn), re-gathering the
same K/V data in backward.  This path keeps the reference's sharding (rank r owns rows
[rR, (r+1)R) of every sequence tensor; ``keys`` is the row side, ``queries``/``values`` the
gathered side; ``layout="zigzag"`` gives rank r chunks r and 2N-1-r of 2N instead, which only the
mask and the rotary positions see: :mod:`xdot.parallel.layout`) and its exact math, but
restructures the work for HBM3E + MFMA + xGMI:

forward
  1. all-gather the gathered-side projections ``q`` and ``v`` ONCE (two RCCL all-gathers on
     the collective stream, issued before any compute);
  2. one flash-attention kernel per rank: S = k·qᵀ·scale, boolean mask, online softmax,
     O = P·v, all in registers/LDS; writes O (B, R, H·dv) in the layout the output Linear
     reads and the per-row log-sum-exp.  Nothing of size R x T touches HBM;
backward (recompute, no stored probabilities)
  3. δ = rowsum(dO ⊙ O);
  4. row-side kernel: dk = Σ_t dS·q_t  (dS = P ⊙ (dP − δ), dP = dO·v_tᵀ);
  5. gathered-side kernel: dq_t = Σ_rows dSᵀ·k, dv_t = Σ_rows Pᵀ·dO for ALL T gathered rows,
     as fp32 partials laid out rank-major, then ONE reduce-scatter each — the ``tn`` pattern
     of the reference, but fused and without re-gathering anything.

The gathered q/v are reused from forward (saved, T x (dh+dv) per head: 77 MB bf16 at
T=25000) instead of the reference's second round of gathers.  A fully masked row yields NaN
like the reference.

attention sinks (``sinks``: one logit ``s_h`` per row head that joins the softmax denominator and
carries no value; appended after mask and scale, so NOT multiplied by ``scale``; zeros are "one extra
key of score 0")
  need no change to any kernel: every forward branch ends in a normalised ``o`` and a natural-log
  ``lse``, and the sink is the fold ``lse' = logaddexp(lse, s_h)``, ``o' = exp(lse - lse') o``
  (``csrc/sink.hip``, once, after whichever branch ran; the folded pair is what is saved).  Steps
  3-5 on ``(o', lse')`` give dk, dq, dv exactly, and ``ds_h = -sum exp(s_h - lse') δ`` is a small
  ordered sum over the δ of step 3.  With sinks a fully masked row gives 0, not NaN; without
  (``sinks=None``) nothing is launched and the result is bit for bit what it was.  On 16-bit tensors
  the one-launch forward's output is rounded twice (by the kernel, by the fold).

CPU tensors (and GPU dtypes the kernels do not take) run the same
schedule with a torch reference implementation of steps 2-5.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .. import _ext
from ..ops import flash
from ..ops.mask import StructuredMask, resolve as resolve_mask
from ..utils import comm as _comm
from ..utils.checks import check_consistent
from ..utils.env import FLAGS
from ..utils.streams import _on_stream, _prep_event, _side_stream
from . import _ref
from ._gathered import GatheredSide, _q_width, pop_sinks, sinks_grad, wire_dtype
from .layout import check_layout

__all__ = ["seq_parallel_attention", "seq_parallel_attention_packed", "start_gather", "flash_supported",
           "SeqParallelAttention"]

# D <= 128: the tuned families (csrc/flash_fwd.hip, flash_bwd.hip, flash_f32.hip); 160-384: the
# wide-head family (csrc/flash_wide.hip: the reference's example.py 768 / 2 heads = 384 and its
# num_heads = 1 gradient test at 256).  Exact fp32 heads past 256 need the score buffer.
FLASH_HEAD_DIMS = (32, 64, 96, 128, 160, 192, 256, 384)
WIDE_F32_NEEDS_SCORES = 256
# bf16/fp16: 32x32x16 MFMA kernels; fp32: exact-f32 MFMA kernels — the reference's own precision
# without materialised scores
FLASH_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def flash_head_dim(head_dim: int, v_head_dim: int) -> Optional[int]:
    """The kernel head dim a (key, value) head pair runs at: itself when both are equal and a
    kernel dim, else the smallest kernel dim holding both (heads zero-padded: zero key / query
    columns add nothing to a score, zero value columns give zero outputs that are dropped), or
    None past 384."""
    m = max(head_dim, v_head_dim)
    return next((d for d in FLASH_HEAD_DIMS if d >= m), None)


def pad_heads(x: Tensor, H: int, d: int, Dp: int) -> Tensor:
    """(B, R, H*d) -> (B, R, H*Dp), every head zero-padded from d to Dp columns (differentiable)."""
    if d == Dp:
        return x
    B, R = x.shape[0], x.shape[1]
    return torch.nn.functional.pad(x.reshape(B, R, H, d), (0, Dp - d)).reshape(B, R, H * Dp)


def unpad_heads(x: Tensor, H: int, d: int, Dp: int) -> Tensor:
    """(B, R, H*Dp) -> (B, R, H*d): the first d columns of every head."""
    if d == Dp:
        return x
    B, R = x.shape[0], x.shape[1]
    return x.reshape(B, R, H, Dp)[..., :d].reshape(B, R, H * d)


def flash_supported(x: Tensor, head_dim: int, v_head_dim: int) -> bool:
    """The flash kernels take this (dtype, device, head dims), directly or zero-padded
    (:func:`flash_head_dim`)."""
    return _kernels_take(x) and flash_head_dim(head_dim, v_head_dim) is not None


def _kernels_take(x: Tensor) -> bool:
    """A GPU tensor of a flash dtype, and the extension with the flash kernels is loaded."""
    return bool(x.is_cuda and x.dtype in FLASH_DTYPES and _ext.use_hip(x) and hasattr(_ext.ops(), "flash_fwd"))


def _hip_ok(k: Tensor, qv: Tensor, H: int, Hg: Optional[int] = None) -> bool:
    """The HIP kernels take this call: a GPU bf16/fp16/fp32 row side, a supported head dim and a
    value width equal to the key width (otherwise the torch path runs, as documented).  ``Hg``:
    gathered heads (None: ``H``); ``qv`` is then ``2 * Hg * D`` wide."""
    C = k.shape[-1]
    return (C % H == 0 and C // H in FLASH_HEAD_DIMS and qv.shape[-1] == 2 * (Hg or H) * (C // H)
            and _kernels_take(k))


def gathered_heads_arg(H: int, gathered_heads: Optional[int]) -> Optional[int]:
    """``gathered_heads`` validated against ``H`` -> None when every row head has its own gathered
    head (the default), else ``Hg`` with ``H % Hg == 0`` (grouped-query attention: gathered head
    ``h // (H // Hg)`` serves row head ``h``)."""
    if gathered_heads is None or int(gathered_heads) == H:
        return None
    Hg = int(gathered_heads)
    if Hg < 1 or H % Hg:
        raise ValueError(f"num_heads {H} must be a multiple of gathered_heads {gathered_heads}")
    return Hg


def sinks_arg(sinks, H: int, like: Tensor):
    """The ``sinks`` argument validated -> None or a float ``(H,)`` tensor on ``like``'s device: one
    logit per ROW head (grouped-query attention does not change it)."""
    if sinks is None:
        return None
    if not isinstance(sinks, Tensor) or not sinks.is_floating_point():
        raise TypeError(f"sinks must be a floating-point tensor of one logit per head or None, got "
                        f"{sinks.dtype if isinstance(sinks, Tensor) else type(sinks).__name__}")
    if sinks.dim() != 1 or sinks.shape[0] != H:
        raise ValueError(f"sinks must be (num_heads,) = ({H},), got {tuple(sinks.shape)}")
    if sinks.device != like.device:
        raise ValueError(f"sinks must be on the tensors' device {like.device}, got {sinks.device}")
    return sinks


def _prescale_rows(k: Tensor) -> bool:
    """The HIP path runs on a pre-scaled row side (``flash.prescale``; XDOT_PRESCALE, default on):
    16-bit rows with a multiple of 8 elements."""
    return bool(FLAGS.prescale and k.numel() % 8 == 0 and k.dtype != torch.float32)


def prescale_wanted(k_like: Tensor, qv_like: Tensor, H: int, Hg: Optional[int] = None) -> bool:
    """The HIP path will run on pre-scaled rows for a row side shaped / typed like ``k_like``
    (the condition :meth:`SeqParallelAttention.forward` applies)."""
    return _hip_ok(k_like, qv_like, H, Hg) and _prescale_rows(k_like)


# ----------------------------------------------------------------------------------------
# gather helpers
# ----------------------------------------------------------------------------------------
def _gather_rows(comm, x: Tensor, async_op: bool = True, out: Optional[Tensor] = None):
    """(B, R, C) -> (N, B, R, C) rank-major (row t = j*R + i of batch b at [j, b, i]).  ``out``:
    the (N, B, R, C) output, whose block ``rank`` may already hold ``x`` (in-place gather)."""
    n = comm.world_size
    x = x.contiguous()
    if n == 1:
        return _comm.Handle(out=x.unsqueeze(0)) if async_op else x.unsqueeze(0)
    if out is None:
        out = torch.empty((n,) + tuple(x.shape), dtype=x.dtype, device=x.device)
    h = comm.all_gather_into(out, x, async_op=async_op)
    return h if async_op else out


def _row_chunks(n: int, R: int, hip: bool, nchunks: Optional[int] = None) -> List[Tuple[int, int]]:
    """Row chunks (r0, rc) of every rank's shard for the pipelined gather of the fused path:
    with several ranks the gathered side can travel in ``XDOT_GATHER_CHUNKS`` all-gathers so
    chunk c+1 is in flight while the kernels consume chunk c (and, in backward, chunk c's
    reduce-scatter runs while chunk c+1's gradients are computed).  Default (auto): 2 chunks
    from 8 ranks on, else 1 — measured on the emulated rank step with a 300 GB/s collective
    link model: N=8 1.621 -> 1.577 ms with 2 chunks, N=4 2.459 -> 2.471 ms (without any
    transfer time 2 chunks cost 23 / 55 µs of compute), profiles/r2_gather_chunks.md."""
    if n == 1:
        return [(0, R)]
    auto = 2 if n >= 8 else 1
    nc = nchunks or ((FLAGS.gather_chunks or auto) if hip else 1)
    nc = max(1, min(nc, R if nchunks else R // 64))  # an explicit plan is honoured down to 1-row chunks
    base, extra = divmod(R, nc)
    out, r0 = [], 0
    for c in range(nc):
        rc = base + (1 if c < extra else 0)
        out.append((r0, rc))
        r0 += rc
    return out


class _PendingGather:
    """All-gathers of the row chunks of one packed operand, issued back to back on the
    collective stream; ``wait(c)`` orders the current stream after chunk c only.

    With several chunks every chunk lands in its own slice of ONE buffer: chunk c's gather
    output (N, B, rc, ·) starts where chunk c-1's ends, so for B = 1 the buffer read as
    (1, T, ·) holds every gathered row in (chunk, source rank, row) order — a column
    permutation of the rank-major order that attention does not see (the mask columns are
    permuted to match, :func:`_perm_cols`), and the backward runs ONE kernel pair over it."""

    def __init__(self, comm, x: Tensor, chunks: List[Tuple[int, int]], out: Optional[Tensor] = None):
        self.chunks = chunks
        self.n = n = comm.world_size
        x = x.contiguous()
        self.flat = None
        if n > 1 and len(chunks) > 1:
            self.flat = torch.empty(n * x.numel(), dtype=x.dtype, device=x.device)
        self.handles = []
        off = 0
        for r0, rc in chunks:
            xc = x[:, r0:r0 + rc]
            if self.flat is None:
                self.handles.append(_gather_rows(comm, xc, out=out))
                continue
            out = self.flat[off:off + n * xc.numel()].view((n,) + tuple(xc.shape))
            off += out.numel()
            self.handles.append(comm.all_gather_into(out, xc.contiguous(), async_op=True))
        self._bufs: List[Optional[Tensor]] = [None] * len(chunks)

    def wait(self, c: int) -> Tensor:
        if self._bufs[c] is None:
            self._bufs[c] = self.handles[c].wait()          # (N, B, rc, 2C)
        return self._bufs[c]

    def wait_all(self) -> List[Tensor]:
        return [self.wait(c) for c in range(len(self.chunks))]

    def permuted(self) -> Optional[Tensor]:
        """(1, T, ·) view of the single buffer in (chunk, rank, row) column order (B = 1, several
        chunks, every chunk waited for), else None."""
        if self.flat is None or self._bufs[0].shape[1] != 1 or any(b is None for b in self._bufs):
            return None
        return self.flat.view(1, -1, self._bufs[0].shape[-1])


def _perm_cols(B: int, R: int, n: int, chunks: List[Tuple[int, int]]):
    """Mask columns in the (chunk, source rank, row) order of :meth:`_PendingGather.permuted`."""
    def view(m):  # leading dims from m: also applied to a (1, 1, T) row of column indices
        m4 = m.reshape(*m.shape[:-1], n, R)
        return torch.cat([m4[..., r0:r0 + rc].reshape(*m.shape[:-1], n * rc) for r0, rc in chunks], dim=-1)
    return view


def _as_global(g: Tensor) -> Tensor:
    """(N, B, R, C) -> (B, T, C) view/copy for the torch reference path."""
    n, B, R, C = g.shape
    return g.permute(1, 0, 2, 3).reshape(B, n * R, C)


# ----------------------------------------------------------------------------------------
# torch path of the per-rank compute (CPU / fallback / testing): layout adapters over _ref
# ----------------------------------------------------------------------------------------
def _segmented_forward_torch(k, qv, mask, gs, pending, n, rank):
    B, R = k.shape[:2]
    plan = _segment_plan(n, rank, len(pending.chunks), FLAGS.local_first)
    parts = []
    if FLAGS.local_first:
        own = None if mask is None else _mask_cols(B, R, n, rank, rank + 1, 0, R)(mask)
        parts.append(gs.ref_fwd(k, qv, own))
    bufs = []
    for c, (r0, rc) in enumerate(pending.chunks):
        g = pending.wait(c)                                      # (N, B, rc, 2C)
        bufs.append(g)
        for _, j0, j1 in (p for p in plan if p[0] == c):
            m = None if mask is None else _mask_cols(B, R, n, j0, j1, r0, rc)(mask)
            parts.append(gs.ref_fwd(k, _as_global(g[j0:j1]), m))
    o, lse = _ref.combine(parts, k.dtype)
    return o, lse, [torch.cat(bufs, dim=2) if len(bufs) > 1 else bufs[0]]


def _backward_torch(ctx, do, k, o, lse, qvg, sinks=None):
    """-> (dk, d[q|v] of this rank's rows, ds or None) from the rank-major gathered ``qvg`` (N, B, R, Cq + Cv)."""
    gs, (n, B, Rg) = ctx.gs, qvg.shape[:3]
    delta = _ref.delta(do, o, gs.H, lse.dtype)
    ds = None if sinks is None else _ref.sink_grad(delta, lse, sinks)
    dk, dq, dv = gs.ref_bwd(do, k, qvg, lse, delta, ctx.mask, rows=_as_global)
    parts = torch.cat([dq, dv], dim=-1).view(B, n, Rg, -1).permute(1, 0, 2, 3).contiguous()  # rank-major
    parts = parts.to(wire_dtype(k.dtype))  # as the HIP path (16-bit: one rounding per partial)
    h, dqv = _reduce_async(ctx.comm, parts)
    if h is not None:
        h.wait()
    return dk, dqv, ds


def _reduce_async(comm, parts, out=None):
    """(N, B, rc, 2C) rank-major partials -> (handle or None, (B, rc, 2C))"""
    if comm.world_size == 1:
        return None, parts[0]
    if out is None:
        out = torch.empty(parts.shape[1:], dtype=parts.dtype, device=parts.device)
    return comm.reduce_scatter(out, parts, async_op=True), out


# ----------------------------------------------------------------------------------------
# the segmented forward
# ----------------------------------------------------------------------------------------
def _segment_plan(n: int, rank: int, nchunks: int, local_first: bool) -> List[Tuple[int, int, int]]:
    """Peer segments (chunk c, source ranks j0..j1-1) of the segmented forward, in launch order;
    the own rank is left out of every chunk when its block runs first."""
    plan = []
    for c in range(nchunks):
        ranges = [(0, rank), (rank + 1, n)] if local_first else [(0, n)]
        plan += [(c, j0, j1) for j0, j1 in ranges if j1 > j0]
    return plan


def _mask_cols(B: int, R: int, n: int, j0: int, j1: int, r0: int, rc: int):
    """Mask columns of source ranks j0..j1-1, rows r0..r0+rc of each (global column j*R + r0 + i)."""
    return lambda m: m.reshape(*m.shape[:-1], n, R)[..., j0:j1, r0:r0 + rc].reshape(*m.shape[:-1], (j1 - j0) * rc)


def _segmented_forward(k, qv, mask, gs, pending, n, rank):
    """Forward of a multi-rank step as column segments merged by one log-sum-exp combine:
    the rank's OWN [q|v] block first (it needs no communication, so its partial runs while the
    all-gather is in flight), then each gathered chunk's peer blocks as soon as that chunk
    lands.  Every segment is a subset of a row's columns, so the partials (o normalised over
    the segment, its lse) merge exactly.  -> (o, lse, gathered buffers saved for backward)."""
    if not gs.use_hip:
        return _segmented_forward_torch(k, qv, mask, gs, pending, n, rank)
    (B, R, C), H = k.shape, gs.H
    chunks = pending.chunks
    local_first = FLAGS.local_first
    plan = _segment_plan(n, rank, len(chunks), local_first)
    if local_first and 0 < rank < n - 1 and SEGMENT_MERGE:
        # a middle rank's peers sit on both sides of its own block in every chunk: ONE partial
        # over the whole chunk with the own columns masked out (their tiles are skipped whole,
        # two boundary tiles per row block take the masked path) instead of two launches
        plan = [(c, 0, -1) for c in range(len(chunks))]
    widths = ([R] if local_first else []) + [(n if j1 == -1 else j1 - j0) * chunks[c][1] for c, j0, j1 in plan]
    ns = [flash.splits(B, R, w, H) for w in widths]
    opart = torch.empty(sum(ns), B, R, C, dtype=torch.float32, device=k.device)
    lpart = torch.empty(sum(ns), B, H, R, dtype=torch.float32, device=k.device)
    slots = iter([(sum(ns[:i]), nsi) for i, nsi in enumerate(ns)])  # (first slot, slots) per launch

    def run(seg, mk):  # seg: (B, Tseg, 2 Cq) = [q | v] of the segment's columns
        gs.fwd_partial(k, gs.view(seg), mk, opart, lpart, *next(slots))

    if local_first:
        own = _mask_cols(B, R, n, rank, rank + 1, 0, R)
        run(qv, flash.prepare_mask_cached(mask, B, R, R, tag=("own", rank, n), view=own))
    bufs = []
    for c, (r0, rc) in enumerate(chunks):
        g = flash.gathered_to_btc(pending.wait(c))          # (B, N*rc, 2C)
        bufs.append(g)
        for _, j0, j1 in (p for p in plan if p[0] == c):
            if j1 == -1:  # merged: every rank of the chunk, the own columns masked out
                run(g, _own_excluded_mask(mask, B, R, n, rank, r0, rc, k.device))
                continue
            mk = flash.prepare_mask_cached(mask, B, R, (j1 - j0) * rc, tag=("seg", r0, rc, n, j0, j1),
                                           view=_mask_cols(B, R, n, j0, j1, r0, rc))
            run(g[:, j0 * rc:j1 * rc], mk)
    o, lse = flash.fwd_combine(opart, lpart, H, k)
    perm = pending.permuted()
    return o, lse, ([perm] if perm is not None else bufs)


_OWN_EX = {}
_NOTHING_MASKED = StructuredMask()
# False: a middle rank launches one partial per peer range (A/B diagnostics: bench_rank.py --no-seg-merge)
SEGMENT_MERGE = True


def _own_excluded_mask(mask, B: int, R: int, n: int, rank: int, r0: int, rc: int, dev):
    """Packed (B, R, n*rc) mask of one gather chunk with this rank's own columns masked (they
    ran first, under the all-gather), OR-ed with the user mask's columns of the chunk.  Cached:
    on the user mask (MASK_CACHE) or, without one, per shape."""
    def own_cols(m):  # (a row of column indices: -1 = always masked)
        m = m.clone()
        m[..., rank * rc:(rank + 1) * rc] = True if m.dtype == torch.bool else -1
        return m

    if mask is not None:
        packed = flash.prepare_mask_cached(mask, B, R, n * rc, tag=("segx", r0, rc, n, rank),
                                           view=lambda m: own_cols(_mask_cols(B, R, n, 0, n, r0, rc)(m)))
        if packed is not None:
            return packed
    key = (B, R, n, rank, rc, dev)
    if key not in _OWN_EX:
        if len(_OWN_EX) >= 8:
            _OWN_EX.pop(next(iter(_OWN_EX)))
        # generated (csrc/mask_pack.hip: mask_gen), not packed from a (B, R, n*rc) tensor of zeros
        segs = [(0, rank * rc, 0), (rank * rc, rc, -1), ((rank + 1) * rc, (n - rank - 1) * rc, (rank + 1) * rc)]
        _OWN_EX[key] = flash.generate_mask(_NOTHING_MASKED, B, R, n * rc, 0, segments=segs, device=dev)
    return _OWN_EX[key]


# The fused backward runs its gathered-side half on a high-priority side stream so the row-side
# kernel fills the column kernel's last, mostly empty workgroup round.  Eager, on one MI355X
# (benchmarks/graph_ab.py, profiles/r3_graph.md), two streams vs one: N=1 8.18 vs 8.60 ms, N=2
# rank 4.38 vs 4.59, N=4 rank 2.40 vs 2.46, N=8 rank 1.39 vs 1.43 (an earlier box: 1.43 vs 1.40,
# within box noise).  Under HIP-graph capture the side stream's priority is lost and two streams
# replay 19-32 % slower at N=1/2, so a captured backward uses one stream.
# ONE_STREAM_BACKWARD: None = that rule, True / False = force (A/B diagnostics).
ONE_STREAM_BACKWARD = None


def _two_stream_backward() -> bool:
    if ONE_STREAM_BACKWARD is not None:
        return not ONE_STREAM_BACKWARD
    return not torch.cuda.is_current_stream_capturing()


# ----------------------------------------------------------------------------------------
# HIP halves of the autograd function
# ----------------------------------------------------------------------------------------
def _score_buffers(k, H, T, fm, one_kernel, segmented):
    """The fp32 score buffers of a forward that a backward will follow -> (sbuf, dsbuf, segmented).
    When a buffer fits (``flash.score_buffer``) the backward reads S / dS instead of recomputing
    them, and ONE kernel runs over the whole gathered side (in fp32 the own-block-first
    segmentation hides < 5 % of a rank's forward): ``segmented`` comes back False.
    ``one_kernel``: the gathered side is (or can be read as) one buffer."""
    B, R, C = k.shape
    D = C // H
    sbuf = dsbuf = None
    if one_kernel:
        if flash.ds_only_wanted(fm, D):  # dS-only: nothing stored by the forward
            dsbuf = flash.score_buffer(B, H, R, T, k.device)
            if dsbuf is not None:
                segmented = False
        else:
            # the fused exact column pass overwrites S with dS in place: no second buffer
            sbs = flash.score_buffers(B, H, R, T, k.device, dsbuf=not flash.fused_cols_wanted(fm, D))
            if sbs is not None:
                sbuf, dsbuf = sbs
                segmented = False
    if D > WIDE_F32_NEEDS_SCORES and sbuf is None:
        # no kernel recomputes an fp32 head this wide (three D-wide register sets) and the torch
        # path would materialise a score matrix larger than the buffer that did not fit
        raise RuntimeError(
            f"xdot: training exact-fp32 attention at head dim {D} needs the flash score buffer "
            f"({4 * flash.score_buffer_numel(B, H, R, T) / 2**30:.1f} GiB), which does not fit "
            f"within XDOT_FP32_SCORES_FRAC={FLAGS.fp32_scores_frac} of the free device memory: shorten the "
            "sequence, raise XDOT_FP32_SCORES_FRAC, or run the module in bf16")
    return sbuf, dsbuf, segmented


def _whole_mask(mask, B, R, n, chunks):
    """Packed (cached) mask of the one gathered buffer: rank-major columns, or with several gather
    chunks their (chunk, rank, row) order."""
    if len(chunks) == 1:
        return flash.prepare_mask_cached(mask, B, R, n * R)
    return flash.prepare_mask_cached(mask, B, R, n * R, tag=("perm", tuple(chunks), n), view=_perm_cols(B, R, n, chunks))


def _backward_masks(ctx, B, R, n, one):
    """The packed masks of the backward's buffers: the forward's, or packed here (cached) after a
    segmented forward."""
    chunks = ctx.chunks
    if ctx.mks is not None and not (one and len(chunks) > 1):
        return ctx.mks
    if one:
        return [_whole_mask(ctx.mask, B, R, n, chunks)]
    return [flash.prepare_mask_cached(ctx.mask, B, R, n * rc, tag=(r0, rc, n),
                                      view=_mask_cols(B, R, n, 0, n, r0, rc)) for r0, rc in chunks]


def _saved_scores(ctx, sbt, k, H):
    """(S buffer, dS buffer) of this backward.  Score buffer: S -> dS in the column kernel, then dK
    from dS.  With a separate dS buffer S stays intact, so a second backward through a retained
    graph reads it again; in place (S overwritten with dS) the first backward consumes it and a
    second one recomputes."""
    has_s, has_ds = getattr(ctx, "sb_kind", (False, False))
    sbuf = sbt[0] if has_s else None
    dsbuf = sbt[-1] if has_ds else None
    if has_s and not has_ds:
        if getattr(ctx, "sb_used", False):
            sbuf = None
        ctx.sb_used = True
    D = k.shape[-1] // H
    if sbuf is None and k.dtype == torch.float32 and D > WIDE_F32_NEEDS_SCORES and ctx.gs.fp32_mode == 0:
        raise RuntimeError(
            f"xdot: a second backward through a retained graph of exact-fp32 attention at head dim "
            f"{D} needs the scores, which the first backward overwrote in place (no kernel "
            "recomputes an fp32 head this wide); set XDOT_FP32_SCORES_DS=1 with room for the "
            "separate dS buffer, or do not retain the graph")
    return sbuf, dsbuf


def _cols_one_buffer(cols, g, mk, sbuf, dsbuf, fused, hi):
    """The column pass(es) over the one gathered buffer -> (d[q|v] (B, T, 2C), the event after
    which the row kernel may read dS from a score buffer, or None)."""
    if dsbuf is not None and sbuf is not None:
        # dQ pass (S -> dS), then the row kernel (reads dS) on `cur` concurrently
        # with the dV pass (reads S) here.  (The dV pass beside the dQ pass on a third
        # stream instead measured 54.62 vs 54.71 ms, and one rep ran 171 ms:
        # profiles/r6_fp32.md)
        dkv, _ = cols(g, mk, sbuf=sbuf, dsbuf=dsbuf, passes=2)
        ev_cols = torch.cuda.Event()
        ev_cols.record(hi)
        cols(g, mk, sbuf=sbuf, dsbuf=dsbuf, passes=1, out_dkv=dkv)
        return dkv, ev_cols
    # (fused exact pass: dP, dQ and dV in one kernel, S -> dS in place)
    dkv, _ = cols(g, mk, sbuf=sbuf, dsbuf=dsbuf, passes=4 if fused else 3)
    if sbuf is None and dsbuf is None:
        return dkv, None
    ev_cols = torch.cuda.Event()  # the row kernel reads the dS this kernel wrote
    ev_cols.record(hi)
    return dkv, ev_cols


def _rows_hip(ctx, do, k, lse, delta, bufs, mks, sbuf, dsbuf, cur):
    """Row-side dk on the current stream: one kernel over the one buffer, or one partial launch
    per chunk buffer and their sum."""
    gs, (B, R, C) = ctx.gs, k.shape
    if len(bufs) == 1:  # (bufs: the kernel views the column kernels read)
        dk = gs.bwd_rows(do, k, bufs[0], lse, delta, mks[0], sbuf, dsbuf)
        if sbuf is not None:
            sbuf.record_stream(cur)
        if dsbuf is not None:
            dsbuf.record_stream(cur)
        return dk
    ns = flash.splits(B, R, ctx.comm.world_size * ctx.chunks[0][1], gs.H, True)
    dpart = torch.empty(len(bufs) * ns, B, R, C, dtype=torch.float32, device=k.device)
    for c, (x, mk) in enumerate(zip(bufs, mks)):
        gs.bwd_rows_partial(do, k, x, lse, delta, mk, dpart, c * ns, ns)
    return flash.bwd_rows_sum(dpart, gs.H, k)


def _backward_hip(ctx, do, k, o, lse, bufs, sbt, sinks=None):
    """δ, then two independent streams: 1) gathered-side grads on a HIGH-priority stream,
    followed there by their reduce-scatter(s), and 2) the row-side dk on the current
    stream.  2) fills the partly occupied last workgroup rounds of 1) and hides the
    reduce-scatter, while the priority keeps 1) (and so the collective) nearly as
    early as when it runs alone.  δ runs on the priority stream too, so 1) reaches
    the GPU first.  Per-chunk kernels (chunk c's reduce-scatter under chunk c+1's
    kernel) only when the chunks are separate buffers (B > 1)."""
    comm, gs, chunks = ctx.comm, ctx.gs, ctx.chunks
    n, H = comm.world_size, gs.H
    B, R, C = k.shape
    bufs = [gs.view(g) for g in bufs]  # (saved at the wire width 2 Cq; both kernels read ONE view of each)
    one = len(bufs) == 1  # one gathered buffer: natural order, or chunks permuted (B = 1)
    mks = _backward_masks(ctx, B, R, n, one)
    cur = torch.cuda.current_stream(do.device)
    # high priority so the gathered side (and its reduce-scatter) finishes early (an
    # ordinary-priority side stream measured slower at N=1 and N=8: profiles/r2_bwd_overlap.md)
    hi = _side_stream(do.device, -1) if _two_stream_backward() else cur
    hi.wait_stream(cur)
    handles, outs = [], []
    gdt = wire_dtype(k.dtype)
    sbuf, dsbuf = _saved_scores(ctx, sbt, k, H)
    ev_cols = None
    with _on_stream(hi, cur):
        delta, lse2 = flash.bwd_prep(do, o, lse, H)  # one prep pass for both kernels
        ev = _prep_event(hi.device)
        ev.record(hi)
        dqv = None
        if n > 1 and len(chunks) > 1 and B == 1:
            dqv = torch.empty(B, R, 2 * gs.Cq, dtype=gdt, device=k.device)
        # partials rounded once to the compute dtype in the kernel (XDOT_GRAD_FP32=1 keeps fp32): half
        # the epilogue stores and half the reduce-scatter bytes; fp32 per row head where they are folded
        def cols(x, mk, **kw):
            return gs.bwd_cols(do, k, x, o, lse, mk, delta, FLAGS.grad_fp32, lse2=lse2, **kw)

        def scatter(part, r0, rc):  # one chunk's (B, n*rc, ·) partial -> the wire width and dtype -> its reduce-scatter
            h, oc = _reduce_async(comm, flash.btc_to_rank_major(gs.fold(part, gdt), n),
                                  None if dqv is None else dqv[:, r0:r0 + rc])
            handles.append(h)
            outs.append(oc)

        if one:
            fused = sbuf is not None and dsbuf is None and flash.fused_cols_wanted(gs.fp32_mode, C // H)
            dkv, ev_cols = _cols_one_buffer(cols, bufs[0], mks[0], sbuf, dsbuf, fused, hi)
            off = 0
            for r0, rc in chunks:  # (chunk, rank, row) order: chunk c's ranks are contiguous
                scatter(dkv if len(chunks) == 1 else dkv[:, off:off + n * rc], r0, rc)
                off += n * rc
        else:
            for c, (r0, rc) in enumerate(chunks):
                scatter(cols(bufs[c], mks[c])[0], r0, rc)
    # the row-side kernel starts as soon as δ exists: back to back measured slower at
    # every rank shape (profiles/r2_bwd_overlap.md)
    cur.wait_event(ev if ev_cols is None else ev_cols)
    delta.record_stream(cur)
    dk = _rows_hip(ctx, do, k, lse, delta, bufs, mks, sbuf, dsbuf, cur)
    # the sink's gradient from the delta both kernels read: a small ordered sum behind the row kernel
    ds = None if sinks is None else flash.sink_grad(delta, lse, sinks)
    with _on_stream(hi, cur):  # the gathered-side grads complete on the priority stream
        for h in handles:
            if h is not None:
                h.wait()
        if dqv is None:
            dqv = outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
    cur.wait_stream(hi)
    for oc in outs:
        oc.record_stream(cur)
    dqv.record_stream(cur)
    # consumers that can run on the priority stream (the packed [q|v] projection's
    # weight gradient, xdot.ops.linear.LinearFn) start there as soon as the
    # reduce-scatter lands, under the row-side kernel still running on `cur`
    if FLAGS.wgrad_side and dqv.dtype == k.dtype:
        dqv._xdot_ready_on = hi
    return dk, dqv, ds


# ----------------------------------------------------------------------------------------
class SeqParallelAttention(torch.autograd.Function):
    """Fused seq-parallel attention on a PACKED gathered-side operand ``qv`` = [q | v]
    (B, R, 2C): all-gather(s) in forward, reduce-scatter(s) in backward.  With several ranks
    the gathered side moves in row chunks (:func:`_row_chunks`): the kernels run per chunk
    into split partials (merged by one combine) so communication overlaps compute."""

    @staticmethod
    @_ext.pinned
    def forward(ctx, k, qv, mask, H, scale, comm, pending=None, k_prescaled=False, grad_on=True, Hg=None,
                layout="contiguous", sinks=None):
        """``k_prescaled``: ``k`` already holds ``rows * scale * log2 e`` (:func:`prescale_wanted`;
        the fused module folds it into the k projection's epilogue).  ``grad_on``: grad mode at the
        call (inside ``forward`` it is always off, and ``needs_input_grad`` ignores it).  ``Hg``:
        gathered heads when fewer than ``H`` (:func:`gathered_heads_arg`); ``qv`` is ``[q | v]`` with
        ``Hg`` heads each.  ``layout``: which global rows this rank's rows are
        (:mod:`xdot.parallel.layout`); only the mask depends on it.  ``sinks``: (H,) attention-sink
        logits (:func:`sinks_arg`) or None: folded once into whichever branch's ``(o, lse)``, and the
        folded pair is what is saved."""
        check_consistent(comm, "seq_parallel_attention", k, qv, H, Hg or H, layout, sinks is not None)
        B, R, C = k.shape
        n, rank = comm.world_size, comm.rank
        T = n * qv.shape[1]
        use_hip = _hip_ok(k, qv, H, Hg)
        if pending is None:
            pending = _PendingGather(comm, qv, _row_chunks(n, qv.shape[1], use_hip))
        chunks = pending.chunks
        prescaled, fm = False, 0  # (fm: the fp32 kernel family (XDOT_FP32_MODE), fixed here for the backward too)
        packed_full = None  # the whole-row packed mask, when the caller packed it ahead
        if use_hip:
            # wide fp32 heads are exact only (the ring asks fp32_code at every head dim: the two rules differ)
            fm =flash.fp32_code(k.dtype) if C // H <= 128 else 0
            # the row side pre-multiplied by scale*log2 e once (XDOT_PRESCALE, default on): the
            # forward and both backward kernels read this same buffer and seed their score
            # accumulators instead of scaling every score (saved in place of k for backward)
            prescaled = _prescale_rows(k)
            if prescaled and not k_prescaled:
                k = flash.prescale(k, scale)
            if isinstance(mask, flash.PendingMask):
                # (packed ahead in the tensor's own column order: the gathered side's only when
                # that is the global order)
                if len(chunks) == 1 and (layout == "contiguous" or n == 1):
                    packed_full = mask.get()
                mask = mask.raw
        mask = getattr(mask, "raw", mask)
        # a StructuredMask: bound to this rank's rows for the kernels' generated packed masks; the
        # torch path below gets its dense tensor, built once here
        mask = resolve_mask(mask, B, R, T, rank, use_hip, k.device, layout)
        gs = GatheredSide(k, H, Hg, scale, use_hip, prescaled, fm)  # how the kernels read the gathered side
        segmented =n > 1 and (FLAGS.local_first or len(chunks) > 1)
        sbuf = dsbuf = None
        # a backward can run on this forward (grad mode is off inside Function.forward: autograd's
        # needs_input_grad, or the fused node's, says it); without one no score buffer is taken
        # (no 20 GB allocation and store pass for inference / no_grad forwards)
        need_bwd = bool(grad_on) and any(getattr(ctx, "needs_input_grad", (True,))[:2])
        if use_hip and k.dtype == torch.float32 and need_bwd:
            sbuf, dsbuf, segmented = _score_buffers(k, H, T, fm, len(chunks) == 1 or B == 1, segmented)
        if segmented:
            o, lse, bufs = _segmented_forward(k, qv, mask, gs, pending, n, rank)
            mks = [packed_full] if packed_full is not None else None  # backward packs its own (cached)
        elif use_hip:  # one kernel over the whole gathered side; the (B, T, 2 Cq) wire buffer is what is saved
            if len(chunks) > 1:  # several gather chunks, one buffer in (chunk, rank, row) order
                pending.wait_all()
                qvg = pending.permuted()
                mk = _whole_mask(mask, B, R, n, chunks)
            else:
                mk = packed_full if packed_full is not None else _whole_mask(mask, B, R, n, chunks)
                qvg = flash.gathered_to_btc(pending.wait(0))     # (B, T, 2C), a view for B = 1
            o, lse = gs.fwd(k, gs.view(qvg), mk, sbuf)
            bufs, mks = [qvg], [mk]
        else:
            qvg = pending.wait(0)                            # (N, B, R, Cq + Cv) rank-major
            # one block, combined alone (a fully masked row comes out NaN)
            o, lse = _ref.combine([gs.ref_fwd(k, qvg, mask, rows=_as_global)], k.dtype)
            bufs, mks = [qvg], [mask]
        o, lse = gs.sink_fold(o, lse, sinks)
        # the score buffers travel as saved tensors: autograd frees them after the backward unless
        # the graph is retained (a ctx attribute would keep 20-40 GB alive as long as the graph is
        # referenced, e.g. through the previous step's loss)
        sbt = tuple(t for t in (sbuf, dsbuf) if t is not None)
        ctx.save_for_backward(k, o, lse, *bufs, *sbt, *(() if sinks is None else (sinks,)))
        ctx.has_sinks = sinks is not None
        ctx.mks, ctx.mask, ctx.chunks, ctx.comm, ctx.gs = mks, mask, chunks, comm, gs
        # (has S buffer, has dS buffer); the in-place mode (S only) is consumed by the first backward
        ctx.sb_kind = (sbuf is not None, dsbuf is not None)
        return o

    @staticmethod
    @_ext.pinned
    def backward(ctx, do):
        k, o, lse, *bufs = ctx.saved_tensors
        sinks = pop_sinks(ctx, bufs)
        nsb = sum(getattr(ctx, "sb_kind", (False, False)))
        bufs, sbt = bufs[:len(bufs) - nsb], bufs[len(bufs) - nsb:]
        do = do.contiguous()
        dk, dqv, ds = (_backward_hip(ctx, do, k, o, lse, bufs, sbt, sinks) if ctx.gs.use_hip else
                       _backward_torch(ctx, do, k, o, lse, bufs[0], sinks))
        return dk.to(k.dtype), dqv.to(k.dtype), None, None, None, None, None, None, None, None, None, sinks_grad(ds, sinks)


def gather_plan(qv_shape, qv: Tensor, comm: _comm.Communicator, chunks: Optional[int] = None):
    """Row chunks of the gathered side's pipeline for a (B, R, C) ``qv`` of this rank."""
    hip = _ext.use_hip(qv) and qv.dtype in FLASH_DTYPES
    return _row_chunks(comm.world_size, qv_shape[1], hip, chunks)


def start_gather(qv: Tensor, comm: Optional[_comm.Communicator] = None,
                 chunks: Optional[int] = None, out: Optional[Tensor] = None) -> "_PendingGather":
    """Issue the all-gather(s) of the packed gathered side early (e.g. before the row-side
    projection GEMM) and hand the result to :func:`seq_parallel_attention_packed`.
    ``chunks``: row chunks of the pipeline (default ``XDOT_GATHER_CHUNKS``).  ``out``: the
    (N, B, R, C) gather output whose block ``rank`` IS ``qv`` (the projection wrote it in place;
    one-chunk plans only)."""
    comm = comm or _comm.get_comm()
    plan = gather_plan(qv.shape, qv, comm, chunks)
    if out is not None and len(plan) != 1:
        raise ValueError("start_gather: an in-place output needs a one-chunk plan")
    return _PendingGather(comm, qv.detach(), plan, out=out)


def _checked_mask(mask, k: Tensor, T: int):
    """The mask argument of a ``*_packed`` entry point, validated: a :class:`StructuredMask`, a
    (B, R, T) tensor (-> bool), a ``flash.PendingMask`` of that shape, or None."""
    if isinstance(mask, StructuredMask):
        mask.check(k.shape[0])
    elif mask is not None:
        if tuple(mask.shape) != (k.shape[0], k.shape[1], T):
            raise ValueError(f"mask must be (B, R, T)=({k.shape[0]}, {k.shape[1]}, {T}), got {tuple(mask.shape)}")
        if isinstance(mask, torch.Tensor):
            mask = mask.to(torch.bool)
    return mask


def seq_parallel_attention_packed(k: Tensor, qv: Tensor, mask: Optional[Tensor], num_heads: int, scale: float,
                                  comm: Optional[_comm.Communicator] = None,
                                  pending: Optional["_PendingGather"] = None, k_prescaled: bool = False, *,
                                  gathered_heads: Optional[int] = None, layout: str = "contiguous",
                                  sinks: Optional[Tensor] = None) -> Tensor:
    """Fused sequence-parallel attention with a packed gathered side ``qv = [q | v]`` (B, R, 2C).

    ``gathered_heads``: heads of ``q`` and of ``v`` when fewer than ``num_heads`` (grouped-query
    attention: gathered head ``h // G`` serves row head ``h``, ``G = num_heads // gathered_heads``);
    ``q`` is then the first ``gathered_heads * (C // num_heads)`` columns of ``qv``.  Everything that
    crosses the wire or stays resident for the backward is that much narrower.

    ``layout``: the row sharding, ``"contiguous"`` (rank ``r`` holds the global rows ``[rR, (r+1)R)``)
    or ``"zigzag"`` (chunks ``r`` and ``2N-1-r`` of ``2N``, which balances a causal mask across ranks:
    :mod:`xdot.parallel.layout`; ``xdot.shard_rows`` / ``xdot.unshard_rows`` split and rebuild a
    sequence).  It decides which global row a local row is for a :class:`xdot.StructuredMask` and
    the global order of the gathered columns; a dense mask keeps local rows and GLOBAL columns.
    Every rank must pass the same one (``XDOT_CHECK`` compares it).

    ``pending``: the handle of :func:`start_gather` on this ``qv`` (the gather is issued here
    otherwise).  ``k_prescaled``: ``k`` already holds ``rows * scale * log2 e`` (only where
    :func:`prescale_wanted`; the gradient returned for it is w.r.t. the unscaled rows).

    ``sinks``: attention sinks, a float ``(num_heads,)`` tensor of one logit per ROW head that takes
    part in the softmax denominator and contributes no value (StreamingLLM / gpt-oss): row ``r`` of
    head ``h`` is ``softmax([scores_r, s_h])[:T] @ v``.  The logit is appended after mask and scale:
    it is NOT multiplied by ``scale``; zeros mean "one extra key of score 0".  With sinks a fully
    masked row gives 0 instead of NaN.  It is differentiable (each rank's gradient is the partial
    over its rows: sum it across ranks, as :class:`xdot.parallel.GradSync` does).  The kernels are
    untouched: one fold pass after the forward (``csrc/sink.hip``; a 16-bit output is rounded once by
    the kernel and once by the fold) and one small ordered sum in the backward.  ``None``: no launch,
    the result of the call without the argument bit for bit.  Every rank must pass sinks or none (``XDOT_CHECK`` compares it)."""
    comm = comm or _comm.get_comm()
    sinks = sinks_arg(sinks, num_heads, k)
    Hg = gathered_heads_arg(num_heads, gathered_heads)
    if k.dim() != 3 or qv.dim() != 3 or k.shape[-1] % num_heads or qv.shape[-1] <= _q_width(k, num_heads, Hg):
        raise ValueError("seq_parallel_attention_packed expects k (B, R, C) and qv (B, R, Cq + Cv) with "
                         "Cq = gathered_heads * C / num_heads")
    if Hg and (qv.shape[-1] - _q_width(k, num_heads, Hg)) % Hg:
        raise ValueError(f"the value half of qv ({qv.shape[-1] - _q_width(k, num_heads, Hg)} columns) does not "
                         f"divide into {Hg} gathered heads")
    mask = _checked_mask(mask, k, qv.shape[1] * comm.world_size)
    return SeqParallelAttention.apply(k, qv, mask, num_heads, float(scale), comm, pending, bool(k_prescaled),
                                      torch.is_grad_enabled(), Hg, check_layout(layout), sinks)


def seq_parallel_attention(k: Tensor, q: Tensor, v: Tensor, mask: Optional[Tensor], num_heads: int,
                           scale: float, comm: Optional[_comm.Communicator] = None, rope=None, *,
                           gathered_heads: Optional[int] = None, layout: str = "contiguous",
                           sinks: Optional[Tensor] = None) -> Tensor:
    """Fused sequence-parallel attention on projected, head-interleaved (B, R, H*d) tensors
    (``q`` / ``v``: ``gathered_heads * d`` columns when given, grouped-query attention).

    ``k``: row side (local rows), ``q``/``v``: gathered side (local shards), ``mask``: bool
    (B, R, T) with True = masked, a :class:`xdot.StructuredMask` (causal / window / lengths / documents; its
    packed form is generated on the GPU, the torch path builds its dense tensor), or None.
    ``rope``: an :class:`xdot.Rotary`; ``k`` and ``q`` are rotated at this rank's global positions
    (``rank * R`` unless the object carries an offset) before the attention, ``v`` is not.
    ``layout``: the row sharding, as :func:`seq_parallel_attention_packed` (the rotation follows it).
    ``sinks``: (H,) attention-sink logits, as :func:`seq_parallel_attention_packed`.
    Returns (B, R, H*dv) in ``k``'s dtype.
    """
    if k.dim() != 3 or q.dim() != 3 or v.dim() != 3:
        raise ValueError("seq_parallel_attention expects (B, R, H*d) tensors")
    if rope is not None:
        from ..ops.rope import rope as _rope

        c = comm or _comm.get_comm()
        off = rope.resolve(c.rank, k.shape[1], c.world_size, check_layout(layout))
        k = _rope(k, num_heads, rope, offset=off)
        q = _rope(q, gathered_heads_arg(num_heads, gathered_heads) or num_heads, rope, offset=off)
    return seq_parallel_attention_packed(k, torch.cat([q, v], dim=-1), mask, num_heads, scale, comm,
                                         gathered_heads=gathered_heads, layout=layout, sinks=sinks)
