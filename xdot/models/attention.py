"""``DistributedDotProductAttn`` — multi-head attention over time-sharded sequences.

Same constructor, forward signature, math and submodule names as the reference
(``distributed_dot_product/module.py:22-76``), so ``state_dict``s interchange:
``keys``/``queries``/``values``/``composition`` Linears, ``S = K·Qᵀ/√(key_dim/H)`` where
**``keys`` is the local/row side and ``queries`` the gathered side**, ``S[mask] = -inf``,
``P = softmax(S)``, ``O = P·V``, ``out = composition(merge(O))``.

Three execution paths, chosen by ``impl``:

``'materialized'`` — the reference's structure, op for op: ``RightTransposeMultiplication``
    → fused scale+mask+softmax kernel → ``FullMultiplication``.  Scores (B, H, T/N, T) are
    materialised once (bf16 on MI355X: 1.25 GB/rank at T=25000, N=8).
``'flash'`` — sequence-parallel fused attention (:mod:`xdot.parallel.attention`): K/V-side
    all-gather once, MFMA flash-attention kernels with online softmax (scores never exist in
    HBM), backward by recomputation with reduce-scatter of the gathered-side gradients.
    Required for long context (T=200000: materialised bf16 scores would be 80 GB per rank).
``'ring'`` — the same kernels fed by a ring of point-to-point RCCL hops
    (:mod:`xdot.parallel.ring`): the gathered side travels one rank-block at a time and is
    never resident in full; its gradient accumulator rides the ring back (no reduce-scatter).
``'auto'`` (default) — ``'flash'`` for bf16/fp16 GPU tensors with a supported head dim, else
    ``'materialized'``.

Extensions over the reference (all backward compatible): ``attn_mask=None`` means no mask,
``value_dim`` may differ from ``key_dim`` with several heads (the reference raises), any
float dtype works, and ``distributed=False`` gives the single-device ground truth.
``attn_mask`` may also be a :class:`xdot.StructuredMask` (causal / sliding window / key lengths):
the flash and ring kernels' packed mask is then generated on the GPU from the description
(``row_offset=None`` resolves to ``rank * R``) and no ``(B, R, T)`` tensor exists; the paths that
only take a dense mask -- ``'materialized'``, CPU tensors, ``backend='torch'`` -- build
``StructuredMask.dense(...)`` once per call and so do allocate it.

Keyword-only knobs (each mirrors an environment flag, the argument wins):

``impl``        ``'auto'`` | ``'flash'`` | ``'ring'`` | ``'materialized'`` (above);
``fused``       ``True`` = ``impl='flash'``, ``False`` = ``impl='materialized'`` (SURVEY name);
``backend``     ``'auto'`` | ``'hip'`` | ``'torch'``: compute backend of this module's ops, forward
                and backward (``XDOT_BACKEND``); ``'torch'`` runs the torch reference math on GPU;
``dtype``       compute-dtype policy: e.g. ``torch.bfloat16`` runs projections and attention in
                bf16 while parameters / inputs stay fp32 (master weights); output in the input
                dtype.  ``None``: compute in the input dtype;
``chunk_plan``  row chunks of the fused path's all-gather / reduce-scatter pipeline
                (``XDOT_GATHER_CHUNKS``); the materialised path's chunking is ``offset``;
``comm``        communicator (default: the process group of :func:`xdot.init`);
``num_gathered_heads``  heads of ``queries`` / ``values`` (the gathered side; grouped-query
                attention's ``num_kv_heads``): gathered head ``h // G`` serves row head ``h``,
                ``G = num_heads // num_gathered_heads``.  ``queries`` / ``values`` project to that
                many heads, so the all-gather, the reduce-scatter, the ring hops and the buffer kept
                for the backward are ``G`` times smaller.  ``None`` (default): ``num_heads``;
``rope``        an :class:`xdot.Rotary`: ``k`` and ``q`` are rotated (rotary position embedding,
                :mod:`xdot.ops.rope`) after their projections, at this rank's global positions
                (``rank * R`` unless the object carries an offset; 0 with ``distributed=False``),
                on every path; ``v`` is untouched.  ``None`` (default): no rotation, no launch.
``layout``      the row sharding of the sequence tensors: ``'contiguous'`` (default, the reference's:
                rank ``r`` holds the global rows ``[rR, (r+1)R)``) or ``'zigzag'`` (the sequence cut
                into ``2N`` chunks, rank ``r`` holds chunks ``r`` and ``2N-1-r``:
                :mod:`xdot.parallel.layout`), under which every rank has about half live score
                tiles of a causal mask instead of ``1/(2N)`` .. ``(2N-1)/(2N)`` of them.  The inputs
                are this rank's rows in that layout (``xdot.shard_rows`` / ``xdot.unshard_rows``); a
                ``StructuredMask`` and ``rope`` follow it (an explicit ``row_offset`` / ``offset``
                contradicts ``'zigzag'``), a dense ``attn_mask`` keeps local rows and GLOBAL columns.
                Communication, gather chunks and kernels are layout-blind; ``distributed=False``
                ignores it (a world of one is the identity).
``qk_norm``     ``True``: QK-norm, an RMSNorm over each head's ``key_dim // num_heads`` features of
                the projected ``k`` (its ``num_heads`` heads) and ``q`` (its ``num_gathered_heads``
                heads) with a learnable gain each: two :class:`xdot.HeadRMSNorm` submodules,
                ``keys_norm`` and ``queries_norm`` (two more ``state_dict`` keys).  Order: projection
                -> norm -> rope -> attention, on every path; ``v`` is untouched.  On the GPU the norm
                and the rotation are ONE pass (:mod:`xdot.ops.headnorm`).  ``False`` (default): no
                submodules, no launch; ``qk_norm_eps`` is the ``eps`` under the square root.
``sinks``       ``True``: attention sinks, one learnable logit per ROW head (``self.sinks``, a
                ``(num_heads,)`` parameter, one more ``state_dict`` key; grouped heads do not change
                it) that takes part in the softmax denominator and contributes no value:
                ``P = softmax([S, s_h])[..., :T]``.  The logit is appended after mask and scale -- it
                is NOT multiplied by ``1/sqrt(d)`` -- and starts at zero: "one extra key of score 0".
                A row whose columns are all masked then gives 0 instead of NaN, on every path.  The
                flash and ring kernels are untouched: one fold pass over the finished ``(o, lse)``
                and one small ordered sum in the backward (``csrc/sink.hip``; a 16-bit output is
                rounded once by the kernel and once by the fold).  The parameter is replicated: each
                rank's gradient is the partial over its rows, which ``GradSync`` sums.  ``False``
                (default): no parameter, no launch, the same result bit for bit.
``gate``        ``'elementwise'`` | ``'headwise'``: gated attention (Qiu et al. 2025; Qwen3-Next), a
                query-dependent sigmoid gate on the merged attention output before ``composition``:
                ``g = gate(keys_input)``, ``o' = o * sigmoid(g)``, ``out = composition(o')``, with
                ``self.gate`` an ``nn.Linear(key_dim, value_dim)`` (``'elementwise'``: one gate value
                per output feature) or ``nn.Linear(key_dim, num_heads)`` (``'headwise'``: one per
                (row, row head), broadcast over that head's features; grouped heads do not change
                it), bias as ``add_bias``, ``nn.Linear``'s own initialisation: a zero pre-activation
                HALVES the output.  The order on every path is attention (sinks included), gate,
                ``composition``; the gate is row-local, so layout, gather chunks, ring hops and
                grouped heads do not see it.  One pass each way (``csrc/gate.hip``,
                :func:`xdot.sigmoid_gate`); no flash kernel changes.  The parameters are replicated
                like the other projections'.  ``None`` (default): no submodule, no ``state_dict``
                key, no launch, the same result bit for bit.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from .. import _ext
from ..ops.gate import sigmoid_gate
from ..ops.linear import linear
from ..ops.mask import StructuredMask
from ..ops.headnorm import HeadRMSNorm
from ..ops.qkprep import prep
from ..ops.rope import Rotary, _table_dtype
from ..ops.softmax import scale_mask_softmax
from ..parallel import attention as pa
from ..parallel.autograd import FullMultiplication, RightTransposeMultiplication
from ..parallel.ring import ring_attention_packed
from ..parallel.layout import check_layout
from ..utils import comm as _comm
from ..utils.env import FLAGS

__all__ = ["DistributedDotProductAttn"]

_LOG2E = 1.4426950408889634  # as xdot.models.fused: the row side's pre-scale is scale * log2 e


def _adjacent(a: Tensor, b: Tensor) -> bool:
    return (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.device == b.device
            and tuple(a.shape[1:]) == tuple(b.shape[1:])
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel())


class _RowsView(torch.autograd.Function):
    """``cat([a, b], 0)`` as a no-copy view of the storage ``a`` and ``b`` share (``b`` stored
    right after ``a``); the gradient splits back into two row views."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.shape[0]
        return a.detach().as_strided((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride(),
                                     a.storage_offset())

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.n], g[ctx.n:]


def _stacked_rows(a: Tensor, b: Tensor) -> Tensor:
    """``cat([a, b], 0)`` for two parameters.  First use (or after ``.to()`` gave them separate
    storages): both are moved into ONE contiguous buffer (``.data`` rebound: the Parameter
    objects, their optimizer state and ``state_dict`` keys are unchanged); every later call is a
    view of it."""
    if not _adjacent(a, b):
        if not (isinstance(a, nn.Parameter) and isinstance(b, nn.Parameter) and a.dtype == b.dtype
                and a.device == b.device and tuple(a.shape[1:]) == tuple(b.shape[1:])) \
                or torch.is_inference_mode_enabled():
            # (under inference mode the packed buffer would be an inference tensor that later
            # in-place optimizer updates could not touch: no repack there)
            return torch.cat([a, b], 0)
        with torch.no_grad():
            packed = torch.empty((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
            packed[:a.shape[0]].copy_(a)
            packed[a.shape[0]:].copy_(b)
            a.data = packed[:a.shape[0]]
            b.data = packed[a.shape[0]:]
    return _RowsView.apply(a, b)


class DistributedDotProductAttn(nn.Module):
    def __init__(self, key_dim: int, value_dim: Optional[int] = None, query_dim: Optional[int] = None,
                 num_heads: int = 1, add_bias: bool = False, offset: Optional[int] = 32,
                 distributed: bool = True, *, impl: str = "auto", fused: Optional[bool] = None,
                 backend: str = "auto", dtype: Optional[torch.dtype] = None, chunk_plan: Optional[int] = None,
                 comm: Optional[_comm.Communicator] = None, rope: Optional[Rotary] = None,
                 num_gathered_heads: Optional[int] = None, layout: str = "contiguous", qk_norm: bool = False,
                 qk_norm_eps: float = 1e-6, sinks: bool = False, gate: Optional[str] = None):
        super().__init__()
        check_layout(layout)
        if fused is not None:
            if impl not in ("auto", "flash" if fused else "materialized"):
                raise ValueError(f"fused={fused} contradicts impl={impl!r}")
            impl = "flash" if fused else "materialized"
        if backend not in ("auto", "hip", "torch"):
            raise ValueError(f"backend must be auto|hip|torch, got {backend!r}")
        if dtype is not None and not (isinstance(dtype, torch.dtype) and dtype.is_floating_point):
            raise ValueError(f"dtype must be a floating torch.dtype or None, got {dtype!r}")
        if chunk_plan is not None and int(chunk_plan) < 1:
            raise ValueError(f"chunk_plan must be a positive number of row chunks, got {chunk_plan!r}")
        if key_dim % num_heads != 0:
            raise ValueError(f"key_dim {key_dim} not divisible by num_heads {num_heads}")
        value_dim = value_dim if value_dim is not None else key_dim
        query_dim = query_dim if query_dim is not None else key_dim
        if value_dim % num_heads != 0:
            raise ValueError(f"value_dim {value_dim} not divisible by num_heads {num_heads}")
        if impl not in ("auto", "flash", "materialized", "ring"):
            raise ValueError(f"impl must be auto|flash|materialized|ring, got {impl!r}")
        if num_gathered_heads is None:
            num_gathered_heads = num_heads
        if int(num_gathered_heads) < 1 or num_heads % int(num_gathered_heads) != 0:
            raise ValueError(f"num_heads {num_heads} not divisible by num_gathered_heads {num_gathered_heads}")
        if rope is not None:
            if not isinstance(rope, Rotary):
                raise TypeError(f"rope must be an xdot.Rotary or None, got {type(rope).__name__}")
            if (key_dim // num_heads) % 2:
                raise ValueError(f"rope needs an even head dim, got {key_dim // num_heads}")
        if not float(qk_norm_eps) > 0.0:
            raise ValueError(f"qk_norm_eps must be positive, got {qk_norm_eps!r}")
        if gate is not None and gate not in ("headwise", "elementwise"):
            raise ValueError(f"gate must be None, 'headwise' or 'elementwise', got {gate!r}")
        self.num_heads = num_heads
        self.num_gathered_heads = int(num_gathered_heads)
        self.value_dim = value_dim
        self.offset = offset
        self.distributed = distributed
        self.dim = key_dim // num_heads
        self.impl = impl
        self.backend = backend
        self.compute_dtype = dtype
        self.chunk_plan = None if chunk_plan is None else int(chunk_plan)
        self.comm = comm
        self.rope = rope
        self.layout = layout
        self.keys = nn.Linear(key_dim, key_dim, bias=add_bias)
        # the gathered side: num_gathered_heads heads (key_dim / value_dim wide by default)
        self.queries = nn.Linear(query_dim, self.num_gathered_heads * self.dim, bias=add_bias)
        self.values = nn.Linear(value_dim, self.num_gathered_heads * (value_dim // num_heads), bias=add_bias)
        self.composition = nn.Linear(value_dim, value_dim, bias=add_bias)
        self.qk_norm = bool(qk_norm)
        self.qk_norm_eps = float(qk_norm_eps)
        if self.qk_norm:  # (no submodule without it: reference checkpoints keep loading)
            self.keys_norm = HeadRMSNorm(self.dim, self.qk_norm_eps)
            self.queries_norm = HeadRMSNorm(self.dim, self.qk_norm_eps)
        if sinks:  # (no parameter without it: reference checkpoints keep loading)
            self.sinks = nn.Parameter(torch.zeros(num_heads))
        else:
            self.register_parameter("sinks", None)
        self.gate_kind = gate
        if gate is not None:  # (no submodule without it: reference checkpoints keep loading)
            # a zero pre-activation halves the output: sigmoid(0) = 1/2
            self.gate = nn.Linear(key_dim, value_dim if gate == "elementwise" else num_heads, bias=add_bias)
        # weakref to an attached xdot.parallel.GradSync (set by it): the fused node hands it the
        # parameter gradients as they are computed (early all-reduce)
        self._xdot_grad_sync = None

    # ------------------------------------------------------------------------------------
    def _pick_impl(self, x: Tensor) -> str:
        if self.impl != "auto":
            return self.impl
        with _ext.backend(self.backend):
            if self.compute_dtype is not None:
                x = x.to(self.compute_dtype) if x.is_floating_point() else x
            return "flash" if pa.flash_supported(x, self.dim, self.value_dim // self.num_heads) else "materialized"

    def forward(self, keys: Tensor, queries: Tensor, values: Tensor, attn_mask: Optional[Tensor] = None) -> Tensor:
        with _ext.backend(self.backend):
            cdt = self.compute_dtype
            if cdt is None or keys.dtype == cdt:
                return self._forward(keys, queries, values, attn_mask)
            out_dt = keys.dtype
            same_qv = queries is values
            keys_c = keys.to(cdt)
            queries_c = keys_c if queries is keys else queries.to(cdt)
            values_c = queries_c if same_qv else (keys_c if values is keys else values.to(cdt))
            return self._forward(keys_c, queries_c, values_c, attn_mask).to(out_dt)

    def _w(self, t: Optional[Tensor]) -> Optional[Tensor]:
        """A parameter in the compute dtype (autograd flows back to the master copy)."""
        if t is None or self.compute_dtype is None or t.dtype == self.compute_dtype:
            return t
        return t.to(self.compute_dtype)

    def _forward(self, keys: Tensor, queries: Tensor, values: Tensor, attn_mask: Optional[Tensor]) -> Tensor:
        if FLAGS.check and self.distributed:
            # ranks that disagree on the gate would hang in GradSync (one more pair of gradients): the
            # kind rides in the fingerprints of the distributed ops below (XDOT_CHECK)
            from ..utils.checks import fingerprint_extra

            with fingerprint_extra("gate", self.gate_kind):
                return self._forward_impl(keys, queries, values, attn_mask)
        return self._forward_impl(keys, queries, values, attn_mask)

    def _forward_impl(self, keys: Tensor, queries: Tensor, values: Tensor, attn_mask: Optional[Tensor]) -> Tensor:
        """The dispatch.  Every path below is: project, prep ``k`` / ``q`` (:meth:`_prep`), attend,
        gate, compose."""
        impl = self._pick_impl(keys)
        lay = self.layout if self.distributed else "contiguous"  # (a world of one: the identity)
        comm = (self.comm or _comm.get_comm()) if self.distributed else _comm.LocalComm()
        scale = 1.0 / math.sqrt(self.dim)
        if impl == "ring":
            return self._ring(keys, queries, values, attn_mask, scale, comm, lay)
        if impl != "flash":
            return self._materialized(keys, queries, values, attn_mask, scale, comm, lay)
        dk, dv = self.dim, self.value_dim // self.num_heads
        Dp = pa.flash_head_dim(dk, dv) if keys.is_cuda else dk
        if keys.is_cuda and Dp is not None and (Dp != dk or Dp != dv):
            return self._flash_padded(keys, queries, values, attn_mask, scale, comm, lay, Dp)
        if isinstance(attn_mask, Tensor) and attn_mask.is_cuda and attn_mask.dim() == 3 and FLAGS.mask_async \
                and (lay == "contiguous" or comm.world_size == 1):
            # pack the mask on a side stream while the projection GEMMs run (its columns as they
            # are: the gathered side's order only under the contiguous layout)
            from ..ops import flash

            attn_mask = flash.prepare_mask_async(attn_mask.to(torch.bool), attn_mask.shape[0],
                                                 attn_mask.shape[1], attn_mask.shape[2])
        if (FLAGS.fused_module and queries is values and self.queries.in_features == self.values.in_features
                and (self.compute_dtype is None or self.keys.weight.dtype == self.compute_dtype)):
            return self._flash_one_node(keys, queries, attn_mask, scale, comm, lay)
        return self._flash_per_op(keys, queries, values, attn_mask, scale, comm, lay)

    @property
    def _gh(self) -> Optional[int]:
        """The gathered heads as the attention functions take them: None for the default."""
        return None if self.num_gathered_heads == self.num_heads else self.num_gathered_heads

    def _flash_padded(self, keys, queries, values, attn_mask, scale, comm, lay, Dp):
        """Head dims the flash kernels do not take (or value width != key width): every head
        zero-padded to the next kernel dim ``Dp``, same scale ``1/sqrt(dk)``."""
        H, Hg, dk, dv = self.num_heads, self.num_gathered_heads, self.dim, self.value_dim // self.num_heads
        qv = self._project_qv(queries, values)
        q, k = qv[..., :Hg * dk], self._proj(self.keys, keys)
        off = self._rope_offset(comm, k.shape[1], lay)
        # at width dk, before the zero padding
        q, k = self._prep(q, Hg * dk, Hg, False, off), self._prep(k, H * dk, H, True, off)
        # (the Hg gathered heads and the H row heads are padded separately)
        qv = torch.cat([pa.pad_heads(q, Hg, dk, Dp), pa.pad_heads(qv[..., Hg * dk:], Hg, dv, Dp)], dim=-1)
        k = pa.pad_heads(k, H, dk, Dp)
        o = pa.seq_parallel_attention_packed(k, qv, attn_mask, H, scale, comm=comm, gathered_heads=self._gh, layout=lay,
                                             sinks=self.sinks)
        return self._proj(self.composition, self._gated(pa.unpad_heads(o, H, dv, Dp), keys))

    def _flash_one_node(self, keys, queries, attn_mask, scale, comm, lay):
        """The whole module as ONE autograd node (:mod:`xdot.models.fused`): same kernels, streams
        and numerics, a fraction of the per-op host work."""
        from .fused import AttnBlockFn

        wq, wv = self.queries.weight, self.values.weight
        bq, bv = self.queries.bias, self.values.bias
        if isinstance(wq, nn.Parameter) and isinstance(wv, nn.Parameter):
            _stacked_rows(wq, wv)  # (re)pack the two parameters into one storage once
            if bq is not None:
                _stacked_rows(bq, bv)
        gs = self._xdot_grad_sync() if self._xdot_grad_sync is not None else None
        sync = None
        if gs is not None and torch.is_grad_enabled():
            gs.note_use(id(self))
            sync = (gs, id(self))
        wkn, wqn = (self.keys_norm.weight, self.queries_norm.weight) if self.qk_norm else (None, None)
        wg, bg = (self.gate.weight, self.gate.bias) if self.gate_kind is not None else (None, None)
        return AttnBlockFn.apply(keys, queries, attn_mask, self.keys.weight, self.keys.bias, wq, bq, wv, bv,
                                 self.composition.weight, self.composition.bias, self.num_heads, scale, comm,
                                 self.chunk_plan, sync, torch.is_grad_enabled(), self.rope, self._gh, lay,
                                 wkn, wqn, self.qk_norm_eps, self.sinks, wg, bg)

    def _flash_per_op(self, keys, queries, values, attn_mask, scale, comm, lay):
        """One autograd node per op.  The gathered side first: its all-gather runs while the
        row-side GEMM computes."""
        H, Hg, dk = self.num_heads, self.num_gathered_heads, self.dim
        qv = self._project_qv(queries, values)
        off = self._rope_offset(comm, qv.shape[1], lay)
        qv = self._prep(qv, Hg * dk, Hg, False, off)  # q before the gather is issued
        pending = pa.start_gather(qv, comm, chunks=self.chunk_plan)
        k = self._proj(self.keys, keys)
        # the row side's pre-scale rides in the rotation / norm pass (its gradient comes back w.r.t.
        # the unscaled rows: no factor in the backward)
        pre = (self.rope is not None or self.qk_norm) and pa.prescale_wanted(k, qv, H, self._gh)
        k = self._prep(k, H * dk, H, True, off, alpha=scale * _LOG2E if pre else 1.0, bwd_alpha=1.0)
        o = pa.seq_parallel_attention_packed(k, qv, attn_mask, H, scale, comm=comm, pending=pending, k_prescaled=pre,
                                             gathered_heads=self._gh, layout=lay, sinks=self.sinks)
        return self._proj(self.composition, self._gated(o, keys))

    def _ring(self, keys, queries, values, attn_mask, scale, comm, lay):
        H, Hg = self.num_heads, self.num_gathered_heads
        qv = self._project_qv(queries, values)
        k = self._proj(self.keys, keys)
        off = self._rope_offset(comm, k.shape[1], lay)
        qv = self._prep(qv, Hg * self.dim, Hg, False, off)
        k = self._prep(k, k.shape[-1], H, True, off)
        o = ring_attention_packed(k, qv, attn_mask, H, scale, comm=comm, gathered_heads=self._gh, layout=lay,
                                  sinks=self.sinks)
        return self._proj(self.composition, self._gated(o, keys))

    def _gated(self, o: Tensor, keys: Tensor) -> Tensor:
        """``o * sigmoid(gate(keys))`` (``o`` itself without a gate): after the attention, sink fold
        included, and before ``composition``."""
        if self.gate_kind is None:
            return o
        return sigmoid_gate(o, self._proj(self.gate, keys), self.num_heads)

    def _rope_offset(self, comm, R: int, lay: str):
        """This rank's rotary positions (None without ``rope``)."""
        return None if self.rope is None else self.rope.resolve(comm.rank, R, comm.world_size, lay)

    def _prep(self, x: Tensor, ncols: int, heads: int, row_side: bool, off, alpha: float = 1.0,
              bwd_alpha: Optional[float] = None) -> Tensor:
        """norm -> rope of the first ``ncols`` features of a projection's output (all of a ``k`` or ``q``; the
        ``q`` part of a packed ``[q | v]``, whose rest is copied) as one autograd node and one pass; ``x`` itself with
        neither.  ``row_side``: ``keys_norm``'s gain, else ``queries_norm``'s; ``off``: :meth:`_rope_offset`."""
        if self.rope is None and not self.qk_norm:
            return x
        tab = None if self.rope is None else self.rope.table(x.shape[1], ncols // heads, off, x.device, _table_dtype(x))
        gain = (self.keys_norm if row_side else self.queries_norm).weight if self.qk_norm else None
        return prep(x, ncols, heads, tab, gain, self.qk_norm_eps, alpha, bwd_alpha)

    def _proj(self, layer: nn.Linear, x: Tensor) -> Tensor:
        """``layer(x)`` (compute dtype) with the split-K MFMA weight gradient (:mod:`xdot.ops.linear`)."""
        return linear(x, self._w(layer.weight), self._w(layer.bias))

    def _project_qv(self, queries: Tensor, values: Tensor) -> Tensor:
        """[q | v] packed (B, R, 2C): ONE GEMM when ``queries is values`` (self-attention), so
        the gathered side travels in one all-gather and its grads in one reduce-scatter.  The
        ``queries`` / ``values`` parameters share one storage (re-packed once after a ``.to()``),
        so the packed weight is a view: no concatenation kernel and no autograd node per step."""
        if queries is values and self.queries.in_features == self.values.in_features:
            w = self._w(_stacked_rows(self.queries.weight, self.values.weight))
            b = None
            if self.queries.bias is not None:
                b = self._w(_stacked_rows(self.queries.bias, self.values.bias))
            return linear(queries, w, b)
        return torch.cat([self._proj(self.queries, queries), self._proj(self.values, values)], dim=-1)

    def _materialized(self, keys, queries, values, attn_mask, scale, comm, lay):
        H = self.num_heads
        k = self._proj(self.keys, keys)
        q = self._proj(self.queries, queries)
        v = self._proj(self.values, values)
        off = self._rope_offset(comm, k.shape[1], lay)
        k = self._prep(k, k.shape[-1], H, True, off)
        q = self._prep(q, q.shape[-1], self.num_gathered_heads, False, off)
        B, R = k.shape[0], k.shape[1]
        if H > 1:
            k = k.view(B, R, H, self.dim).transpose(1, 2)
            Hg = self.num_gathered_heads
            q = q.view(B, q.shape[1], Hg, self.dim).transpose(1, 2)
            v = v.view(B, v.shape[1], Hg, self.value_dim // H).transpose(1, 2)
            if Hg != H:  # grouped heads: every gathered head repeated for its group's products
                q, v = q.repeat_interleave(H // Hg, dim=1), v.repeat_interleave(H // Hg, dim=1)
        if self.distributed:
            s = RightTransposeMultiplication.apply(k, q, self.offset, comm)
        else:
            s = torch.matmul(k, q.transpose(-1, -2))
        if attn_mask is not None:
            # the softmax kernel takes a dense mask: a StructuredMask's (B, R, T) tensor is built
            # here, once; the scores' columns are in rank-major gathered order, which under a
            # layout is not the global order a dense tensor's columns come in
            from ..ops.mask import resolve as resolve_mask

            attn_mask = resolve_mask(attn_mask, B, R, s.shape[-1], comm.rank, False, s.device, lay)
        if self.sinks is not None:
            p = self._sink_softmax(s, attn_mask, scale)
        else:
            p = scale_mask_softmax(s, attn_mask, scale)
        if self.distributed:
            o = FullMultiplication.apply(p, v, self.offset, comm)
        else:
            o = torch.matmul(p, v)
        if H > 1:
            o = o.transpose(1, 2).reshape(B, R, self.value_dim)
        return self._proj(self.composition, self._gated(o, keys))

    def _sink_softmax(self, s: Tensor, mask: Optional[Tensor], scale: float) -> Tensor:
        """``softmax([s * scale (masked), sinks])[..., :T]`` in torch (the reference-structured path):
        the row log-sum-exp of the masked, scaled scores joined with the unscaled sink logit, and the
        probabilities taken against it -- ``exp(-inf - lse')`` is 0, so a fully masked row gives 0."""
        x = s.float() * scale if s.dtype != torch.float64 else s * scale
        if mask is not None:
            x = x.masked_fill(mask.unsqueeze(1) if x.dim() == 4 else mask, -float("inf"))
        sk = self.sinks.to(x.dtype)
        sk = sk.view(1, -1, 1) if x.dim() == 4 else sk.view(1, 1)
        lse = torch.logaddexp(torch.logsumexp(x, dim=-1), sk)
        return torch.exp(x - lse.unsqueeze(-1)).to(s.dtype)

    def extra_repr(self) -> str:
        return (f"heads={self.num_heads}, head_dim={self.dim}, value_dim={self.value_dim}, "
                f"offset={self.offset}, distributed={self.distributed}, impl={self.impl}, backend={self.backend}, "
                f"dtype={self.compute_dtype}, chunk_plan={self.chunk_plan}"
                + (f", rope={self.rope!r}" if self.rope is not None else "")
                + (f", num_gathered_heads={self.num_gathered_heads}" if self.num_gathered_heads != self.num_heads else "")
                + (f", layout={self.layout}" if self.layout != "contiguous" else "")
                + (f", qk_norm=True, qk_norm_eps={self.qk_norm_eps:g}" if self.qk_norm else "")
                + (", sinks=True" if self.sinks is not None else "")
                + (f", gate={self.gate_kind}" if self.gate_kind is not None else ""))
