"""The whole module on the fused (flash) path as ONE autograd node.

Reference structure (``distributed_dot_product/module.py:41-76``): three input projections,
``RightTransposeMultiplication`` -> scale / mask / softmax -> ``FullMultiplication``, the
output projection -- each an autograd node whose backward the engine schedules separately
(``multiplication/ops.py:29-37, :49-54``).  On the flash path the per-node host work (Python
``Function.apply`` / ``backward`` dispatch, argument flattening, saved-tensor bookkeeping) is a
large share of the per-rank step's host time at N=8 (``profiles/r3_rank_host.md``), where the
GPU step is only ~1.4 ms.  :class:`AttnBlockFn` runs

    forward   [q|v] = x_qv Wqvᵀ (+b)  ->  all-gather issued  ->  k = x_k Wkᵀ (+b)
              ->  seq-parallel flash attention  ->  out = o Wcᵀ (+b)
    backward  do = dout Wc  ->  attention backward (both kernels, reduce-scatter)
              ->  dx_k  ->  dx_qv
              beside it: dWc / dbc on a second stream, under the attention backward; dWk / dbk
              there too, under the input-gradient GEMMs; dW[q|v] on the attention backward's
              priority stream as soon as the reduce-scatter lands (under the row-side kernel)

with the same kernels, streams and numerics as the per-op graph (``XDOT_FUSED_MODULE=0``
restores it), and hands back the eight parameter gradients and the input gradients in one go.
With ``rope`` (an :class:`xdot.Rotary`) q is rotated in place in ``[q|v]`` before the gather is
issued and k after its projection; the backward inverse-rotates ``dk`` and ``dq`` in place before
the projections' gradients read them (``csrc/rope.hip``: two launches each way).
With QK-norm (``norm``: the two gains and ``eps``) the same two spots run the norm and the rotation
as one pass (``csrc/headnorm.hip``): the forward's passes also leave ``rstd`` and a bit copy of the
pre-norm ``k`` / ``q`` (both are overwritten in place), the backward's passes run in place on ``dk``
and the ``q`` part of ``d[q|v]`` and return the two gain gradients.
With attention sinks (``sinks``: the (H,) logits) the attention folds them into its finished forward
and its backward hands back their gradient, which goes to ``GradSync`` like every replicated parameter's.
With a gate (``wg`` / ``bg``: the gate projection, ``xdot.ops.gate``) ``g = x_k Wgᵀ (+b)`` is issued beside
the ``k`` projection, under the all-gather; ``o' = o ⊙ σ(g)`` (``csrc/gate.hip``, one launch) runs between
the attention and the output projection, which reads ``o'``.  Kept for the backward: ``o'`` (the output
projection's weight gradient) and ``g``; the ungated ``o`` is the tensor the attention saves anyway.  The
backward runs the output projection's ``linear_backward`` on ``(dout, o')``, one ``gate_backward`` launch
(``do`` in place over ``do'``), the unchanged attention backward on ``do``, then the gate projection's
gradients; its input gradient is ADDED to ``dx_k`` (one add pass).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .. import _ext
from ..ops.linear import linear_backward, native_wgrad, proj, weight_grad_pair
from ..ops.gate import gate_apply, gate_backward
from ..ops.qkprep import prep_apply, prep_backward
from ..ops.rope import _table_dtype
from ..utils.env import FLAGS
from ..utils.streams import _on_stream, _side_stream
from ..parallel.attention import SeqParallelAttention, gather_plan, prescale_wanted, start_gather

_LOG2E = 1.4426950408889634  # as the kernels' scale * log2 e (csrc/flash_common.h, csrc/reduce.hip)

__all__ = ["AttnBlockFn"]

# AttnBlockFn.forward's parameters after ``ctx``, in order (tests/test_fused_args.py holds the two
# together); the backward reads ``needs_input_grad`` and fills its return through ``_I.<name>``
ARG_NAMES = ("xk", "xqv", "mask", "wk", "bk", "wq", "bq", "wv", "bv", "wc", "bc", "H", "scale", "comm", "chunk_plan",
             "sync", "grad_on", "rope", "Hg", "layout", "wkn", "wqn", "norm_eps", "sinks", "wg", "bg")
_I = SimpleNamespace(**{name: i for i, name in enumerate(ARG_NAMES)})


class _Ctx:
    """Stand-in ``ctx`` for calling :class:`SeqParallelAttention`'s forward / backward inline."""

    def save_for_backward(self, *ts):
        self._saved = ts

    @property
    def saved_tensors(self):
        return self._saved


def _rows(a, b):
    """``cat([a, b], 0)``: a view when ``b`` is stored right after ``a`` (the module keeps the
    ``queries`` / ``values`` parameters in one storage), else a copy."""
    from .attention import _adjacent

    if _adjacent(a, b):
        return a.detach().as_strided((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())
    return torch.cat([a, b], 0)


def _wgrad_stream(t):
    """Second compute stream for the weight gradients that only the optimizer needs (None on
    the CPU, under HIP-graph capture, with ``XDOT_WGRAD_SIDE=0`` and when the weight gradients
    are library GEMMs: ``xdot.ops.linear.native_wgrad``)."""
    if not (t.is_cuda and FLAGS.wgrad_side and native_wgrad(t, t)) or torch.cuda.is_current_stream_capturing():
        return None
    return _side_stream(t.device, 0)


def _ready_on(t, side):
    """``side`` ordered after the current stream's work so far (``t`` is complete there)."""
    side.wait_stream(torch.cuda.current_stream(t.device))
    return side


def _prep_backward_dq(dqv, nq, *args, **kw):
    """:func:`prep_backward` in place on the ``q`` part of ``d[q|v]`` -> ``dw``.  d[q|v] may be handed
    on with ``_xdot_ready_on`` (its weight gradient then runs on that stream without waiting for the
    current one): the pass runs on that same stream, and the current stream waits for it."""
    dq, on = dqv[..., :nq], getattr(dqv, "_xdot_ready_on", None)
    if on is None:
        return prep_backward(dq, *args, out=dq, **kw)[1]
    here = torch.cuda.current_stream(dqv.device)
    with _on_stream(on, here):
        dw = prep_backward(dq, *args, out=dq, **kw)[1]
    here.wait_stream(on)
    if dw is not None:
        dw.record_stream(here)
    return dw


class AttnBlockFn(torch.autograd.Function):
    @staticmethod
    @_ext.pinned
    def forward(ctx, xk, xqv, mask, wk, bk, wq, bq, wv, bv, wc, bc, H, scale, comm, chunk_plan, sync, grad_on, rope, Hg,
                layout, wkn, wqn, norm_eps, sinks, wg, bg):
        # every argument is passed, None for an absent feature: the backward returns one gradient per name
        # Hg: gathered heads when fewer than H (grouped-query attention): wq / wv hold Hg heads
        # layout: the row sharding (xdot.parallel.layout): the rotary positions and the mask follow it
        # wkn / wqn: the (D,) gains of QK-norm on k / q (both or neither), norm_eps its eps
        # sinks: the (H,) attention-sink logits (a replicated parameter) or None
        # wg / bg: the gate projection ((C, C): one gate value per feature, (H, C): one per head) or None
        wqv = _rows(wq, wv)
        bqv = _rows(bq, bv) if bq is not None else None
        n = comm.world_size
        B, R = xqv.shape[0], xqv.shape[1]
        gbuf = None
        if n > 1 and comm.inplace_gather and xqv.is_cuda and \
                len(gather_plan((B, R), xqv, comm, chunk_plan)) == 1:
            # the projection writes this rank's block of the gather output directly: the
            # all-gather runs in place (no copy of the own block; RCCL: sendbuff = recvbuff +
            # rank block, the xGMI pull kernel skips its own-block copy)
            gbuf = torch.empty((n, B, R, wqv.shape[0]), dtype=xqv.dtype, device=xqv.device)
            qv = gbuf[comm.rank]
            proj(xqv, wqv, bqv, out=qv.view(-1, qv.shape[-1]))
        else:
            qv = proj(xqv, wqv, bqv)
        nq = wq.shape[0]
        tab = None
        if rope is not None:  # this rank's global positions
            tab = rope.table(R, nq // (Hg or H), rope.resolve(comm.rank, R, n, layout), qv.device, _table_dtype(qv))
        nsaved = ()
        keep = any(ctx.needs_input_grad)  # a backward can run: the norm passes keep their inputs
        if tab is not None or wqn is not None:
            # q normalised and / or rotated in ONE pass, in place and BEFORE the gather is issued (with
            # the in-place gather this block is what the peers pull); v is untouched
            _, rstd_q, q0 = prep_apply(qv[..., :nq], Hg or H, tab, wqn, norm_eps, out=qv[..., :nq], save=keep)
        pending = start_gather(qv, comm, chunks=chunk_plan, out=gbuf)  # in flight under the row-side GEMM
        # the row side's pre-scale (scale * log2 e) folded into the k projection: one rounding, no
        # separate pass (the attention backward's dk is w.r.t. the unscaled k either way)
        # (the probe reads shape, dtype and device only: a stride-0 view shaped like k)
        k_like = qv[..., :wk.shape[0]] if Hg is None else qv[..., :1].expand(B, R, wk.shape[0])
        pre = xk.shape[-1] == wk.shape[1] and prescale_wanted(k_like, qv, H, Hg)
        # with a gain RMSNorm cancels a scalar: the projection runs unscaled and the prep pass carries
        # the pre-scale; without one it sits in the projection (a rotation commutes with a scalar)
        al = scale * _LOG2E if pre else 1.0
        k = proj(xk, wk, bk, alpha=1.0 if wkn is not None else al)
        if tab is not None or wkn is not None:
            _, rstd_k, k0 = prep_apply(k, H, tab, wkn, norm_eps, alpha=al if wkn is not None else 1.0, out=k, save=keep)
            if keep and wkn is not None:
                nsaved = (k0, rstd_k, wkn, q0, rstd_q, wqn)
        # the gate projection beside the k projection: under the all-gather too
        g = proj(xk, wg, bg) if wg is not None else None
        actx = _Ctx()
        actx.needs_input_grad = (any(ctx.needs_input_grad),) * 2  # a backward can run (score buffers)
        o = SeqParallelAttention.forward(actx, k, qv, mask, H, scale, comm, pending, pre, grad_on, Hg,  # k_prescaled
                                         layout, sinks)
        # gated attention: o' = o * sigmoid(g), out of place (the attention keeps o for delta)
        og = gate_apply(o, g, H) if g is not None else o
        out = proj(og, wc, bc)
        ctx.actx = actx
        ctx.sync = sync  # (GradSync, module key) or None
        ctx.params = (wk, bk, wq, bq, wv, bv, wc, bc)
        ctx.sinks = sinks
        ctx.gate = (wg, bg) if wg is not None else None
        ctx.nq = nq
        ctx.rope_tab, ctx.H, ctx.Hg = tab, H, Hg or H
        ctx.has_b = (bk is not None, bq is not None, bc is not None)
        # the attention's tensors go through save_for_backward too (version checks, and a graph
        # retained for a second backward keeps them)
        asaved, actx._saved = actx._saved, None
        ctx.nnorm = len(nsaved)
        gsaved = (og, g, wg) if g is not None and keep else ()
        ctx.ngate = len(gsaved)
        ctx.save_for_backward(xk, xqv, wk, wqv, wc, o, *gsaved, *nsaved, *asaved)
        return out

    @staticmethod
    @_ext.pinned
    def backward(ctx, dout):
        xk, xqv, wk, wqv, wc, o, *asaved = ctx.saved_tensors
        gsaved, asaved = asaved[:ctx.ngate], asaved[ctx.ngate:]
        nsaved, asaved = asaved[:ctx.nnorm], asaved[ctx.nnorm:]
        oc = gsaved[0] if gsaved else o  # what the output projection read: o' with a gate
        ctx.actx._saved = tuple(asaved)
        ng = ctx.needs_input_grad
        hk, hq, hc = ctx.has_b
        dout = dout.contiguous()
        # output projection: d(o) for the attention on this stream; its weight / bias gradients
        # (only needed by the optimizer) on a second stream, under the attention backward
        wk_, bk_, wq_, bq_, wv_, bv_, wc_, bc_ = ctx.params
        sync = None
        if ctx.sync is not None:
            gs, key = ctx.sync
            # deliver only when this forward was the parameters' ONLY use since the last wait():
            # a module called twice has its gradients summed by autograd (AccumulateGrad) first
            sync = gs if gs.sole_use(key) else None
        # weight gradients handed to GradSync in its wire dtype (fp32 for a bf16 module reduced in
        # fp32: straight from the kernels' fp32 sums, no conversion pass before the all-reduce)
        wdt = (lambda *ps: torch.float32 if any(p is not None and sync.wire_dtype(p) == torch.float32 for p in ps)
               else None) if sync is not None else (lambda *ps: None)
        side = _wgrad_stream(dout)
        if side is None:
            do, dwc, dbc = linear_backward(dout, oc, wc, True, ng[_I.wc], hc and ng[_I.bc], dw_dtype=wdt(wc_, bc_))
        else:
            do, _, _ = linear_backward(dout, oc, wc, True, False, False)
            dout._xdot_ready_on = _ready_on(dout, side)
            _, dwc, dbc = linear_backward(dout, oc, wc, False, ng[_I.wc], hc and ng[_I.bc], join=False, dw_dtype=wdt(wc_, bc_))
        # the current stream is only looked up when a side stream is in play (host cost per call)
        cur = torch.cuda.current_stream(dout.device) if side is not None else None
        if sync is not None:  # hand the output projection's gradients to GradSync now: their
            # all-reduce runs under the attention backward (stream None: the current one)
            sync.deliver([(wc_, dwc), (bc_, dbc)], stream=side)
            dwc = dbc = None
        dg = None
        if gsaved:  # do' -> do in place, and dg: one launch
            _, dg = gate_backward(do, o, gsaved[1], ctx.H, out=do)
        agrads = SeqParallelAttention.backward(ctx.actx, do)
        dk, dqv, dsk = agrads[0], agrads[1], agrads[-1]  # (dsk: this rank's rows' share of the sinks' gradient)
        if dsk is not None and not ng[_I.sinks]:
            dsk = None
        if dsk is not None and sync is not None:  # a replicated parameter like the others: summed by GradSync
            sync.deliver([(ctx.sinks, dsk)])
            dsk = None
        dwkn = dwqn = None
        if nsaved or ctx.rope_tab is not None:
            # gradients w.r.t. the normalised and / or rotated k / q -> w.r.t. the projections'
            # outputs, in place, before anything below reads them: the inverse rotation, with QK-norm
            # folded into the norm's backward, whose gain gradients are ordered sums (csrc/headnorm.hip)
            k0, rstd_k, wkn, q0, rstd_q, wqn = nsaved or (None,) * 6
            _, dwkn = prep_backward(dk, ctx.H, ctx.rope_tab, wkn, k0, rstd_k, out=dk, need_dw=ng[_I.wkn])
            dwqn = _prep_backward_dq(dqv, ctx.nq, ctx.Hg, ctx.rope_tab, wqn, q0, rstd_q, need_dw=ng[_I.wqn])
        # the row-side weight gradient also runs beside the input-gradient GEMMs that follow
        # d[q|v] may be ready on the backward's priority stream (``_xdot_ready_on``): its weight
        # gradient runs there, under the row-side kernel (linear_backward)
        qv_on = getattr(dqv, "_xdot_ready_on", None) if native_wgrad(dqv, xqv) else None  # (as linear_backward)
        need_wk, need_wqv, need_bqv = ng[_I.wk], ng[_I.wq] or ng[_I.wv], hq and (ng[_I.bq] or ng[_I.bv])
        kdt, qvdt = wdt(wk_, bk_), wdt(wq_, bq_, wv_, bv_)
        if side is None and qv_on is None and need_wk and need_wqv:
            # one stream: dWk and dW[q|v] in ONE launch (weight_grad_pair)
            dxk, _, dbk = linear_backward(dk, xk, wk, ng[_I.xk], False, hk and ng[_I.bk], dw_dtype=kdt)
            dxqv, _, dbqv = linear_backward(dqv, xqv, wqv, ng[_I.xqv], False, need_bqv, dw_dtype=qvdt)
            dwk, dwqv = weight_grad_pair(dk, xk, dqv, xqv, kdt or qvdt or wk.dtype)
        else:
            if side is None:
                dxk, dwk, dbk = linear_backward(dk, xk, wk, ng[_I.xk], need_wk, hk and ng[_I.bk], dw_dtype=kdt)
            else:
                dk._xdot_ready_on = _ready_on(dk, side)
                dxk, _, _ = linear_backward(dk, xk, wk, ng[_I.xk], False, False)
                _, dwk, dbk = linear_backward(dk, xk, wk, False, need_wk, hk and ng[_I.bk], join=False, dw_dtype=kdt)
            dxqv, dwqv, dbqv = linear_backward(dqv, xqv, wqv, ng[_I.xqv], need_wqv, need_bqv, dw_dtype=qvdt)
        dwg = dbg = None
        if dg is not None:
            # the gate projection reads the row-side input too: its input gradient is added to dx_k
            # (one add pass), its weight / bias gradients are this rank's partial over its rows
            wg_, bg_ = ctx.gate
            dxg, dwg, dbg = linear_backward(dg, xk, gsaved[2], ng[_I.xk], ng[_I.wg], bg_ is not None and ng[_I.bg],
                                            dw_dtype=wdt(wg_, bg_))
            if dxg is not None:
                dxk = dxg if dxk is None else dxk.add_(dxg)
            if sync is not None:
                sync.deliver([(wg_, dwg), (bg_, dbg)])
                dwg = dbg = None
        n = ctx.nq
        dwq = dwv = dbq = dbv = None
        # the packed products cover both halves; hand back only what is asked for (a frozen
        # queries weight next to a trained values weight gets None, and is never delivered)
        if dwqv is not None:
            dwq, dwv = (dwqv[:n] if ng[_I.wq] else None), (dwqv[n:] if ng[_I.wv] else None)
        if dbqv is not None:
            dbq, dbv = (dbqv[:n] if ng[_I.bq] else None), (dbqv[n:] if ng[_I.bv] else None)
        if sync is not None:
            qv_pairs, k_pairs = [(wq_, dwq), (bq_, dbq), (wv_, dwv), (bv_, dbv)], [(wk_, dwk), (bk_, dbk)]
            if qv_on is side:  # one call: the buckets it completes share one grouped all-reduce
                sync.deliver(qv_pairs + k_pairs, stream=side)
            else:
                sync.deliver(qv_pairs, stream=qv_on)
                sync.deliver(k_pairs, stream=side)
            dwq = dbq = dwv = dbv = dwk = dbk = None
        if side is not None:  # the gradients handed on are complete on this stream
            cur.wait_stream(side)
            for t in (dwc, dbc, dwk, dbk) + tuple(p.grad for p in ctx.params if p is not None and sync is not None):
                if t is not None:
                    t.record_stream(cur)
        # the attention's tensors were only borrowed from ctx.saved_tensors (rebuilt from there by
        # every backward): do not keep them alive through the node after this backward
        ctx.actx._saved = None
        grads = [None] * len(ARG_NAMES)  # (a list filled by index: a dict keyed by name costs 2 us more per call)
        grads[_I.xk], grads[_I.xqv], grads[_I.wkn], grads[_I.wqn], grads[_I.sinks] = dxk, dxqv, dwkn, dwqn, dsk
        grads[_I.wk], grads[_I.bk], grads[_I.wq], grads[_I.bq], grads[_I.wv], grads[_I.bv] = dwk, dbk, dwq, dbq, dwv, dbv
        grads[_I.wc], grads[_I.bc], grads[_I.wg], grads[_I.bg] = dwc, dbc, dwg, dbg
        return tuple(grads)
