"""Decode: attention of a few new rows over a sequence-sharded ``q`` / ``v`` cache.

In training the gathered side (``queries`` / ``values``) is sharded by rows and all-gathered every step.
With a cache nothing is gathered: every rank keeps the ``(position, q, v)`` slots it owns, attends the
new rows over its own shard (:func:`xdot.ops.flash.decode`, ``csrc/flash_decode.hip``), and only the
fp32 ``(o, lse)`` cross the wire -- ``H*D + H`` floats per row -- to be merged like the column splits of
a forward.  Softmax does not care about column order, so which rank holds which position, and in which
slot, is free: contiguous or zigzag prefill shards, generated tokens appended round-robin.

The cache holds the compute dtype, or fp8 (``cache_dtype="fp8"``): OCP e4m3fn bytes with one fp32 scale per
(slot, gathered head) for each of ``q`` and ``v``, quantised once when a row is appended
(``csrc/flash_decode8.hip``): ``2*Hg*D + 8*Hg + 4`` bytes per slot instead of ``4*Hg*D + 4``.

A ragged batch (sequences of different lengths that come and go) keeps its slots in pages
(:class:`PagedAttnCache`): one pool shared by the sequences, reached through a block table, with every
sequence's length and row position on the device (:func:`xdot.ops.flash.decode_paged`,
``csrc/flash_paged.hip``).  A sequence that ends gives its pages to the next one, and a generation step is
one launch whose arguments do not change, so it can be captured.  The pool, too, holds the compute dtype or
fp8 (``cache_dtype="fp8"``): the dense fp8 format per page, scales ``(num_pages, 2*Hg, page_size)``, filled by
one quantise-and-scatter launch per append and read by a block-table sweep over the bytes
(``csrc/flash_paged8.hip``).

Forward only, no autograd.  Not covered: document masks at decode time, eviction of single slots (a
sequence frees all its pages or none), a paged chunked-prefill kernel (more than 64 rows per gathered head
over pages gather them, bytes and scales of an fp8 pool as they are, into a dense cache per call), a device-side ``pos0`` for the dense
:class:`AttnCache`, per-channel scales, fp8 rows, and an fp8 kernel for the
shapes neither fp8 kernel takes (fp32 rows, D > 128, Dv != D, more than 128 row heads per gathered head:
they dequantise the whole cache per call).

More than 64 rows per gathered head (chunked prefill, a long user turn or draft) run a row-blocked kernel
under the same contract, through the same calls: ``csrc/flash_extend.hip`` over a 16-bit cache, where D = 96
calls with more than 128 new rows still take the forward kernels over a dense mask
(:func:`xdot.ops.flash.extend_eligible`, ``profiles/extend.md``), and ``csrc/flash_extend8.hip`` over an fp8
cache at every row count (:func:`xdot.ops.flash.extend_fp8_eligible`, ``profiles/extend_fp8.md``)."""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from .. import _ext
from ..ops import flash
from ..utils import comm as _comm
from . import _ref

__all__ = ["AttnCache", "PagedAttnCache", "decode_attention"]


class AttnCache:
    """One rank's shard of the gathered side: ``qv`` (B, capacity, 2*Hg*D), each slot ``[q | v]`` as the
    module's packed projection lays it out (``q`` after norm and rope), ``pos`` (B, capacity) int32 the
    global position of each slot (-1 = empty), and ``fill``, the slots taken, kept on the host.

    ``cache_dtype`` ``"fp8"`` / ``torch.float8_e4m3fn``: ``qv`` holds e4m3fn bytes and ``scales`` (B, 2*Hg,
    capacity) fp32 one factor per slot and chunk (rows ``0..Hg-1`` the ``q`` heads, ``Hg..2*Hg-1`` the ``v``
    heads): value = scale * byte.  A chunk (the D features of one head of ``q`` or ``v`` of one slot) is
    quantised when it is appended: ``s = max|x| / 448``, bytes = ``x / s`` rounded to nearest even; a
    non-finite input makes its chunk non-finite.  ``dtype`` stays the compute dtype: of the rows appended,
    of :meth:`dequant` and of the decode output."""

    def __init__(self, batch: int, capacity: int, Hg: int, D: int, dtype: torch.dtype, device=None, cache_dtype=None):
        if min(int(batch), int(capacity), int(Hg), int(D)) < 1:
            raise ValueError(f"AttnCache: batch, capacity, Hg and D must be positive, got {(batch, capacity, Hg, D)}")
        if cache_dtype not in (None, "fp8", torch.float8_e4m3fn):
            raise ValueError(f"AttnCache: cache_dtype must be None, 'fp8' or torch.float8_e4m3fn, got {cache_dtype!r}")
        self.Hg, self.D, self.capacity, self.fill, self.dtype = int(Hg), int(D), int(capacity), 0, dtype
        self.fp8 = cache_dtype is not None
        # zeros (and scales of 1): the kernels multiply empty slots' v by a probability of 0 and a finite scale
        self.qv = torch.zeros(int(batch), self.capacity, 2 * self.Hg * self.D, device=device,
                              dtype=torch.float8_e4m3fn if self.fp8 else dtype)
        self.scales = torch.ones(int(batch), 2 * self.Hg, self.capacity, dtype=torch.float32, device=device) if self.fp8 else None
        self.pos = torch.full((int(batch), self.capacity), -1, dtype=torch.int32, device=device)

    @property
    def q(self) -> Tensor:
        return self.qv[..., :self.Hg * self.D]

    @property
    def v(self) -> Tensor:
        return self.qv[..., self.Hg * self.D:]

    @property
    def qscale(self) -> Optional[Tensor]:
        """(B, Hg, capacity): the scales of :attr:`q` (None for a cache in the compute dtype)."""
        return self.scales[:, :self.Hg] if self.fp8 else None

    @property
    def vscale(self) -> Optional[Tensor]:
        return self.scales[:, self.Hg:] if self.fp8 else None

    def dequant(self) -> Tuple[Tensor, Tensor]:
        """``(q, v)`` (B, capacity, Hg*D) in the compute dtype: the stored halves, times their scales."""
        if not self.fp8:
            return self.q, self.v
        qv = _ref.cache_dequant(self.qv, self.scales.transpose(1, 2), self.Hg, self.dtype)
        return qv[..., :self.Hg * self.D], qv[..., self.Hg * self.D:]

    @torch.no_grad()
    def append(self, qv: Tensor, positions: Union[int, Tensor]) -> None:
        """Write ``qv`` (B, n, 2*Hg*D) into the next ``n`` free slots.  ``positions``: the global position
        of the first of ``n`` consecutive ones (int), or an ``(n,)`` integer tensor."""
        B, cap = self.pos.shape
        if qv.dim() != 3 or qv.shape[0] != B or qv.shape[2] != self.qv.shape[2]:
            raise ValueError(f"AttnCache.append: qv must be (B, n, 2*Hg*D) = ({B}, n, {self.qv.shape[2]}), got {tuple(qv.shape)}")
        n, at = qv.shape[1], self.fill
        if at + n > cap:
            raise RuntimeError(f"AttnCache.append: {n} rows do not fit, {at} of {cap} slots are taken")
        if isinstance(positions, Tensor):
            if positions.numel() != n:
                raise ValueError(f"AttnCache.append: {positions.numel()} positions for {n} rows")
            p = positions.reshape(1, n).to(device=self.pos.device, dtype=torch.int32)
        else:
            p = torch.arange(int(positions), int(positions) + n, dtype=torch.int32, device=self.pos.device).view(1, n)
        if not self.fp8:
            self.qv[:, at:at + n].copy_(qv)
        elif n and _ext.use_hip(qv) and qv.dtype in (torch.bfloat16, torch.float16) and self.D in (32, 64, 96, 128):
            _ext.ops().cache_quant(qv, self.qv, self.scales, at, self.Hg)  # straight into the slots
        elif n:
            b8, s = _ref.cache_quant(qv, self.Hg)
            self.qv[:, at:at + n].copy_(b8)
            self.scales[:, :, at:at + n].copy_(s.transpose(1, 2))
        self.pos[:, at:at + n] = p
        self.fill = at + n


class PagedAttnCache:
    """One rank's shard of the gathered side of a ragged batch, in pages: ``qv`` (num_pages, page_size,
    2*Hg*D) a pool of slots ``[q | v]`` shared by the ``batch`` sequences, ``pos`` (num_pages, page_size)
    int32 the global position of each slot (-1 = empty), ``table`` (batch, num_pages) int32 the page of each
    logical block of each sequence (-1 past its pages) and ``npages`` (batch,) int32 the entries in use: the
    format of :func:`xdot.ops.flash.decode_paged`, which reads the last three on the device.  The free list and
    the sequences' lengths are kept on the host, so appending and freeing never wait for the device.  A
    sequence takes a page when its last one is full and gives all of them back with :meth:`free`.

    ``cache_dtype`` ``"fp8"`` / ``torch.float8_e4m3fn``: ``qv`` holds e4m3fn bytes and ``scales`` (num_pages,
    2*Hg, page_size) fp32 one factor per slot and chunk, the slot innermost within its page (rows ``0..Hg-1`` the
    ``q`` heads, ``Hg..2*Hg-1`` the ``v`` heads): :class:`AttnCache`'s fp8 format and quantisation rule, bit for
    bit, page by page.  ``dtype`` stays the compute dtype.  :meth:`free` leaves bytes and scales as they are
    (finite); only the positions go to -1."""

    def __init__(self, batch: int, num_pages: int, page_size: int, Hg: int, D: int, dtype: torch.dtype, device=None,
                 cache_dtype=None):
        if min(int(batch), int(num_pages), int(Hg), int(D)) < 1 or int(page_size) not in flash.PAGE_SIZES:
            raise ValueError("PagedAttnCache: batch, num_pages, Hg and D must be positive and page_size one of "
                             f"{flash.PAGE_SIZES}, got {(batch, num_pages, page_size, Hg, D)}")
        if cache_dtype not in (None, "fp8", torch.float8_e4m3fn):
            raise ValueError(f"PagedAttnCache: cache_dtype must be None, 'fp8' or torch.float8_e4m3fn, got {cache_dtype!r}")
        self.Hg, self.D, self.page_size, self.num_pages, self.dtype = int(Hg), int(D), int(page_size), int(num_pages), dtype
        self.fp8 = cache_dtype is not None
        # zeros (and scales of 1): the kernels multiply empty slots' v by a probability of 0 and a finite scale
        self.qv = torch.zeros(self.num_pages, self.page_size, 2 * self.Hg * self.D, device=device,
                              dtype=torch.float8_e4m3fn if self.fp8 else dtype)
        self.scales = (torch.ones(self.num_pages, 2 * self.Hg, self.page_size, dtype=torch.float32, device=device)
                       if self.fp8 else None)
        self.pos = torch.full((self.num_pages, self.page_size), -1, dtype=torch.int32, device=device)
        self.table = torch.full((int(batch), self.num_pages), -1, dtype=torch.int32, device=device)
        self.npages = torch.zeros(int(batch), dtype=torch.int32, device=device)
        self.free_pages = list(range(self.num_pages - 1, -1, -1))  # taken from the end: page 0 first
        self.pages = [[] for _ in range(int(batch))]                # of each sequence, in logical order
        self.lens = [0] * int(batch)                                # slots taken by each sequence

    @property
    def q(self) -> Tensor:
        return self.qv[..., :self.Hg * self.D]

    @property
    def v(self) -> Tensor:
        return self.qv[..., self.Hg * self.D:]

    @property
    def qscale(self) -> Optional[Tensor]:
        """(num_pages, Hg, page_size): the scales of :attr:`q` (None for a pool in the compute dtype)."""
        return self.scales[:, :self.Hg] if self.fp8 else None

    @property
    def vscale(self) -> Optional[Tensor]:
        return self.scales[:, self.Hg:] if self.fp8 else None

    def dequant(self) -> Tuple[Tensor, Tensor]:
        """``(q, v)`` (num_pages, page_size, Hg*D) in the compute dtype: the stored halves, times their scales."""
        if not self.fp8:
            return self.q, self.v
        qv = _ref.cache_dequant(self.qv, self.scales.transpose(1, 2), self.Hg, self.dtype)
        return qv[..., :self.Hg * self.D], qv[..., self.Hg * self.D:]

    def _take(self, seqs, n: int) -> Tensor:
        """Give each sequence of ``seqs`` the pages its next ``n`` rows need (all of them or, on a full pool,
        none) -> the rows' flat slot indices (len(seqs) * n,) int64 on the host."""
        S = self.page_size
        need = [(self.lens[b] + n + S - 1) // S - len(self.pages[b]) for b in seqs]
        if sum(need) > len(self.free_pages):
            raise RuntimeError(f"PagedAttnCache: {n} rows for {len(seqs)} sequence(s) need {sum(need)} pages, "
                               f"{len(self.free_pages)} of {self.num_pages} are free")
        slots = []
        for b, k in zip(seqs, need):
            if k > 0:
                new = [self.free_pages.pop() for _ in range(k)]
                at = len(self.pages[b])
                self.pages[b] += new
                self.table[b, at:at + k] = torch.tensor(new, dtype=torch.int32)
            i = torch.arange(self.lens[b], self.lens[b] + n)
            slots.append(torch.tensor(self.pages[b], dtype=torch.int64)[i // S] * S + i % S)
            self.lens[b] += n
        if any(k > 0 for k in need):
            self.npages.copy_(torch.tensor([len(p) for p in self.pages], dtype=torch.int32))
        return torch.cat(slots)

    def _write(self, seqs, rows: Tensor, first) -> None:
        """``rows`` (len(seqs) * n, 2*Hg*D) into the next slots of ``seqs``, at the positions ``first`` (per
        sequence: the first of ``n`` consecutive ones, or ``n`` of them)."""
        n = rows.shape[0] // len(seqs)
        if n == 0:
            return
        p = torch.stack([f.reshape(n).to("cpu", torch.int64) if isinstance(f, Tensor) else torch.arange(int(f), int(f) + n)
                         for f in first]).reshape(-1)
        at = torch.stack([self._take(seqs, n), p])
        if self.fp8 and _ext.use_hip(rows) and rows.dtype in (torch.bfloat16, torch.float16) and self.D in (32, 64, 96, 128):
            at = at.to(torch.int32).to(self.qv.device)  # one copy to the device, one launch: bytes, scales, positions
            _ext.ops().cache_quant_paged(rows, self.qv, self.scales, self.pos, at[0], at[1], self.Hg)
            return
        at = at.to(self.qv.device)  # one copy to the device
        if self.fp8:
            b8, s = _ref.cache_quant(rows, self.Hg)
            self.qv.view(torch.uint8).view(-1, self.qv.shape[-1]).index_copy_(0, at[0], b8.view(torch.uint8))
            self.scales[at[0] // self.page_size, :, at[0] % self.page_size] = s
        else:
            self.qv.view(-1, self.qv.shape[-1]).index_copy_(0, at[0], rows.to(self.dtype))
        self.pos.view(-1).index_copy_(0, at[0], at[1].to(torch.int32))

    def _rows(self, qv: Tensor, B: int, who: str) -> Tensor:
        if qv.dim() != 3 or qv.shape[0] != B or qv.shape[2] != self.qv.shape[2]:
            raise ValueError(f"PagedAttnCache.{who}: qv must be ({B}, n, 2*Hg*D = {self.qv.shape[2]}), got {tuple(qv.shape)}")
        return qv.reshape(-1, qv.shape[2])

    @torch.no_grad()
    def append(self, qv: Tensor, positions) -> None:
        """Append ``qv`` (B, n, 2*Hg*D): ``n`` rows to every sequence.  ``positions``: the global position of
        the first of the ``n`` consecutive ones, an int for all sequences or a list of ``B`` ints."""
        B = len(self.pages)
        first = [int(p) for p in positions] if isinstance(positions, (list, tuple)) else [int(positions)] * B
        if len(first) != B:
            raise ValueError(f"PagedAttnCache.append: {len(first)} positions for {B} sequences")
        self._write(list(range(B)), self._rows(qv, B, "append"), first)

    @torch.no_grad()
    def append_seq(self, b: int, qv: Tensor, position) -> None:
        """Append ``qv`` (1, n, 2*Hg*D) to sequence ``b`` alone (a ragged prefill).  ``position``: the first of
        ``n`` consecutive global positions (int), or an ``(n,)`` integer tensor."""
        if not 0 <= int(b) < len(self.pages):
            raise IndexError(f"PagedAttnCache.append_seq: sequence {b} of {len(self.pages)}")
        self._write([int(b)], self._rows(qv, 1, "append_seq"), [position])

    @torch.no_grad()
    def free(self, b: int) -> None:
        """Empty sequence ``b``: its slots' positions become -1 and its pages return to the free list."""
        pages = self.pages[b]
        if pages:
            self.pos.index_fill_(0, torch.tensor(pages, dtype=torch.int64).to(self.pos.device), -1)
            self.table[b, :len(pages)] = -1
            self.npages[b] = 0
            self.free_pages += reversed(pages)
        self.pages[b], self.lens[b] = [], 0


@torch.no_grad()
def decode_attention(rows: Tensor, cache: Union[AttnCache, PagedAttnCache], pos0, *, num_heads: int, scale: float,
                     window: Optional[int] = None, sinks: Optional[Tensor] = None,
                     comm: Optional[_comm.Communicator] = None) -> Tuple[Tensor, Tensor]:
    """``rows`` (B, Rn, H*D), the new rows' ``k`` (after norm and rope) at positions ``pos0, pos0 + 1, ...``,
    attended causally (and within ``window``) over the cache shards of all ranks -> (out (B, Rn, H*D) in
    ``rows.dtype``, lse (B, H, Rn)).  All ranks pass the same ``rows`` and get the same result.

    Each rank runs :func:`xdot.ops.flash.decode` over its own shard; with ``comm.world_size > 1`` one
    all-gather of the fp32 ``[o | lse]`` and one merge over the ``N`` slots follow, then the sink fold
    (``sinks`` (H,)), under which a row that sees nothing anywhere gives 0.

    With a :class:`PagedAttnCache` the batch is ragged: ``pos0`` is a list of ``B`` ints or a ``(B,)`` int32
    tensor on the rows' device (negative: the sequence is inactive), and each rank runs
    :func:`xdot.ops.flash.decode_paged` over its pool (with its scales, if it is fp8)."""
    comm = comm if comm is not None else _comm.get_comm()
    H, n = int(num_heads), comm.world_size
    if isinstance(cache, PagedAttnCache):
        p0 = pos0 if isinstance(pos0, Tensor) else torch.tensor([int(p) for p in pos0], dtype=torch.int32).to(rows.device)
        o, lse = flash.decode_paged(rows, cache.q, cache.v, cache.pos, cache.table, cache.npages, p0, H, scale,
                                    int(window or 0), Hg=cache.Hg, out_fp32=n > 1, qscale=cache.qscale, vscale=cache.vscale)
    else:
        o, lse = flash.decode(rows, cache.q, cache.v, cache.pos, int(pos0), H, scale, int(window or 0), Hg=cache.Hg,
                              out_fp32=n > 1, qscale=cache.qscale, vscale=cache.vscale)
    hip = _ext.use_hip(rows)
    if n > 1:
        no = o.numel()
        wire = torch.cat([o.reshape(-1), lse.reshape(-1).to(o.dtype)])
        got = torch.empty(n, wire.numel(), dtype=wire.dtype, device=wire.device)
        comm.all_gather_into(got, wire)
        opart, lpart = got[:, :no].reshape(n, *o.shape), got[:, no:].reshape(n, *lse.shape)
        if hip:
            o, lse = flash.fwd_combine(opart.contiguous(), lpart.contiguous(), H, rows)
        else:
            o, lse = _ref.combine([(opart[r], lpart[r]) for r in range(n)], rows.dtype)
    if sinks is not None:
        o, lse = (flash.sink_fold if hip else _ref.sink_fold)(o, lse, sinks, H)
    return o, lse
